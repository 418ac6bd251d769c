// Device-side decode-step bookkeeping (gfx950).
//
// decode_advance sits at the head of the captured decode graph and derives
// every per-step input of the forward from persistent per-row state plus the
// previous step's sampled tokens, so step n+1 can be enqueued before the host
// has seen step n's tokens.
//
// Persistent per-row state (the graph's io tensors):
//   positions[rows] i64, seq_lens[rows] i32, block_tables[rows, max_blocks] i32
// Outputs consumed by the forward: input_ids[rows] i64, slot_mapping[rows] i64
// (plus the updated state).
//
// ctl is one int32 staging block [4*rows + 4], one H2D copy per step:
//   ctl[0*rows + r]  src_idx   >=0: input id = sampled_prev[src_idx]
//                              -1 : input id / position come from the host
//                              -2 : padding row
//   ctl[1*rows + r]  new_blk   page id to install at table[r, pos/page], or -1
//   ctl[2*rows + r]  host_ids  (src_idx == -1 only)
//   ctl[3*rows + r]  host_pos  (src_idx == -1 only)
//   ctl[4*rows]      n_live    rows >= n_live are padding; < 0: pass-through
//                              (the host filled the io tensors itself)
//
// sampled_prev is read here and rewritten by the argmax at the graph's tail.
// The graph is a single chain on one stream, and the only consumer of the old
// values is this kernel, which copies them into input_ids (another buffer)
// before anything later in the chain runs — so one buffer is enough.

#include <hip/hip_runtime.h>

__global__ __launch_bounds__(256) void decode_advance_kernel(
    long* __restrict__ input_ids, long* __restrict__ positions,
    int* __restrict__ seq_lens, long* __restrict__ slot_mapping,
    int* __restrict__ block_tables, const long* __restrict__ sampled_prev,
    const int* __restrict__ ctl, int rows, int max_blocks, int page) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int n_live = ctl[4 * rows];
  if (n_live < 0) return;                       // pass-through step
  const int src = ctl[r];
  if (r >= n_live || src < -1 || src >= rows) {
    // padding row: attends over one slot of its own table, writes no KV
    input_ids[r] = 0;
    positions[r] = 0;
    seq_lens[r] = 1;
    slot_mapping[r] = -1;
    return;
  }
  long pos;
  if (src >= 0) {
    input_ids[r] = sampled_prev[src];
    pos = positions[r] + 1;
  } else {
    input_ids[r] = (long)ctl[2 * rows + r];
    pos = (long)ctl[3 * rows + r];
  }
  positions[r] = pos;
  seq_lens[r] = (int)pos + 1;
  const long bi = pos / page;
  if (pos < 0 || bi >= max_blocks) {            // never index past the row
    slot_mapping[r] = -1;
    return;
  }
  int* trow = block_tables + (long)r * max_blocks;
  const int nb = ctl[rows + r];
  int blk;
  if (nb >= 0) {
    trow[bi] = nb;
    blk = nb;
  } else {
    blk = trow[bi];
  }
  slot_mapping[r] = (long)blk * page + pos % page;
}

void launch_decode_advance(long* input_ids, long* positions, int* seq_lens,
                           long* slot_mapping, int* block_tables,
                           const long* sampled_prev, const int* ctl, int rows,
                           int max_blocks, int page, hipStream_t stream) {
  decode_advance_kernel<<<dim3((unsigned)((rows + 255) / 256)), 256, 0,
                          stream>>>(input_ids, positions, seq_lens,
                                    slot_mapping, block_tables, sampled_prev,
                                    ctl, rows, max_blocks, page);
}
