// Presence, frequency and repetition penalties on the bf16 logits, with the
// per-row token counts kept in device memory next to them.
//
// State is a table int32 [slots, vocab]; the word of token t in a row is
//     2 * c[t] + (t occurs in the prompt ? 1 : 0)
// where c[t] counts t among the row's generated tokens.  So "t was seen at
// all" is word != 0 and c[t] is word >> 1.  A logits row names its table
// row through slot[r]; slot < 0 (or past the table) = not a penalty row.
//
//   penalty_build  makes table rows encode whole histories (host-known, at a
//                  re-seed or on the synchronous step).  Never captured.
//   penalty_apply  rewrites the seen logits of the penalty rows in place.
//   penalty_note   counts the token each penalty row has just sampled.
//
// apply and note read every per-row parameter from device memory and their
// grids depend on the row count and the vocabulary alone, so both sit in the
// captured decode graph around the sampler.
//
// The arithmetic of penalty_apply is held to bit-equality with an fp32
// reference that does one IEEE operation at a time:
//     q = l > 0 ? l / r : l * r
//     q = q - f * (float)c          (product rounded, then the difference)
//     q = q - (c > 0 ? p : 0)
//     l' = bf16 round-to-nearest-even of q
// `a / b` is the correctly rounded division here; the compiler would fuse
// the product and the difference into one v_fma_f32 (one rounding instead of
// two), which `#pragma clang fp contract(off)` in penalise() forbids.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int kApplyVecs = 4;                      // 8-logit vectors / thread
constexpr int kApplyChunk = 256 * kApplyVecs * 8;  // logits per workgroup

DEV unsigned short penalise(unsigned short b, int word, float r, float p,
                            float f) {
#pragma clang fp contract(off)
  const float l = bf2f(b);
  const int c = word >> 1;
  float q = l > 0.f ? l / r : l * r;
  const float fc = f * (float)c;
  q = q - fc;
  q = q - (c > 0 ? p : 0.f);
  if (q != q) return 0x7fc0u;    // NaN from out-of-contract parameters
  return f2bf(q);
}

DEV bool is_nan_bits(unsigned short b) { return (b & 0x7fffu) > 0x7f80u; }

}  // namespace

// One workgroup per history.  Zero the slot's row, then accumulate the
// history into it with atomics (a token may occur many times, in the hands
// of different threads).
__global__ __launch_bounds__(256) void penalty_build_kernel(
    int* __restrict__ table, const int* __restrict__ slots,
    const int* __restrict__ tokens, const int* __restrict__ offsets,
    const int* __restrict__ prompt_len, int nslots, int vocab, int total) {
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= nslots) return;          // uniform per workgroup
  int* row = table + (long)slot * vocab;
  const int tid = threadIdx.x;

  // zero: scalar head up to the 16-byte grid, vectors, scalar tail
  const int head = min(vocab, (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3));
  const int nvec = (vocab - head) >> 2;
  if (tid < head) row[tid] = 0;
  int4* body = reinterpret_cast<int4*>(row + head);
  for (int v = tid; v < nvec; v += 256) body[v] = make_int4(0, 0, 0, 0);
  for (int j = head + nvec * 4 + tid; j < vocab; j += 256) row[j] = 0;

  // The zeroing stores must have landed before the first atomic on the same
  // word, which may come from another wave.  __syncthreads() is a workgroup-
  // scope release / barrier / acquire, and that is enough here: the waves of
  // a workgroup run on one CU and share its vector-memory path, which hands
  // requests to one address to the L2 channel in issue order; plain stores
  // write through to that L2 and the atomics execute in it, so a store
  // issued before the barrier is performed before an atomic issued after
  // it.  No other workgroup touches this row (the callers never give two
  // histories of one launch the same slot), so no wider scope is needed.
  __syncthreads();

  const int begin = max(offsets[blockIdx.x], 0);
  const int end = min(offsets[blockIdx.x + 1], total);
  const int np = prompt_len[blockIdx.x];
  for (int i = begin + tid; i < end; i += 256) {
    const int t = tokens[i];
    if (t < 0 || t >= vocab) continue;
    if (i - begin < np) atomicOr(&row[t], 1);
    else                atomicAdd(&row[t], 2);     // never carries into bit 0
  }
}

// grid rows * chunks, chunks = ceil((vocab + 8) / kApplyChunk), the chunk
// index varying fastest: workgroups are dealt to the 8 XCDs round-robin by
// their linear id, so the chunks of ONE row spread over the whole chip.
// With the row index fastest, penalty rows on every 8th row of a 2048-row
// batch all landed on one XCD and the launch took 5x as long (measured:
// profiles/r09_penalties.md).  Memory-bound: 2 bytes of logit and 4 bytes of
// state per token, 16-byte loads of both where the rows lie on the 16-byte
// grid (any vocabulary that is a multiple of 8).  A logits row off that
// grid is read from the aligned address below it, as logit_scan.h does; its
// state words are then fetched one by one.
__global__ __launch_bounds__(256) void penalty_apply_kernel(
    bf16* __restrict__ logits, const int* __restrict__ slot_of,
    const float* __restrict__ rep, const float* __restrict__ pres,
    const float* __restrict__ freq, const int* __restrict__ table,
    int nslots, int vocab, int chunks) {
  const int r_ = blockIdx.x / chunks;
  const int chunk = blockIdx.x - r_ * chunks;
  const int slot = slot_of[r_];
  if (slot < 0 || slot >= nslots) return;          // before any logit access
  const float r = rep[r_], p = pres[r_], f = freq[r_];
  unsigned short* row =
      reinterpret_cast<unsigned short*>(logits) + (long)r_ * vocab;
  const int* trow = table + (long)slot * vocab;

  const int a = (int)(((uintptr_t)row >> 1) & 7);  // row's offset in its vector
  uint4* base = reinterpret_cast<uint4*>(row - a);
  const int end = a + vocab;
  const int nvec = (end + 7) >> 3;
  const bool tvec = a == 0 && (((uintptr_t)trow) & 15) == 0;
  const int v0 = chunk * (256 * kApplyVecs);

  #pragma unroll
  for (int k = 0; k < kApplyVecs; ++k) {
    const int v = v0 + k * 256 + threadIdx.x;
    if (v >= nvec) break;
    const int j0 = v * 8;                          // in the aligned frame
    const bool whole = j0 >= a && j0 + 8 <= end;
    const uint4 q = base[v];
    unsigned int wd[4] = {q.x, q.y, q.z, q.w};
    int st[8];
    if (whole && tvec) {
      const int4 s0 = *reinterpret_cast<const int4*>(trow + j0);
      const int4 s1 = *reinterpret_cast<const int4*>(trow + j0 + 4);
      st[0] = s0.x; st[1] = s0.y; st[2] = s0.z; st[3] = s0.w;
      st[4] = s1.x; st[5] = s1.y; st[6] = s1.z; st[7] = s1.w;
    } else {
      #pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = j0 + i;
        st[i] = (j >= a && j < end) ? trow[j - a] : 0;   // 0 = leave alone
      }
    }
    unsigned int changed = 0;
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned short b =
          (unsigned short)(i & 1 ? wd[i >> 1] >> 16 : wd[i >> 1] & 0xffffu);
      if (st[i] == 0 || is_nan_bits(b)) continue;  // unseen, or NaN: as is
      const unsigned short nb = penalise(b, st[i], r, p, f);
      if (nb == b) continue;
      changed |= 1u << i;
      wd[i >> 1] = i & 1 ? (wd[i >> 1] & 0x0000ffffu) | ((unsigned int)nb << 16)
                         : (wd[i >> 1] & 0xffff0000u) | nb;
    }
    if (!changed) continue;
    if (whole) {
      // this thread is the only one that touches the vector: the lanes
      // that did not change go back with the bits they were loaded with
      base[v] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    } else {
      // a vector shared with the neighbouring row: changed logits only
      unsigned short* vec = reinterpret_cast<unsigned short*>(base + v);
      #pragma unroll
      for (int i = 0; i < 8; ++i)
        if (changed & (1u << i))
          vec[i] = (unsigned short)(i & 1 ? wd[i >> 1] >> 16
                                          : wd[i >> 1] & 0xffffu);
    }
  }
}

// One thread per row.  Two rows of a launch never share a slot (the callers
// see to it); the add is atomic all the same.
__global__ __launch_bounds__(256) void penalty_note_kernel(
    int* __restrict__ table, const int* __restrict__ slot_of,
    const long* __restrict__ sampled, int rows, int nslots, int vocab) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int slot = slot_of[r];
  const long t = sampled[r];
  if (slot < 0 || slot >= nslots || t < 0 || t >= vocab) return;
  atomicAdd(&table[(long)slot * vocab + t], 2);
}

void launch_penalty_build(int* table, const int* slots, const int* tokens,
                          const int* offsets, const int* prompt_len, int n,
                          int nslots, int vocab, int total,
                          hipStream_t stream) {
  if (n <= 0) return;
  penalty_build_kernel<<<dim3((unsigned)n), 256, 0, stream>>>(
      table, slots, tokens, offsets, prompt_len, nslots, vocab, total);
}

void launch_penalty_apply(bf16* logits, const int* slot_of, const float* rep,
                          const float* pres, const float* freq,
                          const int* table, long rows, int nslots, int vocab,
                          hipStream_t stream) {
  if (rows <= 0) return;
  // one extra vector covers a row that starts off the 16-byte grid
  const int chunks = (vocab + 8 + kApplyChunk - 1) / kApplyChunk;
  penalty_apply_kernel<<<dim3((unsigned)(rows * chunks)), 256, 0, stream>>>(
      logits, slot_of, rep, pres, freq, table, nslots, vocab, chunks);
}

void launch_penalty_note(int* table, const int* slot_of, const long* sampled,
                         long rows, int nslots, int vocab,
                         hipStream_t stream) {
  if (rows <= 0) return;
  penalty_note_kernel<<<dim3((unsigned)((rows + 255) / 256)), 256, 0,
                        stream>>>(table, slot_of, sampled, (int)rows, nslots,
                                  vocab);
}
