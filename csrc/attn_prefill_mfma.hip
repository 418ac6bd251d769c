// Fresh prefill attention (every sequence of the step starts at position
// 0): the shared MFMA flash body of attn_prefill_core.h with K/V taken
// straight from the qkv projection, ctx = 0.
//
// Replaces the per-row prefill path (each query re-reading its context —
// measured 1.34 ms/layer at 8k prefill tokens, profiles/r01): K/V stream
// through LDS once per 256-row q tile and the matmuls run on the matrix
// cores (v_mfma_f32_32x32x16_bf16).
#include "attn_prefill_core.h"

namespace {

// K/V rows of one (sequence, kv head) in [T, KV, 128] tensors whose row
// stride may be that of a fused qkv buffer.  Position p is row p of the
// sequence; the body asks only for p < n, so no row of another sequence (or
// past T) is read.
struct StridedKV {
  const bf16* k;      // at (row t0, head kvh)
  const bf16* v;
  long sk, sv;        // row strides, elements
  DEV void begin_tile(int) {}
  DEV uint4 k8(int kv0, int r, int col) const {
    return *reinterpret_cast<const uint4*>(k + (long)(kv0 + r) * sk + col);
  }
  DEV uint4 v8(int kv0, int r, int col) const {
    return *reinterpret_cast<const uint4*>(v + (long)(kv0 + r) * sv + col);
  }
};

__global__ __launch_bounds__(512, 1) void attn_prefill_mfma_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const int* __restrict__ seq_start, int num_heads, int num_kv_heads,
    float scale, long sq, long sk, long sv) {
  const int h = blockIdx.y;
  const int kvh = h / (num_heads / num_kv_heads);
  const int z = blockIdx.z;
  const long t0 = seq_start[z];
  const int n = seq_start[z + 1] - (int)t0;
  const int q0 = blockIdx.x * QTILE;
  if (q0 >= n) return;
  StridedKV src{k + t0 * sk + (long)kvh * HD, v + t0 * sv + (long)kvh * HD,
                sk, sv};
  attn_prefill_body(out, q, src, t0, n, 0, q0, h, num_heads, scale, sq);
}

}  // namespace

void launch_attn_prefill_mfma(bf16* out, const bf16* q, const bf16* k,
                              const bf16* v, const int* seq_start,
                              int num_seqs, int max_seqlen, int num_heads,
                              int num_kv_heads, int head_dim, float scale,
                              long sq, long sk, long sv,
                              hipStream_t stream) {
  if (head_dim != HD)
    throw std::runtime_error("attn_prefill_mfma: head_dim must be 128");
  if (num_seqs <= 0 || max_seqlen <= 0) return;
  dim3 grid((unsigned)((max_seqlen + QTILE - 1) / QTILE),
            (unsigned)num_heads, (unsigned)num_seqs);
  attn_prefill_mfma_kernel<<<grid, 512, 0, stream>>>(
      out, q, k, v, seq_start, num_heads, num_kv_heads, scale, sq, sk, sv);
}
