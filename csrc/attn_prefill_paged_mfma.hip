// Prefill attention that takes K/V from the PAGED CACHE: chunked-prefill
// continuation chunks, the uncached remainder after a prefix-cache hit, and
// fp8 (e4m3fn) KV.  The shared MFMA flash body of attn_prefill_core.h;
// head_dim 128, page size 16, cache layout [NB, KV, 16, 128].
//
// Sequence z owns q/out rows seq_start[z] .. seq_start[z+1]-1; its row i
// sits at position ctx_start[z] + i and attends cache positions
// 0 .. ctx_start[z] + i.  The fused RoPE/append kernel has already written
// the chunk's own K/V into the cache, so everything comes from the cache.
//
// What differs from the fresh kernel (attn_prefill_mfma.hip):
//   source   PagedKV below, not StridedKV: a 64-token tile is four pages;
//            the four page ids are read once per tile at a wave-uniform
//            address (begin_tile), not once per 16-byte unit
//   ctx      ctx_start[z], not 0: it enters the body's tile count and
//            causal mask
//   KV8      e4m3fn bytes are widened to bf16 while staging into LDS (3
//            mantissa bits: the conversion is exact; the cache holds plain
//            casts, no scale); everything after the stage is the bf16 path
//
// Bounds: the body asks for no cache row at position >= ctx_start + n (a
// partly filled last page holds stale bytes); no block-table entry at index
// >= ceil((ctx_start + n) / 16) is read; workgroups with q0 >= n return
// before touching anything, n == 0 included.  The grid depends only on
// (max_seqlen, H, num_seqs) and nothing syncs with the host, so the launch
// is hipGraph-capture-safe like its sibling.
#include "attn_prefill_core.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float float2v;

#define PAGE 16       // KV page size in tokens
#define NPG (KVBLK / PAGE)     // pages per KV tile

// two f32 that are exactly representable in bf16 -> packed bf16 pair
DEV unsigned pk_bf16_exact(float2v f) {
  return (__float_as_uint(f.x) >> 16) | (__float_as_uint(f.y) & 0xffff0000u);
}

// 8 e4m3fn bytes -> 8 bf16 (exact: 3 mantissa bits, exponent range inside
// bf16's)
DEV uint4 fp8x8_to_bf16x8(uint2 w) {
  uint4 r;
  r.x = pk_bf16_exact(__builtin_amdgcn_cvt_pk_f32_fp8(w.x, false));
  r.y = pk_bf16_exact(__builtin_amdgcn_cvt_pk_f32_fp8(w.x, true));
  r.z = pk_bf16_exact(__builtin_amdgcn_cvt_pk_f32_fp8(w.y, false));
  r.w = pk_bf16_exact(__builtin_amdgcn_cvt_pk_f32_fp8(w.y, true));
  return r;
}

// 8 consecutive cache elements starting at element offset `off`, as bf16
template <bool KV8>
DEV uint4 load_kv8(const bf16* cache, long off) {
  if constexpr (KV8) {
    return fp8x8_to_bf16x8(*reinterpret_cast<const uint2*>(
        reinterpret_cast<const unsigned char*>(cache) + off));
  } else {
    return *reinterpret_cast<const uint4*>(cache + off);
  }
}

DEV long sel4(const long (&a)[NPG], int j) {
  return j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
}

// K/V of one (sequence, kv head) through the sequence's block-table row.
template <bool KV8>
struct PagedKV {
  const bf16* k_cache;
  const bf16* v_cache;
  const int* bt;      // the sequence's block-table row
  int npages;         // entries of bt that may be read
  int num_kv_heads, kvh;
  long pbase[NPG];    // element offset of each (page, kv head) block

  // The tile's four pages; the index is wave-uniform, one lookup per tile.
  // Pages past the sequence's last are never dereferenced (their rows are
  // at positions >= ctx_start + n).
  DEV void begin_tile(int kt) {
    #pragma unroll
    for (int j = 0; j < NPG; ++j) {
      const int pi = kt * NPG + j;
      const long pg = pi < npages ? bt[pi] : 0;
      pbase[j] = (pg * num_kv_heads + kvh) * (long)(PAGE * HD);
    }
  }
  DEV long off(int r, int col) const {
    return sel4(pbase, r >> 4) + (r & (PAGE - 1)) * HD + col;
  }
  DEV uint4 k8(int, int r, int col) const {
    return load_kv8<KV8>(k_cache, off(r, col));
  }
  DEV uint4 v8(int, int r, int col) const {
    return load_kv8<KV8>(v_cache, off(r, col));
  }
};

template <bool KV8>
__global__ __launch_bounds__(512, 1) void attn_prefill_paged_mfma_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ q,
    const bf16* __restrict__ k_cache, const bf16* __restrict__ v_cache,
    const int* __restrict__ block_tables, const int* __restrict__ seq_start,
    const int* __restrict__ ctx_start, int num_heads, int num_kv_heads,
    int max_blocks, float scale, long sq) {
  const int h = blockIdx.y;
  const int kvh = h / (num_heads / num_kv_heads);
  const int z = blockIdx.z;
  const long t0 = seq_start[z];
  const int n = seq_start[z + 1] - (int)t0;
  const int q0 = blockIdx.x * QTILE;
  if (q0 >= n) return;
  const int ctx = ctx_start[z];
  PagedKV<KV8> src{k_cache, v_cache, block_tables + (long)z * max_blocks,
                   min((ctx + n + PAGE - 1) / PAGE, max_blocks),
                   num_kv_heads, kvh, {}};
  attn_prefill_body(out, q, src, t0, n, ctx, q0, h, num_heads, scale, sq);
}

}  // namespace

void launch_attn_prefill_paged_mfma(
    bf16* out, const bf16* q, const bf16* k_cache, const bf16* v_cache,
    const int* block_tables, const int* seq_start, const int* ctx_start,
    int num_seqs, int max_seqlen, int num_heads, int num_kv_heads,
    int head_dim, int max_blocks, int block_size, float scale,
    long q_stride, bool kv_fp8, hipStream_t stream) {
  if (head_dim != HD)
    throw std::runtime_error("attn_prefill_paged_mfma: head_dim must be 128");
  if (block_size != PAGE)
    throw std::runtime_error("attn_prefill_paged_mfma: block_size must be 16");
  if (num_seqs <= 0 || max_seqlen <= 0) return;
  dim3 grid((unsigned)((max_seqlen + QTILE - 1) / QTILE),
            (unsigned)num_heads, (unsigned)num_seqs);
  if (kv_fp8)
    attn_prefill_paged_mfma_kernel<true><<<grid, 512, 0, stream>>>(
        out, q, k_cache, v_cache, block_tables, seq_start, ctx_start,
        num_heads, num_kv_heads, max_blocks, scale, q_stride);
  else
    attn_prefill_paged_mfma_kernel<false><<<grid, 512, 0, stream>>>(
        out, q, k_cache, v_cache, block_tables, seq_start, ctx_start,
        num_heads, num_kv_heads, max_blocks, scale, q_stride);
}
