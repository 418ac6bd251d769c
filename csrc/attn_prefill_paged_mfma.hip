// Flash-style varlen causal prefill attention on MFMA (gfx950) that takes
// K/V from the PAGED CACHE: chunked-prefill continuation chunks, the
// uncached remainder after a prefix-cache hit, and fp8 (e4m3fn) KV.
// head_dim 128, page size 16, cache layout [NB, KV, 16, 128].
//
// Sequence z owns q/out rows seq_start[z] .. seq_start[z+1]-1; its row i
// sits at position ctx_start[z] + i and attends cache positions
// 0 .. ctx_start[z] + i.  The fused RoPE/append kernel has already written
// the chunk's own K/V into the cache, so everything comes from the cache.
//
// Geometry is the fresh-prefill kernel's (attn_prefill_mfma.hip), on
// purpose: 8 waves x 32 q rows, KV tiles of 64 tokens ALIGNED AT POSITION
// 0, swapped QK^T, online softmax with one shfl_xor(32), P through the
// per-wave LDS tile, V transposed at stage, the same swizzle.  A row's
// math does not depend on the wave or q tile it lands in, and a fully
// masked KV tile is an exact no-op (alpha == 1, contribution 0), so for a
// bf16 cache every row sees the instruction sequence of the fresh kernel:
// chunked and unchunked prefill compute a row the same way.
//
// What differs from the fresh kernel:
//   staging  a 64-token tile is four pages; the four page ids are read once
//            per tile at a wave-uniform address, not once per 16-byte unit
//   tiles    ceil((ctx_start + q_hi) / 64)
//   mask     kv_pos > ctx_start + q_row
//   KV8      e4m3fn bytes are widened to bf16 while staging into LDS (3
//            mantissa bits: the conversion is exact; the cache holds plain
//            casts, no scale); everything after the stage is the bf16 path
//
// Bounds: no cache row at position >= ctx_start + n is loaded (zeros are
// staged: a partly filled last page holds stale bytes and 0 * NaN in PV
// would poison real rows); no block-table entry at index >=
// ceil((ctx_start + n) / 16) is read; workgroups with q0 >= n return
// before touching anything, n == 0 included.  The grid depends only on
// (max_seqlen, H, num_seqs) and nothing syncs with the host, so the launch
// is hipGraph-capture-safe like its sibling.
#include <float.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float float2v;

#define QBLK 32       // q rows per wave
#define NWAVE 8
#define QTILE (QBLK * NWAVE)   // 256 q rows per workgroup
#define KVBLK 64
#define HD 128        // head_dim
#define PAGE 16       // KV page size in tokens
#define NPG (KVBLK / PAGE)     // pages per KV tile

// XOR swizzle: spread a row-major [rows][128] bf16 tile's column slices
// over LDS banks (guide G4: D=128 rows are a 16-way conflict unswizzled)
DEV int swz(int row, int col_byte) { return col_byte ^ ((row & 7) << 4); }

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
  const int kv_end = ctx + n;                  // valid cache positions
  const int npages = min((kv_end + PAGE - 1) / PAGE, max_blocks);
  const int* bt = block_tables + (long)z * max_blocks;

  // LDS: K tile + V^T tile + per-wave P tiles + per-wave alpha/lsum
  __shared__ __attribute__((aligned(16))) short k_lds[KVBLK * HD];
  __shared__ __attribute__((aligned(16))) short vt_lds[HD * KVBLK];
  __shared__ __attribute__((aligned(16))) short p_lds[NWAVE][QBLK * KVBLK];
  __shared__ float alpha_lds[NWAVE][QBLK];
  __shared__ float lsum_lds[NWAVE][QBLK];

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int lcol = lane & 31;     // q column this lane owns in S^T
  const int lhalf = lane >> 5;

  // ---- load this wave's Q as 8 B-fragments (held for the whole loop) ----
  // B[k=dim][j=q]: lane j = lcol, k = c*16 + lhalf*8 + e  (16B per chunk)
  const int qrow = q0 + wid * QBLK + lcol;
  short8 qfrag[8];
  {
    const bf16* qp = q + (t0 + qrow) * sq + (long)h * HD;
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (qrow < n) {
        qfrag[c] = *reinterpret_cast<const short8*>(
            qp + c * 16 + lhalf * 8);
      } else {
        qfrag[c] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }

  f32x16 acc[4];      // O[q][d] per 32-wide d tile
  #pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x16(0.f);
  float m_run = -FLT_MAX, l_run = 0.f;

  const int q_hi = min(q0 + QTILE, n);         // exclusive
  const int nkv_tiles = (ctx + q_hi + KVBLK - 1) / KVBLK;

  for (int kt = 0; kt < nkv_tiles; ++kt) {
    const int kv0 = kt * KVBLK;
    const int kvn = min(KVBLK, kv_end - kv0);
    // ---- the tile's four pages: element offset of each (page, kv head)
    // block; the index is wave-uniform, one lookup per tile.  Pages past
    // the sequence's last are never dereferenced (their rows are >= kvn).
    long pbase[NPG];
    #pragma unroll
    for (int j = 0; j < NPG; ++j) {
      const int pi = kt * NPG + j;
      const long pg = pi < npages ? bt[pi] : 0;
      pbase[j] = (pg * num_kv_heads + kvh) * (long)(PAGE * HD);
    }
    // ---- stage K [64][128] (swizzled) and V^T [128][64] ----
    {
      // K: 1024 16B units; unit u: row r = u/16, colb = (u%16)*16
      #pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int u = tid + it * 512;
        const int r = u >> 4, cb = (u & 15) << 4;
        uint4 val{0, 0, 0, 0};
        if (r < kvn)
          val = load_kv8<KV8>(k_cache, sel4(pbase, r >> 4) +
                                           (r & (PAGE - 1)) * HD + (cb >> 1));
        *reinterpret_cast<uint4*>(
            reinterpret_cast<char*>(k_lds) + r * 256 + swz(r, cb)) = val;
      }
      // V^T: unit u handles kv rows (2p, 2p+1) x 8 dims: 32 pairs x 16
      // dim-chunks = 512 units; both rows of a pair share a page
      {
        const int u = tid;
        const int p2 = u & 31, dc = u >> 5;          // pair, dim chunk
        const int r0 = 2 * p2;
        const long vb = sel4(pbase, r0 >> 4) + (r0 & (PAGE - 1)) * HD +
                        dc * 8;
        uint4 a{0, 0, 0, 0}, b{0, 0, 0, 0};
        if (r0 < kvn) a = load_kv8<KV8>(v_cache, vb);
        if (r0 + 1 < kvn) b = load_kv8<KV8>(v_cache, vb + HD);
        const unsigned* au = reinterpret_cast<const unsigned*>(&a);
        const unsigned* bu = reinterpret_cast<const unsigned*>(&b);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned av = (au[j >> 1] >> ((j & 1) * 16)) & 0xffff;
          const unsigned bv = (bu[j >> 1] >> ((j & 1) * 16)) & 0xffff;
          const int d = dc * 8 + j;
          *reinterpret_cast<unsigned*>(
              reinterpret_cast<char*>(vt_lds) + d * (KVBLK * 2) +
              swz(d, r0 * 2)) = av | (bv << 16);
        }
      }
    }
    __syncthreads();

    // ---- QK^T (swapped): S^T[kv][q] in two 32-row tiles ----
    f32x16 s[2];
    #pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      s[rt] = f32x16(0.f);
      const int arow = rt * 32 + lcol;         // K row this lane feeds
      #pragma unroll
      for (int c = 0; c < 8; ++c) {
        short8 kf = *reinterpret_cast<const short8*>(
            reinterpret_cast<char*>(k_lds) + arow * 256 +
            swz(arow, c * 32 + lhalf * 16));
        s[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfrag[c],
                                                        s[rt], 0, 0, 0);
      }
    }
    // ---- online softmax on the lane's 32 scores (one q column) ----
    const int qg = q0 + wid * QBLK + lcol;     // this lane's q row
    const int qpos = ctx + qg;                 // ... and its position
    float p[2][16];
    float tile_max = -FLT_MAX;
    #pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kvr = kv0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
        float sv_ = s[rt][r] * scale;
        if (kvr > qpos || kvr >= kv_end || qg >= n) sv_ = -FLT_MAX;
        p[rt][r] = sv_;
        tile_max = fmaxf(tile_max, sv_);
      }
    }
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32));
    const float m_new = fmaxf(m_run, tile_max);
    const float alpha = (m_run == -FLT_MAX || m_new == -FLT_MAX)
        ? 0.f : __expf(m_run - m_new);
    float lsum = 0.f;
    #pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = (p[rt][r] == -FLT_MAX || m_new == -FLT_MAX)
            ? 0.f : __expf(p[rt][r] - m_new);
        p[rt][r] = e;
        lsum += e;
      }
    }
    lsum += __shfl_xor(lsum, 32);
    l_run = l_run * alpha + lsum;
    m_run = m_new;
    if (lhalf == 0) alpha_lds[wid][lcol] = alpha;
    // ---- P -> per-wave LDS [32 q][64 kv] bf16 (packed pair writes) ----
    #pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      #pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const int kvr = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
        const unsigned lo = f2bf(p[rt][r]);
        const unsigned hi = f2bf(p[rt][r + 1]);
        *reinterpret_cast<unsigned*>(
            reinterpret_cast<char*>(p_lds[wid]) + lcol * (KVBLK * 2) +
            swz(lcol, kvr * 2)) = lo | (hi << 16);
      }
    }
    // ---- rescale O by alpha of each C row (alphas via wave LDS) ----
    #pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow_c = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
        acc[dt][r] *= alpha_lds[wid][qrow_c];
      }
    }
    // ---- PV: O[q][d] += P[q][kv] * V[kv][d] ----
    #pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      #pragma unroll
      for (int c = 0; c < 4; ++c) {
        // A = P: i=q=lcol, k = c*16 + lhalf*8 (+e)
        short8 pf = *reinterpret_cast<const short8*>(
            reinterpret_cast<char*>(p_lds[wid]) + lcol * (KVBLK * 2) +
            swz(lcol, c * 32 + lhalf * 16));
        // B = V: j=d=dt*32+lcol, k = kv chunk -> V^T row j
        const int vrow = dt * 32 + lcol;
        short8 vf = *reinterpret_cast<const short8*>(
            reinterpret_cast<char*>(vt_lds) + vrow * (KVBLK * 2) +
            swz(vrow, c * 32 + lhalf * 16));
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, acc[dt],
                                                          0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: O /= l, store masked rows ----
  // (lsum_lds is wave-private; in-wave LDS ops are program-ordered)
  if (lhalf == 0) lsum_lds[wid][lcol] = l_run;
  #pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow_c = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
      const int qg = q0 + wid * QBLK + qrow_c;
      if (qg >= n) continue;
      const float l = lsum_lds[wid][qrow_c];
      const float o = l > 0.f ? acc[dt][r] / l : 0.f;
      *(unsigned short*)(out + ((t0 + qg) * (long)num_heads + h) * HD +
                         dt * 32 + lcol) = f2bf(o);
    }
  }
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
