// Fused temperature / top-k / top-p sampling straight from the bf16 logits.
//
// One 256-thread workgroup per row; every per-row parameter is read from
// device memory, so the launch depends on the row count alone and the
// kernel can sit at the tail of the captured decode graph.
//
// A bf16 logit has 65536 possible values and all tokens of one value form
// one exact tie group, so both cuts are found by radix selection over an
// order-preserving 16-bit key instead of a sort:
//
//   pass A  max / argmax (+ count histogram on the key's high byte when
//           top-k is on).  A greedy row (temperature == 0) stops here.
//   pass B  top-k: count histogram on the low byte inside the boundary bin
//           -> tau_k, the k-th largest value.  Ties at the cut all stay.
//   pass C  weights w = exp((x - max)/t) of the tokens >= tau_k, summed as
//           2^-40 fixed-point integers (per high byte when top-p is on).
//   pass D  top-p: count histogram on the low byte inside the boundary bin;
//           the mass of a fine bin is count x weight(value) -> tau_p and
//           the kept mass Z'.  A tie group is kept or dropped whole.
//   pass E  walk the row in vocabulary order in 8192-token chunks until the
//           running kept mass exceeds u * Z'.
//
// Every sum is an integer sum (counts, or weights scaled by 2^40), so the
// result does not depend on the order in which atomics land, the prefix
// sums are exact and the draw always ends on a kept token.  The only
// rounding left is the fp32 weight itself.
#include <float.h>
#include <stdint.h>

#include "logit_scan.h"

using namespace logit_scan;   // logit_key, for_each_logit, select_kth, ...

namespace {

constexpr float kFixScale = 1099511627776.0f;   // 2^40

// exp((x - m) / t) in 2^-40 fixed point; -inf / NaN / +inf weigh nothing.
DEV u64 fix_weight(unsigned short b, float m, float inv_t) {
  const float x = bf2f(b);
  if (!(fabsf(x) <= FLT_MAX)) return 0;
  const float w = __expf((x - m) * inv_t);
  return (w == w) ? (u64)(w * kFixScale) : 0;
}

// Thread t offers (cond, mass prefix) for bin 255 - t; the lowest bin whose
// cond holds wins.  *sel = the winner's thread index (-1: none), *val = v.
DEV void select_lowest(bool cond, u64 v, int* sel, u64* val) {
  if (cond) atomicMax(sel, (int)threadIdx.x);
  __syncthreads();
  if ((int)threadIdx.x == *sel) *val = v;
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(256) void sample_fused_kernel(
    long* __restrict__ out, const bf16* __restrict__ logits,
    const float* __restrict__ temperature, const float* __restrict__ top_p,
    const int* __restrict__ top_k, const float* __restrict__ uniform,
    int vocab) {
  __shared__ u64 hist[256 * kCopies];
  __shared__ u64 s_wt[4];
  __shared__ u64 s_val;
  __shared__ float s_max[4];
  __shared__ int s_idx[4];
  __shared__ int s_sel;
  unsigned int* hist32 = reinterpret_cast<unsigned int*>(hist);

  const int tid = threadIdx.x;
  const int copy = tid & (kCopies - 1);
  const unsigned short* row =
      reinterpret_cast<const unsigned short*>(logits) +
      (long)blockIdx.x * vocab;
  const float t_raw = temperature[blockIdx.x];
  const int k = top_k[blockIdx.x];
  const bool k_on = t_raw != 0.f && k > 0 && k < vocab;

  // ---- pass A: argmax (ties to the smaller index), coarse counts ----
  float best = -FLT_MAX;
  int besti = 0;
  if (k_on) {
    zero_hist(hist);
    for_each_logit(row, vocab, [&](int idx, unsigned short b) {
      const float x = bf2f(b);
      if (x > best) { best = x; besti = idx; }
      atomicAdd(&hist32[(logit_key(b) >> 8) * kCopies + copy], 1u);
    });
  } else {
    for_each_logit(row, vocab, [&](int idx, unsigned short b) {
      const float x = bf2f(b);
      if (x > best) { best = x; besti = idx; }
    });
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(besti, o);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if ((tid & 63) == 0) { s_max[tid >> 6] = best; s_idx[tid >> 6] = besti; }
  if (tid == 0) s_sel = -1;
  __syncthreads();
  best = s_max[0];
  besti = s_idx[0];
  #pragma unroll
  for (int w = 1; w < 4; ++w)
    if (s_max[w] > best || (s_max[w] == best && s_idx[w] < besti)) {
      best = s_max[w]; besti = s_idx[w];
    }
  if (t_raw == 0.f) {
    if (tid == 0) out[blockIdx.x] = besti;
    return;
  }
  __syncthreads();          // s_idx is reused by the fallback below

  // ---- pass B: tau_k ----
  unsigned int cut = 0;     // smallest kept key
  if (k_on) {
    select_kth(hist32, (u64)k, 0, s_wt, &s_sel, &s_val);
    const unsigned int bk = (unsigned int)s_sel;
    const u64 above = s_val;
    zero_hist(hist);
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      const unsigned int key = logit_key(b);
      if ((key >> 8) == bk)
        atomicAdd(&hist32[(key & 0xffu) * kCopies + copy], 1u);
    });
    __syncthreads();
    select_kth(hist32, (u64)k, above, s_wt, &s_sel, &s_val);
    cut = (bk << 8) | (unsigned int)s_sel;
    __syncthreads();
    if (tid == 0) s_sel = -1;
  }

  const float m = best;
  const float inv_t = 1.0f / fmaxf(t_raw, 1e-6f);
  const float p = top_p[blockIdx.x];
  u64 z;                    // kept mass, 2^-40 fixed point
  if (p < 1.0f) {
    // ---- pass C: mass per high byte ----
    zero_hist(hist);
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      const unsigned int key = logit_key(b);
      if (key >= cut) {
        const u64 w = fix_weight(b, m, inv_t);
        if (w) atomicAdd(&hist[(key >> 8) * kCopies + copy], w);
      }
    });
    __syncthreads();
    u64 mass = 0;
    #pragma unroll
    for (int r = 0; r < kCopies; ++r) mass += hist[(255 - tid) * kCopies + r];
    u64 incl = block_scan_incl(mass, s_wt, z);
    if (z == 0) {           // nothing finite in the row
      if (tid == 0) out[blockIdx.x] = besti;
      return;
    }
    // a group stays while the mass strictly above it is < p * Z; the
    // group of the maximum (nothing above it) always stays
    const double thr = (double)p * (double)z;
    u64 ex = incl - mass;
    select_lowest(mass > 0 && (ex == 0 || (double)ex < thr), ex, &s_sel,
                  &s_val);
    const unsigned int bp = 255u - (unsigned int)s_sel;
    const u64 above = s_val;
    // ---- pass D: counts per low byte inside the boundary bin ----
    zero_hist(hist);
    if (tid == 0) s_sel = -1;
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      const unsigned int key = logit_key(b);
      if (key >= cut && (key >> 8) == bp)
        atomicAdd(&hist32[(key & 0xffu) * kCopies + copy], 1u);
    });
    __syncthreads();
    const unsigned int fkey = (bp << 8) | (255u - (unsigned int)tid);
    u64 c = 0;
    #pragma unroll
    for (int r = 0; r < kCopies; ++r)
      c += hist32[(255 - tid) * kCopies + r];
    mass = c * fix_weight(key_bits(fkey), m, inv_t);
    u64 tot;
    incl = block_scan_incl(mass, s_wt, tot) + above;
    ex = incl - mass;
    select_lowest(mass > 0 && (ex == 0 || (double)ex < thr), incl, &s_sel,
                  &s_val);
    cut = (bp << 8) | (255u - (unsigned int)s_sel);
    z = s_val;
  } else {
    // ---- pass C: total mass of the tokens >= tau_k ----
    u64 acc = 0;
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      if (logit_key(b) >= cut) acc += fix_weight(b, m, inv_t);
    });
    block_scan_incl(acc, s_wt, z);
    if (z == 0) {
      if (tid == 0) out[blockIdx.x] = besti;
      return;
    }
  }

  // ---- pass E: first kept token whose running mass exceeds u * Z' ----
  const u64 target =
      (u64)((double)fminf(fmaxf(uniform[blockIdx.x], 0.f), 1.f) * (double)z);
  const int a = (int)(((uintptr_t)row >> 1) & 7);
  const uint4* base = reinterpret_cast<const uint4*>(row - a);
  const int end = a + vocab;
  const int nvec = (end + 7) >> 3;
  u64 running = 0;
  int lastk = -1;           // last kept token with weight, for u >= 1
  bool crossed = false;
  // weight of lane i of vector v (0 outside the row or below the cut)
  auto lane_weight = [&](const uint4& q, int v, int i) -> u64 {
    const unsigned int wd = (&q.x)[i >> 1];
    const unsigned short b =
        (unsigned short)(i & 1 ? wd >> 16 : wd & 0xffffu);
    const int j = v * 8 + i;
    if (j < a || j >= end || logit_key(b) < cut) return 0;
    return fix_weight(b, m, inv_t);
  };
  for (int v0 = 0; v0 < nvec; v0 += 256 * kWalkVecs) {
    // a thread owns kWalkVecs consecutive vectors, so thread order is
    // vocabulary order
    const int vb = v0 + tid * kWalkVecs;
    uint4 q[kWalkVecs];
    #pragma unroll
    for (int n = 0; n < kWalkVecs; ++n)
      q[n] = (vb + n < nvec) ? base[vb + n] : make_uint4(0, 0, 0, 0);
    u64 part = 0;
    #pragma unroll
    for (int n = 0; n < kWalkVecs; ++n) {
      if (vb + n < nvec) {
        #pragma unroll
        for (int i = 0; i < 8; ++i) {
          const u64 w = lane_weight(q[n], vb + n, i);
          if (w) lastk = (vb + n) * 8 + i - a;
          part += w;
        }
      }
    }
    u64 total;
    const u64 incl = running + block_scan_incl(part, s_wt, total);
    if (running + total > target) {
      if (incl - part <= target && target < incl) {
        // exact integer sums: the crossing lies in this thread's run
        u64 csum = incl - part;
        int hit = -1;
        #pragma unroll
        for (int n = 0; n < kWalkVecs; ++n) {
          if (vb + n < nvec) {
            #pragma unroll
            for (int i = 0; i < 8; ++i) {
              csum += lane_weight(q[n], vb + n, i);
              if (hit < 0 && csum > target) hit = (vb + n) * 8 + i - a;
            }
          }
        }
        s_sel = hit;
      }
      crossed = true;
      break;
    }
    running += total;
  }
  if (!crossed) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) lastk = max(lastk, __shfl_xor(lastk, o));
    if ((tid & 63) == 0) s_idx[tid >> 6] = lastk;
  }
  __syncthreads();
  if (tid == 0) {
    int tok = s_sel;
    if (!crossed) {
      tok = max(max(s_idx[0], s_idx[1]), max(s_idx[2], s_idx[3]));
      if (tok < 0) tok = besti;
    }
    out[blockIdx.x] = tok;
  }
}

void launch_sample_fused(long* out, const bf16* logits,
                         const float* temperature, const float* top_p,
                         const int* top_k, const float* uniform, long rows,
                         int vocab, hipStream_t stream) {
  if (rows <= 0) return;
  sample_fused_kernel<<<dim3((unsigned)rows), 256, 0, stream>>>(
      out, logits, temperature, top_p, top_k, uniform, vocab);
}
