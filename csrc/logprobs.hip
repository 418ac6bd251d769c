// Per-token log-probabilities straight from the bf16 logits: the chosen
// token's logprob and the n most likely alternatives of each row.
//
// One 256-thread workgroup per row; every per-row parameter (chosen token,
// n) is read from device memory, so the launch depends on the row count and
// the vocabulary alone and the kernel can sit behind the sampler at the tail
// of the captured decode graph.  A row with n < 0 did not ask: its workgroup
// returns before touching the logits and leaves its outputs alone.
//
// The distribution is the row as handed in (temperature 1, before top-k and
// top-p): lp(x) = x - (m + log(sum exp(x - m))).  Non-finite logits weigh
// nothing, rank below every finite one (among themselves by id) and are
// reported as -inf.
//
//   pass 1  maximum; count histogram on the rank key's high byte (n > 0).
//   pass 2  sum exp(x - m) in fp32; count histogram on the low byte inside
//           the boundary bin -> tau, the n-th largest value, and the count
//           strictly above it (< n).
//   pass 3  (n > 0) walk the row in vocabulary order in 8192-token chunks:
//           tokens above tau are collected as they come, and a block scan
//           over the == tau counts hands the first n - above ids of the tie
//           group their places.  One thread orders the <= 20 candidates.
//
// The normaliser uses no floating-point atomics: a thread adds its logits in
// the fixed order of for_each_logit_ordered (token order, whatever the
// row's alignment), the block reduces in a fixed tree, so a row's result is
// bit-identical from run to run and does not depend on which other rows are
// in the launch, nor on where in it the row sits.  Counts are integers, so
// the selection is exact and ties resolve to ascending token id.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "logit_scan.h"

using namespace logit_scan;

namespace {

constexpr int kMaxTop = 20;
constexpr int kCols = kMaxTop + 1;   // chosen token + alternatives

// logit_key for a finite logit (never 0: key 0 is a NaN's bit pattern);
// 0 for -inf / +inf / NaN, which so form one group below every finite value.
DEV unsigned int rank_key(unsigned short b) {
  return ((b & 0x7f80u) == 0x7f80u) ? 0u : logit_key(b);
}

// for_each_logit in the row's own frame: thread t visits tokens 8w..8w+7 of
// the vectors w = t, t + 256, ... in token order wherever the row starts,
// so a per-thread floating-point accumulation does not depend on the row's
// alignment (row r of a batch and the same row launched alone add in the
// same order).  A row off the 16-byte grid takes its eight tokens from two
// aligned loads, shifted down by the misalignment; the second load is
// issued only where that vector still holds a byte of the row.
template <typename F>
DEV void for_each_logit_ordered(const unsigned short* row, int vocab, F&& f) {
  const int a = (int)(((uintptr_t)row >> 1) & 7);
  const uint4* base = reinterpret_cast<const uint4*>(row - a);
  const int nvec = (a + vocab + 7) >> 3;     // aligned vectors of the row
  const int nw = (vocab + 7) >> 3;           // vectors in the row's frame
  for (int w = threadIdx.x; w < nw; w += 256) {
    const uint4 lo = base[w];                // holds token 8w
    unsigned int wd[8] = {lo.x, lo.y, lo.z, lo.w, 0, 0, 0, 0};
    if (a) {
      if (w + 1 < nvec) {
        const uint4 hi = base[w + 1];
        wd[4] = hi.x; wd[5] = hi.y; wd[6] = hi.z; wd[7] = hi.w;
      }
      if (a & 4) {
        #pragma unroll
        for (int k = 0; k < 6; ++k) wd[k] = wd[k + 2];
      }
      if (a & 2) {
        #pragma unroll
        for (int k = 0; k < 5; ++k) wd[k] = wd[k + 1];
      }
      if (a & 1) {
        #pragma unroll
        for (int k = 0; k < 4; ++k) wd[k] = (wd[k] >> 16) | (wd[k + 1] << 16);
      }
    }
    const int j0 = w * 8;
    #pragma unroll
    for (int i = 0; i < 8; ++i)
      if (j0 + i < vocab)
        f(j0 + i, (unsigned short)(i & 1 ? wd[i >> 1] >> 16
                                         : wd[i >> 1] & 0xffffu));
  }
}

}  // namespace

__global__ __launch_bounds__(256) void token_logprobs_kernel(
    float* __restrict__ out_val, int* __restrict__ out_id,
    const bf16* __restrict__ logits, const long* __restrict__ chosen,
    const int* __restrict__ n_top, int vocab) {
  __shared__ u64 hist[256 * kCopies];
  __shared__ u64 s_wt[4];
  __shared__ u64 s_val;
  __shared__ float s_red[4];
  __shared__ unsigned int s_mk[4];
  __shared__ int s_sel;
  __shared__ int s_ngt;
  __shared__ unsigned int c_key[kMaxTop];
  __shared__ int c_id[kMaxTop];
  unsigned int* hist32 = reinterpret_cast<unsigned int*>(hist);

  int n = n_top[blockIdx.x];
  if (n < 0) return;
  n = min(min(n, kMaxTop), vocab);

  const int tid = threadIdx.x;
  const int copy = tid & (kCopies - 1);
  const unsigned short* row =
      reinterpret_cast<const unsigned short*>(logits) +
      (long)blockIdx.x * vocab;

  // ---- pass 1: largest finite value, coarse counts ----
  unsigned int mk = 0;
  if (n > 0) {
    zero_hist(hist);
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      const unsigned int key = rank_key(b);
      mk = max(mk, key);
      atomicAdd(&hist32[(key >> 8) * kCopies + copy], 1u);
    });
  } else {
    for_each_logit(row, vocab, [&](int, unsigned short b) {
      mk = max(mk, rank_key(b));
    });
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    mk = max(mk, (unsigned int)__shfl_xor((int)mk, o));
  if ((tid & 63) == 0) s_mk[tid >> 6] = mk;
  if (tid == 0) s_ngt = 0;
  __syncthreads();
  mk = max(max(s_mk[0], s_mk[1]), max(s_mk[2], s_mk[3]));
  const bool any = mk != 0;                  // the row has a finite logit
  const float m = any ? bf2f(key_bits(mk)) : 0.f;

  unsigned int bk = 0;      // high byte of tau's key
  u64 above = 0;
  if (n > 0) {
    select_kth(hist32, (u64)n, 0, s_wt, &s_sel, &s_val);
    bk = (unsigned int)s_sel;
    above = s_val;
    zero_hist(hist);
  }

  // ---- pass 2: normaliser, fine counts inside the boundary bin ----
  float acc = 0.f;
  if (n > 0) {
    for_each_logit_ordered(row, vocab, [&](int, unsigned short b) {
      const unsigned int key = rank_key(b);
      if (key) acc += __expf(bf2f(b) - m);
      if ((key >> 8) == bk)
        atomicAdd(&hist32[(key & 0xffu) * kCopies + copy], 1u);
    });
  } else {
    for_each_logit_ordered(row, vocab, [&](int, unsigned short b) {
      if (rank_key(b)) acc += __expf(bf2f(b) - m);
    });
  }
  const float sum = block_reduce_sum_256(acc, s_red);
  const float lse = m + logf(sum);
  // logprob of a rank key; -inf for the non-finite group
  auto key_lp = [&](unsigned int key) -> float {
    return key ? bf2f(key_bits(key)) - lse : -INFINITY;
  };

  // ---- pass 3: the tokens above tau, and tau's first ids ----
  if (n > 0) {
    select_kth(hist32, (u64)n, above, s_wt, &s_sel, &s_val);
    const unsigned int tau = (bk << 8) | (unsigned int)s_sel;
    const int gt = (int)s_val;               // tokens strictly above tau
    const u64 need = (u64)(n - gt);          // places left for tau's group
    const int a = (int)(((uintptr_t)row >> 1) & 7);
    const uint4* base = reinterpret_cast<const uint4*>(row - a);
    const int end = a + vocab;
    const int nvec = (end + 7) >> 3;
    // rank key of lane i of vector v, ~0 outside the row
    auto lane_key = [&](const uint4& q, int v, int i) -> unsigned int {
      const unsigned int wd = (&q.x)[i >> 1];
      const int j = v * 8 + i;
      if (j < a || j >= end) return ~0u;
      return rank_key((unsigned short)(i & 1 ? wd >> 16 : wd & 0xffffu));
    };
    u64 running = 0;        // tau tokens in the chunks before this one
    for (int v0 = 0; v0 < nvec; v0 += 256 * kWalkVecs) {
      // a thread owns kWalkVecs consecutive vectors, so thread order is
      // vocabulary order
      const int vb = v0 + tid * kWalkVecs;
      uint4 q[kWalkVecs];
      #pragma unroll
      for (int w = 0; w < kWalkVecs; ++w)
        q[w] = (vb + w < nvec) ? base[vb + w] : make_uint4(0, 0, 0, 0);
      u64 part = 0;
      #pragma unroll
      for (int w = 0; w < kWalkVecs; ++w) {
        if (vb + w < nvec) {
          #pragma unroll
          for (int i = 0; i < 8; ++i) {
            const unsigned int key = lane_key(q[w], vb + w, i);
            if (key == ~0u) continue;
            if (key > tau) {
              const int slot = atomicAdd(&s_ngt, 1);
              if (slot < kMaxTop) {
                c_key[slot] = key;
                c_id[slot] = (vb + w) * 8 + i - a;
              }
            } else if (key == tau) {
              ++part;
            }
          }
        }
      }
      u64 total;
      const u64 incl = running + block_scan_incl(part, s_wt, total);
      u64 pos = incl - part;                 // tau tokens before this run
      if (part && pos < need) {
        #pragma unroll
        for (int w = 0; w < kWalkVecs; ++w) {
          if (vb + w < nvec) {
            #pragma unroll
            for (int i = 0; i < 8; ++i) {
              if (lane_key(q[w], vb + w, i) == tau) {
                if (pos < need) {
                  c_key[gt + (int)pos] = tau;
                  c_id[gt + (int)pos] = (vb + w) * 8 + i - a;
                }
                ++pos;
              }
            }
          }
        }
      }
      running += total;
    }
    __syncthreads();
  }

  if (tid == 0) {
    float* val = out_val + (long)blockIdx.x * kCols;
    int* id = out_id + (long)blockIdx.x * kCols;
    const long c = chosen[blockIdx.x];
    id[0] = (int)c;
    val[0] = (c >= 0 && c < vocab) ? key_lp(rank_key(row[c])) : -INFINITY;
    // order the candidates by (value descending, id ascending)
    for (int i = 1; i < n; ++i) {
      const unsigned int k = c_key[i];
      const int t = c_id[i];
      int j = i - 1;
      while (j >= 0 && (c_key[j] < k || (c_key[j] == k && c_id[j] > t))) {
        c_key[j + 1] = c_key[j];
        c_id[j + 1] = c_id[j];
        --j;
      }
      c_key[j + 1] = k;
      c_id[j + 1] = t;
    }
    for (int i = 0; i < kMaxTop; ++i) {
      id[1 + i] = i < n ? c_id[i] : -1;
      val[1 + i] = i < n ? key_lp(c_key[i]) : -INFINITY;
    }
  }
}

void launch_token_logprobs(float* out_val, int* out_id, const bf16* logits,
                           const long* chosen, const int* n_top, long rows,
                           int vocab, hipStream_t stream) {
  if (rows <= 0) return;
  token_logprobs_kernel<<<dim3((unsigned)rows), 256, 0, stream>>>(
      out_val, out_id, logits, chosen, n_top, vocab);
}
