// Radix-selection helpers over one bf16 logit row, shared by the kernels
// that cut or rank a row without sorting it (sampling_fused.hip,
// logprobs.hip).  All of them assume a 256-thread workgroup per row.
#pragma once

#include <stdint.h>

#include "common.h"

namespace logit_scan {

typedef unsigned long long u64;

// LDS histograms keep kCopies counters per bin, picked by lane, so that the
// few exponent bins a logit row fills do not serialise a whole wave on one
// address.
constexpr int kCopies = 8;
// vectors (of 8 logits) a thread takes per step of a vocabulary-order walk
constexpr int kWalkVecs = 4;

// bf16 bits -> key with key(a) < key(b) <=> a < b; -0 joins +0's group.
DEV unsigned int logit_key(unsigned short b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (unsigned int)(~b & 0xffffu)
                       : (unsigned int)(b | 0x8000u);
}

DEV unsigned short key_bits(unsigned int key) {
  return (key & 0x8000u) ? (unsigned short)(key & 0x7fffu)
                         : (unsigned short)(~key & 0xffffu);
}

// Visit every logit of the row as f(index, bf16 bits), 16 bytes per load.
// A row need not start on a 16-byte boundary (vocab % 8 != 0): loads are
// taken from the aligned address below it, and the lanes of the first and
// last vector that fall outside the row are masked.  An aligned 16-byte
// load that holds one byte of the row cannot leave the row's page.
template <typename F>
DEV void for_each_logit(const unsigned short* row, int vocab, F&& f) {
  const int a = (int)(((uintptr_t)row >> 1) & 7);
  const uint4* base = reinterpret_cast<const uint4*>(row - a);
  const int end = a + vocab;
  const int nvec = (end + 7) >> 3;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const uint4 q = base[v];
    const unsigned int wd[4] = {q.x, q.y, q.z, q.w};
    const int j0 = v * 8;
    if (j0 >= a && j0 + 8 <= end) {
      #pragma unroll
      for (int i = 0; i < 8; ++i)
        f(j0 + i - a, (unsigned short)(i & 1 ? wd[i >> 1] >> 16
                                             : wd[i >> 1] & 0xffffu));
    } else {
      #pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = j0 + i;
        if (j >= a && j < end)
          f(j - a, (unsigned short)(i & 1 ? wd[i >> 1] >> 16
                                          : wd[i >> 1] & 0xffffu));
      }
    }
  }
}

DEV u64 shfl_up_u64(u64 v, int o) {
  const unsigned int lo = __shfl_up((unsigned int)v, o);
  const unsigned int hi = __shfl_up((unsigned int)(v >> 32), o);
  return ((u64)hi << 32) | lo;
}

// Inclusive prefix sum over the 256 threads in thread order; total is the
// block's sum, valid in every thread.  wt holds 4 entries.
DEV u64 block_scan_incl(u64 v, u64* wt, u64& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  #pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 n = shfl_up_u64(v, o);
    if (lane >= o) v += n;
  }
  if (lane == 63) wt[wid] = v;
  __syncthreads();
  u64 off = 0;
  total = 0;
  #pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wid) off += wt[w];
    total += wt[w];
  }
  __syncthreads();
  return v + off;
}

DEV void zero_hist(u64* hist) {
  #pragma unroll
  for (int i = 0; i < kCopies; ++i) hist[threadIdx.x + 256 * i] = 0;
  __syncthreads();
}

// Thread t owns bin 255 - t of a count histogram, so a prefix over threads
// runs from the largest bin down.  Finds the bin that holds the k-th
// largest element, `above` elements lying in higher bins already;
// *sel = that bin, *val = elements strictly above it.
DEV void select_kth(const unsigned int* h, u64 k, u64 above, u64* wt,
                    int* sel, u64* val) {
  const int bin = 255 - threadIdx.x;
  u64 c = 0;
  #pragma unroll
  for (int r = 0; r < kCopies; ++r) c += h[bin * kCopies + r];
  u64 total;
  const u64 incl = block_scan_incl(c, wt, total) + above;
  if ((incl - c < k && k <= incl) || (threadIdx.x == 255 && k > incl)) {
    *sel = bin;
    *val = incl - c;
  }
  __syncthreads();
}

}  // namespace logit_scan
