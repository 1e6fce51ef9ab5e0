// The 2048-logit tile of the log-softmax stages over fp32 logits [rows][ld] (guidance.hip, dola.hip): the block reduction with its fixed tree, the
// thread's eight logits of a tile, and the fold of a row's (max, sum exp(x - max)) tile partials to its log-sum-exp.  Every order is fixed: the
// same input bits give the same output bits, eager or in a captured graph.  Device code of 256-thread workgroups.
#pragma once
#include "kernels.h"
#include <math.h>

constexpr int GD_TILE = 2048;      // logits per workgroup: 256 threads x two 16-byte pieces

// all 256 threads get the same value; a fixed tree (xor shuffles inside a wave, then the four waves in order)
template <bool MAX>
__device__ inline float gd_block_reduce(float v, float* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();      // (sh may still be read from the reduction before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) : ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}

// the thread's eight logits of its tile: pieces e = 0, 1 at i = t0 + (e * 256 + t) * 4; ids at or beyond V read as -inf
__device__ inline void gd_load(const float* row, int t0, int V, bool vec, float x[8]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = t0 + (e * 256 + (int)threadIdx.x) * 4;
    if (vec && i + 4 <= V) {
      const float4 q = *(const float4*)(row + i);
      x[e * 4] = q.x; x[e * 4 + 1] = q.y; x[e * 4 + 2] = q.z; x[e * 4 + 3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[e * 4 + k] = i + k < V ? row[i + k] : -INFINITY;
    }
  }
}

// log-sum-exp of a row from its nt tile partials (-inf for a row of nothing but -inf); row_max: the row's largest logit as well
__device__ inline float gd_fold(const float2* p, int nt, float* sh, float* row_max = nullptr) {
  const int t = threadIdx.x;
  float m = -INFINITY;
  for (int i = t; i < nt; i += 256) m = fmaxf(m, p[i].x);
  m = gd_block_reduce<true>(m, sh);
  if (row_max) *row_max = m;
  float s = 0.f;
  if (m > -INFINITY)
    for (int i = t; i < nt; i += 256) s += p[i].y * expf(p[i].x - m);
  s = gd_block_reduce<false>(s, sh);
  return m > -INFINITY ? m + logf(s) : -INFINITY;
}
