// Layer-contrastive decoding for generate(dola_layers=): logits fp32 [(k + 1) * b][ld] of ONE forward pass -- rows [0, b) the
// final layer's, row (1 + j) * b + r the head applied to candidate layer j's hidden row of sequence r.  Per sequence r, in fp32:
//   lm = log_softmax(final), lp_j = log_softmax(cand_j)
//   JS_j = 0.5 * mean_v [a (log a - lm) + a (log a - lp_j)],  a = 0.5 (exp lm + exp lp_j), a term with a == 0 contributing 0
//   pick = argmax_j JS_j (the lowest j on equal values; k == 1: that layer, no JS)
//   out[v] = lm[v] < max_v lm + log(relative_top) ? -inf : lm[v] - lp_pick[v]
// -- HF 4.4x's _dola_decoding / _dola_select_contrast / _relative_top_filter, with every row choosing its own layer (HF takes the batch mean
// of JS: the same thing at b = 1).  out goes to the context's copy [b][ld_out]; the picks then run on the copy.
// Three launches: (max, sum exp(x - max)) of every 2048-logit tile of all (k + 1) b rows; the JS sum of every (candidate, row, tile), the two
// log-sum-exps folded from those partials; per (row, tile) the fold of the JS partials, the pick, the filter and the contrast of its own tile.
// k == 1 skips the second.  Every reduction has a fixed order and nothing is accumulated with atomics: the same input bits give the same
// output bits and the same pick, eager or in a captured graph.  The argmax compares the plain sums: the factor 0.5 / V is the same for all j.
// The logits are raw head outputs: finite.  A probability that underflows gives a = 0 or a subnormal a; both count as a == 0 (at most
// 1.2e-38 * |log| per id away from the definition), so no log of 0 and no NaN arises.  tests/dola_ref.py is the float64 restatement.
#include "logits_tile.h"
#include <float.h>

namespace {

__global__ __launch_bounds__(256) void dola_partial_kernel(const float* logits, int ld, int V, int nt, bool vec, float2* part) {
  __shared__ float sh[4];
  const int row = blockIdx.y, tile = blockIdx.x;
  float x[8];
  gd_load(logits + (size_t)row * ld, tile * GD_TILE, V, vec, x);
  float m = x[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) m = fmaxf(m, x[e]);
  m = gd_block_reduce<true>(m, sh);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int e = 0; e < 8; ++e) s += expf(x[e] - m);      // exp(-inf) = 0: the ids at or beyond V
  }
  s = gd_block_reduce<false>(s, sh);
  if (threadIdx.x == 0) part[(size_t)row * nt + tile] = make_float2(m, s);
}

// grid (tile, sequence, candidate): js[(j * b + r) * nt + tile] = sum over the tile of a (log a - lm) + a (log a - lp_j)
__global__ __launch_bounds__(256) void dola_js_kernel(const float* logits, int ld, int b, int V, int nt, bool vec, const float2* part, float* js) {
  __shared__ float sh[4];
  const int tile = blockIdx.x, r = blockIdx.y, j = blockIdx.z;
  const size_t crow = (size_t)(1 + j) * b + r;
  const float lse_f = gd_fold(part + (size_t)r * nt, nt, sh);
  const float lse_c = gd_fold(part + crow * nt, nt, sh);
  float xf[8], xc[8];
  gd_load(logits + (size_t)r * ld, tile * GD_TILE, V, vec, xf);
  gd_load(logits + crow * ld, tile * GD_TILE, V, vec, xc);
  float acc = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float lm = xf[e] - lse_f, lp = xc[e] - lse_c;
    const float a = 0.5f * (expf(lm) + expf(lp));
    const float la = logf(a);
    acc += a >= FLT_MIN ? a * ((la - lm) + (la - lp)) : 0.f;      // (an id at or beyond V has lm = lp = -inf, a = 0: its NaN is never selected)
  }
  acc = gd_block_reduce<false>(acc, sh);
  if (threadIdx.x == 0) js[((size_t)j * b + r) * nt + tile] = acc;
}

// grid (tile, sequence).  picked (or NULL): the candidate's position 0..k-1; rec (or NULL): layers[position] goes to line cnt[r] of the record
// [cap][rec_ld] and cnt[r] moves on (tile 0 only; a full record drops the line, the counter still moves so that a rewind stays in step)
__global__ __launch_bounds__(256) void dola_pick_kernel(const float* logits, int ld, int b, int k, int V, int nt, bool vec, bool vec_out, float log_rt,
                                                        const float2* part, const float* js, float* out, int ld_out, int32_t* picked,
                                                        const int32_t* layers, int32_t* rec, int* cnt, int cap, int rec_ld) {
  __shared__ float sh[4];
  __shared__ float sjs[DOLA_MAX_LAYERS];
  const int tile = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
  int pick = 0;
  if (k > 1) {
    // wave w folds candidates w, w + 4, ..: lane l adds tiles l, l + 64, .. in order, then the xor tree
    for (int j = t >> 6; j < k; j += 4) {
      const float* p = js + ((size_t)j * b + r) * nt;
      float v = 0.f;
      for (int i = t & 63; i < nt; i += 64) v += p[i];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if ((t & 63) == 0) sjs[j] = v;
    }
    __syncthreads();
    float best = sjs[0];
    for (int j = 1; j < k; ++j)
      if (sjs[j] > best) { best = sjs[j]; pick = j; }      // strict: the lowest position wins on equal values
  }
  const size_t crow = (size_t)(1 + pick) * b + r;
  float mx;
  const float lse_f = gd_fold(part + (size_t)r * nt, nt, sh, &mx);
  const float lse_c = gd_fold(part + crow * nt, nt, sh);
  const float thresh = (mx - lse_f) + log_rt;
  float xf[8], xc[8];
  gd_load(logits + (size_t)r * ld, tile * GD_TILE, V, vec, xf);
  gd_load(logits + crow * ld, tile * GD_TILE, V, vec, xc);
  float* o = out + (size_t)r * ld_out;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = tile * GD_TILE + (e * 256 + t) * 4;
    float y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float lm = xf[e * 4 + q] - lse_f, lp = xc[e * 4 + q] - lse_c;
      y[q] = lm < thresh ? -INFINITY : lm - lp;
    }
    if (vec_out && i + 4 <= V) {
      *(float4*)(o + i) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i + q < V) o[i + q] = y[q];
    }
  }
  if (tile == 0 && t == 0) {
    if (picked) picked[r] = pick;
    if (rec) {
      const int n = cnt[r];
      if (n >= 0 && n < cap) rec[(size_t)n * rec_ld + r] = layers[pick];
      cnt[r] = n + 1;
    }
  }
}

}  // namespace

static size_t dola_part_bytes(int b, int k, int V) { return (size_t)(k + 1) * b * cdiv(V, GD_TILE) * sizeof(float2); }

size_t dola_ws_bytes(int b, int k, int V) { return dola_part_bytes(b, k, V) + (size_t)k * b * cdiv(V, GD_TILE) * sizeof(float); }

int launch_dola(const DolaArgs& a, hipStream_t s) {
  OM_CHECK(a.logits && a.ws && a.out && a.b >= 1 && a.k >= 1 && a.k <= DOLA_MAX_LAYERS && a.V >= 1 && a.ld >= a.V && a.ld_out >= a.V,
           "launch_dola: bad argument");
  OM_CHECK((int64_t)(a.k + 1) * a.b <= 65535, "dola: (k + 1) * b rows exceed the grid");
  OM_CHECK(a.relative_top > 0.f && a.relative_top <= 1.f, "dola: relative_top must lie in (0, 1]");
  OM_CHECK(((uintptr_t)a.ws & 7) == 0 && a.ws_bytes >= dola_ws_bytes(a.b, a.k, a.V), "dola: the workspace must be 8-byte aligned and hold dola_ws_bytes");
  OM_CHECK(!a.rec || (a.layers && a.cnt && a.cap >= 1 && a.rec_ld >= a.b), "dola: a record needs the layer list, the counters and its geometry");
  const int nt = cdiv(a.V, GD_TILE);
  const bool vec = a.ld % 4 == 0 && ((uintptr_t)a.logits & 15) == 0;
  const bool vec_out = a.ld_out % 4 == 0 && ((uintptr_t)a.out & 15) == 0;
  float2* part = (float2*)a.ws;
  float* js = (float*)((char*)a.ws + dola_part_bytes(a.b, a.k, a.V));
  hipLaunchKernelGGL(dola_partial_kernel, dim3(nt, (a.k + 1) * a.b), dim3(256), 0, s, a.logits, a.ld, a.V, nt, vec, part);
  if (a.k > 1) hipLaunchKernelGGL(dola_js_kernel, dim3(nt, a.b, a.k), dim3(256), 0, s, a.logits, a.ld, a.b, a.V, nt, vec, (const float2*)part, js);
  hipLaunchKernelGGL(dola_pick_kernel, dim3(nt, a.b), dim3(256), 0, s, a.logits, a.ld, a.b, a.k, a.V, nt, vec, vec_out, logf(a.relative_top),
                     (const float2*)part, (const float*)js, a.out, a.ld_out, a.picked, a.layers, a.rec, a.cnt, a.cap, a.rec_ld);
  OM_LAUNCH_CHECK();
  return 0;
}
