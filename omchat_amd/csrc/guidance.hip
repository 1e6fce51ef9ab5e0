// Classifier-free guidance for generate(guidance_scale=): logits fp32 [2b][ld], rows [0, b) conditional and rows
// [b, 2b) their twins over the negative prompt.  out[r] = scale * (lc - lu) + lu with lc = log_softmax(logits[r]), lu = log_softmax(logits[b + r])
// -- HF's UnbatchedClassifierFreeGuidanceLogitsProcessor -- written to the context's copy [b][ld_out]; the picks then run on the copy.
// Two launches: the partial pass leaves (max, sum exp(x - max)) of every 2048-logit tile of all 2b rows in a workspace; in the mix pass every
// workgroup folds the partials of its row and of the twin to the two log-sum-exps and combines its own tile, which it reads from L2.
// Every reduction has a fixed order and nothing is accumulated with atomics: the same input bits give the same output bits, eager or in a
// captured graph.
// The -inf rule (HF's formula gives NaN there): where the conditional or the twin logit is -inf the output is -inf -- an id that one of the two
// contexts excludes stays excluded.  -inf entries add nothing to a row's sum, and a row of nothing but -inf gives nothing but -inf.
// tests/guidance_ref.py is the float64 restatement, pinned to HF's processor.
#include "logits_tile.h"

namespace {

__global__ __launch_bounds__(256) void guidance_partial_kernel(const float* logits, int ld, int V, int nt, bool vec, float2* ws) {
  __shared__ float sh[4];
  const int row = blockIdx.y, tile = blockIdx.x;
  float x[8];
  gd_load(logits + (size_t)row * ld, tile * GD_TILE, V, vec, x);
  float m = x[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) m = fmaxf(m, x[k]);
  m = gd_block_reduce<true>(m, sh);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s += expf(x[k] - m);      // exp(-inf) = 0
  }
  s = gd_block_reduce<false>(s, sh);
  if (threadIdx.x == 0) ws[(size_t)row * nt + tile] = make_float2(m, s);
}

__device__ __forceinline__ float gd_mix(float xc, float xu, float lse_c, float lse_u, float scale) {
  if (xc == -INFINITY || xu == -INFINITY) return -INFINITY;
  const float lc = xc - lse_c, lu = xu - lse_u;
  return scale * (lc - lu) + lu;
}

__global__ __launch_bounds__(256) void guidance_mix_kernel(const float* logits, int ld, int b, int V, int nt, bool vec, bool vec_out, float scale,
                                                           const float2* ws, float* out, int ld_out) {
  __shared__ float sh[4];
  const int row = blockIdx.y, t0 = blockIdx.x * GD_TILE;
  const float lse_c = gd_fold(ws + (size_t)row * nt, nt, sh);
  const float lse_u = gd_fold(ws + (size_t)(b + row) * nt, nt, sh);
  float xc[8], xu[8];
  gd_load(logits + (size_t)row * ld, t0, V, vec, xc);
  gd_load(logits + (size_t)(b + row) * ld, t0, V, vec, xu);
  float* o = out + (size_t)row * ld_out;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = t0 + (e * 256 + (int)threadIdx.x) * 4;
    float y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = gd_mix(xc[e * 4 + k], xu[e * 4 + k], lse_c, lse_u, scale);
    if (vec_out && i + 4 <= V) {
      *(float4*)(o + i) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < V) o[i + k] = y[k];
    }
  }
}

// behind the pick of the b conditional rows: the twins are fed their row's id; with pos / len the decode positions of all 2b rows move
__global__ void guidance_twin_kernel(int32_t* next, int b, int* pos, int* len) {
  const int i = threadIdx.x;
  if (i < b) next[b + i] = next[i];
  if (pos && i < 2 * b) { pos[i] += 1; len[i] += 1; }
}

}  // namespace

size_t guidance_ws_bytes(int b, int V) { return (size_t)2 * b * cdiv(V, GD_TILE) * sizeof(float2); }

int launch_guidance(const float* logits, int ld, int b, int V, float scale, void* ws, float* out, int ld_out, hipStream_t s) {
  OM_CHECK(logits && ws && out && b >= 1 && V >= 1 && ld >= V && ld_out >= V, "launch_guidance: bad argument");
  OM_CHECK(isfinite(scale), "guidance: the scale must be finite");
  OM_CHECK(((uintptr_t)ws & 7) == 0, "guidance: the workspace must be 8-byte aligned");
  const int nt = cdiv(V, GD_TILE);
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const bool vec_out = ld_out % 4 == 0 && ((uintptr_t)out & 15) == 0;
  hipLaunchKernelGGL(guidance_partial_kernel, dim3(nt, 2 * b), dim3(256), 0, s, logits, ld, V, nt, vec, (float2*)ws);
  hipLaunchKernelGGL(guidance_mix_kernel, dim3(nt, b), dim3(256), 0, s, logits, ld, b, V, nt, vec, vec_out, scale, (const float2*)ws, out, ld_out);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_guidance_twin(int32_t* next_tokens, int b, int* pos, int* len, hipStream_t s) {
  OM_CHECK(next_tokens && b >= 1 && 2 * b <= 1024 && (pos == nullptr) == (len == nullptr), "launch_guidance_twin: bad argument");
  hipLaunchKernelGGL(guidance_twin_kernel, dim3(1), dim3(64 > 2 * b ? 64 : 2 * b), 0, s, next_tokens, b, pos, len);
  OM_LAUNCH_CHECK();
  return 0;
}
