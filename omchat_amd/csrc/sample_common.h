// The processed value of one logit as the sampler (sample.hip) and the log-probability stage (logprob.hip) both evaluate it, in fp32 as HF
// computes it: RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, and the order-preserving key the kept set is compared in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t smp_key(float f) {
  uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);     // -0 and +0 are one key (HF compares values)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// RepetitionPenaltyLogitsProcessor (seen: < 0 -> * p, else / p), then TemperatureLogitsWarper (/ T), in fp32 as HF computes them
__device__ __forceinline__ float smp_penalise(float l, float pen) { return l < 0.f ? __fmul_rn(l, pen) : __fdiv_rn(l, pen); }
__device__ __forceinline__ float smp_penalised(const float* row, const uint32_t* seen, int i, float pen) {
  float l = row[i];
  if (seen && ((seen[i >> 5] >> (i & 31)) & 1u)) l = smp_penalise(l, pen);
  return l;
}
// typical_p's distance of a processed logit from the entropy, |-log p - H| with -log p = L - x (L = max + log Z), in fp32 as HF computes it
__device__ __forceinline__ float smp_typ_dist(float x, float L, float H) { return fabsf(__fsub_rn(__fsub_rn(L, x), H)); }
