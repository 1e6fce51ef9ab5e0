// On-device sampling for generate(do_sample=True): repetition penalty, temperature, top-k, top-p and the categorical draw, in the order of
// HF's sampling path.  No sort: the top-k / top-p thresholds are found by a radix select over the order-preserving
// uint32 key of each processed fp32 logit (11 / 11 / 10 bits), the draw is an exponential race (Gumbel-max) whose noise is a counter-based
// hash of (seed, row, step, GLOBAL vocabulary index).  Every quantity that crosses workgroups or ranks is an integer (token counts, fixed-point
// probability mass, max keys), so the kept set -- and with the global-index noise the picked id -- is the same at every TP degree and in
// every launch order.  tests/sampling_ref.py is the CPU restatement, bit for bit.
// Behind top-p: HF's MinP, Typical, Epsilon and Eta warpers (SampleFilters).  Each is a threshold on the processed logit, found from the
// fixed-point normaliser Z and entropy sum of the current kept set; typical_p is a second radix select, ascending over |-log p - H|, whose
// cut maps back to a key INTERVAL [lo, hi] of the logits.  tests/sampling_ref2.py restates the interval form.
#include "kernels.h"
#include "sample_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SMP_BINS = 2048;         // 11-bit digits (the last round uses 1024 of them)
constexpr int SMP_XS = 3 * SMP_BINS;   // exchange row under TP: every bin as three 21-bit limbs in fp32
constexpr int SMP_HIST_CH = 16;        // workgroups per row of the histogram / max passes
constexpr int SMP_RACE_CH = 64;        // workgroups per row of the race (= the 64 lanes of the final wave)
constexpr int SMP_ST = 8;              // int64 state words per row
// state words
// (ST_TK: the top-k threshold while top-p runs, later the typical cut; ST_AUX: typical's fp32 log-normaliser | entropy << 32)
enum { ST_PREFIX = 0, ST_CUM = 1, ST_TK = 2, ST_MKEY = 3, ST_TARGET = 4, ST_THR = 5, ST_HI = 6, ST_AUX = 7 };
// stages of smp_filter_kernel
enum { FL_MINP = 0, FL_TYP = 1, FL_BOUNDS = 2, FL_EPS = 3, FL_ETA = 4 };
constexpr double SMP_FIX = 4294967296.0;    // probability mass in units of 2^-32 of the max token's weight

__device__ __forceinline__ uint64_t smp_mix(uint64_t x) {      // splitmix64, as elementwise.hip's fill_uniform_kernel
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t smp_row_key(uint64_t seed, int row, int step) {
  return smp_mix(seed ^ smp_mix(((uint64_t)(uint32_t)row << 32) | (uint32_t)step));
}
// Gumbel noise -log(E), E = -log(U) ~ Exp(1), U in (0, 1) from 52 hash bits; evaluated in fp64 and rounded once to fp32
__device__ __forceinline__ float smp_noise(uint64_t rk, uint32_t gi) {
  const uint64_t h = smp_mix(rk + (uint64_t)gi * 0x9E3779B97F4A7C15ull);
  const double u = ((double)(h >> 12) + 0.5) * 0x1p-52;
  return (float)(-log(-log(u)));
}
__device__ __forceinline__ void smp_better(float& best, int& besti, float v, int i) {
  if (v > best || (v == best && i < besti)) { best = v; besti = i; }
}
__device__ __forceinline__ int smp_shift(int round) { return round == 0 ? 21 : round == 1 ? 10 : 0; }

// local max key of the processed logits (top-p needs the max for its softmax): one u64 atomicMax per workgroup into bin 0 of the row
__global__ __launch_bounds__(256) void smp_max_kernel(const float* logits, int ld, int V, const uint32_t* seen, int bmw, float pen, float T,
                                                      uint64_t* hist) {
  const int row = blockIdx.y;
  const float* lg = logits + (size_t)row * ld;
  const uint32_t* sn = seen ? seen + (size_t)row * bmw : nullptr;
  const int per = (V + SMP_HIST_CH - 1) / SMP_HIST_CH;
  const int lo = blockIdx.x * per, hi = min(lo + per, V);
  uint32_t m = 0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) m = max(m, smp_key(__fdiv_rn(smp_penalised(lg, sn, i, pen), T)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  __shared__ uint32_t wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
    atomicMax((unsigned long long*)&hist[(size_t)row * SMP_BINS], (unsigned long long)m);
  }
}

// one radix round: MASS = 0 counts the tokens per digit, MASS = 1 sums their fixed-point weight exp(x - m) * 2^32 over keys >= the top-k
// threshold.  Only keys whose higher digits equal the prefix found so far take part.  Integer LDS atomics, then one global atomic per digit.
// MASS = 2 (typical_p): the same mass, binned by the COMPLEMENT of the key of d = |(L - x) - H| (fp32; L = max + log Z, H = entropy, both left
// in ST_AUX), so that the select's walk from the top digit runs over d ascending; keys >= ST_THR take part (no upper bound exists yet).
template <int MASS>
__global__ __launch_bounds__(256) void smp_hist_kernel(const float* logits, int ld, int V, const uint32_t* seen, int bmw, float pen, float T,
                                                       const int64_t* st, uint64_t* hist, int round) {
  __shared__ unsigned long long bins[SMP_BINS];
  const int row = blockIdx.y;
  for (int j = threadIdx.x; j < SMP_BINS; j += 256) bins[j] = 0;
  __syncthreads();
  const float* lg = logits + (size_t)row * ld;
  const uint32_t* sn = seen ? seen + (size_t)row * bmw : nullptr;
  const int64_t* s = st + (size_t)row * SMP_ST;
  const uint32_t prefix = (uint32_t)s[ST_PREFIX];
  const int shift = smp_shift(round), hs = round == 1 ? 21 : 10;
  const uint32_t lo_key = MASS == 2 ? (uint32_t)s[ST_THR] : MASS ? (uint32_t)s[ST_TK] : 0u;
  const float tL = MASS == 2 ? __uint_as_float((uint32_t)s[ST_AUX]) : 0.f, tH = MASS == 2 ? __uint_as_float((uint32_t)((uint64_t)s[ST_AUX] >> 32)) : 0.f;
  const double m = MASS ? (double)smp_unkey((uint32_t)s[ST_MKEY]) : 0.0;
  const int per = (V + SMP_HIST_CH - 1) / SMP_HIST_CH;
  const int lo = blockIdx.x * per, hi = min(lo + per, V);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float x = __fdiv_rn(smp_penalised(lg, sn, i, pen), T);
    uint32_t k = smp_key(x);
    if (k < lo_key) continue;
    if (MASS == 2) k = ~smp_key(smp_typ_dist(x, tL, tH));
    if (round > 0 && (k >> hs) != (prefix >> hs)) continue;
    const int bin = (k >> shift) & (round == 2 ? 1023u : 2047u);
    const unsigned long long w = MASS ? (unsigned long long)llrint(exp((double)x - m) * SMP_FIX) : 1ull;
    if (w) atomicAdd(&bins[bin], w);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < SMP_BINS; j += 256)
    if (bins[j]) atomicAdd((unsigned long long*)&hist[(size_t)row * SMP_BINS + j], bins[j]);
}

// tensor parallelism: the row's integer bins -> three exact fp32 limbs each (the all-reduce sums at most 8 ranks: < 2^24 per limb); the max
// stage puts this rank's key as two 16-bit limbs into its own slot and zeros in the others'
__global__ __launch_bounds__(256) void smp_to_limbs_kernel(const uint64_t* hist, float* xb, int max_stage, int rank) {
  const int row = blockIdx.x;
  const uint64_t* h = hist + (size_t)row * SMP_BINS;
  float* x = xb + (size_t)row * SMP_XS;
  if (max_stage) {
    for (int j = threadIdx.x; j < 32; j += 256) {      // bin 0 in [0, 16), bin 1 (the typical bounds pass) in [16, 32)
      const uint32_t k = (uint32_t)h[j >> 4];
      const int jj = j & 15;
      x[j] = jj == 2 * rank ? (float)(k & 0xFFFFu) : jj == 2 * rank + 1 ? (float)(k >> 16) : 0.f;
    }
    return;
  }
  for (int j = threadIdx.x; j < SMP_BINS; j += 256) {
    const uint64_t v = h[j];
    x[3 * j] = (float)(v & 0x1FFFFFull);
    x[3 * j + 1] = (float)((v >> 21) & 0x1FFFFFull);
    x[3 * j + 2] = (float)(v >> 42);
  }
}

// Close a round (one workgroup per row): read the row's bins (summed over the ranks), find the digit at which the running total from the top
// reaches the target -- k tokens, or top_p of the kept mass -- and fix it in the prefix; the mass strictly above it carries to the next round.
// stage: 0 = max, 1 = count round, 2 = mass round, 3 = typical mass round (top_p = typical_p; the cut's complemented key lands in ST_TK).
// Zeroes the row's bins for the next pass.
__global__ __launch_bounds__(256) void smp_select_kernel(uint64_t* hist, const float* xb, int tp, int64_t* st, int stage, int round, int top_k,
                                                         double top_p, int p_follows) {
  const int row = blockIdx.x, t = threadIdx.x;
  uint64_t* h = hist + (size_t)row * SMP_BINS;
  const float* x = xb ? xb + (size_t)row * SMP_XS : nullptr;
  int64_t* s = st + (size_t)row * SMP_ST;
  if (stage == 0) {
    __syncthreads();
    if (t == 0) {
      uint32_t m = 0;
      if (x) {
        for (int r = 0; r < tp; ++r) m = max(m, (uint32_t)x[2 * r] | ((uint32_t)x[2 * r + 1] << 16));
      } else {
        m = (uint32_t)h[0];
      }
      s[ST_MKEY] = m;
      h[0] = 0;
    }
    return;
  }
  __shared__ unsigned long long tot[256];
  __shared__ int pick;
  __shared__ unsigned long long above;
  constexpr int PER = SMP_BINS / 256;
  unsigned long long v[PER];
  unsigned long long mine = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int j = t * PER + e;
    v[e] = x ? (unsigned long long)x[3 * j] + ((unsigned long long)x[3 * j + 1] << 21) + ((unsigned long long)x[3 * j + 2] << 42) : h[j];
    h[j] = 0;
    mine += v[e];
  }
  tot[t] = mine;
  if (t == 0) { pick = -1; above = 0; }
  __syncthreads();
  // inclusive suffix sums over the thread totals (digit order = thread order): tot[t] = sum of threads >= t
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long add = t + o < 256 ? tot[t + o] : 0ull;
    __syncthreads();
    tot[t] += add;
    __syncthreads();
  }
  const unsigned long long cum = (unsigned long long)s[ST_CUM];
  double target;
  if (stage == 1) {
    target = (double)top_k;
  } else if (round == 0) {
    target = top_p * (double)tot[0];          // Z = the whole kept mass (keys >= the top-k threshold); P = top_p * Z
  } else {
    target = __longlong_as_double(s[ST_TARGET]);
  }
  // the largest digit j with cum + (mass of digits >= j) >= target; digits run upwards inside a thread's PER
  unsigned long long run = (t + 1 < 256 ? tot[t + 1] : 0ull);     // everything above this thread's digits
  int found = -1;
  unsigned long long found_above = 0;
#pragma unroll
  for (int e = PER - 1; e >= 0; --e) {
    const unsigned long long incl = run + v[e];
    if (found < 0 && (double)(cum + incl) >= target) { found = t * PER + e; found_above = run; }
    run = incl;
  }
  __syncthreads();
  if (found >= 0) atomicMax(&pick, found);
  __syncthreads();
  if (found >= 0 && found == pick) above = found_above;
  __syncthreads();
  if (t == 0) {
    const int j = pick < 0 ? 0 : pick;                 // (a target beyond the total cannot occur for valid parameters: keep everything)
    const uint32_t prefix = (uint32_t)s[ST_PREFIX] | ((uint32_t)j << smp_shift(round));
    if (stage >= 2 && round == 0) s[ST_TARGET] = __double_as_longlong(target);
    if (round < 2) {
      s[ST_PREFIX] = prefix;
      s[ST_CUM] = (int64_t)(cum + (pick < 0 ? 0ull : above));
    } else {
      s[ST_PREFIX] = 0; s[ST_CUM] = 0;
      if (stage == 1 || stage == 3) s[ST_TK] = prefix;
      if (stage == 2 || (stage == 1 && !p_follows)) s[ST_THR] = prefix;
    }
  }
}

// Z = sum w and E = sum w * (m - x) over the current kept interval, w = the fixed-point weight of the mass rounds, both as integers in units
// of 2^-32: bins 0 and 1 of the row.  A token of weight 0 (-inf among them) adds to neither.  entropy = log Z + E / Z.
__global__ __launch_bounds__(256) void smp_stat_kernel(const float* logits, int ld, int V, const uint32_t* seen, int bmw, float pen, float T,
                                                       const int64_t* st, int use_hi, uint64_t* hist) {
  __shared__ unsigned long long acc[2];
  const int row = blockIdx.y;
  if (threadIdx.x < 2) acc[threadIdx.x] = 0;
  __syncthreads();
  const float* lg = logits + (size_t)row * ld;
  const uint32_t* sn = seen ? seen + (size_t)row * bmw : nullptr;
  const int64_t* s = st + (size_t)row * SMP_ST;
  const uint32_t klo = (uint32_t)s[ST_THR], khi = use_hi ? (uint32_t)s[ST_HI] : 0xFFFFFFFFu;
  const double m = (double)smp_unkey((uint32_t)s[ST_MKEY]);
  const int per = (V + SMP_HIST_CH - 1) / SMP_HIST_CH;
  const int lo = blockIdx.x * per, hi = min(lo + per, V);
  unsigned long long z = 0, e = 0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float x = __fdiv_rn(smp_penalised(lg, sn, i, pen), T);
    const uint32_t k = smp_key(x);
    if (k < klo || k > khi) continue;
    const double ex = exp((double)x - m);
    const unsigned long long w = (unsigned long long)llrint(ex * SMP_FIX);
    if (!w) continue;
    z += w;
    e += (unsigned long long)llrint(ex * (m - (double)x) * SMP_FIX);
  }
  if (z) { atomicAdd(&acc[0], z); atomicAdd(&acc[1], e); }
  __syncthreads();
  if (threadIdx.x < 2 && acc[threadIdx.x]) atomicAdd((unsigned long long*)&hist[(size_t)row * SMP_BINS + threadIdx.x], acc[threadIdx.x]);
}

// typical_p's cut back to the logits: the largest and the smallest key among the tokens of the kept set with d <= the cut (bin 0: max key,
// bin 1: max complemented key).  d is monotone on either side of its minimum, so these tokens are exactly the keys in [min, max].
__global__ __launch_bounds__(256) void smp_bounds_kernel(const float* logits, int ld, int V, const uint32_t* seen, int bmw, float pen, float T,
                                                         const int64_t* st, uint64_t* hist) {
  const int row = blockIdx.y;
  const float* lg = logits + (size_t)row * ld;
  const uint32_t* sn = seen ? seen + (size_t)row * bmw : nullptr;
  const int64_t* s = st + (size_t)row * SMP_ST;
  const uint32_t klo = (uint32_t)s[ST_THR], cut = (uint32_t)s[ST_TK];
  const float tL = __uint_as_float((uint32_t)s[ST_AUX]), tH = __uint_as_float((uint32_t)((uint64_t)s[ST_AUX] >> 32));
  const int per = (V + SMP_HIST_CH - 1) / SMP_HIST_CH;
  const int lo = blockIdx.x * per, hi = min(lo + per, V);
  uint32_t mx = 0, mn = 0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float x = __fdiv_rn(smp_penalised(lg, sn, i, pen), T);
    const uint32_t k = smp_key(x);
    if (k < klo || ~smp_key(smp_typ_dist(x, tL, tH)) < cut) continue;
    mx = max(mx, k);
    mn = max(mn, ~k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    mn = max(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
  }
  __shared__ uint32_t wx[4], wn[4];
  if ((threadIdx.x & 63) == 0) { wx[threadIdx.x >> 6] = mx; wn[threadIdx.x >> 6] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(wx[0], wx[1]), max(wx[2], wx[3]));
    mn = max(max(wn[0], wn[1]), max(wn[2], wn[3]));
    atomicMax((unsigned long long*)&hist[(size_t)row * SMP_BINS], (unsigned long long)mx);
    atomicMax((unsigned long long*)&hist[(size_t)row * SMP_BINS + 1], (unsigned long long)mn);
  }
}

// the smallest fp32 >= v as a key: a token is kept iff (double)x >= v
__device__ __forceinline__ uint32_t smp_key_at_least(double v) {
  float f = (float)v;
  if ((double)f < v) f = nextafterf(f, INFINITY);
  return smp_key(f);
}

// Close a filter (one thread per row): bins 0 and 1 of the row (summed over the ranks; the bounds stage takes the maximum over them) and
// the state -> the new lower key, for typical_p its fp32 constants (FL_TYP) and then both ends (FL_BOUNDS).  A threshold never rises above
// the largest kept key, so that token and its ties stay (min_tokens_to_keep = 1).  par: log(min_p) / log(epsilon) / log(eta).
__global__ __launch_bounds__(64) void smp_filter_kernel(uint64_t* hist, const float* xb, int tp, int64_t* st, int what, double par, int use_hi) {
  if (threadIdx.x != 0) return;
  const int row = blockIdx.x;
  uint64_t* h = hist + (size_t)row * SMP_BINS;
  const float* x = xb ? xb + (size_t)row * SMP_XS : nullptr;
  int64_t* s = st + (size_t)row * SMP_ST;
  const uint32_t mkey = (uint32_t)s[ST_MKEY];
  const uint32_t top = use_hi ? (uint32_t)s[ST_HI] : mkey;
  const uint32_t lo = (uint32_t)s[ST_THR];
  const double m = (double)smp_unkey(mkey);
  if (what == FL_MINP) {
    s[ST_THR] = max(lo, min(smp_key_at_least((double)smp_unkey(top) + par), top));
    return;
  }
  uint64_t v0, v1;
  if (what == FL_BOUNDS) {
    if (x) {
      v0 = v1 = 0;
      for (int r = 0; r < tp; ++r) {
        v0 = max(v0, (uint64_t)((uint32_t)x[2 * r] | ((uint32_t)x[2 * r + 1] << 16)));
        v1 = max(v1, (uint64_t)((uint32_t)x[16 + 2 * r] | ((uint32_t)x[16 + 2 * r + 1] << 16)));
      }
    } else {
      v0 = h[0]; v1 = h[1];
    }
    h[0] = 0; h[1] = 0;
    s[ST_HI] = (uint32_t)v0;
    s[ST_THR] = (uint32_t)~(uint32_t)v1;
    return;
  }
  if (x) {
    v0 = (uint64_t)x[0] + ((uint64_t)x[1] << 21) + ((uint64_t)x[2] << 42);
    v1 = (uint64_t)x[3] + ((uint64_t)x[4] << 21) + ((uint64_t)x[5] << 42);
  } else {
    v0 = h[0]; v1 = h[1];
  }
  h[0] = 0; h[1] = 0;
  const double lz = log((double)v0 * (1.0 / SMP_FIX));
  const double H = lz + (double)v1 / (double)v0;
  if (what == FL_TYP) {
    const uint32_t L32 = __float_as_uint((float)(m + lz)), H32 = __float_as_uint((float)H);
    s[ST_AUX] = (int64_t)((uint64_t)L32 | ((uint64_t)H32 << 32));
    return;
  }
  const double lp = what == FL_EPS ? par : fmin(par, 0.5 * par - H);      // log of the probability threshold
  s[ST_THR] = max(lo, min(smp_key_at_least(m + (lz + lp)), top));
}

// the race over the kept tokens (key >= threshold): argmax of x + Gumbel noise, first (global) index on ties.  greedy = 1 (top_k == 1): the
// argmax of the penalised logits without noise or temperature, i.e. greedy_pick's id.
__global__ __launch_bounds__(256) void smp_race_kernel(const float* logits, int ld, int V, const uint32_t* seen, int bmw, float pen, float T,
                                                       const int64_t* st, int use_thr, int use_hi, int greedy, uint64_t seed, const int* step,
                                                       int vfy, int gbase, float* pv, int* pi) {
  const int row = blockIdx.y;
  const float* lg = logits + (size_t)row * ld;
  const uint32_t* sn = seen ? seen + (size_t)row * bmw : nullptr;
  const uint32_t thr = use_thr ? (uint32_t)st[(size_t)row * SMP_ST + ST_THR] : 0u;
  const uint32_t top = use_hi ? (uint32_t)st[(size_t)row * SMP_ST + ST_HI] : 0xFFFFFFFFu;
  // verify form: row j is sequence 0 at step[0] + j, so it draws what a plain step of sequence 0 draws there
  const uint64_t rk = vfy ? smp_row_key(seed, 0, step[0] + row) : smp_row_key(seed, row, step[row]);
  const int per = (V + SMP_RACE_CH - 1) / SMP_RACE_CH;
  const int lo = blockIdx.x * per, hi = min(lo + per, V);
  float best = -INFINITY;
  int besti = INT_MAX;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float l = smp_penalised(lg, sn, i, pen);
    if (greedy) { smp_better(best, besti, l, gbase + i); continue; }
    const float x = __fdiv_rn(l, T);
    const uint32_t k = smp_key(x);
    if (k < thr || k > top) continue;
    smp_better(best, besti, __fadd_rn(x, smp_noise(rk, (uint32_t)(gbase + i))), gbase + i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smp_better(best, besti, __shfl_xor(best, o, 64), __shfl_xor(besti, o, 64));
  __shared__ float bv[4];
  __shared__ int bi[4];
  if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) smp_better(best, besti, bv[w], bi[w]);
    pv[row * SMP_RACE_CH + blockIdx.x] = best;
    pi[row * SMP_RACE_CH + blockIdx.x] = besti;
  }
}

// verify form, repetition penalty: the seen set of row j = sequence 0's bitmap + tokens[1..j] (the drafts in front of the row), this rank's
// bits only; ids outside [0, V_total) or the shard are ignored.  One thread per word of a row's bitmap: out [T][bmw]
__global__ __launch_bounds__(256) void smp_verify_seen_kernel(const uint32_t* base, const int32_t* tokens, int gbase, int V, int V_total,
                                                              int bmw, uint32_t* out) {
  const int w = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (w >= bmw) return;
  uint32_t v = base[w];
  for (int t = 1; t <= row; ++t) {
    const int id = tokens[t];
    if (id < gbase || id >= V_total) continue;      // (gbase >= 0: a negative id goes here too)
    const int li = id - gbase;
    if (li < V && (li >> 5) == w) v |= 1u << (li & 31);
  }
  out[(size_t)row * bmw + w] = v;
}

// the picked id of a row: record it in the repetition bitmap (its own shard's bit; `last` remembers a newly set bit for omchat_kv_rewind),
// advance the step counter and the decode positions
__device__ __forceinline__ void smp_commit(int row, int id, int gbase, int V, uint32_t* bm, int bmw, int* last, int* step, int* adv_pos,
                                           int* adv_len, int* out) {
  out[row] = id;
  if (bm) {
    const int li = id - gbase;
    int set = -1;
    if (li >= 0 && li < V) {
      uint32_t* w = bm + (size_t)row * bmw + (li >> 5);
      const uint32_t bit = 1u << (li & 31);
      if (!(*w & bit)) { *w |= bit; set = li; }
    }
    last[row] = set;
  }
  step[row] += 1;
  if (adv_pos) adv_pos[row] += 1;
  if (adv_len) adv_len[row] += 1;
}

// the 64 race partials of a row -> its winner.  TP = 1: commit.  TP > 1: (value, global index) into this rank's slot of the zeroed table that
// the greedy exchange uses (pick.hip: tp_argmax_scatter_kernel's layout)
__global__ __launch_bounds__(64) void smp_final_kernel(const float* pv, const int* pi, int b, int tp, int rank, float* table, int gbase, int V,
                                                       uint32_t* bm, int bmw, int* last, int* step, int* adv_pos, int* adv_len, int* out,
                                                       const int64_t* st, uint32_t* thr_out, uint32_t* hi_out, int use_hi, int commit) {
  const int row = blockIdx.x;
  float best = pv[row * SMP_RACE_CH + threadIdx.x];
  int besti = pi[row * SMP_RACE_CH + threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smp_better(best, besti, __shfl_xor(best, o, 64), __shfl_xor(besti, o, 64));
  if (threadIdx.x != 0) return;
  if (thr_out) thr_out[row] = (uint32_t)st[(size_t)row * SMP_ST + ST_THR];
  if (hi_out) {
    const int64_t* s = st + (size_t)row * SMP_ST;
    hi_out[row] = use_hi && (uint32_t)s[ST_HI] != (uint32_t)s[ST_MKEY] ? (uint32_t)s[ST_HI] : 0xFFFFFFFFu;
  }
  if (tp > 1) {
    table[((size_t)rank * b + row) * 2] = best;
    table[((size_t)rank * b + row) * 2 + 1] = besti == INT_MAX ? -1.f : (float)besti;
    return;
  }
  if (!commit) { out[row] = besti == INT_MAX ? 0 : besti; return; }      // verify form: the acceptance commits (model.hip)
  smp_commit(row, besti == INT_MAX ? 0 : besti, gbase, V, bm, bmw, last, step, adv_pos, adv_len, out);
}

// after the exchange: ranks hold ascending index ranges, so strict > keeps the first index on ties (pick.hip: tp_argmax_pick_kernel's rule)
__global__ void smp_tp_pick_kernel(const float* table, int b, int tp, int gbase, int V, uint32_t* bm, int bmw, int* last, int* step,
                                   int* adv_pos, int* adv_len, int* out, int commit) {
  const int i = threadIdx.x;
  if (i >= b) return;
  float best = table[(size_t)i * 2];
  int bi = (int)table[(size_t)i * 2 + 1];
  for (int r = 1; r < tp; ++r) {
    const float v = table[((size_t)r * b + i) * 2];
    if (v > best) { best = v; bi = (int)table[((size_t)r * b + i) * 2 + 1]; }
  }
  if (!commit) { out[i] = bi < 0 ? 0 : bi; return; }
  smp_commit(i, bi < 0 ? 0 : bi, gbase, V, bm, bmw, last, step, adv_pos, adv_len, out);
}

__global__ void smp_rewind_kernel(uint32_t* bm, int bmw, int* last, int* step, int b, int n) {
  const int i = threadIdx.x;
  if (i >= b) return;
  if (bm && last[i] >= 0) bm[(size_t)i * bmw + (last[i] >> 5)] &= ~(1u << (last[i] & 31));
  if (bm) last[i] = -1;
  step[i] -= n;
}

// take back the last r of the cnt picks a sampled verify step committed to sequence 0: their newly set bits (vlast) and the step counter
__global__ void smp_rewind_verify_kernel(uint32_t* bm, int* vlast, int* step, int cnt, int r) {
  if (threadIdx.x != 0) return;
  for (int i = cnt - r; i < cnt; ++i) {
    if (bm && vlast[i] >= 0) bm[vlast[i] >> 5] &= ~(1u << (vlast[i] & 31));
    vlast[i] = -1;
  }
  step[0] -= r;
}

}  // namespace

size_t sample_ws_bytes(int b) {
  return (size_t)b * (SMP_BINS * 8 + SMP_ST * 8 + SMP_XS * 4 + SMP_RACE_CH * 8);
}

// where the log-probability stage (logprob.hip) finds the kept-set threshold key that the last launch_sample with these parameters left for
// row r: words[r * stride] (the low word of ST_THR); nullptr when the parameters keep every token
const uint32_t* sample_thr_words(const void* ws, int b, int V_total, int top_k, double top_p, const SampleFilters& f, int* stride,
                                 const uint32_t** hi) {
  const bool use = top_k != 1 && ((top_k > 1 && top_k < V_total) || top_p < 1.0 || f.any());
  *hi = nullptr;
  if (!use) return nullptr;
  *stride = SMP_ST * 2;
  const uint32_t* st = (const uint32_t*)((const char*)ws + (size_t)b * SMP_BINS * 8);
  if (f.typical_on()) *hi = st + ST_HI * 2;
  return st + ST_THR * 2;
}

int launch_sample(const SampleArgs& a, hipStream_t s) {
  OM_CHECK(a.b >= 1 && a.V >= 1 && a.ws && a.out && a.step, "launch_sample: bad argument");
  OM_CHECK(a.temperature > 0.f, "sampling: temperature must be > 0");
  OM_CHECK(a.top_p > 0.0 && a.top_p <= 1.0, "sampling: top_p in (0, 1]");
  OM_CHECK(a.tp == 1 || (a.xchg && a.table), "sampling under tensor parallelism needs the exchange");
  OM_CHECK(a.tp >= 1 && a.tp <= 8, "sampling: the limb exchange holds at most 8 ranks");
  OM_CHECK(!(a.f.min_p > 1.0) && !(a.f.typical_p <= 0.0) && !(a.f.epsilon <= 0.0) && !(a.f.eta <= 0.0), "sampling: filter parameters out of range");
  const int b = a.b, V = a.V;
  const bool vfy = a.vtokens != nullptr;
  OM_CHECK(!vfy || (b >= 2 && b <= SMP_VERIFY_ROWS), "sampling, verify form: 2 <= rows <= 16");
  char* w = (char*)a.ws;
  uint64_t* hist = (uint64_t*)w;                 w += (size_t)b * SMP_BINS * 8;
  int64_t* st = (int64_t*)w;                     w += (size_t)b * SMP_ST * 8;
  float* xb = (float*)w;                         w += (size_t)b * SMP_XS * 4;
  float* pv = (float*)w;                         w += (size_t)b * SMP_RACE_CH * 4;
  int* pi = (int*)w;
  const int gbase = a.rank * V;
  const bool pen = a.bitmap && a.penalty != 1.f;
  OM_CHECK(!(vfy && pen) || a.vseen, "sampling, verify form: the repetition penalty needs the bitmap scratch");
  const uint32_t* seen = pen ? (vfy ? a.vseen : a.bitmap) : nullptr;
  if (vfy && pen)
    hipLaunchKernelGGL(smp_verify_seen_kernel, dim3((a.bm_words + 255) / 256, b), dim3(256), 0, s, a.bitmap, a.vtokens, gbase, V, a.V_total,
                       a.bm_words, a.vseen);
  const bool greedy = a.top_k == 1;
  const bool use_k = !greedy && a.top_k > 1 && a.top_k < a.V_total;
  const bool use_p = !greedy && a.top_p < 1.0;
  const bool use_f = !greedy && a.f.any();           // (top_k == 1 leaves the maxima, which every later warper keeps)
  const bool use_hi = use_f && a.f.typical_on();
  float* xbp = a.tp > 1 ? xb : nullptr;
  auto exchange = [&](int max_stage, int rows) -> int {
    if (a.tp == 1) return 0;
    hipLaunchKernelGGL(smp_to_limbs_kernel, dim3(rows), dim3(256), 0, s, hist, xb, max_stage, a.rank);
    return a.xchg(a.xchg_user, xb, (size_t)rows * SMP_XS, s);
  };
  if (use_k || use_p || use_f) {
    OM_HIP(hipMemsetAsync(hist, 0, (size_t)b * (SMP_BINS + SMP_ST) * 8, s));
    const dim3 hg(SMP_HIST_CH, b);
    if (use_k) {
      for (int r = 0; r < 3; ++r) {
        hipLaunchKernelGGL(smp_hist_kernel<0>, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, st, hist, r);
        if (int rc = exchange(0, b)) return rc;
        hipLaunchKernelGGL(smp_select_kernel, dim3(b), dim3(256), 0, s, hist, xbp, a.tp, st, 1, r, a.top_k, a.top_p, (int)use_p);
      }
    }
    if (use_p) {
      hipLaunchKernelGGL(smp_max_kernel, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, hist);
      if (int rc = exchange(1, b)) return rc;
      hipLaunchKernelGGL(smp_select_kernel, dim3(b), dim3(256), 0, s, hist, xbp, a.tp, st, 0, 0, a.top_k, a.top_p, 1);
      for (int r = 0; r < 3; ++r) {
        hipLaunchKernelGGL(smp_hist_kernel<1>, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, st, hist, r);
        if (int rc = exchange(0, b)) return rc;
        hipLaunchKernelGGL(smp_select_kernel, dim3(b), dim3(256), 0, s, hist, xbp, a.tp, st, 2, r, a.top_k, a.top_p, 1);
      }
    }
    if (use_f) {
      const SampleFilters& f = a.f;
      if (!use_p) {      // the four work relative to the row's maximum
        hipLaunchKernelGGL(smp_max_kernel, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, hist);
        if (int rc = exchange(1, b)) return rc;
        hipLaunchKernelGGL(smp_select_kernel, dim3(b), dim3(256), 0, s, hist, xbp, a.tp, st, 0, 0, a.top_k, a.top_p, 1);
      }
      // Z and the entropy sum over the interval as it stands, then the filter's close
      auto stat_close = [&](int what, double par, int hi_now) -> int {
        hipLaunchKernelGGL(smp_stat_kernel, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, st, hi_now, hist);
        if (int rc = exchange(0, b)) return rc;
        hipLaunchKernelGGL(smp_filter_kernel, dim3(b), dim3(64), 0, s, hist, xbp, a.tp, st, what, par, hi_now);
        return 0;
      };
      if (f.min_p_on()) hipLaunchKernelGGL(smp_filter_kernel, dim3(b), dim3(64), 0, s, hist, xbp, a.tp, st, (int)FL_MINP, log(f.min_p), 0);
      if (f.typical_on()) {
        if (int rc = stat_close(FL_TYP, 0.0, 0)) return rc;
        for (int r = 0; r < 3; ++r) {
          hipLaunchKernelGGL(smp_hist_kernel<2>, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, st, hist, r);
          if (int rc = exchange(0, b)) return rc;
          hipLaunchKernelGGL(smp_select_kernel, dim3(b), dim3(256), 0, s, hist, xbp, a.tp, st, 3, r, a.top_k, f.typical_p, 1);
        }
        hipLaunchKernelGGL(smp_bounds_kernel, hg, dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature, st, hist);
        if (int rc = exchange(1, b)) return rc;
        hipLaunchKernelGGL(smp_filter_kernel, dim3(b), dim3(64), 0, s, hist, xbp, a.tp, st, (int)FL_BOUNDS, 0.0, 0);
      }
      if (f.epsilon_on()) if (int rc = stat_close(FL_EPS, log(f.epsilon), (int)use_hi)) return rc;
      if (f.eta_on()) if (int rc = stat_close(FL_ETA, log(f.eta), (int)use_hi)) return rc;
    }
  }
  if (a.tp > 1) OM_HIP(hipMemsetAsync(a.table, 0, (size_t)a.tp * b * 2 * 4, s));
  hipLaunchKernelGGL(smp_race_kernel, dim3(SMP_RACE_CH, b), dim3(256), 0, s, a.logits, a.ld, V, seen, a.bm_words, a.penalty, a.temperature,
                     st, (int)(use_k || use_p || use_f), (int)use_hi, (int)greedy, a.seed, a.step, (int)vfy, gbase, pv, pi);
  uint32_t* bm = pen && !vfy ? a.bitmap : nullptr;
  hipLaunchKernelGGL(smp_final_kernel, dim3(b), dim3(64), 0, s, pv, pi, b, a.tp, a.rank, a.table, gbase, V, bm, a.bm_words, a.last_set, a.step,
                     a.adv_pos, a.adv_len, a.out, st, (use_k || use_p || use_f) ? a.thr_out : nullptr, a.hi_out, (int)use_hi, (int)!vfy);
  if (a.tp > 1) {
    // the greedy exchange: zeroed table, one slot per rank, summed
    OM_LAUNCH_CHECK();
    if (int rc = a.xchg(a.xchg_user, a.table, (size_t)a.tp * b * 2, s)) return rc;
    hipLaunchKernelGGL(smp_tp_pick_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, a.table, b, a.tp, gbase, V, bm, a.bm_words, a.last_set, a.step,
                       a.adv_pos, a.adv_len, a.out, (int)!vfy);
  }
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_sample_rewind(uint32_t* bitmap, int bm_words, int* last_set, int* step, int b, int n, hipStream_t s) {
  hipLaunchKernelGGL(smp_rewind_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, bitmap, bm_words, last_set, step, b, n);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_sample_rewind_verify(uint32_t* bitmap, int* vlast, int* step, int cnt, int r, hipStream_t s) {
  OM_CHECK(vlast && step && r >= 0 && r <= cnt && cnt <= SMP_VERIFY_ROWS, "launch_sample_rewind_verify: bad argument");
  hipLaunchKernelGGL(smp_rewind_verify_kernel, dim3(1), dim3(64), 0, s, bitmap, vlast, step, cnt, r);
  OM_LAUNCH_CHECK();
  return 0;
}
