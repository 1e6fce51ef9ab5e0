// Per-token log-probabilities of the ids generate() picks: for every row the raw value log_softmax(logits)[id] and the
// processed value log_softmax(scores)[id], scores = what HF's processors leave (banned ids at -inf, repetition penalty, / T, ids outside the
// kept interval of top-k / top-p / min_p / typical_p / epsilon / eta at -inf).  The processed row is never materialised: every element is evaluated on the fly exactly as sample.hip
// evaluates it.  One launch of (LP_CH, b) workgroups leaves an online (max, sum exp(x - max)) pair per statistic and slice, one wave per row
// folds the LP_CH pairs in a fixed tree and writes x_id - (max + log sum).  No float atomics and no arrival-order folds: the same bits come out
// of the eager step and of the captured graph.  tests/logprob_ref.py is the fp64 restatement.
#include "kernels.h"
#include "sample_common.h"
#include <math.h>

namespace {

#ifndef OMCHAT_LP_CH
#define OMCHAT_LP_CH 64        // (other multiples of 64 for A/B builds)
#endif
constexpr int LP_CH = OMCHAT_LP_CH;      // slices (workgroups) per row: one per lane of the finishing wave
static_assert(LP_CH >= 64 && LP_CH % 64 == 0, "the finishing wave takes the slices 64 at a time");
constexpr int LP_TS = 8;       // fp32 words per (rank, row) slot of the tensor-parallel exchange

// x joins the running (m, s = sum exp(. - m)); -inf contributes nothing.  top1 (the sampler's top_k == 1: only the maxima are kept): s counts them
__device__ __forceinline__ void lp_add(float& m, float& s, float x, int top1) {
  if (x > m) {
    s = top1 ? 1.f : __fadd_rn(__fmul_rn(s, expf(m - x)), 1.f);
    m = x;
  } else if (x != -INFINITY) {
    s = __fadd_rn(s, top1 ? (x == m ? 1.f : 0.f) : expf(x - m));
  }
}
// a slice that is entirely -inf has (m, s) = (-inf, 0) and must not reach exp(-inf - -inf)
__device__ __forceinline__ void lp_merge(float& m, float& s, float m2, float s2, int top1) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) { s = 0.f; return; }
  if (top1) s = __fadd_rn(m == M ? s : 0.f, m2 == M ? s2 : 0.f);
  else s = __fadd_rn(__fmul_rn(s, expf(m - M)), __fmul_rn(s2, expf(m2 - M)));
  m = M;
}
__device__ __forceinline__ void lp_wave_merge(float& m, float& s, int top1) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lp_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64), top1);
}
__device__ __forceinline__ float lp_value(float x, float m, float s) {
  return x == -INFINITY ? -INFINITY : __fsub_rn(x, __fadd_rn(m, logf(s)));
}

struct LpK {
  const float* raw; int raw_ld;
  const float* proc; int proc_ld;
  int V;
  const uint32_t* ban; const uint32_t* seen; int bmw;
  const int* last;
  float pen, T;
  const uint32_t* thr; const uint32_t* thr_hi; int thr_stride;
  int top1;
};
// the processed value of local id i of a row
struct LpProc {
  const uint32_t *ban, *seen; int skip; float pen, T; uint32_t thr, top;
  __device__ __forceinline__ LpProc(const LpK& a, int row)
      : ban(a.ban ? a.ban + (size_t)row * a.bmw : nullptr), seen(a.seen ? a.seen + (size_t)row * a.bmw : nullptr),
        skip(a.seen && a.last ? a.last[row] : -1), pen(a.pen), T(a.T), thr(a.thr ? a.thr[(size_t)row * a.thr_stride] : 0u),
        top(a.thr_hi ? a.thr_hi[(size_t)row * a.thr_stride] : 0xFFFFFFFFu) {}
  __device__ __forceinline__ float operator()(float x, int i) const {
    if (ban && ((ban[i >> 5] >> (i & 31)) & 1u)) return -INFINITY;
    // HF scores this step with the seen set from before the pick: the bit the pick itself set (`skip`) does not count
    if (seen && i != skip && ((seen[i >> 5] >> (i & 31)) & 1u)) x = smp_penalise(x, pen);
    x = __fdiv_rn(x, T);
    const uint32_t k = smp_key(x);
    return k < thr || k > top ? -INFINITY : x;
  }
};

// elements [lo, hi) of a row: scalar head up to a 16-byte boundary, 16-byte loads, scalar tail
template <class F>
__device__ __forceinline__ void lp_scan(const float* r, int lo, int hi, F&& f) {
  int a0 = lo + (int)((4u - (unsigned)(((uintptr_t)(r + lo) >> 2) & 3u)) & 3u);
  a0 = min(a0, hi);
  const int nv = (hi - a0) >> 2;
  for (int i = lo + threadIdx.x; i < a0; i += 256) f(r[i], i);
  const float4* v = (const float4*)(r + a0);
  for (int j = threadIdx.x; j < nv; j += 256) {
    const float4 q = v[j];
    const int i = a0 + 4 * j;
    f(q.x, i); f(q.y, i + 1); f(q.z, i + 2); f(q.w, i + 3);
  }
  for (int i = a0 + 4 * nv + threadIdx.x; i < hi; i += 256) f(r[i], i);
}

// part[row][slice] = (max, sum) of the raw logits and, TWO, of the processed values over the slice
template <int TWO>
__global__ __launch_bounds__(256) void lp_partial_kernel(LpK a, float4* part) {
  const int row = blockIdx.y;
  const float* rr = a.raw + (size_t)row * a.raw_ld;
  const int per = ((a.V + LP_CH - 1) / LP_CH + 3) & ~3;
  const int lo = min((int)blockIdx.x * per, a.V), hi = min(lo + per, a.V);
  float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f;
  if (TWO) {
    const LpProc p(a, row);
    const float* pr = a.proc + (size_t)row * a.proc_ld;
    const int top1 = a.top1;
    if (pr == rr) {
      lp_scan(rr, lo, hi, [&](float x, int i) { lp_add(m0, s0, x, 0); lp_add(m1, s1, p(x, i), top1); });
    } else {
      lp_scan(rr, lo, hi, [&](float x, int) { lp_add(m0, s0, x, 0); });
      lp_scan(pr, lo, hi, [&](float x, int i) { lp_add(m1, s1, p(x, i), top1); });
    }
  } else {
    lp_scan(rr, lo, hi, [&](float x, int) { lp_add(m0, s0, x, 0); });
  }
  lp_wave_merge(m0, s0, 0);
  if (TWO) lp_wave_merge(m1, s1, a.top1);
  __shared__ float4 wv[4];
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = make_float4(m0, s0, m1, s1);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lp_merge(m0, s0, wv[w].x, wv[w].y, 0);
      if (TWO) lp_merge(m1, s1, wv[w].z, wv[w].w, a.top1);
    }
    part[(size_t)row * LP_CH + blockIdx.x] = make_float4(m0, s0, m1, s1);
  }
}

// the row's record at its counter (a counter beyond the record writes nothing), then the counter advances
__device__ __forceinline__ void lp_store(float* rec, int* cnt, int row, int max_new, int rec_ld, float v0, float v1) {
  const int t = cnt[row];
  if (t >= 0 && t < max_new) {
    rec[(size_t)t * rec_ld + row] = v0;
    rec[((size_t)max_new + t) * rec_ld + row] = v1;
  }
  cnt[row] = t + 1;
}

// one wave per row: the LP_CH pairs folded by a fixed tree.  TP = 1: the record.  TP > 1: this rank's pairs, and from the rank that owns the id
// its two values, into the rank's own slot of the zeroed table
__global__ __launch_bounds__(64) void lp_finish_kernel(LpK a, const float4* part, const int* ids, int gbase, int two, int b, int tp, int rank,
                                                       float* table, float* rec, int* cnt, int max_new, int rec_ld) {
  const int row = blockIdx.x;
  const float4 q = part[(size_t)row * LP_CH + threadIdx.x];
  float m0 = q.x, s0 = q.y, m1 = q.z, s1 = q.w;
#pragma unroll
  for (int j = 64; j < LP_CH; j += 64) {      // (A/B builds with more slices: lane order first, then the tree)
    const float4 r = part[(size_t)row * LP_CH + j + threadIdx.x];
    lp_merge(m0, s0, r.x, r.y, 0);
    if (two) lp_merge(m1, s1, r.z, r.w, a.top1);
  }
  lp_wave_merge(m0, s0, 0);
  if (two) lp_wave_merge(m1, s1, a.top1);
  if (threadIdx.x != 0) return;
  if (!two) { m1 = m0; s1 = s0; }
  const int li = ids[row] - gbase;
  float x0 = 0.f, x1 = 0.f;
  if (li >= 0 && li < a.V) {
    x0 = a.raw[(size_t)row * a.raw_ld + li];
    x1 = two ? LpProc(a, row)(a.proc[(size_t)row * a.proc_ld + li], li) : x0;
  }
  if (tp > 1) {
    float* t = table + ((size_t)rank * b + row) * LP_TS;
    t[0] = m0; t[1] = s0; t[2] = m1; t[3] = s1; t[4] = x0; t[5] = x1;
    return;
  }
  if (a.top1 && x1 != m1) x1 = -INFINITY;      // top_k == 1 keeps the maxima only: any other id was cut
  lp_store(rec, cnt, row, max_new, rec_ld, lp_value(x0, m0, s0), lp_value(x1, m1, s1));
}

// after the exchange every rank folds the slots in rank order: the same number everywhere
__global__ void lp_tp_fold_kernel(const float* table, int b, int tp, int top1, float* rec, int* cnt, int max_new, int rec_ld) {
  const int i = threadIdx.x;
  if (i >= b) return;
  float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f, x0 = 0.f, x1 = 0.f;
  for (int r = 0; r < tp; ++r) {
    const float* t = table + ((size_t)r * b + i) * LP_TS;
    lp_merge(m0, s0, t[0], t[1], 0);
    lp_merge(m1, s1, t[2], t[3], top1);
    x0 += t[4]; x1 += t[5];      // zero in every slot but the owner's
  }
  if (top1 && x1 != m1) x1 = -INFINITY;
  lp_store(rec, cnt, i, max_new, rec_ld, lp_value(x0, m0, s0), lp_value(x1, m1, s1));
}

__global__ void lp_rewind_kernel(int* cnt, int b, int n) {
  const int i = threadIdx.x;
  if (i < b) cnt[i] = max(cnt[i] - n, 0);
}

}  // namespace

size_t logprob_ws_bytes(int b) { return (size_t)b * LP_CH * sizeof(float4); }
size_t logprob_table_bytes(int b, int tp) { return (size_t)tp * b * LP_TS * 4 + 16; }

int launch_logprob(const LogprobArgs& a, hipStream_t s) {
  OM_CHECK(a.raw && a.ids && a.ws && a.rec && a.cnt && a.b >= 1 && a.V >= 1 && a.max_new >= 1 && a.rec_ld >= a.b, "launch_logprob: bad argument");
  OM_CHECK(a.tp == 1 || (a.xchg && a.table), "log-probabilities under tensor parallelism need the exchange");
  const bool pen = a.seen && a.penalty != 1.f;
  const bool two = a.proc != a.raw || a.ban || pen || a.temperature != 1.f || a.thr || a.thr_hi || a.top1;
  LpK k;
  k.raw = a.raw; k.raw_ld = a.raw_ld; k.proc = a.proc ? a.proc : a.raw; k.proc_ld = a.proc ? a.proc_ld : a.raw_ld; k.V = a.V;
  k.ban = a.ban; k.seen = pen ? a.seen : nullptr; k.bmw = a.bm_words; k.last = a.last_set;
  k.pen = a.penalty; k.T = a.temperature; k.thr = a.thr; k.thr_hi = a.thr_hi; k.thr_stride = a.thr_stride; k.top1 = a.top1;
  float4* part = (float4*)a.ws;
  if (two) hipLaunchKernelGGL(lp_partial_kernel<1>, dim3(LP_CH, a.b), dim3(256), 0, s, k, part);
  else hipLaunchKernelGGL(lp_partial_kernel<0>, dim3(LP_CH, a.b), dim3(256), 0, s, k, part);
  if (a.tp > 1) OM_HIP(hipMemsetAsync(a.table, 0, (size_t)a.tp * a.b * LP_TS * 4, s));
  hipLaunchKernelGGL(lp_finish_kernel, dim3(a.b), dim3(64), 0, s, k, part, a.ids, a.rank * a.V, (int)two, a.b, a.tp, a.rank, a.table, a.rec, a.cnt,
                     a.max_new, a.rec_ld);
  if (a.tp > 1) {
    OM_LAUNCH_CHECK();
    if (int rc = a.xchg(a.xchg_user, a.table, (size_t)a.tp * a.b * LP_TS, s)) return rc;
    hipLaunchKernelGGL(lp_tp_fold_kernel, dim3(1), dim3(64 > a.b ? 64 : a.b), 0, s, a.table, a.b, a.tp, a.top1, a.rec, a.cnt, a.max_new, a.rec_ld);
  }
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_logprob_rewind(int* cnt, int b, int n, hipStream_t s) {
  hipLaunchKernelGGL(lp_rewind_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, cnt, b, n);
  OM_LAUNCH_CHECK();
  return 0;
}
