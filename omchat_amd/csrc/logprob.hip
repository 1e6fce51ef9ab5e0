// Per-token log-probabilities of the ids generate() picks: for every row the raw value log_softmax(logits)[id] and the
// processed value log_softmax(scores)[id], scores = what HF's processors leave (banned ids at -inf, repetition penalty, / T, ids outside the
// kept interval of top-k / top-p / min_p / typical_p / epsilon / eta at -inf).  The processed row is never materialised: every element is evaluated on the fly exactly as sample.hip
// evaluates it.  One launch of (LP_CH, b) workgroups leaves an online (max, sum exp(x - max)) pair per statistic and slice, one wave per row
// folds the LP_CH pairs in a fixed tree and writes x_id - (max + log sum).  No float atomics and no arrival-order folds: the same bits come out
// of the eager step and of the captured graph.  tests/logprob_ref.py is the fp64 restatement.
// Extras (top_n alternatives and scored ids under the raw distribution; tests/toplogprob_ref.py): a launch of its own leaves every slice's
// top_n candidates, sorted, and the finishing wave merges the LP_CH sorted lists -- comparisons of one 64-bit word only, the picks' kernels
// above untouched when the extras are off.
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

// the LP_CH pairs of a row folded by a fixed tree: every lane of the wave ends with the same (m0, s0, m1, s1)
__device__ __forceinline__ void lp_fold_slices(const float4* part, int row, int two, int top1, float& m0, float& s0, float& m1, float& s1) {
  const float4 q = part[(size_t)row * LP_CH + threadIdx.x];
  m0 = q.x; s0 = q.y; m1 = q.z; s1 = q.w;
#pragma unroll
  for (int j = 64; j < LP_CH; j += 64) {      // (A/B builds with more slices: lane order first, then the tree)
    const float4 r = part[(size_t)row * LP_CH + j + threadIdx.x];
    lp_merge(m0, s0, r.x, r.y, 0);
    if (two) lp_merge(m1, s1, r.z, r.w, top1);
  }
  lp_wave_merge(m0, s0, 0);
  if (two) lp_wave_merge(m1, s1, top1);
}
// lane 0 of the finishing wave.  TP = 1: the record.  TP > 1: this rank's pairs, and from the rank that owns the id its two values, into the
// rank's own slot of the zeroed table
__device__ __forceinline__ void lp_finish_row(const LpK& a, int row, const int* ids, int gbase, int two, int b, int tp, int rank, float* table,
                                              float* rec, int* cnt, int max_new, int rec_ld, float m0, float s0, float m1, float s1) {
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

// one wave per row
__global__ __launch_bounds__(64) void lp_finish_kernel(LpK a, const float4* part, const int* ids, int gbase, int two, int b, int tp, int rank,
                                                       float* table, float* rec, int* cnt, int max_new, int rec_ld) {
  const int row = blockIdx.x;
  float m0, s0, m1, s1;
  lp_fold_slices(part, row, two, a.top1, m0, s0, m1, s1);
  if (threadIdx.x != 0) return;
  lp_finish_row(a, row, ids, gbase, two, b, tp, rank, table, rec, cnt, max_new, rec_ld, m0, s0, m1, s1);
}

// after the exchange every rank folds the slots in rank order: the same number everywhere
__device__ __forceinline__ void lp_tp_fold_row(const float* table, int i, int b, int tp, int top1, float& m0, float& s0, float& m1, float& s1,
                                               float& x0, float& x1) {
  m0 = -INFINITY; s0 = 0.f; m1 = -INFINITY; s1 = 0.f; x0 = 0.f; x1 = 0.f;
  for (int r = 0; r < tp; ++r) {
    const float* t = table + ((size_t)r * b + i) * LP_TS;
    lp_merge(m0, s0, t[0], t[1], 0);
    lp_merge(m1, s1, t[2], t[3], top1);
    x0 += t[4]; x1 += t[5];      // zero in every slot but the owner's
  }
  if (top1 && x1 != m1) x1 = -INFINITY;
}
__global__ void lp_tp_fold_kernel(const float* table, int b, int tp, int top1, float* rec, int* cnt, int max_new, int rec_ld) {
  const int i = threadIdx.x;
  if (i >= b) return;
  float m0, s0, m1, s1, x0, x1;
  lp_tp_fold_row(table, i, b, tp, top1, m0, s0, m1, s1, x0, x1);
  lp_store(rec, cnt, i, max_new, rec_ld, lp_value(x0, m0, s0), lp_value(x1, m1, s1));
}

// ---- extras: the top_n alternatives and the scored ids of a row under the raw distribution ("Extras")
// The order of the contract as one word: value descending (smp_key: -0 and +0 one key, -inf behind every finite value), then global id
// ascending.  Every real element's word is > 0; 0 pads a list that holds fewer than top_n.
__device__ __forceinline__ uint64_t lp_word(float x, int gid) { return ((uint64_t)smp_key(x) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)gid); }
__device__ __forceinline__ int lp_word_id(uint64_t w) { return (int)(0xFFFFFFFFu - (uint32_t)w); }
__device__ __forceinline__ uint64_t lp_wave_max64(uint64_t w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t h = __shfl_xor((uint32_t)(w >> 32), o, 64), l = __shfl_xor((uint32_t)w, o, 64);
    const uint64_t v = ((uint64_t)h << 32) | l;
    w = v > w ? v : w;
  }
  return w;
}

// cand[row][slice][0 .. top_n) = the slice's top_n words, descending: round r takes the largest word below round r - 1's.  The slice (9.5 KB
// at the OmChat vocabulary) is read from the cache top_n times; no element is moved, so rows of any alignment and size take this one path
__global__ __launch_bounds__(256) void lp_top_slice_kernel(const float* raw, int raw_ld, int V, int gbase, int top_n, uint64_t* cand) {
  const int row = blockIdx.y;
  const float* rr = raw + (size_t)row * raw_ld;
  const int per = ((V + LP_CH - 1) / LP_CH + 3) & ~3;
  const int lo = min((int)blockIdx.x * per, V), hi = min(lo + per, V);
  uint64_t* out = cand + ((size_t)row * LP_CH + blockIdx.x) * top_n;
  __shared__ uint64_t wv[2][4];
  uint64_t bound = ~0ull;
  for (int r = 0; r < top_n; ++r) {
    uint64_t best = 0;
    if (bound) lp_scan(rr, lo, hi, [&](float x, int i) {
      const uint64_t w = lp_word(x, gbase + i);
      if (w < bound && w > best) best = w;
    });
    best = lp_wave_max64(best);
    if ((threadIdx.x & 63) == 0) wv[r & 1][threadIdx.x >> 6] = best;
    __syncthreads();      // (one barrier a round: round r + 1 writes the other half of wv)
    const uint64_t* q = wv[r & 1];
    best = q[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = q[w] > best ? q[w] : best;
    if (threadIdx.x == 0) out[r] = best;
    bound = best;
  }
}

// NL sorted lists a lane (one wave): head(j, pos) = word `pos` of the lane's list j, 0 behind its end.  Round r takes the largest head of the
// wave and its owner moves on; the r-th best word of all lists comes back in lane r (0: fewer than r + 1 real words).  Words are distinct.
template <int NL, class H>
__device__ __forceinline__ uint64_t lp_merge_lists(int top_n, H&& head) {
  int hp[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) hp[j] = 0;
  uint64_t mine = 0;
  for (int r = 0; r < top_n; ++r) {
    uint64_t h = 0; int hj = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const uint64_t w = hp[j] < top_n ? head(j, hp[j]) : 0;
      if (w > h) { h = w; hj = j; }
    }
    const uint64_t best = lp_wave_max64(h);
    if (best != 0 && h == best) {
#pragma unroll
      for (int j = 0; j < NL; ++j) if (j == hj) ++hp[j];
    }
    if ((int)threadIdx.x == r) mine = best;
  }
  return mine;
}

struct LpX {
  int top_n, n_score;
  const int* sid;              // [n_score] global ids, device
  const uint64_t* cand;        // [b][LP_CH][top_n]
  float* top_v; int* top_i;    // [max_new][rec_ld][top_n]
  float* sc;                   // [max_new][rec_ld][n_score]
};
static_assert(LP_MAX_TOP <= 64 && LP_MAX_SCORED <= 64, "one lane of the finishing wave per alternative and per scored id");
__host__ __device__ __forceinline__ int lp_xslot(int top_n, int n_score) { return 2 * top_n + n_score; }

// lp_finish_kernel with the extras: lane j < top_n takes the j-th best candidate of the row, lane k < n_score the k-th scored id; both are
// written at the row's counter before lane 0's lp_store advances it.  TP > 1: the shard's candidates as (logit, float(global id)) -- id -1
// where the shard holds fewer -- and the scored logits this rank owns, behind the LP_TS words of all slots
__global__ __launch_bounds__(64) void lp_finish_ex_kernel(LpK a, const float4* part, const int* ids, int gbase, int two, int b, int tp, int rank,
                                                          float* table, float* rec, int* cnt, int max_new, int rec_ld, LpX x) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int t = cnt[row];
  float m0, s0, m1, s1;
  lp_fold_slices(part, row, two, a.top1, m0, s0, m1, s1);
  const float* rr = a.raw + (size_t)row * a.raw_ld;
  const int xs = lp_xslot(x.top_n, x.n_score);
  float* slot = tp > 1 ? table + (size_t)tp * b * LP_TS + ((size_t)rank * b + row) * xs : nullptr;
  const bool room = t >= 0 && t < max_new;
  if (x.top_n) {
    const uint64_t* c = x.cand + (size_t)row * LP_CH * x.top_n;
    const int top_n = x.top_n;
    const uint64_t w = lp_merge_lists<LP_CH / 64>(top_n, [&](int j, int pos) { return c[(size_t)(j * 64 + lane) * top_n + pos]; });
    if (lane < top_n) {
      const int gid = w ? lp_word_id(w) : -1;
      const float xv = w ? rr[gid - gbase] : -INFINITY;      // the logit itself, not the key's value: -0 stays -0, as the picked id's does
      if (tp > 1) {
        slot[2 * lane] = w ? xv : 0.f; slot[2 * lane + 1] = (float)gid;
      } else if (room) {
        const size_t o = ((size_t)t * rec_ld + row) * top_n + lane;
        x.top_v[o] = lp_value(xv, m0, s0); x.top_i[o] = gid;
      }
    }
  }
  if (lane < x.n_score) {
    const int li = x.sid[lane] - gbase;
    const bool own = li >= 0 && li < a.V;
    if (tp > 1) { if (own) slot[2 * x.top_n + lane] = rr[li]; }
    else if (room) x.sc[((size_t)t * rec_ld + row) * x.n_score + lane] = own ? lp_value(rr[li], m0, s0) : -INFINITY;
  }
  if (lane == 0) lp_finish_row(a, row, ids, gbase, two, b, tp, rank, table, rec, cnt, max_new, rec_ld, m0, s0, m1, s1);
}

// lp_tp_fold_kernel with the extras, one wave per row: lane r < tp owns rank r's sorted candidates, the merge is the one of the slices
// (x + 0 of the exchange leaves -inf and every id as they were; -0 arrives as +0, as the picked id's logit does)
__global__ __launch_bounds__(64) void lp_tp_fold_ex_kernel(const float* table, int b, int tp, int top1, float* rec, int* cnt, int max_new, int rec_ld,
                                                           LpX x) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int t = cnt[i];
  float m0, s0, m1, s1, x0, x1;
  lp_tp_fold_row(table, i, b, tp, top1, m0, s0, m1, s1, x0, x1);
  const int xs = lp_xslot(x.top_n, x.n_score);
  const float* xt = table + (size_t)tp * b * LP_TS;
  const bool room = t >= 0 && t < max_new;
  if (x.top_n) {
    const int top_n = x.top_n;
    const float* mine = xt + ((size_t)min(lane, tp - 1) * b + i) * xs;
    const uint64_t w = lp_merge_lists<1>(top_n, [&](int, int pos) {
      const float v = mine[2 * pos], id = mine[2 * pos + 1];
      return lane < tp && id >= 0.f ? lp_word(v, (int)id) : (uint64_t)0;
    });
    if (lane < top_n && room) {
      const size_t o = ((size_t)t * rec_ld + i) * top_n + lane;
      x.top_v[o] = w ? lp_value(smp_unkey((uint32_t)(w >> 32)), m0, s0) : -INFINITY;
      x.top_i[o] = w ? lp_word_id(w) : -1;
    }
  }
  if (lane < x.n_score && room) {
    float v = 0.f;
    for (int r = 0; r < tp; ++r) v += xt[((size_t)r * b + i) * xs + 2 * x.top_n + lane];      // zero in every slot but the owner's
    x.sc[((size_t)t * rec_ld + i) * x.n_score + lane] = lp_value(v, m0, s0);
  }
  if (lane == 0) lp_store(rec, cnt, i, max_new, rec_ld, lp_value(x0, m0, s0), lp_value(x1, m1, s1));
}

__global__ void lp_rewind_kernel(int* cnt, int b, int n) {
  const int i = threadIdx.x;
  if (i < b) cnt[i] = max(cnt[i] - n, 0);
}

}  // namespace

size_t logprob_ws_bytes(int b) { return (size_t)b * LP_CH * sizeof(float4); }
size_t logprob_table_bytes(int b, int tp) { return (size_t)tp * b * LP_TS * 4 + 16; }
size_t logprob_top_ws_bytes(int b, int top_n) { return (size_t)b * LP_CH * top_n * sizeof(uint64_t); }
size_t logprob_table_bytes_ex(int b, int tp, int top_n, int n_score) { return (size_t)tp * b * (LP_TS + lp_xslot(top_n, n_score)) * 4 + 16; }

int launch_logprob(const LogprobArgs& a, hipStream_t s) {
  OM_CHECK(a.raw && a.ids && a.ws && a.rec && a.cnt && a.b >= 1 && a.V >= 1 && a.max_new >= 1 && a.rec_ld >= a.b, "launch_logprob: bad argument");
  OM_CHECK(a.tp == 1 || (a.xchg && a.table), "log-probabilities under tensor parallelism need the exchange");
  const bool ex = a.top_n > 0 || a.n_score > 0;
  if (ex) {
    OM_CHECK(a.top_n >= 0 && a.top_n <= LP_MAX_TOP && a.n_score >= 0 && a.n_score <= LP_MAX_SCORED, "launch_logprob: top_n <= 20, n_score <= 32");
    OM_CHECK((int64_t)a.top_n <= (int64_t)a.V * a.tp, "launch_logprob: top_n exceeds the vocabulary");
    OM_CHECK((!a.top_n || (a.top_ws && a.top_vals && a.top_ids)) && (!a.n_score || (a.score_ids && a.scored)), "launch_logprob: extras without their buffers");
    OM_CHECK(a.tp == 1 || (int64_t)a.V * a.tp < (1 << 24), "launch_logprob: ids cross the exchange as fp32 (vocabulary < 2^24)");
  }
  const bool pen = a.seen && a.penalty != 1.f;
  const bool two = a.proc != a.raw || a.ban || pen || a.temperature != 1.f || a.thr || a.thr_hi || a.top1;
  LpK k;
  k.raw = a.raw; k.raw_ld = a.raw_ld; k.proc = a.proc ? a.proc : a.raw; k.proc_ld = a.proc ? a.proc_ld : a.raw_ld; k.V = a.V;
  k.ban = a.ban; k.seen = pen ? a.seen : nullptr; k.bmw = a.bm_words; k.last = a.last_set;
  k.pen = a.penalty; k.T = a.temperature; k.thr = a.thr; k.thr_hi = a.thr_hi; k.thr_stride = a.thr_stride; k.top1 = a.top1;
  float4* part = (float4*)a.ws;
  if (two) hipLaunchKernelGGL(lp_partial_kernel<1>, dim3(LP_CH, a.b), dim3(256), 0, s, k, part);
  else hipLaunchKernelGGL(lp_partial_kernel<0>, dim3(LP_CH, a.b), dim3(256), 0, s, k, part);
  const size_t words = (size_t)a.tp * a.b * (LP_TS + (ex ? lp_xslot(a.top_n, a.n_score) : 0));
  if (a.tp > 1) OM_HIP(hipMemsetAsync(a.table, 0, words * 4, s));
  LpX x;
  x.top_n = a.top_n; x.n_score = a.n_score; x.sid = a.score_ids; x.cand = (const uint64_t*)a.top_ws;
  x.top_v = a.top_vals; x.top_i = a.top_ids; x.sc = a.scored;
  if (!ex) {
    hipLaunchKernelGGL(lp_finish_kernel, dim3(a.b), dim3(64), 0, s, k, part, a.ids, a.rank * a.V, (int)two, a.b, a.tp, a.rank, a.table, a.rec, a.cnt,
                       a.max_new, a.rec_ld);
  } else {
    if (a.top_n) hipLaunchKernelGGL(lp_top_slice_kernel, dim3(LP_CH, a.b), dim3(256), 0, s, a.raw, a.raw_ld, a.V, a.rank * a.V, a.top_n, (uint64_t*)a.top_ws);
    hipLaunchKernelGGL(lp_finish_ex_kernel, dim3(a.b), dim3(64), 0, s, k, part, a.ids, a.rank * a.V, (int)two, a.b, a.tp, a.rank, a.table, a.rec,
                       a.cnt, a.max_new, a.rec_ld, x);
  }
  if (a.tp > 1) {
    OM_LAUNCH_CHECK();
    if (int rc = a.xchg(a.xchg_user, a.table, words, s)) return rc;
    if (!ex) hipLaunchKernelGGL(lp_tp_fold_kernel, dim3(1), dim3(64 > a.b ? 64 : a.b), 0, s, a.table, a.b, a.tp, a.top1, a.rec, a.cnt, a.max_new, a.rec_ld);
    else hipLaunchKernelGGL(lp_tp_fold_ex_kernel, dim3(a.b), dim3(64), 0, s, a.table, a.b, a.tp, a.top1, a.rec, a.cnt, a.max_new, a.rec_ld, x);
  }
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_logprob_rewind(int* cnt, int b, int n, hipStream_t s) {
  hipLaunchKernelGGL(lp_rewind_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, cnt, b, n);
  OM_LAUNCH_CHECK();
  return 0;
}
