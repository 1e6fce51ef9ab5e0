// Beam search on the device for generate(num_beams=N): HF's _beam_search step -- log_softmax, accumulated scores,
// top (max(2, 1 + n_eos) * N) continuations over N x V, finished set with the length penalty and the early-stop heuristic -- without a sort
// of the vocabulary and without a host sync per step.  tests/beam_ref.py is the CPU restatement.
//
// One pass over the logits (beam_select_kernel, one workgroup per (row, vocabulary slice)): the slice's max, the fixed-point sum of
// exp(x - max) (integers, so the sum does not depend on order) and the slice's top K raw (value, global index) pairs.  The vocabulary is cut
// into the same slices at every TP degree (beam_slices), so a rank owns whole slices and the exchange table -- zero-filled, every rank
// writes its own slices, one fp32 all-reduce -- holds the same numbers as a TP = 1 run.  x -> fl(fl(x - max) - lse) + r is monotone in
// x within a row, so the prompt's top K accumulated candidates are inside the union of the rows' top K raw logits.  That argument holds for
// the plain search only.  With omchat_beam_processors a ban removes candidates and the repetition penalty moves the seen ids, so the
// selection runs on the processed log-probabilities themselves: a statistics launch (SEL_STATS) leaves the slices' maxima and sums in the
// table, the selection launch (SEL_PROC) recomputes the row's max and lse from them -- every workgroup of a row the same numbers, in slice
// order -- applies penalty and ban in registers from two bitmaps (constrain.hip's ban pass builds both from the row's own path history) and
// keeps the top K (lp, index) pairs; beam_finish_kernel then takes the table's values as log-probabilities (BeamFinishArgs::proc).
// fl(lp + r) is monotone in lp, so the same union argument holds for the processed values.  The histories follow the backpointers in
// beam_hist_move_kernel, which also clears the two bitmaps (a vocabulary slice does not own whole bitmap words, so no reader can).
//
// beam_finish_kernel (one workgroup per prompt) merges the slices, scores the candidates in HF's order of fp32 operations and updates the
// running beams, the finished set and the per-prompt done flag.  A done prompt is frozen: later steps leave its state alone.
// launch_kv_gather moves KV-cache rows (16-bit cache, and the e4m3 replica with its scales) between sequences.
#include "ctx.h"
#include <math.h>
#include <string.h>
#include <algorithm>

// no fused multiply-adds: the fp64 lse sum and every fp32 score are rounded after each operation, as tests/beam_ref.py rounds them
#pragma clang fp contract(off)

namespace {

constexpr int SEL_THREADS = 512;
constexpr int SEL_PER = BEAM_SLICE_CAP / SEL_THREADS;     // logits per thread, held in registers between the three reductions
constexpr double BEAM_FIX = 4294967296.0;                 // exp(x - max) in units of 2^-32
constexpr float NEG = -1.0e9f;                            // HF's mask constant
constexpr int FIN_THREADS = 256;

__device__ __forceinline__ bool beats(float v, int g, float v2, int g2) { return v > v2 || (v == v2 && g < g2); }

// ---------------------------------------------------------------------------------------------------------------- select
// a row's max and log-sum-exp from its ns table entries: the slices' sums rebased to the row max in fp64, in slice order
__device__ __forceinline__ void row_lse(const float* tr, int ns, int K, float& M_out, float& L_out) {
  float M = -INFINITY;
  for (int s = 0; s < ns; ++s) M = fmaxf(M, tr[s * (4 + 2 * K)]);
  double S = 0.0;
  for (int s = 0; s < ns; ++s) {
    const float* e = tr + s * (4 + 2 * K);
    const unsigned long long q = (unsigned long long)e[1] + ((unsigned long long)e[2] << 21) + ((unsigned long long)e[3] << 42);
    S += ldexp((double)q, -32) * exp((double)e[0] - (double)M);
  }
  M_out = M;
  L_out = (float)log(S);
}

// SEL_PLAIN: statistics and the top K raw logits (the plain search, every TP degree); SEL_STATS: the statistics alone; SEL_PROC: the top K
// processed log-probabilities, from a table that holds the statistics of every slice of the row (TP = 1)
enum { SEL_PLAIN = 0, SEL_STATS = 1, SEL_PROC = 2 };
struct SelProc { const uint32_t* ban = nullptr; const uint32_t* seen = nullptr; int bmw = 0; float penalty = 1.f; };

// grid (slices of this rank, rows); table row: [ns][4 + 2K] fp32 = max, three 21-bit limbs of the fixed-point sum, K x (value, global index)
template <int MODE>
__global__ __launch_bounds__(SEL_THREADS) void beam_select_kernel(const float* logits, int ld, int sl, int s0, int gbase, int ns, int K,
                                                                  float* table, SelProc pr) {
  const int row = blockIdx.y, sloc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* x = logits + (size_t)row * ld + (size_t)sloc * sl;
  __shared__ float red_v[SEL_THREADS / 64];
  __shared__ int red_i[SEL_THREADS / 64];
  __shared__ unsigned long long red_s[SEL_THREADS / 64];
  __shared__ int winner;
  float v[SEL_PER];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k) {
    const int i = k * SEL_THREADS + tid;
    v[k] = i < sl ? x[i] : -INFINITY;
    m = fmaxf(m, v[k]);
  }
  float* out = table + (size_t)row * ns * (4 + 2 * K) + (size_t)(s0 + sloc) * (4 + 2 * K);
  if (MODE != SEL_PROC) {
    m = wave_max(m);
    if (lane == 0) red_v[wid] = m;
    __syncthreads();
    m = red_v[0];
#pragma unroll
    for (int w = 1; w < SEL_THREADS / 64; ++w) m = fmaxf(m, red_v[w]);
    // fixed-point sum: terms below 2^-33 of the max round to 0 and are skipped
    unsigned long long acc = 0;
#pragma unroll
    for (int k = 0; k < SEL_PER; ++k) {
      const double d = (double)v[k] - (double)m;
      if (d >= -23.0) acc += (unsigned long long)llrint(exp(d) * BEAM_FIX);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) red_s[wid] = acc;
    __syncthreads();
    if (tid == 0) {
      unsigned long long s = 0;
      for (int w = 0; w < SEL_THREADS / 64; ++w) s += red_s[w];
      out[0] = m;
      out[1] = (float)(s & 0x1FFFFFull);
      out[2] = (float)((s >> 21) & 0x1FFFFFull);
      out[3] = (float)(s >> 42);
    }
    if (MODE == SEL_STATS) return;
  } else {
    // HF's order: log_softmax, RepetitionPenaltyLogitsProcessor on the log-probabilities, then the bans
    __shared__ float s_ml[2];
    if (tid == 0) row_lse(table + (size_t)row * ns * (4 + 2 * K), ns, K, s_ml[0], s_ml[1]);
    __syncthreads();
    const float M = s_ml[0], L = s_ml[1];
    const uint32_t* bb = pr.ban + (size_t)row * pr.bmw;
    const uint32_t* sb = pr.seen ? pr.seen + (size_t)row * pr.bmw : nullptr;
#pragma unroll
    for (int k = 0; k < SEL_PER; ++k) {
      const int i = k * SEL_THREADS + tid;
      if (i >= sl) continue;
      const int g = gbase + sloc * sl + i;      // < bmw * 32 (launch_beam_select_processed)
      const uint32_t bit = 1u << (g & 31);
      float lp = __fsub_rn(__fsub_rn(v[k], M), L);
      if (sb && (sb[g >> 5] & bit)) lp = lp < 0.f ? __fmul_rn(lp, pr.penalty) : __fdiv_rn(lp, pr.penalty);
      if (bb[g >> 5] & bit) lp = -INFINITY;
      v[k] = lp;
    }
  }
  // top K by (value desc, index asc): K rounds of a block argmax over every thread's best remaining element
  float bv = -INFINITY; int bk = -1;
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k)
    if (v[k] > bv) { bv = v[k]; bk = k; }      // strict: the lowest k (lowest index) wins a tie
  for (int r = 0; r < K; ++r) {
    float wv = bv; int wi = bk >= 0 ? bk * SEL_THREADS + tid : 0x7FFFFFFF;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64); const int oi = __shfl_xor(wi, o, 64);
      if (beats(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    }
    if (lane == 0) { red_v[wid] = wv; red_i[wid] = wi; }
    __syncthreads();
    if (tid == 0) {
      float gv = red_v[0]; int gi = red_i[0];
      for (int w = 1; w < SEL_THREADS / 64; ++w)
        if (beats(red_v[w], red_i[w], gv, gi)) { gv = red_v[w]; gi = red_i[w]; }
      const bool ok = gi != 0x7FFFFFFF && gv != -INFINITY;
      out[4 + 2 * r] = ok ? gv : -INFINITY;
      out[5 + 2 * r] = ok ? (float)(gbase + sloc * sl + gi) : -1.f;
      winner = ok ? gi : -1;
    }
    __syncthreads();
    const int w = winner;
    if (w >= 0 && (w % SEL_THREADS) == tid) {
      const int kk = w / SEL_THREADS;
      bv = -INFINITY; bk = -1;
#pragma unroll
      for (int k = 0; k < SEL_PER; ++k) {
        if (k == kk) v[k] = -INFINITY;
        if (v[k] > bv) { bv = v[k]; bk = k; }
      }
    }
    __syncthreads();      // red_v / red_i / winner are reused by the next round
  }
}

// ---------------------------------------------------------------------------------------------------------------- finish
__device__ __forceinline__ float ld_f(const int* p) { return __int_as_float(*p); }
__device__ __forceinline__ void st_f(int* p, float v) { *p = __float_as_int(v); }

__global__ __launch_bounds__(FIN_THREADS) void beam_finish_kernel(BeamFinishArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int N = a.N, K = a.K, KB = a.KB, ns = a.ns, b = a.b, t = a.t;
  const int bN = b * N;
  const int rows_pp = t == 0 ? 1 : N;
  const int rbase = t == 0 ? i : i * N;
  const int TS = ns * (4 + 2 * K);
  const bool last = t + 1 >= a.max_new;
  int* st = a.state;
  int* run = st + BST_RUN * bN;
  int* fsc = st + BST_FSC * bN;
  int* ffl = st + BST_FFL * bN;
  int* fstp = st + BST_FSTEP * bN;
  int* fpa = st + BST_FPAR * bN;
  int* ftk = st + BST_FTOK * bN;
  int* unsat_w = st + 6 * bN;
  int* done_w = unsat_w + b;
  int* bp = done_w + b + (size_t)t * bN * 2;
  int* ctr = st + beam_state_words(b, N, a.max_new) - 2;     // [0] prompts done, [1] ticket of the last workgroup

  __shared__ float sM[BEAM_NMAX], sL[BEAM_NMAX];
  __shared__ float sv_acc[BEAM_NMAX * BEAM_KMAX], sv_raw[BEAM_NMAX * BEAM_KMAX];
  __shared__ int sv_g[BEAM_NMAX * BEAM_KMAX];
  __shared__ float c_acc[BEAM_KMAX], c_raw[BEAM_KMAX], c_trl[BEAM_KMAX], c_s[BEAM_KMAX];
  __shared__ int c_row[BEAM_KMAX], c_tok[BEAM_KMAX], c_hit[BEAM_KMAX];
  __shared__ float o_sc[BEAM_NMAX]; __shared__ int o_fl[BEAM_NMAX], o_st[BEAM_NMAX], o_pa[BEAM_NMAX], o_tk[BEAM_NMAX];
  __shared__ int new_run[BEAM_NMAX], new_fin[BEAM_NMAX];
  __shared__ int s_unsat, s_done_old;

  if (tid == 0) {
    s_unsat = t == 0 ? 1 : unsat_w[i];
    s_done_old = t == 0 ? 0 : done_w[i];
  }
  if (tid < N) {      // the finished set before this step (HF's initial one at step 0)
    const int r = i * N + tid;
    o_sc[tid] = t == 0 ? NEG : ld_f(fsc + r);
    o_fl[tid] = t == 0 ? 0 : ffl[r];
    o_st[tid] = t == 0 ? -1 : fstp[r];
    o_pa[tid] = t == 0 ? 0 : fpa[r];
    o_tk[tid] = t == 0 ? 0 : ftk[r];
    new_run[tid] = 0; new_fin[tid] = 0;      // (ranks form a permutation; this only keeps NaN logits inside the arrays)
  }
  __syncthreads();
  const bool frozen = s_done_old != 0;
  if (!frozen) {
    // lse of every row: the slices' sums rebased to the row max in fp64, in slice order
    // (a.proc: the selection pass has applied it already, the table's values are log-probabilities)
    if (tid < rows_pp && !a.proc) row_lse(a.table + (size_t)(rbase + tid) * TS, ns, K, sM[tid], sL[tid]);
    __syncthreads();
    // a row with fewer than K finite values leaves survivor slots unwritten: they start as -inf with distinct out-of-vocabulary ids, so
    // the ranking below stays a permutation.  Such a row is outside the contract: model logits are finite, and omchat_beam_processors
    // refuses lists and lengths whose bans could leave a row fewer than K of them.  Under a.proc an id of such a slot is fed as 0.
    for (int e = tid; e < rows_pp * K; e += FIN_THREADS) { sv_acc[e] = -INFINITY; sv_raw[e] = -INFINITY; sv_g[e] = a.V_total + e; }
    __syncthreads();
    // each row's top K over its slices' sorted lists: rank = position in its own list + entries of the other lists that beat it
    const int ncand = rows_pp * ns * K;
    for (int c = tid; c < ncand; c += FIN_THREADS) {
      const int j = c / (ns * K), s = (c / K) % ns, p = c % K;
      const float* tr = a.table + (size_t)(rbase + j) * TS;
      const float v = tr[s * (4 + 2 * K) + 4 + 2 * p];
      const int g = (int)tr[s * (4 + 2 * K) + 5 + 2 * p];
      if (g < 0) continue;
      int rank = p;
      for (int s2 = 0; s2 < ns && rank < K; ++s2) {
        if (s2 == s) continue;
        const float* l2 = tr + s2 * (4 + 2 * K) + 4;
        for (int q = 0; q < K; ++q) {
          const int g2 = (int)l2[2 * q + 1];
          if (g2 < 0 || !beats(l2[2 * q], g2, v, g)) break;
          ++rank;
        }
      }
      if (rank < K) {
        const float r0 = t == 0 ? 0.f : ld_f(run + i * N + j);
        // HF: log_softmax = (x - max) - log(sum), then + running score, all fp32
        const float lp = a.proc ? v : __fsub_rn(__fsub_rn(v, sM[j]), sL[j]);
        sv_acc[j * K + rank] = __fadd_rn(lp, r0);
        sv_raw[j * K + rank] = v;
        sv_g[j * K + rank] = g;
      }
    }
    __syncthreads();
    // the prompt's top KB by (accumulated desc, raw desc, flat index asc)
    for (int e = tid; e < rows_pp * K; e += FIN_THREADS) {
      const float ea = sv_acc[e], er = sv_raw[e];
      const int ej = e / K, eg = sv_g[e];
      int rank = 0;
      for (int f = 0; f < rows_pp * K; ++f) {
        const float fa = sv_acc[f], fr = sv_raw[f];
        const int fj = f / K, fg = sv_g[f];
        rank += fa > ea || (fa == ea && (fr > er || (fr == er && (fj < ej || (fj == ej && fg < eg)))));
      }
      if (rank < KB) { c_acc[rank] = ea; c_raw[rank] = er; c_row[rank] = ej; c_tok[rank] = eg; }
    }
    __syncthreads();
    const bool full = a.es == 1 && [&] { for (int j = 0; j < N; ++j) if (!o_fl[j]) return false; return true; }();
    if (tid < KB) {
      bool hit = last;
      for (int q = 0; q < a.n_eos; ++q) hit = hit || c_tok[tid] == a.eos[q];
      c_hit[tid] = hit;
      c_trl[tid] = hit ? __fadd_rn(c_acc[tid], NEG) : c_acc[tid];
      // _update_finished_beams: / generated_len ** length_penalty, then the three -1e9 masks in HF's order
      float s = __fdiv_rn(c_acc[tid], a.dn[t + 1]);
      if (full) s = __fadd_rn(s, NEG);
      if (!s_unsat) s = __fadd_rn(s, NEG);
      if (!(hit && tid < N)) s = __fadd_rn(s, NEG);
      c_s[tid] = s;
    }
    __syncthreads();
    if (tid < KB) {       // the best N non-finished continuations (ties: lower position first)
      int rank = 0;
      for (int k = 0; k < KB; ++k) rank += c_trl[k] > c_trl[tid] || (c_trl[k] == c_trl[tid] && k < tid);
      if (rank < N) new_run[rank] = tid;
    }
    if (tid < N + KB) {   // merge [old finished | this step's candidates], keep the best N
      const float val = tid < N ? o_sc[tid] : c_s[tid - N];
      int rank = 0;
      for (int e = 0; e < N + KB; ++e) {
        const float ov = e < N ? o_sc[e] : c_s[e - N];
        rank += ov > val || (ov == val && e < tid);
      }
      if (rank < N) new_fin[rank] = tid;
    }
    __syncthreads();
    if (tid < N) {
      const int r = i * N + tid, k = new_run[tid];
      st_f(run + r, c_trl[k]);
      a.tokens[r] = a.proc && c_tok[k] >= a.V_total ? 0 : c_tok[k];
      a.parents[r] = t == 0 ? r : i * N + c_row[k];
      bp[2 * r] = c_row[k]; bp[2 * r + 1] = c_tok[k];
      const int e = new_fin[tid];
      if (e < N) {
        st_f(fsc + r, o_sc[e]); ffl[r] = o_fl[e]; fstp[r] = o_st[e]; fpa[r] = o_pa[e]; ftk[r] = o_tk[e];
      } else {
        const int q = e - N;
        st_f(fsc + r, c_s[q]); ffl[r] = c_hit[q] && q < N; fstp[r] = t; fpa[r] = c_row[q]; ftk[r] = c_tok[q];
      }
    }
    __syncthreads();
    if (tid == 0) {
      // _check_early_stop_heuristic on the new running scores and finished set
      const float hd = (a.es == 2 && a.lp_pos) ? a.dn[a.max_new] : a.dn[t + 1];
      const float best = __fdiv_rn(c_trl[new_run[0]], hd);
      float mn = INFINITY; bool all_fin = true;
      for (int j = 0; j < N; ++j) { mn = fminf(mn, ld_f(fsc + i * N + j)); all_fin = all_fin && ffl[i * N + j]; }
      bool any = false;
      for (int j = 0; j < N; ++j) any = any || best > (ffl[i * N + j] ? mn : NEG);
      const int unsat = s_unsat && any;
      const int done = !unsat || (a.es == 1 && all_fin) || last;
      unsat_w[i] = unsat;
      done_w[i] = done;
      if (done) atomicAdd(ctr, 1);
    }
  } else if (tid < N) {   // frozen: every row keeps its cache (parent = itself); the fed token is never read back
    const int r = i * N + tid;
    a.tokens[r] = 0;
    a.parents[r] = r;
    bp[2 * r] = tid; bp[2 * r + 1] = 0;
  }
  if (tid == 0) {
    // the last workgroup of the step publishes "every prompt done"
    __threadfence();
    const int ticket = atomicAdd(ctr + 1, 1);
    if ((ticket + 1) % b == 0) {
      __threadfence();
      const int n = atomicAdd(ctr, 0);
      if (a.done_word) *a.done_word = n >= b ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- KV gather
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void copy_nt(char* dst, const char* src, int n16) {
  const u32x4* s = (const u32x4*)src;
  u32x4* d = (u32x4*)dst;
  for (int i = threadIdx.x; i < n16; i += blockDim.x) __builtin_nontemporal_store(__builtin_nontemporal_load(s + i), d + i);
}
__device__ __forceinline__ void copy_f32(float* dst, const float* src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// phase 0: rows [row0, row0 + nrows) <- fork_src (parents == nullptr) or <- parents[r], straight from the cache (no row is both read and
// written); phase 1: rows that are both a destination and some other row's parent -> stash; phase 2: every destination <- its parent,
// from the stash when the parent is itself a destination
__global__ __launch_bounds__(256) void kv_gather_kernel(KvGatherArgs a, const int* parents, int row0, int nrows, int fork_src, int lo, int hi,
                                                        int phase) {
  const int r = row0 + blockIdx.x, h = blockIdx.y, l = blockIdx.z;
  int src_row, dst_row;
  bool from_stash = false, to_stash = false;
  if (phase == 1) {
    if (parents[r] == r) return;
    bool needed = false;
    for (int q = row0; q < row0 + nrows; ++q) needed = needed || (q != r && parents[q] == r);
    if (!needed) return;
    src_row = r; dst_row = r; to_stash = true;
  } else {
    const int p = parents ? parents[r] : fork_src;
    if (p == r) return;
    src_row = p; dst_row = r;
    from_stash = phase == 2 && parents[p] != p;
  }
  const int n = hi - lo;
  const int64_t c_src = (((int64_t)l * a.rows_cap + src_row) * a.kvh + h) * a.max_seq + lo;      // slot index in the cache
  const int64_t c_dst = (((int64_t)l * a.rows_cap + dst_row) * a.kvh + h) * a.max_seq + lo;
  const int64_t s_idx = (((int64_t)l * a.st_rows + (to_stash ? dst_row : src_row)) * a.kvh + h) * a.st_slots;      // slot index in the stash
  const int64_t src = from_stash ? s_idx : c_src, dst = to_stash ? s_idx : c_dst;
  const char* k_src = from_stash ? a.sk : a.k;  char* k_dst = to_stash ? a.sk : a.k;
  const char* v_src = from_stash ? a.sv : a.v;  char* v_dst = to_stash ? a.sv : a.v;
  copy_nt(k_dst + dst * 256, k_src + src * 256, n * 16);
  copy_nt(v_dst + dst * 256, v_src + src * 256, n * 16);
  if (a.k8) {
    const char* k8s = from_stash ? a.sk8 : a.k8;  char* k8d = to_stash ? a.sk8 : a.k8;
    const char* v8s = from_stash ? a.sv8 : a.v8;  char* v8d = to_stash ? a.sv8 : a.v8;
    copy_nt(k8d + dst * 128, k8s + src * 128, n * 8);
    copy_nt(v8d + dst * 128, v8s + src * 128, n * 8);
    copy_f32((to_stash ? a.sks : a.ks) + dst, (from_stash ? a.sks : a.ks) + src, n);
    copy_f32((to_stash ? a.svs : a.vs) + dst, (from_stash ? a.svs : a.vs) + src, n);
  }
}

// ---------------------------------------------------------------------------------------------------------------- path histories
constexpr int HM_CLEAR = 64;      // workgroups behind the row ones that zero the bitmaps

// workgroups [0, rows): row r of dst takes its parent's generated ids and the token it was just given; the others zero bm[0, bm_words)
__global__ __launch_bounds__(256) void beam_hist_move_kernel(const int32_t* src, int32_t* dst, int rows, int N, int ld, int P, int g,
                                                             const int* parents, const int* tokens, int* len, uint32_t* bm, size_t bm_words) {
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= rows) {
    for (size_t i = (size_t)(r - rows) * 256 + tid; i < bm_words; i += (size_t)HM_CLEAR * 256) bm[i] = 0u;
    return;
  }
  int p = parents[r];
  if (p < r / N * N || p >= r / N * N + N) p = r;      // (never, behind beam_finish_kernel: no read outside the prompt's rows)
  const int32_t* s = src + (size_t)p * ld + P;
  int32_t* d = dst + (size_t)r * ld + P;
  for (int i = tid; i < g; i += 256) d[i] = s[i];
  if (tid == 0) { d[g] = tokens[r]; len[r] = P + g + 1; }
}

}  // namespace

int launch_beam_stats(const float* logits, int ld, int rows, int V, int ns, int K, float* table, hipStream_t s) {
  OM_CHECK(ns >= 1 && K >= 1 && K <= BEAM_KMAX && rows >= 1 && V % ns == 0 && V / ns <= BEAM_SLICE_CAP, "beam statistics: bad geometry");
  hipLaunchKernelGGL(beam_select_kernel<SEL_STATS>, dim3(ns, rows), dim3(SEL_THREADS), 0, s, logits, ld, V / ns, 0, 0, ns, K, table, SelProc{});
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_beam_select_processed(const float* logits, int ld, int rows, int V, int ns, int K, float* table, const uint32_t* ban,
                                 const uint32_t* seen, int bmw, float penalty, hipStream_t s) {
  OM_CHECK(ns >= 1 && K >= 1 && K <= BEAM_KMAX && rows >= 1 && V % ns == 0 && V / ns <= BEAM_SLICE_CAP, "beam select: bad geometry");
  OM_CHECK(ban && (int64_t)bmw * 32 >= V && penalty > 0.f && isfinite(penalty), "beam select: bitmaps narrower than the vocabulary, or penalty <= 0");
  SelProc pr;
  pr.ban = ban; pr.seen = seen; pr.bmw = bmw; pr.penalty = penalty;
  hipLaunchKernelGGL(beam_select_kernel<SEL_PROC>, dim3(ns, rows), dim3(SEL_THREADS), 0, s, logits, ld, V / ns, 0, 0, ns, K, table, pr);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_beam_hist_move(const int32_t* src, int32_t* dst, int rows, int N, int ld, int P, int g, const int* parents, const int* tokens, int* len,
                          uint32_t* bm, size_t bm_words, hipStream_t s) {
  OM_CHECK(rows >= 0 && N >= 1 && (rows == 0 || (src && dst && src != dst && parents && tokens && len && P >= 0 && g >= 0 && P + g + 1 <= ld)),
           "beam history: no room for one more id, or a null buffer");
  OM_CHECK(bm || bm_words == 0, "beam history: null bitmaps");
  hipLaunchKernelGGL(beam_hist_move_kernel, dim3(rows + HM_CLEAR), dim3(256), 0, s, src, dst, rows, N, ld, P, g, parents, tokens, len, bm, bm_words);
  OM_LAUNCH_CHECK();
  return 0;
}

int beam_slices(int V_total, int tp) {
  if (V_total < 1 || tp < 1) return -1;
  for (int n = 1; n <= V_total && n <= BEAM_NS_MAX; ++n) {
    if (V_total % n || V_total / n > BEAM_SLICE_CAP) continue;
    if (V_total % 8 == 0 ? n % 8 != 0 : n % tp != 0) continue;
    if (n % tp) continue;
    return n;
  }
  return -1;
}

int launch_beam_select(const float* logits, int ld, int rows, int V_local, int rank, int tp, int ns, int K, float* table, hipStream_t s) {
  OM_CHECK(ns >= 1 && ns % tp == 0 && K >= 1 && K <= BEAM_KMAX && rows >= 1, "beam select: bad geometry");
  const int nl = ns / tp, sl = V_local / nl;
  OM_CHECK(sl * nl == V_local && sl <= BEAM_SLICE_CAP, "beam select: the rank's vocabulary is not whole slices");
  hipLaunchKernelGGL(beam_select_kernel<SEL_PLAIN>, dim3(nl, rows), dim3(SEL_THREADS), 0, s, logits, ld, sl, rank * nl, rank * V_local, ns, K, table,
                     SelProc{});
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_beam_finish(const BeamFinishArgs& a, hipStream_t s) {
  OM_CHECK(a.b >= 1 && a.N >= 1 && a.N <= BEAM_NMAX && a.KB <= BEAM_KMAX && a.K == a.KB && a.n_eos <= BEAM_EOS_MAX &&
           a.ns <= BEAM_NS_MAX && a.t >= 0 && a.t < a.max_new, "beam finish: bad geometry");
  if (a.t == 0) OM_HIP(hipMemsetAsync(a.state + beam_state_words(a.b, a.N, a.max_new) - 2, 0, 8, s));
  hipLaunchKernelGGL(beam_finish_kernel, dim3(a.b), dim3(FIN_THREADS), 0, s, a);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_kv_gather(const KvGatherArgs& a, const int* parents, int row0, int nrows, int fork_src, int lo, int hi, hipStream_t s) {
  OM_CHECK(row0 >= 0 && nrows >= 1 && row0 + nrows <= a.rows_cap && lo >= 0 && hi <= a.max_seq, "kv gather: rows / slots out of range");
  if (hi <= lo) return 0;
  if (!parents) {
    OM_CHECK(fork_src >= 0 && fork_src < a.rows_cap, "kv gather: fork source out of range");
    hipLaunchKernelGGL(kv_gather_kernel, dim3(nrows, a.kvh, a.layers), dim3(256), 0, s, a, parents, row0, nrows, fork_src, lo, hi, 0);
    OM_LAUNCH_CHECK();
    return 0;
  }
  OM_CHECK(a.sk && a.sv && row0 + nrows <= a.st_rows && hi - lo <= a.st_slots && (!a.k8 || (a.sk8 && a.sv8 && a.sks && a.svs)),
           "kv gather: stash too small");
  hipLaunchKernelGGL(kv_gather_kernel, dim3(nrows, a.kvh, a.layers), dim3(256), 0, s, a, parents, row0, nrows, -1, lo, hi, 1);
  hipLaunchKernelGGL(kv_gather_kernel, dim3(nrows, a.kvh, a.layers), dim3(256), 0, s, a, parents, row0, nrows, -1, lo, hi, 2);
  OM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// context entry points (include/omchat_hip.h): the search state (BeamState, ctx.h) lives on the device
// ---------------------------------------------------------------------------------------------------------
static KvGatherArgs beam_kv_args(omchat_ctx* ctx, bool with_stash) {
  const omchat_config& c = ctx->c;
  KvGatherArgs g;
  g.k = (char*)ctx->kcache; g.v = (char*)ctx->vcache;
  g.layers = c.t_layers; g.kvh = c.t_kv_heads; g.max_seq = c.max_seq; g.rows_cap = c.max_batch;
  const bool f8 = ctx->fp8_kv && ctx->kv8_valid;
  if (f8) { g.k8 = (char*)ctx->k8cache; g.v8 = (char*)ctx->v8cache; g.ks = ctx->ks8; g.vs = ctx->vs8; }
  if (with_stash) {
    const int rows = ctx->beam.cur.b * ctx->beam.cur.N;
    const size_t slots = (size_t)c.t_layers * rows * c.t_kv_heads * ctx->beam.cur.max_new;
    char* p = (char*)ctx->beam.stash.p;
    g.sk = p; g.sv = p + slots * 256;
    if (f8 && ctx->beam.stash8) {
      g.sk8 = p + slots * 512; g.sv8 = p + slots * 640;
      g.sks = (float*)(p + slots * 768); g.svs = (float*)(p + slots * 772);
    }
    g.st_rows = rows; g.st_slots = ctx->beam.cur.max_new;
  }
  return g;
}

extern "C" int omchat_beam_begin(omchat_ctx* ctx, int b, int num_beams, float length_penalty, int early_stopping, const int32_t* eos_ids,
                                 int n_eos, int max_new, int prompt_tok_len, void* stream) {
  OM_CHECK(ctx, "null ctx");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  const int N = num_beams;
  OM_CHECK(b >= 1 && N >= 2 && N <= BEAM_NMAX, "beam search: b >= 1 and 2 <= num_beams <= 16");
  OM_CHECK(!ctx->pick.constraints_on(), "beam search: constraints are on (omchat_set_constraints with b = 0 first); HF applies them to log-softmax scores there");
  OM_CHECK(!ctx->pick.logprobs_on(), "beam search: logprobs are on (omchat_set_logprobs with b = 0 first); a beam search reports sequences_scores");
  OM_CHECK(!ctx->pick.fsm_on(), "beam search: a token FSM is on (omchat_fsm_begin with b = 0 first); each beam row would need its parent's state");
  OM_CHECK(!ctx->pick.guidance_on(), "beam search: guidance is on (omchat_set_guidance with b = 0 first); each beam row would need its twin");
  OM_CHECK(!ctx->pick.dola_on(), "beam search: layer-contrastive decoding is on (omchat_set_dola with b = 0 first); each beam row would need its candidate rows");
  OM_CHECK(!ctx->contrastive_on(), "beam search: contrastive search is on (omchat_set_contrastive with k = 0 first); its k rows are one sequence's candidates");
  OM_CHECK(b * N <= c.max_batch, "beam search: b * num_beams exceeds max_batch");
  OM_CHECK(n_eos >= 0 && n_eos <= BEAM_EOS_MAX && (n_eos == 0 || eos_ids), "beam search: at most 8 eos ids");
  const int KB = std::max(2, 1 + n_eos) * N;
  OM_CHECK(KB <= BEAM_KMAX, "beam search: max(2, 1 + n_eos) * num_beams must not exceed 32");
  OM_CHECK(early_stopping >= 0 && early_stopping <= 2, "beam search: early_stopping 0 (False), 1 (True) or 2 (never)");
  OM_CHECK(isfinite(length_penalty), "beam search: length_penalty must be finite");
  OM_CHECK(max_new >= 1 && prompt_tok_len >= 1 && prompt_tok_len + max_new - 1 <= c.max_seq, "beam search: prompt + max_new exceed max_seq");
  OM_CHECK(c.t_vocab_total >= KB, "beam search: vocabulary smaller than the candidates kept per step");
  const int ns = beam_slices(c.t_vocab_total, ctx->tp_size);
  OM_CHECK(ns >= 1, "beam search: the vocabulary cannot be cut into equal slices of <= 20480 ids for this TP degree");
  OM_CHECK(!ctx->left_padded && ctx->dec_mode != 2, "beam search: a left-padded or masked-decode batch (pad equal or use b = 1)");
  OM_CHECK(!ctx->group.on(), "beam search: a sampled group shares its prompt (omchat_group_begin with b = 0 first)");
  BeamState::Search& B = ctx->beam.cur;
  B = BeamState::Search{};
  ctx->beam.proc = BeamState::Proc{};
  B.b = b; B.N = N; B.KB = KB; B.max_new = max_new; B.P = prompt_tok_len; B.es = early_stopping; B.ns = ns; B.lp = length_penalty;
  B.eos.assign(eos_ids, eos_ids + n_eos);
  const int rows = b * N;
  const size_t TS = (size_t)ns * (4 + 2 * KB);
  const bool f8 = ctx->fp8_kv && ctx->kv8_valid;
  const size_t slots = (size_t)c.t_layers * rows * c.t_kv_heads * max_new;
  TRY(ctx->grow(ctx->beam.state, beam_state_words(b, N, max_new) * 4));
  TRY(ctx->grow(ctx->beam.table, (rows * TS + 16) * 4));
  TRY(ctx->grow(ctx->beam.dn, (size_t)(max_new + 1) * 4));
  TRY(ctx->grow(ctx->beam.parents, (size_t)rows * 4));
  TRY(ctx->grow(ctx->beam.stash, slots * (f8 ? 776 : 512)));
  ctx->beam.stash8 = f8;
  std::vector<float> dn(max_new + 1, 1.f);      // fp32(pow(g, length_penalty)): the Python float HF divides by, rounded as torch rounds it
  for (int g = 1; g <= max_new; ++g) dn[g] = (float)pow((double)g, (double)length_penalty);
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemcpyAsync(ctx->beam.dn.p, dn.data(), dn.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipStreamSynchronize(s));      // host vector
  B.on = true;
  return 0;
}

// aux layout: [CON_LIST_WORDS id lists | len [b * N] | plen [b * N]]
static ConstrainArgs beam_proc_ban_args(omchat_ctx* ctx, int rows) {
  const BeamState::Search& B = ctx->beam.cur;
  const BeamState::Proc& Q = ctx->beam.proc;
  const int bN = B.b * B.N;
  ConstrainArgs a;
  // step 0 runs on the prompts' own rows: prompt i's history is row i * N of the first buffer
  a.hist = (int32_t*)ctx->beam.hist.p + (size_t)(B.t & 1) * bN * Q.ld;
  a.hist_ld = B.t == 0 ? B.N * Q.ld : Q.ld;
  int32_t* aux = (int32_t*)ctx->beam.aux.p;
  constrain_bind_lists(aux, a);
  a.len = aux + CON_LIST_WORDS; a.plen = aux + CON_LIST_WORDS + bN;
  a.b = rows; a.V = a.V_total = ctx->c.t_vocab_total; a.gbase = 0;
  a.ngram = Q.ngram; a.min_new = Q.min_new; a.min_len = Q.min_len;
  a.n_eos = Q.n_eos; a.n_sup = Q.n_sup; a.n_bsup = Q.n_bsup; a.n_bw = Q.n_bw;
  a.ban = (uint32_t*)ctx->beam.bm.p; a.bmw = Q.bmw;
  a.seen = Q.penalty != 1.f ? a.ban + (size_t)bN * Q.bmw : nullptr;
  return a;
}

extern "C" int omchat_beam_processors(omchat_ctx* ctx, float rep_penalty, int no_repeat_ngram_size, int min_new_tokens, int min_length,
                                      const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress,
                                      const int32_t* bad_word_ids, const int32_t* bad_word_offsets, int n_bad_words, const int32_t* prompt_ids,
                                      int prompt_len, void* stream) {
  OM_CHECK(ctx, "null ctx");
  BeamState::Search& B = ctx->beam.cur;
  const omchat_config& c = ctx->c;
  // every refusal before anything is enqueued or changed
  OM_CHECK(B.on && B.t == 0, "beam processors: valid between omchat_beam_begin and the first omchat_beam_step");
  OM_CHECK(ctx->tp_size == 1, "beam processors: tensor-parallel contexts are not implemented (DESIGN.md section 7): the row's log-sum-exp would need an exchange of its own in front of the selection");
  OM_CHECK(isfinite(rep_penalty) && rep_penalty > 0.f, "beam processors: repetition_penalty must be a finite float > 0");
  OM_CHECK(no_repeat_ngram_size >= 0 && no_repeat_ngram_size <= CON_NGRAM_MAX, "beam processors: 0 <= no_repeat_ngram_size <= 64 (0 = off)");
  OM_CHECK(min_new_tokens >= 0 && min_length >= 0, "beam processors: min_new_tokens and min_length >= 0");
  OM_CHECK(prompt_ids && prompt_len >= 1, "beam processors: the b prompt rows [b][prompt_len], prompt_len >= 1");
  std::vector<int32_t> lists(CON_LIST_WORDS);
  ConstrainArgs la;
  TRY(constrain_pack_lists(B.eos.data(), (int)B.eos.size(), suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_word_ids,
                           bad_word_offsets, n_bad_words, lists.data(), la));
  BeamState::Proc Q;
  Q.penalty = rep_penalty; Q.ngram = no_repeat_ngram_size;
  Q.min_new = la.n_eos ? min_new_tokens : 0; Q.min_len = la.n_eos ? min_length : 0;      // HF: no length processor without an EOS id
  Q.n_eos = la.n_eos; Q.n_sup = la.n_sup; Q.n_bsup = la.n_bsup; Q.n_bw = la.n_bw;
  if (Q.penalty == 1.f && !Q.ngram && !Q.min_new && !Q.min_len && !Q.n_sup && !Q.n_bsup && !Q.n_bw) return 0;      // the plain search
  // the n-gram stage bans at most one id per history position, a bad word at most its last id: every row keeps KB finite scores
  const int64_t can_ban = (int64_t)Q.n_sup + Q.n_bsup + Q.n_bw + Q.n_eos + prompt_len + B.max_new;
  OM_CHECK(c.t_vocab_total - can_ban >= B.KB, "beam processors: the bans could leave a row fewer finite scores than the candidates kept per step");
  const int bN = B.b * B.N;
  Q.P = prompt_len; Q.ld = (prompt_len + B.max_new + 3) / 4 * 4; Q.bmw = (c.t_vocab_total + 31) / 32;
  TRY(ctx->grow(ctx->beam.hist, (size_t)2 * bN * Q.ld * 4));
  TRY(ctx->grow(ctx->beam.aux, ((size_t)CON_LIST_WORDS + 2 * (size_t)bN) * 4));
  TRY(ctx->grow(ctx->beam.bm, (size_t)2 * bN * Q.bmw * 4));
  // the prompt part of every row, in both buffers, written once
  std::vector<int32_t> h((size_t)2 * bN * Q.ld, 0), len((size_t)2 * bN, prompt_len);
  for (int u = 0; u < 2; ++u)
    for (int r = 0; r < bN; ++r)
      std::copy(prompt_ids + (size_t)(r / B.N) * prompt_len, prompt_ids + (size_t)(r / B.N + 1) * prompt_len, h.begin() + ((size_t)u * bN + r) * Q.ld);
  hipStream_t s = (hipStream_t)stream;
  int32_t* aux = (int32_t*)ctx->beam.aux.p;
  OM_HIP(hipMemcpyAsync(ctx->beam.hist.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(aux, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(aux + CON_LIST_WORDS, len.data(), len.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemsetAsync(ctx->beam.bm.p, 0, (size_t)2 * bN * Q.bmw * 4, s));
  OM_HIP(hipStreamSynchronize(s));      // host vectors and the caller's ids
  Q.on = true;
  ctx->beam.proc = Q;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// sampled groups (include/omchat_hip.h: omchat_group_begin)
// ---------------------------------------------------------------------------------------------------------
static const char* group_share_refusal(const omchat_ctx* ctx, int N) {
  const omchat_config& c = ctx->c;
  if (ctx->fp8_kv) return "shared-prompt mode: the e4m3 KV cache is not implemented (DESIGN.md section 7): share = 0, or omchat_enable_fp8_kv(ctx, 0)";
  if (ctx->tp_size != 1) return "shared-prompt mode: tensor-parallel contexts are not implemented (DESIGN.md section 7): share = 0";
  if (c.t_kv_heads < 1 || c.t_heads % c.t_kv_heads) return "shared-prompt mode: q heads must be a multiple of kv heads";
  if (N < 2 || N > VERIFY_MAX_T || N * (c.t_heads / c.t_kv_heads) > 128)
    return "shared-prompt mode: 2 <= N <= 16 and N * (q heads per kv head) <= 128 (the shared attention's query rows): share = 0";
  return nullptr;
}

extern "C" int omchat_group_share_available(omchat_ctx* ctx, int N) { return ctx && ctx->c.t_layers > 0 && !group_share_refusal(ctx, N); }

extern "C" int omchat_group_begin(omchat_ctx* ctx, int b, int N, int prompt_len, int share, void* stream) {
  OM_CHECK(ctx, "null ctx");
  if (b == 0) { ctx->group.end(); return 0; }
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(b >= 1 && N >= 1, "sampled group: b >= 1 prompts, N >= 1 rows each");
  OM_CHECK(!ctx->beam.on(), "sampled group: a beam search is active");
  OM_CHECK(!ctx->pick.guidance_on(), "sampled group: guidance is on (omchat_set_guidance with b = 0 first); each sibling row would need its twin");
  OM_CHECK(!ctx->pick.dola_on(), "sampled group: layer-contrastive decoding is on (omchat_set_dola with b = 0 first); each sibling row would need its candidate rows");
  OM_CHECK(!ctx->contrastive_on() || (!ctx->cs.forked && b == 1 && N == ctx->cs.k), "sampled group: contrastive search is on and forks its own k rows (omchat_set_contrastive with k = 0 first)");
  OM_CHECK(b * N <= c.max_batch, "sampled group: b * N exceeds max_batch");
  OM_CHECK(!ctx->left_padded && ctx->dec_mode != 2, "sampled group: a left-padded or masked-decode batch (pad equal or use b = 1)");
  OM_CHECK(prompt_len >= 1 && prompt_len < c.max_seq, "sampled group: prompt_len outside [1, max_seq)");
  for (int i = 0; i < b; ++i) OM_CHECK(ctx->h_len[i] == prompt_len, "sampled group: rows 0..b-1 must hold exactly prompt_len keys (pad equal or use b = 1)");
  if (share) { const char* why = group_share_refusal(ctx, N); OM_CHECK(!why, why); }
  hipStream_t s = (hipStream_t)stream;
  GroupState& G = ctx->group;
  const int P = prompt_len, bN = b * N;
  // last prompt first: its target rows lie above every source row not yet read.  share: only the group's first row takes the prompt
  const KvGatherArgs g = beam_kv_args(ctx, false);
  for (int i = b - 1; i >= (share ? 1 : 0); --i) TRY(launch_kv_gather(g, nullptr, i * N, share ? 1 : N, i, 0, P, s));
  G.hpos.assign(bN, P);
  G.hlen.assign(bN, P + 1);
  for (int r = 0; r < bN; ++r) ctx->h_len[r] = P;
  OM_HIP(hipMemcpyAsync(ctx->d_pos, G.hpos.data(), (size_t)bN * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(ctx->d_len, G.hlen.data(), (size_t)bN * 4, hipMemcpyHostToDevice, s));
  G.share = share != 0; G.b = b; G.N = N; G.P = P;
  return 0;
}

extern "C" int omchat_beam_step(omchat_ctx* ctx, const float* logits, int rows, int32_t* next_tokens, int32_t* done_word, void* stream) {
  OM_CHECK(ctx && logits && next_tokens, "null argument");
  BeamState::Search& B = ctx->beam.cur;
  OM_CHECK(B.on, "omchat_beam_step without omchat_beam_begin (or after a new prefill)");
  OM_CHECK(B.t < B.max_new, "beam search: max_new steps taken");
  OM_CHECK(rows == (B.t == 0 ? B.b : B.b * B.N), "beam step: rows = b on the prefill logits, b * num_beams afterwards");
  const omchat_config& c = ctx->c;
  hipStream_t s = (hipStream_t)stream;
  const size_t TS = (size_t)B.ns * (4 + 2 * B.KB);
  float* table = (float*)ctx->beam.table.p;
  const BeamState::Proc& Q = ctx->beam.proc;
  if (Q.on) {
    // (B.t < max_new, checked above, is the history's room: row length P + t <= ld - 1 here)
    const ConstrainArgs ca = beam_proc_ban_args(ctx, rows);
    TRY(launch_constrain_ban(ca, s));
    TRY(launch_beam_stats(logits, c.t_vocab, rows, c.t_vocab, B.ns, B.KB, table, s));
    TRY(launch_beam_select_processed(logits, c.t_vocab, rows, c.t_vocab, B.ns, B.KB, table, ca.ban, ca.seen, Q.bmw, Q.penalty, s));
  } else {
    if (ctx->tp_size > 1) OM_HIP(hipMemsetAsync(table, 0, rows * TS * 4, s));
    TRY(launch_beam_select(logits, c.t_vocab, rows, c.t_vocab, ctx->tp_rank, ctx->tp_size, B.ns, B.KB, table, s));
    if (ctx->tp_size > 1) TRY(ctx->allreduce_f32(table, rows * TS, s));
  }
  BeamFinishArgs a;
  a.proc = Q.on;
  a.table = table; a.ns = B.ns; a.K = a.KB = B.KB; a.V_total = c.t_vocab_total;
  a.b = B.b; a.N = B.N; a.t = B.t; a.max_new = B.max_new; a.es = B.es; a.lp_pos = B.lp > 0.f;
  a.dn = (const float*)ctx->beam.dn.p;
  a.n_eos = (int)B.eos.size();
  for (int q = 0; q < a.n_eos; ++q) a.eos[q] = B.eos[q];
  a.state = (int*)ctx->beam.state.p; a.tokens = next_tokens; a.parents = (int*)ctx->beam.parents.p; a.done_word = done_word;
  TRY(launch_beam_finish(a, s));
  const int bN = B.b * B.N;
  if (Q.on) {
    // the next step's histories: row r continues its parent's path with the token it was just given (nothing moves behind the last step);
    // the launch also clears the two bitmaps this step's selection read
    int32_t* h = (int32_t*)ctx->beam.hist.p;
    int32_t* aux = (int32_t*)ctx->beam.aux.p;
    const size_t half = (size_t)bN * Q.ld;
    TRY(launch_beam_hist_move(h + (B.t & 1) * half, h + ((B.t + 1) & 1) * half, B.t + 1 < B.max_new ? bN : 0, B.N, Q.ld, Q.P, B.t, a.parents,
                              next_tokens, aux + CON_LIST_WORDS, (uint32_t*)ctx->beam.bm.p, (size_t)2 * bN * Q.bmw, s));
  }
  if (B.t == 0) {
    // fork: prompt i's row -> rows i*N .. i*N+N-1, last prompt first (its target rows lie above every source row not yet read)
    const KvGatherArgs g = beam_kv_args(ctx, false);
    for (int i = B.b - 1; i >= 0; --i) TRY(launch_kv_gather(g, nullptr, i * B.N, B.N, i, 0, B.P, s));
    ctx->beam.hpos.assign(bN, B.P);
    ctx->beam.hlen.assign(bN, B.P + 1);
    for (int r = 0; r < bN; ++r) ctx->h_len[r] = B.P;
    OM_HIP(hipMemcpyAsync(ctx->d_pos, ctx->beam.hpos.data(), (size_t)bN * 4, hipMemcpyHostToDevice, s));
    OM_HIP(hipMemcpyAsync(ctx->d_len, ctx->beam.hlen.data(), (size_t)bN * 4, hipMemcpyHostToDevice, s));
  } else {
    const int L = ctx->h_len[0];
    for (int r = 1; r < bN; ++r) OM_CHECK(ctx->h_len[r] == L, "beam step: the beam rows differ in length");
    if (L > B.P) TRY(launch_kv_gather(beam_kv_args(ctx, true), (const int*)ctx->beam.parents.p, 0, bN, -1, B.P, L, s));
  }
  B.t++;
  return 0;
}

extern "C" int omchat_beam_result(omchat_ctx* ctx, int num_return, int32_t* tokens, int32_t* lengths, float* scores, int max_len) {
  OM_CHECK(ctx && tokens && lengths && scores, "null argument");
  const BeamState::Search& B = ctx->beam.cur;
  OM_CHECK(B.b > 0 && B.t > 0, "omchat_beam_result before a beam step");
  OM_CHECK(num_return >= 1 && num_return <= B.N, "num_return_sequences must be in [1, num_beams]");
  OM_HIP(hipDeviceSynchronize());
  std::vector<int> st(beam_state_words(B.b, B.N, B.max_new));
  OM_HIP(hipMemcpy(st.data(), ctx->beam.state.p, st.size() * 4, hipMemcpyDeviceToHost));
  const int bN = B.b * B.N;
  const int* bp = st.data() + 6 * bN + 2 * B.b;
  for (int i = 0; i < B.b; ++i)
    for (int q = 0; q < num_return; ++q) {
      const int e = i * B.N + q, o = i * num_return + q;
      float sc; memcpy(&sc, &st[BST_FSC * bN + e], 4);
      scores[o] = sc;
      const int step = st[BST_FSTEP * bN + e];
      const int n = step + 1;
      OM_CHECK(n <= max_len, "beam result: max_len too small");
      lengths[o] = n;
      if (n == 0) continue;
      tokens[(size_t)o * max_len + step] = st[BST_FTOK * bN + e];
      int beam = st[BST_FPAR * bN + e];
      for (int u = step - 1; u >= 0; --u) {
        const int* rec = bp + ((size_t)u * bN + i * B.N + beam) * 2;
        tokens[(size_t)o * max_len + u] = rec[1];
        beam = rec[0];
      }
    }
  return 0;
}
