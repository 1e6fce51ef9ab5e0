// Contrastive search on the device for generate(penalty_alpha=, top_k=) (Su et al., "A Contrastive Framework for Neural
// Text Generation"; HF 4.4x's _contrastive_search).  Per emitted token: the k candidates of the last top-k run as ONE k-row decode step over the
// same cache (the group machinery of beam.hip), then four launches --
//   penalty   pen_i = max_j cos(h_i, H_ctx[j]) over the history of post-final-norm hidden rows: every history row is read once for all k
//             candidates (MFMA 16 rows x 16 candidates), partial maxima per row chunk
//   select    the fold of the partials, score_i = (1 - alpha) p_i - alpha pen_i, the first maximum, the emitted id, the EOS word, the append
//             of h_pick to the history, the step's record, parents[r] = pick
//   gather    launch_kv_gather over the ONE new slot with those parents: every row keeps the picked row's slot
//   top-k     the k largest ids of logits row `pick` (ties to the lower id) with their softmax probabilities: the next candidates
// Every order is fixed and nothing is accumulated with atomics: the same input bits give the same bits, eager or between graph replays.
// tests/contrastive_ref.py is the float64 restatement.
#include "ctx.h"
#include "logits_tile.h"
#include <limits.h>
#include <string.h>

// every fp32 score is rounded after each operation, as torch rounds (1 - alpha) * p - alpha * pen
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool cs_beats(float v, int g, float v2, int g2) { return v > v2 || (v == v2 && g < g2); }

// ---------------------------------------------------------------------------------------------------------------- inverse norms
// one wave per row, lane l takes the 16-byte pieces l, l + 64, ...; fixed tree
template <typename T>
__global__ __launch_bounds__(256) void cs_norms_kernel(const T* rows, int n, int H, float* inv) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= n) return;
  const T* x = rows + (size_t)r * H;
  float s = 0.f;
  for (int c = lane * 8; c < H; c += 512) {
    const typename V8<T>::type v = ld8(x + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = tof(v[j]); s += f * f; }
  }
  s = wave_sum(s);
  if (lane == 0) inv[r] = (float)(1.0 / sqrt((double)s));      // correctly rounded: the table's error is half an ulp
}

// ---------------------------------------------------------------------------------------------------------------- penalty
// One wave per chunk of rpc rows (a multiple of 16).  A 16x16x32 MFMA per 32 columns: A = 16 history rows, B = the k <= 16 candidates (the
// lanes of a candidate at or beyond k read candidate k - 1 and write nothing), fp32 accumulators; rows at or beyond the chunk's end read the
// last row of the history and are left out of the maximum.  The candidates' squared norms fall out of the first group's B fragments.
template <typename T>
__global__ __launch_bounds__(64) void cs_penalty_kernel(const T* hist, const float* inv, int L, int H, const T* cand, int cand_nb, int k, int rpc,
                                                        float* part, float* cand_inv) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int row_lo = blockIdx.x * rpc, row_hi = min(L, row_lo + rpc);
  const int cr = min(r, k - 1);
  float best = -INFINITY, csq = 0.f, cinv = 0.f;
  for (int base = row_lo; base < row_hi; base += 16) {
    const bool first = base == row_lo;
    const T* hrow = hist + (size_t)min(base + r, L - 1) * H + 8 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < H; k0 += 32) {
      const typename V8<T>::type a = ld8(hrow + k0);
      const int kk = k0 + 8 * g;
      const typename V8<T>::type b = ld8(cand + (cand_nb ? packed_x_index(cr, kk, cand_nb) : (size_t)cr * H + kk));
      acc = mfma16(a, b, acc);
      if (first) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = tof(b[j]); csq += f * f; }
      }
    }
    if (first) {
      csq += __shfl_xor(csq, 16, 64);
      csq += __shfl_xor(csq, 32, 64);
      cinv = (float)(1.0 / sqrt((double)csq));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = base + 4 * g + q;
      if (row < row_hi) best = fmaxf(best, (float)((double)acc[q] * (double)inv[row] * (double)cinv));      // one rounding for the two scalings
    }
  }
  best = fmaxf(best, __shfl_xor(best, 16, 64));
  best = fmaxf(best, __shfl_xor(best, 32, 64));
  if (g == 0 && r < k) {
    part[(size_t)blockIdx.x * CS_KMAX + r] = best;
    if (blockIdx.x == 0) cand_inv[r] = cinv;
  }
}

// ---------------------------------------------------------------------------------------------------------------- top-k with probabilities
// the block's best (value, id) pair: a fixed tree; every thread gets it
__device__ inline void cs_block_best(float& v, int& i, float* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
    if (cs_beats(ov, oi, v, i)) { v = ov; i = oi; }
  }
  __syncthreads();      // (sv / si may still be read from the round before)
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = sv[0]; i = si[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (cs_beats(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

// grid = tiles of 2048 ids: the tile's (max, sum exp(x - max)) and its k best (value, id) pairs in order; round r takes the best pair behind
// round r - 1's in the order (value descending, id ascending), so nothing is marked.  A tile with fewer than k ids ends its list with id -1.
__global__ __launch_bounds__(256) void cs_topk_tile_kernel(const float* logits, int ld, const int* row_sel, int V, int k, bool vec, float2* lse,
                                                           float2* best) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  const int tile = blockIdx.x, t0 = tile * GD_TILE;
  const float* row = logits + (size_t)(row_sel ? *row_sel : 0) * ld;
  float x[8];
  gd_load(row, t0, V, vec, x);
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
  if (threadIdx.x == 0) lse[tile] = make_float2(m, s);
  float pv = INFINITY; int pi = -1;
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY; int bi = INT_MAX;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int id = t0 + ((e >> 2) * 256 + (int)threadIdx.x) * 4 + (e & 3);
      if (id < V && cs_beats(pv, pi, x[e], id) && cs_beats(x[e], id, bv, bi)) { bv = x[e]; bi = id; }
    }
    cs_block_best(bv, bi, sv, si);
    const bool ok = bi != INT_MAX;
    if (threadIdx.x == 0) best[(size_t)tile * CS_KMAX + r] = make_float2(ok ? bv : -INFINITY, __int_as_float(ok ? bi : -1));
    if (ok) { pv = bv; pi = bi; }
    else { pv = -INFINITY; pi = INT_MAX; }      // nothing is behind the end of the list
  }
}

// one workgroup: the row's (max, sum) from the tile partials, then k rounds over the tiles' lists
__global__ __launch_bounds__(256) void cs_topk_merge_kernel(const float2* lse, const float2* best, int nt, int k, int32_t* ids, float* probs) {
  __shared__ float sh[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  const int t = threadIdx.x;
  float m = -INFINITY;
  for (int i = t; i < nt; i += 256) m = fmaxf(m, lse[i].x);
  m = gd_block_reduce<true>(m, sh);
  float s = 0.f;
  if (m > -INFINITY)
    for (int i = t; i < nt; i += 256) s += lse[i].y * expf(lse[i].x - m);
  s = gd_block_reduce<false>(s, sh);
  float pv = INFINITY; int pi = -1;
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY; int bi = INT_MAX;
    for (int c = t; c < nt * k; c += 256) {
      const float2 e = best[(size_t)(c / k) * CS_KMAX + (c % k)];
      const int id = __float_as_int(e.y);
      if (id >= 0 && cs_beats(pv, pi, e.x, id) && cs_beats(e.x, id, bv, bi)) { bv = e.x; bi = id; }
    }
    cs_block_best(bv, bi, sv, si);
    if (t == 0) {
      ids[r] = bi == INT_MAX ? -1 : bi;
      probs[r] = bi == INT_MAX ? 0.f : expf(bv - m) / s;
    }
    if (bi != INT_MAX) { pv = bv; pi = bi; }
    else { pv = -INFINITY; pi = INT_MAX; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- select and commit
template <typename T>
__global__ __launch_bounds__(256) void cs_select_kernel(CsSelectArgs a) {
  __shared__ float s_pen[CS_KMAX], s_score[CS_KMAX];
  __shared__ int s_pick;
  const int t = threadIdx.x, k = a.k;
  if (t < k) {
    float pen = -INFINITY;
    for (int c = 0; c < a.chunks; ++c) pen = fmaxf(pen, a.part[(size_t)c * CS_KMAX + t]);
    s_pen[t] = pen;
    s_score[t] = __fsub_rn(__fmul_rn(a.one_minus_alpha, a.probs[t]), __fmul_rn(a.alpha, pen));
  }
  __syncthreads();
  if (t == 0) {
    int pick = 0;
    for (int i = 1; i < k; ++i)
      if (s_score[i] > s_score[pick]) pick = i;      // strict: the first maximum, the lower rank
    s_pick = pick;
    const int tok = a.ids[pick];
    bool hit = a.last != 0;
    for (int q = 0; q < a.n_eos; ++q) hit = hit || tok == a.eos[q];
    if (a.sel) *a.sel = pick;
    if (a.token) *a.token = tok;
    if (a.done_word) *a.done_word = hit ? 1 : 0;
    if (a.inv) a.inv[a.n_hist] = a.cand_inv[pick];
    if (a.rec) { a.rec[48] = pick; a.rec[49] = tok; a.rec[50] = a.chunks; a.rec[51] = a.n_hist; }
  }
  __syncthreads();
  const int pick = s_pick;
  if (t < CS_KMAX && a.rec) {
    a.rec[t] = t < k ? a.ids[t] : -1;
    a.rec[16 + t] = __float_as_int(t < k ? a.probs[t] : 0.f);
    a.rec[32 + t] = __float_as_int(t < k ? s_pen[t] : 0.f);
  }
  if (t < k && a.parents) a.parents[t] = pick;
  if (a.hist) {
    const T* cand = (const T*)a.cand;
    T* dst = (T*)a.hist + (size_t)a.n_hist * a.H;
    for (int c = t * 8; c < a.H; c += 256 * 8)
      st8(dst + c, ld8(cand + (a.cand_nb ? packed_x_index(pick, c, a.cand_nb) : (size_t)pick * a.H + c)));
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- launchers
void cs_plan(int L, int cus, int* chunks, int* rows_per_chunk) {
  const int waves = 4 * (cus > 0 ? cus : 1);
  const int groups = (L + 15) / 16;                        // 16-row MFMA groups
  const int gpc = std::max(1, (groups + waves - 1) / waves);
  *rows_per_chunk = gpc * 16;
  *chunks = std::max(1, (L + gpc * 16 - 1) / (gpc * 16));
}

int launch_cs_norms(int dtype, const void* rows, int n, int H, float* inv, hipStream_t s) {
  OM_CHECK(rows && inv && n >= 1 && H >= 8 && H % 8 == 0, "contrastive norms: n >= 1 rows of H % 8 == 0 elements");
  OM_CHECK(((uintptr_t)rows & 15) == 0, "contrastive norms: rows must be 16-byte aligned");
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(cs_norms_kernel<f16>, dim3((n + 3) / 4), dim3(256), 0, s, (const f16*)rows, n, H, inv);
  else hipLaunchKernelGGL(cs_norms_kernel<bf16>, dim3((n + 3) / 4), dim3(256), 0, s, (const bf16*)rows, n, H, inv);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_cs_penalty(int dtype, const void* hist, const float* inv, int L, int H, const void* cand, int cand_nb, int k, float* part,
                      float* cand_inv, hipStream_t s) {
  OM_CHECK(hist && inv && cand && part && cand_inv, "contrastive penalty: null argument");
  OM_CHECK(L >= 1 && H >= 32 && H % 32 == 0 && k >= 1 && k <= CS_KMAX, "contrastive penalty: L >= 1, H % 32 == 0, 1 <= k <= 16");
  OM_CHECK(cand_nb >= 0 && cand_nb <= 2 && (cand_nb == 0 || H % 64 == 0), "contrastive penalty: packed candidates in 1 or 2 blocks of 16 rows, H % 64 == 0");
  OM_CHECK((((uintptr_t)hist | (uintptr_t)cand) & 15) == 0, "contrastive penalty: rows must be 16-byte aligned");
  int chunks = 0, rpc = 0;
  cs_plan(L, device_cus(), &chunks, &rpc);
  if (dtype == OMCHAT_F16)
    hipLaunchKernelGGL(cs_penalty_kernel<f16>, dim3(chunks), dim3(64), 0, s, (const f16*)hist, inv, L, H, (const f16*)cand, cand_nb, k, rpc, part, cand_inv);
  else
    hipLaunchKernelGGL(cs_penalty_kernel<bf16>, dim3(chunks), dim3(64), 0, s, (const bf16*)hist, inv, L, H, (const bf16*)cand, cand_nb, k, rpc, part, cand_inv);
  OM_LAUNCH_CHECK();
  return 0;
}

size_t cs_topk_ws_bytes(int V) {
  const size_t nt = (size_t)(V + GD_TILE - 1) / GD_TILE;
  return nt * (1 + CS_KMAX) * sizeof(float2);
}

int launch_cs_topk(const float* logits, int ld, const int* row_sel, int V, int k, int32_t* ids, float* probs, void* ws, hipStream_t s) {
  OM_CHECK(logits && ids && probs && ws, "contrastive top-k: null argument");
  OM_CHECK(k >= 1 && k <= CS_KMAX && V >= k && ld >= V, "contrastive top-k: 1 <= k <= 16 <= V <= ld");
  const int nt = (V + GD_TILE - 1) / GD_TILE;
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  float2* lse = (float2*)ws;
  float2* best = lse + nt;
  hipLaunchKernelGGL(cs_topk_tile_kernel, dim3(nt), dim3(256), 0, s, logits, ld, row_sel, V, k, vec, lse, best);
  hipLaunchKernelGGL(cs_topk_merge_kernel, dim3(1), dim3(256), 0, s, (const float2*)lse, (const float2*)best, nt, k, ids, probs);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_cs_select(int dtype, const CsSelectArgs& a, hipStream_t s) {
  OM_CHECK(a.part && a.ids && a.probs && a.cand_inv, "contrastive select: null argument");
  OM_CHECK(a.chunks >= 1 && a.k >= 1 && a.k <= CS_KMAX && a.n_eos >= 0 && a.n_eos <= CS_EOS_MAX, "contrastive select: chunks >= 1, 1 <= k <= 16, at most 8 eos ids");
  if (a.hist) {
    OM_CHECK(a.cand && a.inv && a.n_hist >= 0 && a.H >= 8 && a.H % 8 == 0 && (a.cand_nb == 0 || a.H % 64 == 0), "contrastive select: the append needs the candidates' rows, the norm table and H % 8 == 0");
    OM_CHECK((((uintptr_t)a.hist | (uintptr_t)a.cand) & 15) == 0, "contrastive select: rows must be 16-byte aligned");
  }
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(cs_select_kernel<f16>, dim3(1), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(cs_select_kernel<bf16>, dim3(1), dim3(256), 0, s, a);
  OM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// context entry points (include/omchat_hip.h)
// ---------------------------------------------------------------------------------------------------------
const char* contrastive_state_refusal(const omchat_ctx* ctx) {
  if (ctx->tp_size > 1) return "contrastive search: tensor-parallel contexts are not implemented (DESIGN.md section 7)";
  if (ctx->fp8_kv) return "contrastive search: the e4m3 KV cache is not implemented (omchat_enable_fp8_kv(ctx, 0) first)";
  if (ctx->fp8_prefill) return "contrastive search: fp8 x fp8 prefill GEMMs are not implemented (omchat_enable_fp8_prefill(ctx, 0) first)";
  if (ctx->mxfp4_mode == 1) return "contrastive search: MXFP4 decode mode 1 covers batch-1 steps only, and every step here has k rows (omchat_enable_mxfp4_decode(ctx, 0 or 2) first)";
  if (ctx->beam.on()) return "contrastive search: a beam search is active";
  if (ctx->pick.guidance_on()) return "contrastive search: guidance is on (omchat_set_guidance with b = 0 first)";
  if (ctx->pick.dola_on()) return "contrastive search: layer-contrastive decoding is on (omchat_set_dola with b = 0 first)";
  if (ctx->pick.fsm_on()) return "contrastive search: a token FSM is on (omchat_fsm_begin with b = 0 first)";
  if (ctx->pick.constraints_on()) return "contrastive search: constraints are on (omchat_set_constraints with b = 0 first)";
  if (ctx->pick.logprobs_on()) return "contrastive search: logprobs are on (omchat_set_logprobs with b = 0 first)";
  if (ctx->pick.sampling_on()) return "contrastive search: sampling is on (omchat_set_sampling with b = 0 first)";
  return nullptr;
}

extern "C" int omchat_set_contrastive(omchat_ctx* ctx, int k, double alpha, int max_new, int share, const int32_t* eos_ids, int n_eos, void* stream) {
  (void)stream;
  OM_CHECK(ctx, "null ctx");
  ContrastiveState& C = ctx->cs;
  const omchat_config& c = ctx->c;
  if (k <= 0) {
    C.on = false; C.have_hist = false; C.forked = false;
    return 0;
  }
  // every refusal before anything is allocated or changed
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  if (const char* why = contrastive_state_refusal(ctx)) OM_CHECK(false, why);
  OM_CHECK(!ctx->group.on(), "contrastive search: a sampled group shares its prompt (omchat_group_begin with b = 0 first)");
  OM_CHECK(k >= 2 && k <= CS_KMAX && k <= c.max_batch, "contrastive search: 2 <= top_k <= min(16, max_batch)");
  OM_CHECK(alpha > 0.0 && alpha <= 1.0, "contrastive search: penalty_alpha must lie in (0, 1]");
  OM_CHECK(max_new >= 1 && max_new < c.max_seq, "contrastive search: 1 <= max_new < max_seq");
  OM_CHECK(n_eos >= 0 && n_eos <= CS_EOS_MAX && (n_eos == 0 || eos_ids), "contrastive search: at most 8 eos ids");
  OM_CHECK(c.t_hidden % 32 == 0, "contrastive search: the hidden size must be a multiple of 32");
  OM_CHECK(c.t_vocab >= k, "contrastive search: vocabulary smaller than top_k");
  if (share) { OM_CHECK(omchat_group_share_available(ctx, k), "contrastive search: the shared-prompt attention does not take these k rows (share = 0)"); }
  TRY(ctx->grow(C.small, 128 * 4));
  TRY(ctx->grow(C.rec, (size_t)max_new * CS_REC_WORDS * 4));
  TRY(ctx->grow(C.stash, (size_t)c.t_layers * k * c.t_kv_heads * 512));
  TRY(ctx->grow(C.tk_ws, cs_topk_ws_bytes(c.t_vocab)));      // (the penalty's partials are taken at the prefill, when the history's rows are known)
  C.on = true; C.k = k; C.alpha = (float)alpha; C.max_new = max_new; C.share = share != 0;
  C.one_minus = (float)(1.0 - alpha);
  C.eos.assign(eos_ids, eos_ids + n_eos);
  C.have_hist = false; C.forked = false; C.t = 0; C.n_hist = 0; C.P = 0;
  return 0;
}

// prefill_impl, before anything is enqueued: the history's room for a prompt of P positions
int contrastive_prefill_admit(omchat_ctx* ctx, int P) {
  ContrastiveState& C = ctx->cs;
  const omchat_config& c = ctx->c;
  if (const char* why = contrastive_state_refusal(ctx)) OM_CHECK(false, why);
  OM_CHECK(P + C.max_new <= c.max_seq, "contrastive search: prompt + max_new exceed max_seq");
  const int cap = P + C.max_new;
  TRY(ctx->grow(C.hist, (size_t)cap * c.t_hidden * 2));
  TRY(ctx->grow(C.inv, (size_t)cap * 4));
  TRY(ctx->grow(C.part, (size_t)((cap + 15) / 16) * CS_KMAX * 4));
  C.cap = cap;
  C.have_hist = false; C.forked = false;
  return 0;
}

// ... and behind its last layer: x = the residual stream [P][H]; the final norm writes the history, one launch its inverse norms
int contrastive_prefill_keep(omchat_ctx* ctx, const void* x, int P, hipStream_t s) {
  ContrastiveState& C = ctx->cs;
  const omchat_config& c = ctx->c;
  TRY(launch_rmsnorm(ctx->dt, x, c.t_hidden, ctx->t_norm, C.hist.p, c.t_hidden, P, c.t_hidden, c.t_eps, s));
  TRY(launch_cs_norms(ctx->dt, C.hist.p, P, c.t_hidden, (float*)C.inv.p, s));
  C.P = P; C.n_hist = P; C.t = 0; C.have_hist = true; C.forked = false;
  return 0;
}

extern "C" int omchat_contrastive_step(omchat_ctx* ctx, const float* logits, int rows, int32_t* next_tokens, int32_t* done_word, void* stream) {
  OM_CHECK(ctx && logits && next_tokens, "null argument");
  ContrastiveState& C = ctx->cs;
  const omchat_config& c = ctx->c;
  OM_CHECK(C.on, "omchat_contrastive_step without omchat_set_contrastive");
  OM_CHECK(C.have_hist, "omchat_contrastive_step: no b = 1 prefill has run since omchat_set_contrastive");
  if (const char* why = contrastive_state_refusal(ctx)) OM_CHECK(false, why);
  hipStream_t s = (hipStream_t)stream;
  const int k = C.k, H = c.t_hidden;
  if (!C.forked) {
    OM_CHECK(rows == 1, "contrastive step: rows = 1 on the prefill's logits, top_k afterwards");
    OM_CHECK(ctx->h_len[0] == C.P && ctx->dec_mode == 0, "contrastive step: a decode step has run since the prefill");
    TRY(launch_cs_topk(logits, c.t_vocab, nullptr, c.t_vocab, k, C.cand_ids(), C.cand_probs(), C.tk_ws.p, s));
    TRY(omchat_group_begin(ctx, 1, k, C.P, C.share ? 1 : 0, stream));
    OM_HIP(hipMemsetAsync(next_tokens + k, 0xFF, 4, s));      // no id is emitted yet: -1
    OM_HIP(hipMemcpyAsync(next_tokens, C.cand_ids(), (size_t)k * 4, hipMemcpyDeviceToDevice, s));
    C.forked = true;
    return 0;
  }
  OM_CHECK(rows == k, "contrastive step: rows = 1 on the prefill's logits, top_k afterwards");
  OM_CHECK(C.t < C.max_new, "contrastive search: max_new steps taken");
  const int L = C.P + C.t + 1;
  for (int r = 0; r < k; ++r) OM_CHECK(ctx->h_len[r] == L, "contrastive step: one k-row decode step runs between two calls");
  OM_CHECK(C.n_hist == C.P + C.t && C.n_hist < C.cap, "contrastive search: history out of step");
  const int pk = decode_x_pack_nb(ctx, k);
  int chunks = 0, rpc = 0;
  cs_plan(C.n_hist, device_cus(), &chunks, &rpc);
  TRY(launch_cs_penalty(ctx->dt, C.hist.p, (const float*)C.inv.p, C.n_hist, H, ctx->tw_xn, pk, k, (float*)C.part.p, C.cand_inv(), s));
  CsSelectArgs a;
  a.part = (const float*)C.part.p; a.chunks = chunks; a.k = k; a.alpha = C.alpha; a.one_minus_alpha = C.one_minus;
  a.ids = C.cand_ids(); a.probs = C.cand_probs(); a.cand_inv = C.cand_inv();
  a.cand = ctx->tw_xn; a.cand_nb = pk; a.H = H;
  a.hist = C.hist.p; a.inv = (float*)C.inv.p; a.n_hist = C.n_hist;
  a.n_eos = (int)C.eos.size();
  for (int q = 0; q < a.n_eos; ++q) a.eos[q] = C.eos[q];
  a.last = C.t + 1 >= C.max_new;
  a.rec = (int32_t*)C.rec.p + (size_t)C.t * CS_REC_WORDS;
  a.parents = C.parents(); a.sel = C.sel(); a.token = next_tokens + k; a.done_word = done_word;
  TRY(launch_cs_select(ctx->dt, a, s));
  // the one new slot [L - 1, L): every row keeps the picked row's (that row itself is not copied)
  KvGatherArgs g;
  g.k = (char*)ctx->kcache; g.v = (char*)ctx->vcache;
  g.layers = c.t_layers; g.kvh = c.t_kv_heads; g.max_seq = c.max_seq; g.rows_cap = c.max_batch;
  const size_t slots = (size_t)c.t_layers * k * c.t_kv_heads;
  g.sk = (char*)C.stash.p; g.sv = g.sk + slots * 256;
  g.st_rows = k; g.st_slots = 1;
  TRY(launch_kv_gather(g, C.parents(), 0, k, -1, L - 1, L, s));
  if (C.t + 1 < C.max_new) {
    TRY(launch_cs_topk(logits, c.t_vocab, C.sel(), c.t_vocab, k, C.cand_ids(), C.cand_probs(), C.tk_ws.p, s));
    OM_HIP(hipMemcpyAsync(next_tokens, C.cand_ids(), (size_t)k * 4, hipMemcpyDeviceToDevice, s));
  }
  C.n_hist++; C.t++;      // the host counters move last: a launch that fails above leaves them where the device's state is
  return 0;
}

extern "C" int omchat_contrastive_read(omchat_ctx* ctx, int32_t* out, int steps) {
  OM_CHECK(ctx && out, "null argument");
  const ContrastiveState& C = ctx->cs;
  OM_CHECK(C.rec.p && steps >= 0 && steps <= C.t, "omchat_contrastive_read: more steps than picks since the prefill");
  OM_HIP(hipDeviceSynchronize());
  if (steps) OM_HIP(hipMemcpy(out, C.rec.p, (size_t)steps * CS_REC_WORDS * 4, hipMemcpyDeviceToHost));
  return 0;
}

// test hook: the history's rows [row0, row0 + n) and inverse norms, and the final-normed rows of the last k-row step in row-major order
extern "C" int omchat_contrastive_rows(omchat_ctx* ctx, int row0, int n, void* hist_out, float* inv_out, void* cand_out) {
  OM_CHECK(ctx, "null argument");
  const ContrastiveState& C = ctx->cs;
  const int H = ctx->c.t_hidden;
  OM_CHECK(C.on && C.have_hist && row0 >= 0 && n >= 0 && row0 + n <= C.n_hist, "omchat_contrastive_rows: rows outside the history");
  OM_HIP(hipDeviceSynchronize());
  if (hist_out && n) OM_HIP(hipMemcpy(hist_out, (const char*)C.hist.p + (size_t)row0 * H * 2, (size_t)n * H * 2, hipMemcpyDeviceToHost));
  if (inv_out && n) OM_HIP(hipMemcpy(inv_out, (const float*)C.inv.p + row0, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (cand_out) {
    const int pk = decode_x_pack_nb(ctx, C.k);
    std::vector<uint16_t> raw((size_t)(pk ? pk * 16 : C.k) * H);
    OM_HIP(hipMemcpy(raw.data(), ctx->tw_xn, raw.size() * 2, hipMemcpyDeviceToHost));
    uint16_t* o = (uint16_t*)cand_out;
    for (int r = 0; r < C.k; ++r)
      for (int cidx = 0; cidx < H; ++cidx) o[(size_t)r * H + cidx] = raw[pk ? packed_x_index(r, cidx, pk) : (size_t)r * H + cidx];
  }
  return 0;
}
