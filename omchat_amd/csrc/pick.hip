// The token pick of a step, with its state (PickState, ctx.h): the guidance stage (guidance.hip) or the layer-contrast stage (dola.hip), the ban stage of the logits constraints (constrain.hip), the automaton
// stage of the token FSM (fsm.hip), the argmax (elementwise.hip) or the sampler (sample.hip), the record stage of the per-token log-probabilities (logprob.hip) -- their order, the
// refusals and host counters in front of a step, their setters and their rewind.  model.hip sees the functions ctx.h declares.  Host C++.
#include "ctx.h"
#include <math.h>
#include <algorithm>

namespace {

// vocab-parallel greedy: every rank contributes (max logit, global index) per sequence; summed into a zeroed table
__global__ void tp_argmax_scatter_kernel(const float* logits, int ld, const int* local_idx, int b, int rank, int v_local, float* table) {
  const int i = threadIdx.x;
  if (i < b) {
    table[((size_t)rank * b + i) * 2] = logits[(size_t)i * ld + local_idx[i]];
    table[((size_t)rank * b + i) * 2 + 1] = (float)(rank * v_local + local_idx[i]);
  }
}
__global__ void tp_argmax_pick_kernel(const float* table, int b, int size, int* out) {
  const int i = threadIdx.x;
  if (i < b) {
    float best = table[(size_t)i * 2]; int bi = (int)table[(size_t)i * 2 + 1];
    for (int r = 1; r < size; ++r) {            // ranks hold ascending index ranges: strict > keeps the first index on ties
      const float v = table[((size_t)r * b + i) * 2];
      if (v > best) { best = v; bi = (int)table[((size_t)r * b + i) * 2 + 1]; }
    }
    out[i] = bi;
  }
}

int smp_xchg(void* user, float* buf, size_t count, hipStream_t s) { return ((omchat_ctx*)user)->allreduce_f32(buf, count, s); }

ConstrainArgs con_args(omchat_ctx* ctx, int b, const int32_t* fed) {
  const omchat_config& c = ctx->c;
  const PickState& P = ctx->pick;
  ConstrainArgs a;
  a.hist = (int32_t*)P.con_hist.p; a.hist_ld = P.con_ld; a.len = P.con_len; a.plen = P.con_plen; a.tok = fed;
  a.b = b; a.V = c.t_vocab; a.V_total = c.t_vocab_total; a.gbase = ctx->tp_rank * c.t_vocab;
  a.ngram = P.con.ngram; a.min_new = P.con.min_new; a.min_len = P.con.min_len;
  constrain_bind_lists(P.con_lists, a);
  a.n_eos = P.con.n_eos; a.n_sup = P.con.n_sup; a.n_bsup = P.con.n_bsup; a.n_bw = P.con.n_bw;
  a.ban = P.con_ban; a.bmw = P.con_bmw;
  return a;
}

// The ban stage in front of a pick (omchat_set_constraints; nothing when constraints are off): `fed` = the tokens the decode step was fed
// (appended to the history first), NULL at the first pick after the prefill.  *lg then points at the context's banned copy of the logits;
// the caller's logits are not written.
int ban_stage(omchat_ctx* ctx, const float** lg, int b, const int32_t* fed, hipStream_t s) {
  const PickState& P = ctx->pick;
  if (!P.con.on) return 0;
  OM_CHECK(b <= P.con.b, "constraints are on for fewer rows than this pick has (omchat_set_constraints)");
  const omchat_config& c = ctx->c;
  TRY(launch_constrain_ban(con_args(ctx, b, fed), s));
  TRY(launch_constrain_apply(*lg, c.t_vocab, b, c.t_vocab, P.con_ban, P.con_bmw, P.con_logits, fed ? P.con_len : nullptr, P.con_ld, s));
  *lg = P.con_logits;
  return 0;
}

FsmArgs fsm_args(omchat_ctx* ctx, int b, const int32_t* fed) {
  const PickState& P = ctx->pick;
  FsmArgs a;
  a.trail = (int32_t*)P.fsm_trail.p; a.cap = P.fsm_cap; a.cnt = P.fsm_cnt; a.cur = P.fsm_cur; a.fed = fed;
  a.b = b; a.V = ctx->c.t_vocab; a.gbase = ctx->tp_rank * ctx->c.t_vocab;
  a.bm = P.fsm_bm; a.bmw = P.fsm_bmw;
  return a;
}

// The automaton stage behind the ban stage (omchat_fsm_begin; nothing when it is off): the rows' states advance over `fed`, then every id
// that is no edge of a row's state goes to -inf in the context's copy -- in place when the ban stage already wrote it.
int fsm_stage(omchat_ctx* ctx, const float** lg, int b, const int32_t* fed, hipStream_t s) {
  const PickState& P = ctx->pick;
  if (!P.fsm.on) return 0;
  OM_CHECK(b <= P.fsm.b, "the token FSM is on for fewer rows than this pick has (omchat_fsm_begin)");
  const FsmArgs a = fsm_args(ctx, b, fed);
  TRY(launch_fsm_mark(P.fsm_tab, a, s));
  TRY(launch_fsm_apply(*lg, ctx->c.t_vocab, a, P.con_logits, fed != nullptr, s));
  *lg = P.con_logits;
  return 0;
}

// The guidance stage in front of the ban stage (omchat_set_guidance; nothing when it is off): the pick was handed 2b rows; *lg then points
// at the context's copy with the b rows of guided scores, which the stages behind it write in place, and *b is the b rows that pick.
int guidance_stage(omchat_ctx* ctx, const float** lg, int* b, hipStream_t s) {
  const PickState& P = ctx->pick;
  if (!P.gd.on) return 0;
  OM_CHECK(*b == 2 * P.gd.b, "guidance is on: a pick takes the 2b rows omchat_set_guidance was given (conditional rows, then their twins)");
  const omchat_config& c = ctx->c;
  TRY(launch_guidance(*lg, c.t_vocab, P.gd.b, c.t_vocab, P.gd.scale, P.gd_ws, P.con_logits, c.t_vocab, s));
  *lg = P.con_logits;
  *b = P.gd.b;
  return 0;
}

// The layer-contrast stage in the same place (omchat_set_dola; nothing when it is off; the two exclude each other): the pick was handed the
// (k + 1) b rows a prefill or step left in the context -- the final rows, then the candidates' --; *lg then points at the context's copy with
// the b rows of contrasted scores, *b is the b rows that pick, and the record takes the layer every row chose.
int dola_stage(omchat_ctx* ctx, const float** lg, int* b, hipStream_t s) {
  const PickState& P = ctx->pick;
  if (!P.dola.on) return 0;
  OM_CHECK(*b == P.dola.rows() && *lg == P.dola_logits, "layer-contrastive decoding is on: a pick takes the (k + 1) b rows of the last prefill or step");
  const omchat_config& c = ctx->c;
  DolaArgs a;
  a.logits = *lg; a.ld = c.t_vocab; a.V = c.t_vocab; a.b = P.dola.b; a.k = P.dola.k; a.relative_top = P.dola.relative_top;
  a.out = P.con_logits; a.ld_out = c.t_vocab; a.ws = P.dola_ws; a.ws_bytes = P.dola_ws_cap;
  a.layers = P.dola_layers; a.rec = (int32_t*)P.dola_rec.p; a.cnt = P.dola_cnt; a.cap = P.dola_cap; a.rec_ld = c.max_batch;
  TRY(launch_dola(a, s));
  *lg = P.con_logits;
  *b = P.dola.b;
  return 0;
}

// a pick entry's rows while layer-contrastive decoding is on: the context's own (the caller's b rows are the final rows of the same call)
int dola_entry_rows(omchat_ctx* ctx, const float** lg, int* b) {
  const PickState& P = ctx->pick;
  if (!P.dola.on) return 0;
  OM_CHECK(P.dola_fresh, "layer-contrastive decoding is on: no prefill or step since omchat_set_dola has left the rows of this pick");
  *lg = P.dola_logits;
  *b = P.dola.rows();
  return 0;
}

// The record stage behind a pick (omchat_set_logprobs; nothing when it is off): raw = the caller's logits (under guidance its first b rows:
// the conditional rows' raw logits), proc = what the pick ran on (the guided scores when guidance is on, with the bans and the automaton's
// mask when those are on).  The sampler's parameters, seen bitmap, newly-set bits and thresholds are read where the pick left them.
int logprob_stage(omchat_ctx* ctx, const float* raw, const float* proc, int b, const int32_t* ids, hipStream_t s) {
  const PickState& P = ctx->pick;
  if (!P.lp.on) return 0;
  const omchat_config& c = ctx->c;
  LogprobArgs a;
  a.raw = raw; a.raw_ld = c.t_vocab; a.proc = proc; a.proc_ld = c.t_vocab;
  a.b = std::min(b, P.lp.b); a.V = c.t_vocab; a.rank = ctx->tp_rank; a.tp = ctx->tp_size;
  a.ids = ids;
  if (P.smp.on) {
    a.temperature = P.smp.temperature; a.penalty = P.smp.penalty;
    if (P.smp.penalty != 1.f) { a.seen = P.smp_bm; a.bm_words = P.smp_bmw; a.last_set = P.smp_last; }
    a.top1 = P.smp.top_k == 1;
    a.thr = sample_thr_words(P.smp_ws, b, c.t_vocab_total, P.smp.top_k, P.smp.top_p, P.smp_f, &a.thr_stride, &a.thr_hi);
  }
  a.ws = P.lp_ws; a.table = P.lp_table; a.xchg = smp_xchg; a.xchg_user = ctx;
  a.rec = (float*)P.lp_rec.p; a.cnt = P.lp_cnt; a.max_new = P.lp_cap; a.rec_ld = c.max_batch;
  if (P.lpx.on()) {      // the same counters, the same lines: nothing of its own to rewind or to bound
    a.top_n = P.lpx.top_n; a.n_score = P.lpx.n_score; a.score_ids = P.lp_sid; a.top_ws = P.lp_xws;
    a.top_vals = P.lpx_vals(); a.top_ids = P.lpx_ids(P.lp_cap, c.max_batch); a.scored = P.lpx_scored(P.lp_cap, c.max_batch);
    if (ctx->tp_size > 1) a.table = P.lp_xtable;
  }
  return launch_logprob(a, s);
}

// one more pick feeds the record: refuse before anything is enqueued when it is full (max_new of omchat_set_logprobs)
int lp_room(omchat_ctx* ctx) {
  OM_CHECK(!ctx->pick.lp.on || ctx->pick.lp_picks < ctx->pick.lp.max_new, "logprobs: more picks than the max_new given to omchat_set_logprobs");
  return 0;
}

// one more decode step feeds the history: refuse before the step is enqueued when it has no room left (max_new of omchat_set_constraints)
int con_count_step(omchat_ctx* ctx) {
  if (!ctx->pick.con.on) return 0;
  OM_CHECK(ctx->pick.con_fed + 1 < ctx->pick.con_room, "constraints: more decode steps than the max_new given to omchat_set_constraints");
  ctx->pick.con_fed += 1;
  return 0;
}

// ... and the trail of the token FSM (max_new of omchat_fsm_begin)
int fsm_count_step(omchat_ctx* ctx) {
  if (!ctx->pick.fsm.on) return 0;
  OM_CHECK(ctx->pick.fsm_fed < ctx->pick.fsm.max_new, "token FSM: more decode steps than the max_new given to omchat_fsm_begin");
  return 0;
}

}  // namespace

int pick_alloc(omchat_ctx* ctx, int rows) {
  TRY(ctx->alloc(&ctx->pick.arg_scratch, argmax_scratch_bytes(rows)));
  return ctx->alloc((void**)&ctx->pick.tp_table, (size_t)ctx->tp_size * rows * 2 * 4);
}

int pick_admit(omchat_ctx* ctx, bool picks, bool feeds) {
  // the filters behind top-p are kernel arguments of the captured decode graphs: other values than they were captured with drop them
  if (!(ctx->pick.smp_f == ctx->pick.smp_f_graph)) {
    drop_decode_graphs(ctx);
    ctx->pick.smp_f_graph = ctx->pick.smp_f;
  }
  if (picks) TRY(lp_room(ctx));
  if (feeds) TRY(fsm_count_step(ctx));      // (checked in front of the history's counter: a refusal leaves both counters as they are)
  if (feeds) TRY(con_count_step(ctx));
  if (feeds && ctx->pick.fsm.on) ctx->pick.fsm_fed += 1;
  ctx->pick.smp_vcommit = 0;      // a sampled verify step's picks are no longer the last thing the cache holds
  if (ctx->pick.lp.on && picks) ctx->pick.lp_picks += 1;
  return 0;
}

// greedy argmax over (rank-local) logits; under tensor parallelism the (max, index) pairs are exchanged
int greedy_pick(omchat_ctx* ctx, const float* lg, int b, int32_t* next_tokens, hipStream_t s, bool advance) {
  const omchat_config& c = ctx->c;
  float* table = ctx->pick.tp_table;
  TRY(launch_argmax(lg, c.t_vocab, b, c.t_vocab, next_tokens, ctx->pick.arg_scratch, s, advance ? ctx->d_pos : nullptr, advance ? ctx->d_len : nullptr));
  if (ctx->tp_size > 1) {
    const size_t n = (size_t)ctx->tp_size * b * 2;
    OM_HIP(hipMemsetAsync(table, 0, n * 4, s));
    hipLaunchKernelGGL(tp_argmax_scatter_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, lg, c.t_vocab, next_tokens, b, ctx->tp_rank, c.t_vocab, table);
    TRY(ctx->allreduce_f32(table, n, s));
    hipLaunchKernelGGL(tp_argmax_pick_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, table, b, ctx->tp_size, next_tokens);
  }
  return 0;
}

int pick_run(omchat_ctx* ctx, const float* lg, int b, int32_t* next_tokens, hipStream_t s, bool advance, const int32_t* fed, bool force_greedy) {
  const PickState& P = ctx->pick;
  const float* raw = lg;
  TRY(guidance_stage(ctx, &lg, &b, s));
  TRY(dola_stage(ctx, &lg, &b, s));      // (raw stays the first b of its rows: the final rows)
  // under guidance the pick's launches move nothing: the twin launch behind them copies the ids and moves the positions of all 2b rows
  const bool guided = P.gd.on;
  const bool adv = advance;
  advance = advance && !guided;
  auto finish = [&]() -> int {
    if (guided) TRY(launch_guidance_twin(next_tokens, b, adv ? ctx->d_pos : nullptr, adv ? ctx->d_len : nullptr, s));
    return logprob_stage(ctx, raw, lg, b, next_tokens, s);
  };
  TRY(ban_stage(ctx, &lg, b, fed, s));
  TRY(fsm_stage(ctx, &lg, b, fed, s));
  if (force_greedy || !P.smp.on) {
    TRY(greedy_pick(ctx, lg, b, next_tokens, s, advance));
    return finish();
  }
  const omchat_config& c = ctx->c;
  SampleArgs a;
  a.logits = lg; a.ld = c.t_vocab; a.b = b; a.V = c.t_vocab; a.V_total = c.t_vocab_total;
  a.rank = ctx->tp_rank; a.tp = ctx->tp_size;
  a.seed = P.smp.seed; a.temperature = P.smp.temperature; a.top_k = P.smp.top_k; a.top_p = P.smp.top_p; a.penalty = P.smp.penalty;
  a.f = P.smp_f;
  if (P.smp.penalty != 1.f) { a.bitmap = P.smp_bm; a.bm_words = P.smp_bmw; }
  a.last_set = P.smp_last; a.step = P.smp_step;
  if (advance) { a.adv_pos = ctx->d_pos; a.adv_len = ctx->d_len; }
  a.out = next_tokens; a.ws = P.smp_ws; a.table = P.tp_table;
  a.xchg = smp_xchg; a.xchg_user = ctx;
  TRY(launch_sample(a, s));
  return finish();
}

const char* pick_rows_refusal(omchat_ctx* ctx, int rows) {
  const PickState& P = ctx->pick;
  if (P.gd.on && rows != 2 * P.gd.b) return "guidance is on: this call takes exactly 2b rows -- the b conditional rows, then their twins (omchat_set_guidance with b = 0 first)";
  if (P.dola.on && rows != P.dola.b) return "layer-contrastive decoding is on: this call takes exactly the b rows omchat_set_dola was given (omchat_set_dola with b = 0 first)";
  return nullptr;
}

const char* dola_state_refusal(const omchat_ctx* ctx) {
  if (ctx->tp_size > 1) return "layer-contrastive decoding: one GPU (the vocabulary-parallel exchange of the log-sum-exps and divergences is not built)";
  if (ctx->beam.on()) return "layer-contrastive decoding: a beam search is active";
  if (ctx->contrastive_on()) return "layer-contrastive decoding: contrastive search is on (omchat_set_contrastive with k = 0 first); each candidate row would need its layers' rows";
  if (ctx->pick.gd.on) return "layer-contrastive decoding: guidance is on (omchat_set_guidance with b = 0 first); the two stages write the same copy";
  if (ctx->group.on()) return "layer-contrastive decoding: a sampled group shares its prompt (omchat_group_begin with b = 0 first)";
  if (ctx->fp8_decode) return "layer-contrastive decoding: the e4m3 decode replica is on, and the head pass over the candidate rows is 16-bit only (omchat_enable_fp8_decode(ctx, 0) first)";
  if (ctx->mxfp4_mode) return "layer-contrastive decoding: the MXFP4 decode replica is on, and the head pass over the candidate rows is 16-bit only (omchat_enable_mxfp4_decode(ctx, 0) first)";
  return nullptr;
}

const char* pick_verify_refusal(omchat_ctx* ctx, int flags) {
  const PickState& P = ctx->pick;
  if (!(flags & OMCHAT_VERIFY_SAMPLE)) {
    if (P.smp.on) return "sampling is on: prompt-lookup decoding is greedy only";
  } else {
    if (!P.smp.on) return "OMCHAT_VERIFY_SAMPLE: sampling is off (omchat_set_sampling first)";
    if (flags & OMCHAT_VERIFY_KEEP_ALL) return "OMCHAT_VERIFY_SAMPLE with OMCHAT_VERIFY_KEEP_ALL: the slots behind a rejected draw are not the sampled sequence's";
  }
  return nullptr;
}

int pick_verify_prepare(omchat_ctx* ctx) {
  PickState& P = ctx->pick;
  if (P.smp.penalty != 1.f && !P.smp_vseen) TRY(ctx->alloc((void**)&P.smp_vseen, (size_t)SMP_VERIFY_ROWS * P.smp_bmw * 4));
  return 0;
}

int pick_verify(omchat_ctx* ctx, const float* lg, int T, const int32_t* tokens, int32_t* picks, hipStream_t s, bool sample) {
  if (!sample) return greedy_pick(ctx, lg, T, picks, s);
  const PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  SampleArgs a;
  a.logits = lg; a.ld = c.t_vocab; a.b = T; a.V = c.t_vocab; a.V_total = c.t_vocab_total;
  a.rank = ctx->tp_rank; a.tp = ctx->tp_size;
  a.seed = P.smp.seed; a.temperature = P.smp.temperature; a.top_k = P.smp.top_k; a.top_p = P.smp.top_p; a.penalty = P.smp.penalty;
  a.f = P.smp_f;
  if (P.smp.penalty != 1.f) { a.bitmap = P.smp_bm; a.bm_words = P.smp_bmw; a.vseen = P.smp_vseen; }
  a.step = P.smp_step; a.vtokens = tokens;
  a.out = picks; a.ws = P.smp_ws; a.table = P.tp_table;
  a.xchg = smp_xchg; a.xchg_user = ctx;
  return launch_sample(a, s);
}

void pick_verify_committed(omchat_ctx* ctx, int n_picks) { ctx->pick.smp_vcommit = n_picks; }

// (rows beyond those the constraints are on for are not the history's: no refusal here, unlike the ban stage of a step that picks)
int pick_feed(omchat_ctx* ctx, const int32_t* fed, int b, hipStream_t s) {
  const PickState& P = ctx->pick;
  b = P.pick_rows(b);      // (under guidance the twins are fed their rows' ids: the first b of `fed`)
  if (P.con.on && b <= P.con.b) TRY(launch_constrain_append((int32_t*)P.con_hist.p, P.con_ld, P.con_len, fed, b, s));
  if (P.fsm.on && b <= P.fsm.b) TRY(launch_fsm_advance(P.fsm_tab, fsm_args(ctx, b, fed), s));
  return 0;
}

const char* pick_rewind_refusal(omchat_ctx* ctx, int b, int n) {
  const PickState& P = ctx->pick;
  if (const char* why = pick_rows_refusal(ctx, b)) return why;
  b = P.pick_rows(b);      // 2b cache rows go back, b rows of pick state
  if (P.lp.on && b < P.lp.b) return "rewind of fewer rows than omchat_set_logprobs switched on: the rows' records would fall out of step";
  if (P.smp.on && b == 1 && P.smp_vcommit > 0 && n <= P.smp_vcommit) return nullptr;      // the picks of a sampled verify step
  if (P.smp.on && n != 1 && P.smp.penalty != 1.f) return "rewind of more than one step with the repetition penalty on: only the last pick's bit is recorded";
  return nullptr;
}

int pick_rewind(omchat_ctx* ctx, int b, int n, hipStream_t s) {
  PickState& P = ctx->pick;
  b = P.pick_rows(b);
  if (P.smp.on && b == 1 && P.smp_vcommit > 0 && n <= P.smp_vcommit) {
    // the last picks are a sampled verify step's: each recorded the bit it newly set
    TRY(launch_sample_rewind_verify(P.smp.penalty != 1.f ? P.smp_bm : nullptr, P.smp_vlast, P.smp_step, P.smp_vcommit, n, s));
    P.smp_vcommit -= n;
  } else if (P.smp.on) {
    P.smp_vcommit = 0;
    // the sampler's step counters go back with the slots, and the seen bit the last pick set is cleared (only that pick is recorded)
    TRY(launch_sample_rewind(P.smp.penalty != 1.f ? P.smp_bm : nullptr, P.smp_bmw, P.smp_last, P.smp_step, b, n, s));
  }
  if (P.lp.on) {
    // the record forgets the picks of those steps
    TRY(launch_logprob_rewind(P.lp_cnt, std::min(b, P.lp.b), n, s));
    P.lp_picks = std::max(0, P.lp_picks - n);
  }
  if (P.con.on) {
    // the history forgets the fed ids with the slots
    TRY(launch_constrain_rewind(P.con_len, P.con_plen, std::min(b, P.con.b), n, s));
    P.con_fed = std::max(0, P.con_fed - n);
  }
  if (P.dola.on) TRY(launch_logprob_rewind(P.dola_cnt, std::min(b, P.dola.b), n, s));      // the layer record forgets those picks too
  if (P.fsm.on) {
    // the trail keeps every state: going back is the counts alone
    TRY(launch_fsm_rewind(P.fsm_cnt, std::min(b, P.fsm.b), n, s));
    P.fsm_fed = std::max(0, P.fsm_fed - n);
  }
  return 0;
}

extern "C" int omchat_greedy(omchat_ctx* ctx, const float* logits, int b, int32_t* next_tokens, void* stream) {
  OM_CHECK(ctx && logits && next_tokens && b >= 1 && b <= ctx->c.max_batch, "bad argument");
  if (const char* why = pick_rows_refusal(ctx, b)) OM_CHECK(false, why);
  TRY(lp_room(ctx));      // (in front of the refusal below as well: a full record is the first thing this call reports)
  // (the sampler's state is not this pick's: with sampling on, the first token comes from omchat_sample)
  OM_CHECK(!ctx->pick.lp.on || !ctx->pick.smp.on, "logprobs: omchat_greedy while sampling is on (omchat_sample picks the first token then)");
  TRY(dola_entry_rows(ctx, &logits, &b));
  TRY(pick_admit(ctx, true, false));
  return pick_run(ctx, logits, b, next_tokens, (hipStream_t)stream, false, nullptr, true);
}

// the first token after the prefill (omchat_greedy's sampled counterpart): advances the step counters, not the decode positions
extern "C" int omchat_sample(omchat_ctx* ctx, const float* logits, int b, int32_t* next_tokens, void* stream) {
  OM_CHECK(ctx && logits && next_tokens && b >= 1 && b <= ctx->c.max_batch, "bad argument");
  if (const char* why = pick_rows_refusal(ctx, b)) OM_CHECK(false, why);
  TRY(dola_entry_rows(ctx, &logits, &b));
  TRY(pick_admit(ctx, true, false));
  return pick_run(ctx, logits, b, next_tokens, (hipStream_t)stream);
}

// Sampling parameters live in the kernel arguments of the captured decode graphs: a change drops them (re-captured on the next step).
extern "C" int omchat_set_sampling(omchat_ctx* ctx, int b, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                                   const int32_t* seen_ids, const int32_t* n_seen_per_row, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  PickState::Sampling p;
  p.on = b > 0;
  if (p.on) {
    OM_CHECK(b <= c.max_batch, "sampling: batch exceeds max_batch");
    OM_CHECK(!ctx->contrastive_on(), "sampling: contrastive search is on (omchat_set_contrastive with k = 0 first); it is a deterministic strategy");
    OM_CHECK(temperature > 0.f && isfinite(temperature), "sampling: temperature must be a strictly positive float (greedy: do_sample=False)");
    OM_CHECK(top_k >= 0, "sampling: top_k >= 0 (0 = off)");
    OM_CHECK(top_p > 0.0 && top_p <= 1.0, "sampling: top_p in (0, 1] (1 = off)");
    OM_CHECK(rep_penalty > 0.f && isfinite(rep_penalty), "sampling: repetition_penalty must be a strictly positive float");
    p.seed = seed; p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.penalty = rep_penalty;
  }
  const PickState::Sampling& o = P.smp;
  const bool same = o.on == p.on && o.seed == p.seed && o.temperature == p.temperature && o.top_k == p.top_k && o.top_p == p.top_p &&
                    o.penalty == p.penalty;
  if (!same) drop_decode_graphs(ctx);
  P.smp = p;
  P.smp_vcommit = 0;
  P.smp_f = SampleFilters{};      // off until omchat_set_sampling_filters (the graphs are checked against them in front of the next step)
  if (!p.on) return 0;
  if (!P.smp_ws) {
    P.smp_bmw = (c.t_vocab + 31) / 32;
    TRY(ctx->alloc(&P.smp_ws, sample_ws_bytes(std::max(c.max_batch, SMP_VERIFY_ROWS))));      // (a verify step picks up to 16 rows)
    TRY(ctx->alloc((void**)&P.smp_vlast, (size_t)SMP_VERIFY_ROWS * 4));
    TRY(ctx->alloc((void**)&P.smp_bm, (size_t)c.max_batch * P.smp_bmw * 4));
    TRY(ctx->alloc((void**)&P.smp_last, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&P.smp_step, (size_t)c.max_batch * 4));
  }
  // this rank's slice of the seen sets; ids outside the vocabulary (the -200 image sentinel) are never seen
  std::vector<uint32_t> bm((size_t)c.max_batch * P.smp_bmw, 0u);
  if (rep_penalty != 1.f && seen_ids && n_seen_per_row) {
    const int64_t lo = (int64_t)ctx->tp_rank * c.t_vocab;
    size_t off = 0;
    for (int i = 0; i < b; ++i) {
      OM_CHECK(n_seen_per_row[i] >= 0, "sampling: n_seen_per_row >= 0");
      for (int j = 0; j < n_seen_per_row[i]; ++j) {
        const int64_t li = (int64_t)seen_ids[off + j] - lo;
        if (seen_ids[off + j] >= 0 && seen_ids[off + j] < c.t_vocab_total && li >= 0 && li < c.t_vocab)
          bm[(size_t)i * P.smp_bmw + (li >> 5)] |= 1u << (li & 31);
      }
      off += (size_t)n_seen_per_row[i];
    }
  }
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemcpyAsync(P.smp_bm, bm.data(), bm.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemsetAsync(P.smp_step, 0, (size_t)c.max_batch * 4, s));
  OM_HIP(hipMemsetAsync(P.smp_last, 0xFF, (size_t)c.max_batch * 4, s));
  OM_HIP(hipMemsetAsync(P.smp_vlast, 0xFF, (size_t)SMP_VERIFY_ROWS * 4, s));
  OM_HIP(hipStreamSynchronize(s));     // host vector
  return 0;
}

// test accessor (include/omchat_hip.h): a row's step counter and its rank-local seen bitmap
extern "C" int omchat_read_sampling_state(omchat_ctx* ctx, int row, int* step, uint32_t* seen_words) {
  OM_CHECK(ctx && step, "null argument");
  const PickState& P = ctx->pick;
  OM_CHECK(P.smp.on && P.smp_ws, "omchat_read_sampling_state: sampling is off");
  OM_CHECK(row >= 0 && row < ctx->c.max_batch, "omchat_read_sampling_state: row out of range");
  OM_HIP(hipDeviceSynchronize());
  OM_HIP(hipMemcpy(step, P.smp_step + row, 4, hipMemcpyDeviceToHost));
  if (seen_words) OM_HIP(hipMemcpy(seen_words, P.smp_bm + (size_t)row * P.smp_bmw, (size_t)P.smp_bmw * 4, hipMemcpyDeviceToHost));
  return 0;
}

// HF's MinP / Typical / Epsilon / Eta warpers behind top-p for the sampling state omchat_set_sampling just configured (include/omchat_hip.h)
extern "C" int omchat_set_sampling_filters(omchat_ctx* ctx, double min_p, double typical_p, double epsilon_cutoff, double eta_cutoff, void* stream) {
  (void)stream;
  OM_CHECK(ctx, "null ctx");
  OM_CHECK(ctx->pick.smp.on, "sampling filters: sampling is off (omchat_set_sampling first)");
  OM_CHECK(!(min_p > 1.0) && min_p == min_p, "sampling: min_p in [0, 1] (negative = off)");
  OM_CHECK(typical_p > 0.0, "sampling: typical_p in (0, 1) (1 or more = off)");
  OM_CHECK(epsilon_cutoff > 0.0, "sampling: epsilon_cutoff in (0, 1) (1 or more = off)");
  OM_CHECK(eta_cutoff > 0.0, "sampling: eta_cutoff in (0, 1) (1 or more = off)");
  SampleFilters f;
  f.min_p = min_p < 0.0 ? -1.0 : min_p;
  f.typical_p = typical_p < 1.0 ? typical_p : 1.0;
  f.epsilon = epsilon_cutoff < 1.0 ? epsilon_cutoff : 1.0;
  f.eta = eta_cutoff < 1.0 ? eta_cutoff : 1.0;
  ctx->pick.smp_f = f;
  return 0;
}

// Constraint parameters live in the kernel arguments of the captured decode graphs, as the sampling ones do: a change (or a history buffer
// that had to grow) drops them.  The id lists are read from device memory at every pick, so new contents of the same size keep the graphs.
extern "C" int omchat_set_constraints(omchat_ctx* ctx, int b, int no_repeat_ngram_size, int min_new_tokens, int min_length, const int32_t* eos_ids,
                                      int n_eos, const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress,
                                      const int32_t* bad_word_ids, const int32_t* bad_word_offsets, int n_bad_words, const int32_t* prompt_ids,
                                      const int32_t* prompt_len, int max_new, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  if (b <= 0) {
    if (P.con.on) drop_decode_graphs(ctx);
    P.con = PickState::Constraints{};
    return 0;
  }
  // every refusal before anything is enqueued or changed
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(b <= c.max_batch, "constraints: batch exceeds max_batch");
  OM_CHECK(no_repeat_ngram_size >= 0 && no_repeat_ngram_size <= CON_NGRAM_MAX, "constraints: 0 <= no_repeat_ngram_size <= 64 (0 = off)");
  OM_CHECK(min_new_tokens >= 0 && min_length >= 0, "constraints: min_new_tokens and min_length >= 0");
  OM_CHECK(prompt_ids && prompt_len && max_new >= 1, "constraints: prompt ids, per-row lengths and max_new >= 1");
  OM_CHECK(!ctx->beam.on(), "constraints: a beam search is active (the processors act on log-softmax scores there)");
  OM_CHECK(!ctx->contrastive_on(), "constraints: contrastive search is on (omchat_set_contrastive with k = 0 first); its pick runs on no banned copy");
  int maxP = 0;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(prompt_len[i] >= 0, "constraints: prompt_len >= 0");
    maxP = std::max(maxP, prompt_len[i]);
  }
  PickState::Constraints p;
  p.on = true; p.b = b; p.ngram = no_repeat_ngram_size; p.min_new = min_new_tokens; p.min_len = min_length;
  std::vector<int32_t> lists(CON_LIST_WORDS);
  ConstrainArgs la;
  TRY(constrain_pack_lists(eos_ids, n_eos, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_word_ids, bad_word_offsets,
                           n_bad_words, lists.data(), la));
  p.n_eos = la.n_eos; p.n_sup = la.n_sup; p.n_bsup = la.n_bsup; p.n_bw = la.n_bw;
  if (!P.con_lists) {
    P.con_bmw = (c.t_vocab + 31) / 32;
    TRY(ctx->alloc((void**)&P.con_lists, (size_t)CON_LIST_WORDS * 4));
    TRY(ctx->alloc((void**)&P.con_len, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&P.con_plen, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&P.con_ban, (size_t)c.max_batch * P.con_bmw * 4));
    TRY(ctx->alloc((void**)&P.con_logits, (size_t)c.max_batch * c.t_vocab * 4));
  }
  // history rows: the prompt, one id per decode step, grown on demand and never shrunk; rows 16-byte aligned
  const int need = (maxP + max_new + 1 + 3) / 4 * 4;
  void* old = P.con_hist.p;
  if (need > P.con_ld) {
    TRY(ctx->grow(P.con_hist, (size_t)c.max_batch * need * 4));
    P.con_ld = need;
  }
  if (!(p == P.con) || old != P.con_hist.p) drop_decode_graphs(ctx);
  P.con = p;
  P.con_fed = 0;
  P.con_room = P.con_ld - maxP;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> len(c.max_batch, 0);
  std::copy(prompt_len, prompt_len + b, len.begin());
  OM_HIP(hipMemcpyAsync(P.con_lists, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(P.con_len, len.data(), len.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(P.con_plen, len.data(), len.size() * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemsetAsync(P.con_ban, 0, (size_t)c.max_batch * P.con_bmw * 4, s));
  size_t off = 0;
  for (int i = 0; i < b; ++i) {
    if (prompt_len[i])
      OM_HIP(hipMemcpyAsync((int32_t*)P.con_hist.p + (size_t)i * P.con_ld, prompt_ids + off, (size_t)prompt_len[i] * 4, hipMemcpyHostToDevice, s));
    off += (size_t)prompt_len[i];
  }
  OM_HIP(hipStreamSynchronize(s));     // host vectors and the caller's ids
  return 0;
}

// Per-token log-probabilities (include/omchat_hip.h).  The record and its geometry live in the kernel arguments of the captured decode graphs:
// switching on or off, another b / max_new or a record that had to grow drops them.
extern "C" int omchat_set_logprobs(omchat_ctx* ctx, int b, int max_new, void* stream) {
  return omchat_set_logprobs_ex(ctx, b, max_new, 0, nullptr, 0, stream);
}

// (the extras -- top_n and the scored ids -- are kernel arguments of the same graphs: a change of either, or of a buffer's address, drops them)
extern "C" int omchat_set_logprobs_ex(omchat_ctx* ctx, int b, int max_new, int top_n, const int32_t* score_ids, int n_score, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  if (b <= 0) {
    if (P.lp.on) drop_decode_graphs(ctx);
    P.lp = PickState::Logprobs{};
    P.lpx = PickState::Extras{};
    P.lp_picks = 0;
    return 0;
  }
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(!ctx->contrastive_on(), "logprobs: contrastive search is on (omchat_set_contrastive with k = 0 first); its record holds the candidates' probabilities");
  OM_CHECK(b <= c.max_batch, "logprobs: batch exceeds max_batch");
  OM_CHECK(max_new >= 1, "logprobs: max_new >= 1");
  OM_CHECK(!ctx->beam.on(), "logprobs: a beam search is active (it reports sequences_scores)");
  PickState::Extras x;
  OM_CHECK(top_n >= 0 && top_n <= OMCHAT_LP_MAX_TOP, "logprobs: 0 <= top_n <= 20 (0 = no alternatives)");
  OM_CHECK(top_n <= c.t_vocab_total, "logprobs: top_n exceeds the vocabulary");
  OM_CHECK(n_score >= 0 && n_score <= OMCHAT_LP_MAX_SCORED && (n_score == 0 || score_ids), "logprobs: 0 <= n_score <= 32 scored ids");
  x.top_n = top_n; x.n_score = n_score;
  if (n_score) x.ids.assign(score_ids, score_ids + n_score);
  for (int i = 0; i < n_score; ++i) {
    OM_CHECK(x.ids[i] >= 0 && x.ids[i] < c.t_vocab_total, "logprobs: scored id outside the vocabulary");
    for (int j = 0; j < i; ++j) OM_CHECK(x.ids[j] != x.ids[i], "logprobs: scored ids must be distinct");
  }
  OM_CHECK(!x.on() || ctx->tp_size == 1 || c.t_vocab_total < (1 << 24), "logprobs: under tensor parallelism the alternatives' ids cross the exchange as fp32 (vocabulary < 2^24)");
  if (!P.lp_cnt) {
    TRY(ctx->alloc((void**)&P.lp_cnt, (size_t)c.max_batch * 4));
    TRY(ctx->alloc(&P.lp_ws, logprob_ws_bytes(c.max_batch)));
    if (ctx->tp_size > 1) TRY(ctx->alloc((void**)&P.lp_table, logprob_table_bytes(c.max_batch, ctx->tp_size)));
  }
  // the extras' fixed buffers at their caps, each when it is first asked for
  if (x.top_n && !P.lp_xws) TRY(ctx->alloc(&P.lp_xws, logprob_top_ws_bytes(c.max_batch, OMCHAT_LP_MAX_TOP)));
  if (x.n_score && !P.lp_sid) TRY(ctx->alloc((void**)&P.lp_sid, (size_t)OMCHAT_LP_MAX_SCORED * 4));
  if (x.on() && ctx->tp_size > 1 && !P.lp_xtable)
    TRY(ctx->alloc((void**)&P.lp_xtable, logprob_table_bytes_ex(c.max_batch, ctx->tp_size, OMCHAT_LP_MAX_TOP, OMCHAT_LP_MAX_SCORED)));
  // the captured graphs hold the record's address, its capacity (the stride of the processed plane) and b: another max_new within the
  // capacity keeps them (the host refuses the picks beyond it)
  void* old = P.lp_rec.p;
  void* oldx = P.lp_xrec.p;
  const int old_cap = P.lp_cap;
  if (max_new > P.lp_cap) {
    TRY(ctx->grow(P.lp_rec, (size_t)2 * max_new * c.max_batch * 4));
    P.lp_cap = max_new;
  }
  if (x.on()) TRY(ctx->grow(P.lp_xrec, (size_t)P.lp_cap * c.max_batch * (2 * x.top_n + x.n_score) * 4));
  if (!P.lp.on || P.lp.b != b || old != P.lp_rec.p || old_cap != P.lp_cap || !(x == P.lpx) || (x.on() && oldx != P.lp_xrec.p)) drop_decode_graphs(ctx);
  P.lp.on = true; P.lp.b = b; P.lp.max_new = max_new;
  P.lpx = x;
  P.lp_picks = 0;
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemsetAsync(P.lp_cnt, 0, (size_t)c.max_batch * 4, s));
  if (n_score) {
    OM_HIP(hipMemcpyAsync(P.lp_sid, P.lpx.ids.data(), (size_t)n_score * 4, hipMemcpyHostToDevice, s));
    OM_HIP(hipStreamSynchronize(s));     // host vector
  }
  return 0;
}

extern "C" int omchat_read_logprobs(omchat_ctx* ctx, int b, float* raw, float* processed, int32_t* counts, int max_len) {
  OM_CHECK(ctx && raw && processed && counts, "null argument");
  const PickState& P = ctx->pick;
  OM_CHECK(P.lp.on && b >= 1 && b <= P.lp.b, "omchat_read_logprobs: rows that omchat_set_logprobs switched on");
  const int mb = ctx->c.max_batch, mn = P.lp_cap;
  OM_HIP(hipDeviceSynchronize());
  std::vector<float> rec((size_t)2 * mn * mb);
  std::vector<int> cnt(mb);
  OM_HIP(hipMemcpy(rec.data(), P.lp_rec.p, rec.size() * 4, hipMemcpyDeviceToHost));
  OM_HIP(hipMemcpy(cnt.data(), P.lp_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < b; ++i) {
    const int n = std::min(std::max(cnt[i], 0), P.lp.max_new);
    OM_CHECK(n <= max_len, "omchat_read_logprobs: max_len too small");
    counts[i] = n;
    for (int t = 0; t < n; ++t) {
      raw[(size_t)i * max_len + t] = rec[(size_t)t * mb + i];
      processed[(size_t)i * max_len + t] = rec[((size_t)mn + t) * mb + i];
    }
  }
  return 0;
}

extern "C" int omchat_read_logprob_extras(omchat_ctx* ctx, int b, float* top_vals, int32_t* top_ids, float* scored, int32_t* counts, int max_len) {
  OM_CHECK(ctx && counts, "null argument");
  const PickState& P = ctx->pick;
  OM_CHECK(P.lp.on && P.lpx.on(), "omchat_read_logprob_extras: the extras are off (omchat_set_logprobs_ex with top_n or scored ids first)");
  OM_CHECK(b >= 1 && b <= P.lp.b, "omchat_read_logprob_extras: rows that omchat_set_logprobs_ex switched on");
  const int mb = ctx->c.max_batch, mn = P.lp_cap, tn = P.lpx.top_n, ns = P.lpx.n_score;
  OM_HIP(hipDeviceSynchronize());
  std::vector<int> cnt(mb);
  OM_HIP(hipMemcpy(cnt.data(), P.lp_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
  int lines = 0;
  for (int i = 0; i < b; ++i) {
    counts[i] = std::min(std::max(cnt[i], 0), P.lp.max_new);
    OM_CHECK(counts[i] <= max_len, "omchat_read_logprob_extras: max_len too small");
    lines = std::max(lines, counts[i]);
  }
  // the first `lines` lines of a plane [lp_cap][max_batch][w] -> host [b][max_len][w]
  auto plane = [&](const void* dev, void* host, int w) -> int {
    if (!host || !w || !lines) return 0;
    std::vector<uint32_t> h((size_t)lines * mb * w);
    OM_HIP(hipMemcpy(h.data(), dev, h.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < b; ++i)
      for (int t = 0; t < counts[i]; ++t)
        std::copy_n(&h[((size_t)t * mb + i) * w], w, (uint32_t*)host + ((size_t)i * max_len + t) * w);
    return 0;
  };
  TRY(plane(P.lpx_vals(), top_vals, tn));
  TRY(plane(P.lpx_ids(mn, mb), top_ids, tn));
  TRY(plane(P.lpx_scored(mn, mb), scored, ns));
  return 0;
}

// ---- finite-state token constraints (include/omchat_hip.h)
// The table's addresses and the trail's are kernel arguments of the captured decode graphs: a new table, a buffer that had to grow, or
// switching the stage on, off or to another b drops them; the same table and the same b on the next call keep them.
extern "C" int omchat_fsm_load(omchat_ctx* ctx, int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  OM_CHECK(!ctx->beam.on(), "token FSM: a beam search is active");
  if (n_states <= 0) {      // unload: the stage goes off with its table (the buffer stays, counted, for the next table)
    if (P.fsm.on || P.fsm_tab.n_states) drop_decode_graphs(ctx);
    P.fsm = PickState::Fsm{};
    P.fsm_tab = FsmTable{};
    P.fsm_off_host.clear();
    return 0;
  }
  OM_CHECK(ctx->c.t_layers > 0, "context has no decoder");
  TRY(fsm_validate(n_states, off, tok, nxt, ctx->c.t_vocab_total));
  const size_t E = (size_t)off[n_states];
  const size_t n_off = ((size_t)n_states + 1 + 3) / 4 * 4, n_tok = (E + 3) / 4 * 4 + 4;      // tok 16-byte aligned, whole int4 pieces behind the last edge
  TRY(ctx->grow(P.fsm_mem, (n_off + n_tok + E + 4) * 4));
  drop_decode_graphs(ctx);
  P.fsm = PickState::Fsm{};      // rows begin again on the new table (omchat_fsm_begin)
  int32_t* base = (int32_t*)P.fsm_mem.p;
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemcpyAsync(base, off, ((size_t)n_states + 1) * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemsetAsync(base + n_off, 0, n_tok * 4, s));
  if (E) {
    OM_HIP(hipMemcpyAsync(base + n_off, tok, E * 4, hipMemcpyHostToDevice, s));
    OM_HIP(hipMemcpyAsync(base + n_off + n_tok, nxt, E * 4, hipMemcpyHostToDevice, s));
  }
  OM_HIP(hipStreamSynchronize(s));     // the caller's arrays
  P.fsm_off_host.assign(off, off + n_states + 1);
  P.fsm_tab.off = base; P.fsm_tab.tok = base + n_off; P.fsm_tab.nxt = base + n_off + n_tok; P.fsm_tab.n_states = n_states;
  return 0;
}

extern "C" int omchat_fsm_begin(omchat_ctx* ctx, int b, const int32_t* start_states, int max_new, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  if (b <= 0) {
    if (P.fsm.on) drop_decode_graphs(ctx);
    P.fsm = PickState::Fsm{};
    return 0;
  }
  // every refusal before anything is enqueued or changed
  OM_CHECK(!ctx->contrastive_on(), "token FSM: contrastive search is on (omchat_set_contrastive with k = 0 first); its pick runs on no masked copy");
  OM_CHECK(P.fsm_tab.n_states > 0, "token FSM: no table is loaded (omchat_fsm_load first)");
  OM_CHECK(b <= c.max_batch, "token FSM: batch exceeds max_batch");
  OM_CHECK(start_states && max_new >= 1, "token FSM: start states and max_new >= 1");
  OM_CHECK(!ctx->beam.on(), "token FSM: a beam search is active (the processors act on log-softmax scores there)");
  hipStream_t s = (hipStream_t)stream;
  // a start state must have an edge, as every state a row can reach has (omchat_fsm_load)
  for (int i = 0; i < b; ++i) {
    OM_CHECK(start_states[i] >= 0 && start_states[i] < P.fsm_tab.n_states, "token FSM: start state outside the table");
    OM_CHECK(P.fsm_off_host[start_states[i] + 1] > P.fsm_off_host[start_states[i]],
             "token FSM: start state " + std::to_string(start_states[i]) + " has no edge: every row there would be -inf; add an EOS edge");
  }
  void* old_trail = P.fsm_trail.p;
  void* old_copy = P.con_logits;
  if (!P.fsm_cnt) {
    P.fsm_bmw = (c.t_vocab + 31) / 32;
    TRY(ctx->alloc((void**)&P.fsm_cnt, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&P.fsm_cur, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&P.fsm_bm, (size_t)c.max_batch * P.fsm_bmw * 4));
    OM_HIP(hipMemsetAsync(P.fsm_bm, 0, (size_t)c.max_batch * P.fsm_bmw * 4, s));
  }
  if (!P.con_logits) TRY(ctx->alloc((void**)&P.con_logits, (size_t)c.max_batch * c.t_vocab * 4));
  // the trail: one state per fed token and the start state, grown on demand and never shrunk
  if (max_new + 1 > P.fsm_cap) {
    TRY(ctx->grow(P.fsm_trail, (size_t)c.max_batch * (max_new + 1) * 4));
    P.fsm_cap = max_new + 1;
  }
  if (!P.fsm.on || P.fsm.b != b || old_trail != P.fsm_trail.p || old_copy != P.con_logits) drop_decode_graphs(ctx);
  P.fsm.on = true; P.fsm.b = b; P.fsm.max_new = max_new;
  P.fsm_fed = 0;
  OM_HIP(hipMemsetAsync(P.fsm_cnt, 0, (size_t)c.max_batch * 4, s));
  OM_HIP(hipMemcpy2DAsync(P.fsm_trail.p, (size_t)P.fsm_cap * 4, start_states, 4, 4, (size_t)b, hipMemcpyHostToDevice, s));
  OM_HIP(hipStreamSynchronize(s));     // the caller's states
  return 0;
}

extern "C" int omchat_fsm_states(omchat_ctx* ctx, int b, int32_t* out, void* stream) {
  OM_CHECK(ctx && out, "null argument");
  const PickState& P = ctx->pick;
  OM_CHECK(P.fsm.on && b >= 1 && b <= P.fsm.b, "omchat_fsm_states: rows that omchat_fsm_begin switched on");
  (void)stream;
  // (as the other accessors read: the device idle, then blocking copies -- the counts and the rows' trails)
  OM_HIP(hipDeviceSynchronize());
  std::vector<int> cnt(b);
  std::vector<int32_t> trail((size_t)b * P.fsm_cap);
  OM_HIP(hipMemcpy(cnt.data(), P.fsm_cnt, (size_t)b * 4, hipMemcpyDeviceToHost));
  OM_HIP(hipMemcpy(trail.data(), P.fsm_trail.p, trail.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < b; ++i) out[i] = trail[(size_t)i * P.fsm_cap + std::min(std::max(cnt[i], 0), P.fsm_cap - 1)];
  return 0;
}

// ---- classifier-free guidance (include/omchat_hip.h)
// The scale, b and the buffers are kernel arguments of the captured decode graphs, as the sampler's parameters are: a change drops them, the
// same b and scale on the next call keep them.
extern "C" int omchat_set_guidance(omchat_ctx* ctx, int b, float scale, void* stream) {
  (void)stream;
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  if (b <= 0) {
    if (P.gd.on) drop_decode_graphs(ctx);
    P.gd = PickState::Guidance{};
    return 0;
  }
  // every refusal before anything is allocated or changed
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(ctx->tp_size == 1, "guidance: one GPU (the vocabulary-parallel exchange of the two log-sum-exps is not built)");
  OM_CHECK(2 * b <= c.max_batch, "guidance: b rows and their b twins exceed max_batch");
  OM_CHECK(isfinite(scale), "guidance: the scale must be a finite float");
  OM_CHECK(!ctx->beam.on(), "guidance: a beam search is active");
  OM_CHECK(!ctx->group.on(), "guidance: a sampled group shares its prompt (omchat_group_begin with b = 0 first)");
  OM_CHECK(!P.dola.on, "guidance: layer-contrastive decoding is on (omchat_set_dola with b = 0 first); the two stages write the same copy");
  OM_CHECK(!ctx->contrastive_on(), "guidance: contrastive search is on (omchat_set_contrastive with k = 0 first); each candidate row would need its twin");
  void* old_copy = P.con_logits;
  if (!P.gd_ws) TRY(ctx->alloc(&P.gd_ws, guidance_ws_bytes(c.max_batch / 2, c.t_vocab)));
  if (!P.con_logits) TRY(ctx->alloc((void**)&P.con_logits, (size_t)c.max_batch * c.t_vocab * 4));
  if (!P.gd.on || P.gd.b != b || P.gd.scale != scale || old_copy != P.con_logits) drop_decode_graphs(ctx);
  P.gd.on = true; P.gd.b = b; P.gd.scale = scale;
  return 0;
}

// ---- layer-contrastive decoding (include/omchat_hip.h)
// b, k, the layers, relative_top, norm and the buffers are kernel arguments (or launches) of the captured decode graphs: a change drops them,
// the same values on the next call keep them.  Every call begins a new record.
extern "C" int omchat_set_dola(omchat_ctx* ctx, int b, const int32_t* layers, int k, float relative_top, int norm, void* stream) {
  OM_CHECK(ctx, "null ctx");
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  if (b <= 0) {
    if (P.dola.on) drop_decode_graphs(ctx);
    P.dola = PickState::Dola{};
    P.dola_fresh = false;
    return 0;
  }
  // every refusal before anything is allocated or changed
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  if (const char* why = dola_state_refusal(ctx)) OM_CHECK(false, why);
  OM_CHECK(layers && k >= 1 && k <= OMCHAT_DOLA_MAX_LAYERS, "layer-contrastive decoding: 1 <= k <= 16 candidate layers");
  const int R = std::min(c.max_batch, 32);
  OM_CHECK((int64_t)(k + 1) * b <= R, "layer-contrastive decoding: (k + 1) * b rows go through the head in one pass: at most min(max_batch, 32)");
  OM_CHECK(relative_top > 0.f && relative_top <= 1.f, "layer-contrastive decoding: relative_top must lie in (0, 1]");
  PickState::Dola p;
  p.on = true; p.norm = norm != 0; p.b = b; p.k = k; p.relative_top = relative_top;
  for (int j = 0; j < k; ++j) {
    OM_CHECK(layers[j] >= 0 && layers[j] < c.t_layers, "layer-contrastive decoding: a candidate index outside [0, num_hidden_layers) of HF's hidden_states");
    for (int i = 0; i < j; ++i) OM_CHECK(layers[i] != layers[j], "layer-contrastive decoding: the candidate layers must be distinct");
    p.layers[j] = layers[j];
  }
  void* old_copy = P.con_logits;
  if (!P.dola_logits) {
    const size_t nt = (size_t)cdiv(c.t_vocab, 2048);
    TRY(ctx->alloc((void**)&P.dola_logits, (size_t)R * c.t_vocab * 4));
    TRY(ctx->alloc(&P.dola_hid, (size_t)R * c.t_hidden * 2));
    P.dola_ws_cap = (size_t)R * nt * 12;      // >= dola_ws_bytes(b, k, V) for every (k + 1) * b <= R
    TRY(ctx->alloc(&P.dola_ws, P.dola_ws_cap));
    TRY(ctx->alloc((void**)&P.dola_layers, (size_t)OMCHAT_DOLA_MAX_LAYERS * 4));
    TRY(ctx->alloc((void**)&P.dola_cnt, (size_t)c.max_batch * 4));
    P.dola_cap = c.max_seq + 1;      // a sequence cannot be picked for more often than it has slots
    TRY(ctx->grow(P.dola_rec, (size_t)P.dola_cap * c.max_batch * 4));
  }
  OM_CHECK(dola_ws_bytes(b, k, c.t_vocab) <= P.dola_ws_cap, "layer-contrastive decoding: workspace");
  if (!P.con_logits) TRY(ctx->alloc((void**)&P.con_logits, (size_t)c.max_batch * c.t_vocab * 4));
  if (!(p == P.dola) || old_copy != P.con_logits) drop_decode_graphs(ctx);
  P.dola = p;
  P.dola_fresh = false;
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemcpyAsync(P.dola_layers, P.dola.layers, (size_t)OMCHAT_DOLA_MAX_LAYERS * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemsetAsync(P.dola_cnt, 0, (size_t)c.max_batch * 4, s));
  OM_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" int omchat_dola_read(omchat_ctx* ctx, int32_t* out, int rows, int steps) {
  OM_CHECK(ctx && out, "null argument");
  const PickState& P = ctx->pick;
  const int mb = ctx->c.max_batch;
  OM_CHECK(P.dola_cnt && rows >= 1 && rows <= mb && steps >= 0, "omchat_dola_read: rows that omchat_set_dola switched on");
  OM_HIP(hipDeviceSynchronize());
  std::vector<int> cnt(mb);
  OM_HIP(hipMemcpy(cnt.data(), P.dola_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
  const int lines = std::min(steps, P.dola_cap);
  std::vector<int32_t> rec((size_t)lines * mb);
  if (lines) OM_HIP(hipMemcpy(rec.data(), P.dola_rec.p, rec.size() * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < rows; ++r)
    for (int t = 0; t < steps; ++t) out[(size_t)r * steps + t] = t < lines && t < cnt[r] ? rec[(size_t)t * mb + r] : -1;
  return 0;
}

extern "C" int omchat_dola_rows(omchat_ctx* ctx, float* out) {
  OM_CHECK(ctx && out, "null argument");
  const PickState& P = ctx->pick;
  OM_CHECK(P.dola.on && P.dola_fresh, "omchat_dola_rows: no prefill or step has run since omchat_set_dola");
  OM_HIP(hipDeviceSynchronize());
  OM_HIP(hipMemcpy(out, P.dola_logits, (size_t)P.dola.rows() * ctx->c.t_vocab * 4, hipMemcpyDeviceToHost));
  return 0;
}
