// The context of one tensor-parallel rank and the state of the stages that own a part of it.  Private: for the .hip files that implement
// context-level entry points (model.hip, pick.hip, beam.hip); the public interface is include/omchat_hip.h.
#pragma once
#include "kernels.h"
#include "../../include/omchat_hip.h"
#include <rccl/rccl.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

extern int g_fuse_peer_norm;      // model.hip: omchat_op_set_tuning key 9

enum RouteKind { R_PLAIN = 0, R_GATE = 1, R_UP = 2, R_PATCH = 3 };
struct Route {
  void* dst = nullptr;
  int64_t rows = 0, cols = 0;     // logical source shape (2-D view)
  int64_t dst_ld = 0;             // destination row stride (elements)
  int kind = R_PLAIN;
  bool loaded = false;
  float synth_std = 0.02f, synth_off = 0.f;
};

// a device buffer grown on demand and never shrunk (omchat_ctx::grow)
struct Grown {
  void* p = nullptr; size_t cap = 0;
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// The token pick of a step (pick.hip): guidance or layer-contrast stage, ban stage, automaton stage, argmax or sampler, record stage -- with everything the
// stages keep between picks.
struct PickState {
  void* arg_scratch = nullptr;      // partials of the two-stage argmax
  float* tp_table = nullptr;        // (max, index) / sampler exchange table under tensor parallelism
  // on-device sampling (omchat_set_sampling; sample.hip): uniform parameters for the batch, per-row device step counters, the repetition
  // penalty's seen-token bitmap of this rank's vocabulary slice [max_batch][smp_bmw] and the local index of the bit each row's last pick set
  struct Sampling { bool on = false; uint64_t seed = 0; float temperature = 1.f; int top_k = 0; double top_p = 1.0; float penalty = 1.f; };
  Sampling smp;
  // the four filters behind top-p (omchat_set_sampling_filters; off after omchat_set_sampling).  They live in the kernel arguments of the
  // captured decode graphs like the other parameters: smp_f_graph = what the graphs were captured with, compared in front of every step
  // (pick_admit), so that the set_sampling + set_sampling_filters pair of a generate() call with unchanged values keeps the graphs
  SampleFilters smp_f, smp_f_graph;
  void* smp_ws = nullptr;
  uint32_t* smp_bm = nullptr; int smp_bmw = 0;
  int *smp_last = nullptr, *smp_step = nullptr;
  // sampled verify step (omchat_decode_verify with OMCHAT_VERIFY_SAMPLE): the per-row seen bitmaps [16][smp_bmw] (allocated by the first such
  // step with the penalty on), the local indices of the bits its committed picks newly set (device [16], -1 = none: the verify counterpart of
  // smp_last) and how many of those picks omchat_kv_rewind can still take back (host; 0 once any other pick ran)
  uint32_t* smp_vseen = nullptr;
  int* smp_vlast = nullptr;
  int smp_vcommit = 0;
  // HF logits constraints (omchat_set_constraints; constrain.hip): uniform parameters, the rows' token history as HF's processors see it
  // [max_batch][con_ld] with device lengths, the id lists, the ban bitmap of this rank's vocabulary slice (all-zero between picks) and the
  // banned copy of the logits the pick runs on.  con_fed: decode steps fed since the begin (host bound for the history's capacity).
  struct Constraints {
    bool on = false; int b = 0, ngram = 0, min_new = 0, min_len = 0, n_eos = 0, n_sup = 0, n_bsup = 0, n_bw = 0;
    bool operator==(const Constraints& o) const {
      return on == o.on && b == o.b && ngram == o.ngram && min_new == o.min_new && min_len == o.min_len && n_eos == o.n_eos && n_sup == o.n_sup &&
             n_bsup == o.n_bsup && n_bw == o.n_bw;
    }
  };
  Constraints con;
  int con_ld = 0, con_fed = 0, con_room = 0;
  int *con_len = nullptr, *con_plen = nullptr;
  int32_t* con_lists = nullptr;
  uint32_t* con_ban = nullptr; int con_bmw = 0;
  float* con_logits = nullptr;
  // per-token log-probabilities of the picked ids (omchat_set_logprobs; logprob.hip): the record float [2][max_new][max_batch] (raw, processed)
  // with a device counter per row, the slice partials, the exchange table under tensor parallelism; lp_picks: picks enqueued since the
  // begin (host bound for the record's capacity)
  struct Logprobs { bool on = false; int b = 0, max_new = 0; };
  Logprobs lp;
  // extras of the record (omchat_set_logprobs_ex; nothing of this is allocated before they are asked for): top_n alternatives and the
  // n_score scored ids of every pick.  lp_xrec = [vals float | ids int32][lp_cap][max_batch][top_n] then scored float
  // [lp_cap][max_batch][n_score], written at the same device counters as lp_rec; lp_xws the slices' candidates, lp_sid the scored ids
  // (device), lp_xtable the exchange table with room for them (it replaces lp_table while they are on)
  struct Extras {
    int top_n = 0, n_score = 0; std::vector<int32_t> ids;
    bool on() const { return top_n > 0 || n_score > 0; }
    bool operator==(const Extras& o) const { return top_n == o.top_n && n_score == o.n_score && ids == o.ids; }
  };
  Extras lpx;
  void* lp_xws = nullptr;
  int32_t* lp_sid = nullptr;
  float* lp_xtable = nullptr;
  Grown lp_xrec;
  float* lpx_vals() const { return (float*)lp_xrec.p; }
  int32_t* lpx_ids(int cap, int mb) const { return (int32_t*)lp_xrec.p + (size_t)cap * mb * lpx.top_n; }
  float* lpx_scored(int cap, int mb) const { return (float*)lp_xrec.p + (size_t)2 * cap * mb * lpx.top_n; }
  int lp_picks = 0;
  int lp_cap = 0;      // lines per plane of the record as allocated (>= lp.max_new; grown, never shrunk): the stride the kernels are given
  int* lp_cnt = nullptr;
  void* lp_ws = nullptr;
  float* lp_table = nullptr;
  Grown con_hist;    // token history of the logits constraints (omchat_set_constraints)
  Grown lp_rec;      // record of the per-token log-probabilities (omchat_set_logprobs)
  // finite-state token constraints (omchat_fsm_load / omchat_fsm_begin; fsm.hip): the table [off | tok | nxt] in one buffer, sticky until
  // replaced; the rows' state trail [max_batch][fsm_cap] with device counts, the state of the current pick, the allowed bitmap of this
  // rank's vocabulary slice (all-zero between picks).  The masked copy is con_logits, shared with the ban stage (allocated by whichever
  // setter comes first).  fsm_fed: decode steps fed since the begin (host bound for the trail's room)
  struct Fsm { bool on = false; int b = 0, max_new = 0; };
  Fsm fsm;
  FsmTable fsm_tab;
  std::vector<int32_t> fsm_off_host;      // the table's offsets on the host: the begin checks that a start state has an edge
  Grown fsm_mem, fsm_trail;
  int fsm_cap = 0, fsm_fed = 0;
  int *fsm_cnt = nullptr;
  int32_t* fsm_cur = nullptr;
  uint32_t* fsm_bm = nullptr; int fsm_bmw = 0;
  // classifier-free guidance (omchat_set_guidance; guidance.hip): while it is on for b rows a pick is handed 2b rows of logits -- rows
  // [b, 2b) the twins over the negative prompt -- and picks b ids from the guided scores, which the stage writes to con_logits (shared
  // with the two stages behind it); every other piece of pick state keeps b rows.  gd_ws: the tile partials of the two log-sum-exps
  struct Guidance { bool on = false; int b = 0; float scale = 1.f; };
  Guidance gd;
  void* gd_ws = nullptr;
  // layer-contrastive decoding (omchat_set_dola; dola.hip): while it is on for b rows a prefill or step leaves (k + 1) b raw rows in
  // dola_logits -- the final rows, then candidate j's at (1 + j) b + r -- from the hidden rows dola_hid [(k + 1) b][H] it kept at the layers
  // of the list (device copy dola_layers, for the record); the stage writes the b rows of contrasted scores to con_logits.  dola_rec int32
  // [dola_cap][max_batch] with a device counter per row: the HF index of every pick's layer.  dola_fresh: dola_logits holds the rows of the
  // last prefill or step (a pick without them is refused)
  struct Dola {
    bool on = false, norm = false; int b = 0, k = 0; float relative_top = 0.1f; int layers[DOLA_MAX_LAYERS] = {};
    bool operator==(const Dola& o) const {
      return on == o.on && norm == o.norm && b == o.b && k == o.k && relative_top == o.relative_top && std::equal(layers, layers + DOLA_MAX_LAYERS, o.layers);
    }
    int rows() const { return (k + 1) * b; }
    int slot(int hf_index) const { for (int j = 0; j < k; ++j) if (layers[j] == hf_index) return j; return -1; }      // position in the list, or -1
  };
  Dola dola;
  float* dola_logits = nullptr;
  void* dola_hid = nullptr;
  void* dola_ws = nullptr; size_t dola_ws_cap = 0;
  int32_t* dola_layers = nullptr;
  int* dola_cnt = nullptr;
  Grown dola_rec; int dola_cap = 0;
  bool dola_fresh = false;
  bool dola_on() const { return dola.on; }
  bool guidance_on() const { return gd.on; }
  int pick_rows(int rows) const { return gd.on ? rows / 2 : rows; }      // the rows that pick, of the rows a step runs
  bool sampling_on() const { return smp.on; }
  bool constraints_on() const { return con.on; }
  bool logprobs_on() const { return lp.on; }
  bool fsm_on() const { return fsm.on; }
  void release() { con_hist.release(); lp_rec.release(); lp_xrec.release(); fsm_mem.release(); fsm_trail.release(); dola_rec.release(); }
};

// beam search (omchat_beam_begin; beam.hip): parameters of the current search, its step counter, and device buffers grown on demand
// (state words, exchange table, length-penalty denominators, parent rows, stash of the KV gather)
struct BeamState {
  struct Search { bool on = false; int b = 0, N = 0, KB = 0, max_new = 0, P = 0, es = 0, ns = 1, t = 0; float lp = 1.f; std::vector<int> eos; };
  Search cur;
  // the search runs on processed scores (omchat_beam_processors; off after every omchat_beam_begin): penalty and ban parameters, the two
  // per-path history buffers [2][b * N][ld] used in turn (hist), the id lists with the rows' lengths behind them (aux) and the ban and seen
  // bitmaps [2][b * N][bmw], all-zero between steps (bm)
  struct Proc { bool on = false; float penalty = 1.f; int ngram = 0, min_new = 0, min_len = 0, n_eos = 0, n_sup = 0, n_bsup = 0, n_bw = 0, P = 0, ld = 0, bmw = 0; };
  Proc proc;
  Grown state, table, dn, parents, stash, hist, aux, bm;
  bool stash8 = false;
  std::vector<int> hpos, hlen;      // host sources of the fork's device lengths (alive until the next begin)
  bool on() const { return cur.on; }
  void end() { cur.on = false; }
  void release() { for (Grown* g : {&state, &table, &dn, &parents, &stash, &hist, &aux, &bm}) g->release(); }
};

// sampled groups (omchat_group_begin; beam.hip): the shared-prompt mode of the decode step -- b prompts x N sibling rows whose prompt keys
// [0, P) only the group's first row holds -- and the partials of its attention (grown on demand)
struct GroupState {
  bool share = false; int b = 0, N = 0, P = 0;
  Grown ws;
  std::vector<int> hpos, hlen;      // host sources of the begin's device lengths (alive until the next begin)
  bool on() const { return share; }
  void end() { share = false; }
  void release() { ws.release(); }
};

// contrastive search (omchat_set_contrastive; contrastive.hip): the history H_ctx of post-final-norm hidden rows
// [cap][t_hidden] (16-bit) with one fp32 inverse L2 norm per row, the candidates of the next k-row step (ids, probabilities), the partial
// maxima of the penalty launch (part), the top-k's tile partials (tk_ws), the parents / selected row of the last pick, the per-step record
// and the one-slot stash of the KV gather.
// n_hist: rows of the history (host; P after the prefill, + 1 per pick); t: picks made; forked: the prompt row was forked / shared into k rows
struct ContrastiveState {
  bool on = false, share = false; int k = 0, max_new = 0; float alpha = 0.f, one_minus = 1.f;      // (one_minus: fp32(1 - alpha), as torch rounds the scalar)
  std::vector<int> eos;
  int cap = 0, n_hist = 0, t = 0, P = 0;
  bool have_hist = false, forked = false;
  Grown hist, inv, part, tk_ws, small, rec, stash;
  // `small` (int32 words): [0, 16) candidate ids, [16, 32) candidate probabilities, [32, 48) inverse norms of the step's rows, [48, 64) parents,
  // [64] the selected row
  int32_t* cand_ids() const { return (int32_t*)small.p; }
  float* cand_probs() const { return (float*)small.p + 16; }
  float* cand_inv() const { return (float*)small.p + 32; }
  int* parents() const { return (int*)small.p + 48; }
  int* sel() const { return (int*)small.p + 64; }
  void release() { for (Grown* g : {&hist, &inv, &part, &tk_ws, &small, &rec, &stash}) g->release(); }
};

struct omchat_ctx {
  omchat_config c;
  int dt = OMCHAT_BF16;
  int tp_rank = 0, tp_size = 1;
  ncclComm_t comm = nullptr;
  std::vector<void*> allocs;
  size_t bytes = 0;
  std::unordered_map<std::string, Route> routes;

  // derived geometry
  int v_np = 0, v_ntok = 0, v_Cq = 0, v_kpad = 0, v_hd = 128;
  int t_qdim = 0, t_kvdim = 0, t_qkvdim = 0;

  // weights (device, compute dtype)
  struct VitLayer { void *ls1, *ls2, *n1, *n2, *n1b, *n2b, *wqkv, *qn, *kn, *wproj, *bproj, *w1, *b1, *w2, *b2; };
  struct DecLayer { void *ln1, *ln2, *wqkv, *bqkv, *wo, *wgu, *wd; };
  // The decode step streams five projections per pass -- qkv, o_proj, gate|up, down_proj of every layer and the lm_head -- and can read each
  // of them in one of the formats of omchat_weight_format (include/omchat_hip.h).  wt[format] is that format's table: layers * 4 + 1
  // references in layer order, the lm_head last, plus the replica's state.
  //   16-bit         a view of dl[] / t_lm filled at context build: never stale.  Prefill and the experiments launches read dl[] itself
  //   16-bit packed  MFMA fragment order for BATCHED steps (2 <= b <= 32), every wave load 1 KiB contiguous (gemv.hip: gemv_pk_kernel; +14 GB at
  //                  OmChat-13B, built on the first batched step; omchat_op_set_tuning key 6 = 0 disables it).  Optional: when it does not
  //                  fit, the context remembers that (W_UNAVAILABLE) and batched steps keep streaming the row-major weights
  //   e4m3           omchat_enable_fp8_decode: OCP e4m3 bytes + one fp32 scale per output row (batch-1 steps; the fp8 x fp8 prefill GEMMs too)
  //   MXFP4          omchat_enable_mxfp4_decode: two e2m1 codes per byte [N][K / 2] + one e8m0 byte per 32 consecutive
  //                  k [N][K / 32], row-major (batch-1 steps)
  //   MXFP4 packed   mode 2: the same codes and scales in the packed layout of the batched GEMV forms (common.h: packed_w4_index /
  //                  packed_s4_index; launch_pack_w4 shuffles the row-major replica, the quantiser stays the one source of the codes)
  // A replica's buffers are taken all or nothing (alloc_group) and rebuilt IN PLACE after omchat_load_tensor: same device pointers, so a
  // captured decode graph stays valid (model.hip: build_replica).
  enum Proj { P_QKV = 0, P_O = 1, P_GU = 2, P_DOWN = 3, P_LM = 4 };      // P_LM: the one entry behind the layers
  struct WRef { void* W = nullptr; int ldw = 0; float* w_scale = nullptr; unsigned char* mx_scale = nullptr; int packed = 0; };
  enum WState { W_ABSENT = 0, W_BUILT, W_STALE, W_UNAVAILABLE };      // (W_UNAVAILABLE: the 16-bit packed replica did not fit, stop trying)
  struct WTable { std::vector<WRef> e; int state = W_ABSENT; };
  WTable wt[OMCHAT_WFMT_COUNT];
  const WRef* layer_w(int fmt, int layer) const { return &wt[fmt].e[(size_t)layer * 4]; }      // [P_QKV .. P_DOWN]
  const WRef& lm_w(int fmt) const { return wt[fmt].e.back(); }
  bool built(int fmt) const { return wt[fmt].state == W_BUILT; }
  // bf16x12: the lossless 12-bit coding of the three long batch-1 launches' bf16 rows -- another encoding of the
  // OMCHAT_WFMT_16 weights, bit for bit, so a table of its own and no value of the public enum.  One table per role (gate|up and down_proj of
  // every layer, the lm_head), each taken all or nothing and built by the first batch-1 step that will use it; an entry whose tensor has a
  // row over the patch cap is not coded (ok = false) and its projection keeps the 16-bit launch.  W_UNAVAILABLE: no room, or a K the forms
  // do not take -- nothing is retried.  Re-encoded in place after omchat_load_tensor.
  enum X12Role { X12_GU = 0, X12_DOWN = 1, X12_LM = 2, X12_ROLES = 3 };
  struct X12Ref { void* W = nullptr; unsigned char* top = nullptr; unsigned char* cnt = nullptr; unsigned* patch = nullptr; bool ok = false; };
  struct X12Table { std::vector<X12Ref> e; int state = W_ABSENT; };
  X12Table x12[X12_ROLES];
  int* x12_over = nullptr;      // device: one flag per entry of the role being encoded
  long x12_launches[X12_ROLES] = {0, 0, 0};      // coded launches enqueued by eager steps and captures, per role (omchat_bf16x12_stats: the tests ask which launch a projection took)
  bool fp8_decode = false;
  int mxfp4_mode = 0;      // omchat_enable_mxfp4_decode: 0 = off, 1 = batch-1 steps, 2 = steps of 2 <= b <= 32 rows as well
  // BASELINE configs[4]: fp8 KV cache for decode (e4m3 bytes in the layout of the 16-bit cache + one fp32 scale per (layer, sequence,
  // kv head, position)) and fp8 x fp8 MFMA prefill GEMMs (qkv and gate|up: the activations come quantised per token from the RMSNorm)
  void *k8cache = nullptr, *v8cache = nullptr;
  float *ks8 = nullptr, *vs8 = nullptr;
  bool fp8_kv = false, kv8_valid = false, fp8_prefill = false;
  void* tw_q8 = nullptr; float* tw_q8s = nullptr;
  int64_t scale_layer_stride() const { return (int64_t)c.max_batch * c.t_kv_heads * c.max_seq; }
  // decode step as a hipGraph (omchat_enable_decode_graph): ~230 launches per token replayed as one graph launch.  Captured on a
  // context-owned stream (the caller's may be the legacy null stream, which cannot capture) with context-owned token / logits
  // buffers so that every kernel argument is replay-invariant; the split-KV attention grid is captured for `cap_len` keys
  // (empty splits exit at once) and the graph is re-captured when a sequence outgrows it.
  // (shared-prompt mode of a sampled group: N, P and the workspace are kernel arguments too, so the graph remembers them and is captured again
  // when they change; its cap_len is the suffix bucket the eager step would take, so both issue the same launches)
  struct DecodeGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int cap_len = 0, grp_N = 0, grp_P = 0; const void* grp_ws = nullptr; };
  std::unordered_map<int, DecodeGraph> graphs;      // key = b * 8 + (MXFP4 weights ? 4 : 0) + (fp8 weights ? 2 : 0) + (fp8 KV cache ? 1 : 0), the weights by the step's format; + (1 << 19) with layer-contrastive decoding on, + (1 << 20) in the shared-prompt mode, + the bf16x12 roles << 21 (b <= 32: the fields do not overlap)
  bool graph_on = false;
  hipStream_t graph_stream = nullptr;
  hipEvent_t graph_ev_in = nullptr, graph_ev_out = nullptr;
  int32_t *d_tok_in = nullptr, *d_tok_out = nullptr;
  long graph_steps = 0, graph_replays = 0, graph_captures = 0;
  void *v_cls = nullptr, *v_pos = nullptr, *v_wpatch = nullptr, *v_bpatch = nullptr;
  std::vector<VitLayer> vl;
  void *p_w0 = nullptr, *p_b0 = nullptr, *p_w2 = nullptr, *p_b2 = nullptr;
  void *t_embed = nullptr, *t_norm = nullptr, *t_lm = nullptr;
  std::vector<DecLayer> dl;
  float* rope = nullptr;          // [max_seq][64][2]

  // workspaces
  void *vw_cols = nullptr, *vw_pe = nullptr, *vw_x = nullptr, *vw_x2 = nullptr, *vw_xn = nullptr, *vw_qkv = nullptr, *vw_ao = nullptr,
       *vw_h = nullptr, *vw_feat = nullptr, *vw_proj = nullptr;
  float* vw_sumsq = nullptr;
  // round 6, fused ViT layer (vit_run): statistics slots left by the GEMM epilogues, the row scale finished from them, and the copies of
  // the qkv / fc1 weights with norm1 / norm2's weight folded into their columns (W'[n][k] = T(W[n][k] * w_norm[k])); rebuilt after a reload
  float *vw_stats_x = nullptr, *vw_stats_qk = nullptr, *vw_rstd = nullptr;
  int vw_stats_x_ld = 0, vw_stats_qk_ld = 0, vw_stats_x_ld_used = 1;      // (_used: slots of x's statistics written by the last producer)
  struct VitFold { void *wqkv = nullptr, *w1 = nullptr; };
  std::vector<VitFold> vfold;
  bool vfold_stale = true;
  void *tw_x = nullptr, *tw_x2 = nullptr, *tw_xn = nullptr, *tw_qkv = nullptr, *tw_ao = nullptr, *tw_act = nullptr, *tw_last = nullptr;
  float* tw_logits = nullptr;
  void* sk_ws = nullptr; size_t sk_ws_bytes = 0;      // stream-K slabs + flags of the MFMA GEMM
  float* tp_f32_ws = nullptr; size_t tp_f32_bytes = 0;      // fp32 partial sums of a row-parallel projection (tuning key 29), grown on demand
  float* tw_part = nullptr;       // split-K fp32 slices of the decode o_proj / down_proj [KS_MAX][max_batch][H]
  float* tw_attn_ws = nullptr;
  size_t tw_attn_ws_bytes = 0;
  // fused attention + merge + o_proj launch of the batch-1 decode step (fused_decode.hip): granule buffers, sticky time-out word, and the
  // launch counter that tags the granules of one launch
  void* fd_ws = nullptr;
  unsigned* fd_err = nullptr;
  unsigned fd_epoch = 0;
  long n_fused_launches = 0;
  // one-launch decoder layer (decode_layer.hip): granule buffers; shares the error word and the launch counter above
  void* dl_ws = nullptr;
  long n_layer_launches = 0;
  unsigned long long* dbg_stamps = nullptr;      // experiments build: [layers][8] clock stamps of the last decode step (tuning key 42 bit 4)
  unsigned* dyn_ctr = nullptr;      // [layers][65 * 64] work counters of the dynamic gate|up GEMV (gemv_rows_norm_dyn_kernel), zero between launches
  int *d_pos = nullptr, *d_len = nullptr, *d_idx = nullptr, *d_start = nullptr;
  int* d_verify_n = nullptr;      // omchat_decode_verify: accepted drafts of the last verify step
  PickState pick;
  BeamState beam;
  GroupState group;
  ContrastiveState cs;
  bool contrastive_on() const { return cs.on; }
  Grown ext_ws;      // partials of the split-KV block attention (omchat_prefill_extend)
  Grown score_ws;    // (max, sum) planes and target logits of teacher-forced scoring (omchat_score_hidden)
  int grow(Grown& g, size_t n) {
    if (n <= g.cap) return 0;
    if (g.p) { hipFree(g.p); bytes -= g.cap; g.p = nullptr; g.cap = 0; }
    hipError_t e = hipMalloc(&g.p, n);
    if (e != hipSuccess) { omchat_set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e)); return 2; }
    g.cap = n; bytes += n;
    return 0;
  }
  bool left_padded = false;
  // decode of a padded batch as the reference computes it (omchat_decode_step_masked): every row's cache holds pre_S + masked_steps slots;
  // dec_mode: 0 = no decode step since the prefill, 1 = omchat_decode_step (per-sequence lengths), 2 = omchat_decode_step_masked
  int pre_S = 0, pre_b = 0, masked_steps = 0, dec_mode = 0;
  unsigned char* d_mask = nullptr; int64_t mask_sb = 0;
  bool mask_on_device = false;      // d_mask holds [prompt mask | ones] for the whole cache (omchat_masked_decode_begin)
  void *kcache = nullptr, *vcache = nullptr;   // [layers][max_batch][kv_heads][max_seq][128]
  std::vector<int> h_len;
  // optional per-kernel-class HIP-event timing (bench.py roofline): category -> event pairs recorded on the launch stream
  struct Prof { std::vector<hipEvent_t> ev; size_t used = 0; double ms = 0; long count = 0; };
  bool prof_on = false;
  Prof prof[OMCHAT_PROF_CATS];
  void prof_mark(int cat, hipStream_t s) {
    if (!prof_on) return;
    Prof& p = prof[cat];
    if (p.used == p.ev.size()) { hipEvent_t e; hipEventCreate(&e); p.ev.push_back(e); }
    hipEventRecord(p.ev[p.used++], s);
  }
  void* stage_f32 = nullptr; size_t stage_f32_bytes = 0;
  void* stage_t = nullptr; size_t stage_t_bytes = 0;

  int alloc(void** p, size_t n) {
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(p, n);
    if (e != hipSuccess) { omchat_set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e)); return 2; }
    allocs.push_back(*p);
    bytes += n;
    return 0;
  }
  // a group of buffers or none: sizes[i] bytes into *slots[i]; when one hipMalloc fails the ones already taken are freed, nothing is recorded
  // and every slot is null again (a half-built table must never reach a launch)
  int alloc_group(const std::vector<void**>& slots, const std::vector<size_t>& sizes) {
    std::vector<void*> got;
    size_t total = 0;
    for (size_t i = 0; i < slots.size(); ++i) {
      const size_t n = sizes[i] ? sizes[i] : 16;
      const hipError_t e = hipMalloc(slots[i], n);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void* p : got) (void)hipFree(p);
        for (void** s : slots) *s = nullptr;
        omchat_set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
        return 2;
      }
      got.push_back(*slots[i]);
      total += n;
    }
    for (void* p : got) allocs.push_back(p);
    bytes += total;
    return 0;
  }
  size_t esz() const { return 2; }
  int64_t cache_layer_stride() const { return (int64_t)c.max_batch * c.t_kv_heads * c.max_seq * 128; }
  int64_t cache_sb() const { return (int64_t)c.t_kv_heads * c.max_seq * 128; }
  int64_t cache_sh() const { return (int64_t)c.max_seq * 128; }
  static constexpr float T_ATTN_SCALE = 0.08838834764831845f;      // the decoder's softmax scale: head_dim ** -0.5, head dim 128
  // The operands of layer i's split-KV attention (launch_attn_decode, launch_attn_block): Q = the q columns of tw_qkv, one row per token;
  // K / V = the layer's cache planes; O = tw_ao.  new_rows: with the fused-append view -- the rope table and the raw k / v columns of tw_qkv.
  // The caller chooses the workspace, o_pack_nb and the launch's own integers.
  void bind_attn(AttnOperands& a, int i, bool new_rows) const {
    a.Q = tw_qkv; a.q_sb = t_qkvdim; a.q_sh = 128;
    a.K = (char*)kcache + (size_t)i * cache_layer_stride() * 2; a.k_sb = cache_sb(); a.k_sh = cache_sh(); a.k_sr = 128;
    a.V = (char*)vcache + (size_t)i * cache_layer_stride() * 2; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = 128;
    a.O = tw_ao; a.o_sb = t_qdim; a.o_sh = 128;
    a.q_heads = c.t_heads; a.kv_heads = c.t_kv_heads; a.scale = T_ATTN_SCALE;
    if (!new_rows) return;
    a.rope = rope; a.rope_max = c.max_seq; a.new_sb = t_qkvdim;
    a.k_new = (const char*)tw_qkv + (size_t)t_qdim * 2; a.v_new = (const char*)tw_qkv + (size_t)(t_qdim + t_kvdim) * 2;
  }

  omchat_allreduce_fn hook = nullptr;
  void* hook_user = nullptr;
  // tensor-parallel prefill / ViT: the all-reduce of a row-parallel projection runs on its own stream, one row chunk behind the GEMM
  static constexpr int AR_CHUNKS = 4;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_chunk[AR_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_comm_done = nullptr;
  // sequence-parallel form: the all-gather of row chunk i is done (communication stream); the NEXT column-parallel GEMM is issued per row chunk
  // behind these events, so the exchange of chunk i + 1 also runs under the consumer's chunk i (gemm_sp / gemm_after_sp)
  hipEvent_t ev_ag[AR_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
  int sp_pend_nch = 0, sp_pend_rows_per = 0;
  // transports of the tensor-parallel sum, in order of precedence: the test hook; the peer (IPC / xGMI) all-reduce of comm.hip for
  // messages up to peer_max bytes (one-shot: decode-sized) or for every size when there is no RCCL communicator / peer_all is set;
  // RCCL otherwise.  Every buffer passed here is context-owned with >= 16 bytes of slack, so the peer path may round the count up
  // to whole 16-byte pieces (the extra elements are summed and never read).
  omchat_peer* peer = nullptr;
  size_t peer_max = 256 * 1024;
  bool peer_all = false;
  long n_ar_peer = 0, n_ar_rccl = 0;
  int allreduce_any(void* buf, size_t count, int dtype, hipStream_t s) {
    if (tp_size == 1) return 0;
    if (hook) return hook(hook_user, buf, count, dtype, s);
    const size_t esz = dtype == OMCHAT_F32 ? 4 : 2;
    if (peer && (count * esz <= peer_max || !comm || peer_all)) {
      const size_t per16 = 16 / esz;
      ++n_ar_peer;
      return omchat_peer_allreduce(peer, buf, (count + per16 - 1) / per16 * per16, dtype, s);
    }
    if (!comm) { omchat_set_error("tensor-parallel context without a transport: pass an RCCL communicator or call omchat_ctx_set_peer"); return 1; }
    ++n_ar_rccl;
    const ncclDataType_t t = dtype == OMCHAT_F32 ? ncclFloat32 : (dtype == OMCHAT_F16 ? ncclFloat16 : ncclBfloat16);
    ncclResult_t r = ncclAllReduce(buf, buf, count, t, ncclSum, comm, s);
    if (r != ncclSuccess) { omchat_set_error(std::string("ncclAllReduce: ") + ncclGetErrorString(r)); return 3; }
    return 0;
  }
  // decode: sum of the split-K slices over the ranks + residual + RMSNorm.  With the peer transport that is ONE launch
  // (omchat_peer_resid_rmsnorm, same bits); with the hook or RCCL: all-reduce of the slices, then the local kernel.
  long n_fused_norm = 0;
  int reduce_resid_rmsnorm(void* x, int ldx, float* part, int ks, const void* w, void* xn, int ldn, int rows, int H, float eps, int pack_nb,
                           hipStream_t s) {
    const size_t bytes = (size_t)ks * rows * H * 4;
    if (tp_size > 1 && !hook && peer && g_fuse_peer_norm && rows <= 128 && bytes <= omchat_peer_capacity(peer) &&
        (bytes <= peer_max || !comm || peer_all)) {
      ++n_fused_norm;
      return omchat_peer_resid_rmsnorm(peer, dt, x, ldx, part, ks, w, xn, ldn, rows, H, eps, pack_nb, s);
    }
    if (tp_size > 1) { const int rc = allreduce_any(part, (size_t)ks * rows * H, OMCHAT_F32, s); if (rc) return rc; }
    return launch_resid_rmsnorm(dt, x, ldx, part, ks, w, xn, ldn, rows, H, eps, s, pack_nb);
  }
  // Sequence-parallel form (round 6): buf = [tp_size][blk_rows][N] 16-bit rows.  reduce_scatter_rows: afterwards block tp_rank holds the sum over
  // the ranks (the other blocks are undefined); all_gather_rows: every rank contributes block tp_rank, afterwards all blocks are whole everywhere.
  // RCCL: ncclReduceScatter / ncclAllGather in place -- together the bytes of ONE all-reduce; peer transport: the two halves of its two-shot
  // all-reduce as kernels of their own (comm.hip omchat_peer_reduce_scatter / omchat_peer_all_gather).  The test hook has all-reduce only:
  // reduce-scatter = all-reduce (every block comes back summed), all-gather = zero the foreign blocks, then all-reduce (x + 0 is exact).
  long n_rs = 0, n_ag = 0;
  bool sp_native(size_t bytes) const { return !hook && comm && !(peer && (bytes <= peer_max || peer_all)); }
  bool sp_peer(size_t bytes) const { return !hook && peer && (bytes <= peer_max || !comm || peer_all); }
  int reduce_scatter_rows(void* buf, int blk_rows, int N, hipStream_t s) {
    if (tp_size == 1) return 0;
    ++n_rs;
    const size_t blk = (size_t)blk_rows * N;
    if (sp_peer(blk * tp_size * 2)) { ++n_ar_peer; return omchat_peer_reduce_scatter(peer, buf, blk, dt, s); }
    if (!sp_native(blk * tp_size * 2)) return allreduce_any(buf, blk * tp_size, dt, s);
    ++n_ar_rccl;
    ncclResult_t r = ncclReduceScatter(buf, (char*)buf + (size_t)tp_rank * blk * 2, blk, dt == OMCHAT_F16 ? ncclFloat16 : ncclBfloat16, ncclSum, comm, s);
    if (r != ncclSuccess) { omchat_set_error(std::string("ncclReduceScatter: ") + ncclGetErrorString(r)); return 3; }
    return 0;
  }
  int all_gather_rows(void* buf, int blk_rows, int N, hipStream_t s) {
    if (tp_size == 1) return 0;
    ++n_ag;
    const size_t blk = (size_t)blk_rows * N;
    if (sp_peer(blk * tp_size * 2)) { ++n_ar_peer; return omchat_peer_all_gather(peer, buf, blk, dt, s); }
    if (!sp_native(blk * tp_size * 2)) {
      if (hook == omchat_allreduce_noop) return 0;      // bench.py --shard-of: one rank's compute with the exchanges removed
      if (tp_rank > 0 && hipMemsetAsync(buf, 0, (size_t)tp_rank * blk * 2, s) != hipSuccess) { omchat_set_error("all_gather_rows: memset"); return 2; }
      if (tp_rank + 1 < tp_size && hipMemsetAsync((char*)buf + (size_t)(tp_rank + 1) * blk * 2, 0, (size_t)(tp_size - 1 - tp_rank) * blk * 2, s) != hipSuccess) {
        omchat_set_error("all_gather_rows: memset"); return 2;
      }
      return allreduce_any(buf, blk * tp_size, dt, s);
    }
    ++n_ar_rccl;
    ncclResult_t r = ncclAllGather((char*)buf + (size_t)tp_rank * blk * 2, buf, blk, dt == OMCHAT_F16 ? ncclFloat16 : ncclBfloat16, comm, s);
    if (r != ncclSuccess) { omchat_set_error(std::string("ncclAllGather: ") + ncclGetErrorString(r)); return 3; }
    return 0;
  }
  int allreduce(void* buf, size_t count, hipStream_t s) { return allreduce_any(buf, count, dt, s); }
  int allreduce_f32(float* buf, size_t count, hipStream_t s) { return allreduce_any(buf, count, OMCHAT_F32, s); }
};

// the weight operand of a GEMV from a table reference: W, ldw, the scales and w_packed -- nothing else
inline void use_weight(GemvArgs& g, const omchat_ctx::WRef& w) {
  g.W = w.W; g.ldw = w.ldw; g.w_scale = w.w_scale; g.mx_scale = w.mx_scale; g.w_packed = w.packed;
}

// ... and from its bf16x12 coding (K = the projection's reduction length)
inline void use_weight_x12(GemvArgs& g, const omchat_ctx::X12Ref& r, int K) {
  g.W = r.W; g.ldw = K / 2 * 3; g.w_scale = nullptr; g.mx_scale = nullptr; g.w_packed = 0;
  g.x12_top = r.top; g.x12_cnt = r.cnt; g.x12_patch = r.patch;
}

// ---- model.hip
int decode_x_pack_nb(const omchat_ctx* ctx, int rows);      // blocks of 16 rows of the packed x layout a decode step of `rows` rows leaves its norm buffer in (0: row-major)
void drop_decode_graphs(omchat_ctx* ctx);      // pick parameters live in the kernel arguments of the captured decode graphs: a change drops them

// ---- pick.hip: what model.hip knows of the pick pipeline
int pick_alloc(omchat_ctx* ctx, int rows);      // context build: scratch of the argmax and the exchange table for picks of up to `rows` rows
// every pick-side refusal of a step before anything is enqueued (the record's room when the step picks, then the history's when it feeds a
// token), then the host counters
int pick_admit(omchat_ctx* ctx, bool picks, bool feeds);
// bare argmax of (rank-local) logits, no stage; `advance` moves the decode positions in the same launch
int greedy_pick(omchat_ctx* ctx, const float* lg, int b, int32_t* next_tokens, hipStream_t s, bool advance = false);
// the pick of a step with its stages: greedy unless the sampler is on (or force_greedy); fed = the tokens the step was fed (NULL at the first
// pick after the prefill)
int pick_run(omchat_ctx* ctx, const float* lg, int b, int32_t* next_tokens, hipStream_t s, bool advance = false, const int32_t* fed = nullptr,
             bool force_greedy = false);
// the picks of a verify step's T rows (tokens = what the rows were fed): bare argmax, or with `sample` the sampler's verify form, which
// commits nothing (pick_verify_committed follows the acceptance)
int pick_verify(omchat_ctx* ctx, const float* lg, int T, const int32_t* tokens, int32_t* picks, hipStream_t s, bool sample);
const char* pick_verify_refusal(omchat_ctx* ctx, int flags);      // why the sampler's state does not go with omchat_decode_verify's flags, or NULL
int pick_verify_prepare(omchat_ctx* ctx);      // allocations of a sampled verify step, before anything is enqueued
void pick_verify_committed(omchat_ctx* ctx, int n_picks);      // the acceptance committed n_picks sampled picks to sequence 0
int pick_feed(omchat_ctx* ctx, const int32_t* fed, int b, hipStream_t s);      // a step that picks nothing still feeds the history
const char* pick_rewind_refusal(omchat_ctx* ctx, int b, int n);      // why the pick state cannot go back n steps, or NULL
int pick_rewind(omchat_ctx* ctx, int b, int n, hipStream_t s);
// while guidance is on for b rows a step, a pick or a rewind takes exactly 2b rows, while layer-contrastive decoding is on exactly its b: why
// `rows` will not do, or NULL (NULL when both are off)
const char* pick_rows_refusal(omchat_ctx* ctx, int rows);
// layer-contrastive decoding (omchat_set_dola): why this context's state does not go with it, or NULL -- asked by the setter and again by
// every prefill and step while it is on (the replica switches may have come later)
const char* dola_state_refusal(const omchat_ctx* ctx);

// ---- contrastive.hip
const char* contrastive_state_refusal(const omchat_ctx* ctx);      // why this context's state does not go with contrastive search, or NULL
int contrastive_prefill_admit(omchat_ctx* ctx, int P);      // a b = 1 prefill while the mode is on, before anything is enqueued: the history's room
int contrastive_prefill_keep(omchat_ctx* ctx, const void* x, int P, hipStream_t s);      // ... behind its last layer: the history and its inverse norms
