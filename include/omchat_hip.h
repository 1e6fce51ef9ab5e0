/* omchat_hip.h -- C ABI of libomchat_hip.so: the MI355X (gfx950) implementation of the OmChat inference hot path
 * (InternViT vision tower -> mlp2x_gelu projector -> image-token splice -> Qwen2 prefill -> greedy decode).
 *
 * The reference (om-ai-lab/OmChat) has no FFI of its own: its seams are Python class boundaries.  Each entry point
 * below names the reference interface it stands behind (file:line relative to the reference repo; Qwen2 lines refer
 * to transformers/models/qwen2/modeling_qwen2.py which the reference inherits at
 * omchat/model/language_model/omchat_qwen2.py:7,22,29).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: plain pointers + sizes, no framework types.  Device pointers unless stated.  All 16-bit tensors use
 * the context's compute dtype (OMCHAT_F16 / OMCHAT_BF16), row-major.  `stream` is a hipStream_t (NULL = default
 * stream); every call only enqueues work on it.  Return 0 on success; otherwise omchat_last_error() (thread-local)
 * explains, and the Python mirror re-raises ValueError / RuntimeError like the reference does.
 */
#ifndef OMCHAT_HIP_H
#define OMCHAT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMCHAT_F16 0
#define OMCHAT_BF16 1
#define OMCHAT_F32 2            /* accepted as a SOURCE dtype by omchat_load_tensor and as an output dtype of omchat_preproc_anyres */
#define OMCHAT_PAD_ROW INT32_MIN /* splice index: zero row */

typedef struct omchat_ctx omchat_ctx;

/* Per-rank (already tensor-parallel-local) model geometry.  Field names follow InternVisionConfig
 * (multimodal_encoder/intern_vit_6b/configuration_intern_vit.py:63-83) and Qwen2Config. */
typedef struct {
  /* vision tower */
  int v_hidden;        /* hidden_size (3200) */
  int v_heads;         /* LOCAL attention heads (25 at TP=1; zero-padded shards otherwise), head_dim is 128 */
  int v_qk_channels;   /* divisor of the joint q/k RMSNorm = full hidden_size (3200) (modeling_intern_vit.py:143-146) */
  int v_mlp;           /* LOCAL intermediate_size (12800 / tp) */
  int v_layers;        /* num_hidden_layers (45) */
  int v_patch;         /* 14 */
  int v_image;         /* 448 */
  float v_eps;         /* layer_norm_eps 1e-6 */
  /* decoder */
  int t_hidden;        /* 3584 */
  int t_layers;        /* 28 */
  int t_heads;         /* LOCAL query heads */
  int t_kv_heads;      /* LOCAL kv heads */
  int t_mlp;           /* LOCAL intermediate_size */
  int t_vocab;         /* LOCAL lm_head rows */
  int t_vocab_total;   /* embed_tokens rows (replicated) */
  float t_eps;         /* rms_norm_eps */
  float rope_theta;    /* 1e6 */
  /* capacities */
  int max_seq;         /* KV positions per sequence */
  int max_batch;       /* sequences */
  int max_tiles;       /* ViT tiles per launch batch */
  int max_prefill_rows;/* b * S rows of one prefill call */
  int dtype;           /* OMCHAT_F16 | OMCHAT_BF16 */
  /* tower variant (0 = the InternViT-6B defaults, so older callers that zero the tail are unchanged):
   * InternViT-300M (intern_vit_300m/configuration_intern_vit.py:60-80) = head_dim 64, LayerNorm, no q/k norm */
  int v_head_dim;      /* 0 or 128 | 64 */
  int v_norm_type;     /* 0 = InternRMSNorm, 1 = nn.LayerNorm (weight + bias) */
  int v_no_qk_norm;    /* 0 = joint-head q/k RMSNorm (qk_normalization=True), 1 = none */
} omchat_config;

const char* omchat_last_error(void);
const char* omchat_version(void);

/* ---- loader: stands behind load_pretrained_model (omchat/model/builder.py:22-35) -------------------------------- */
/* rccl_comm: ncclComm_t of the tensor-parallel group or NULL (tp_size == 1, or a peer group is attached with omchat_ctx_set_peer). */
int omchat_ctx_create(const omchat_config* cfg, int tp_rank, int tp_size, void* rccl_comm, omchat_ctx** out);
void omchat_ctx_destroy(omchat_ctx* ctx);
/* name: omchat-native checkpoint key, e.g. "model.layers.3.mlp.gate_proj.weight";
 * data: host OR device pointer to the (rank-local) tensor, contiguous; src_dtype: ctx dtype or OMCHAT_F32. */
int omchat_load_tensor(omchat_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim, int src_dtype);
/* fills every weight with omchat_amd/synth.py's deterministic generator (same values as the host generator). */
int omchat_fill_synthetic(omchat_ctx* ctx, uint64_t seed);
/* number of tensors still missing (0 = ready); names of missing tensors are put in omchat_last_error(). */
int omchat_weights_missing(omchat_ctx* ctx);
size_t omchat_device_bytes(omchat_ctx* ctx);

/* ---- tower: InternVITVisionTower.forward + feature_select (internVIT_encoder.py:35-56) -------------------------- */
/* pixels [n_tiles,3,v_image,v_image]; out [n_tiles, ntok, v_hidden], ntok = patches (+1 when keep_cls).
 * select_layer indexes hidden_states like the reference (0 = embeddings, -1 = last layer). */
int omchat_vit_forward(omchat_ctx* ctx, const void* pixels, int n_tiles, int select_layer, int keep_cls, void* out, void* stream);
/* ---- projector: build_vision_projector('mlp2x_gelu').forward (multimodal_projector/builder.py:54-61) ------------ */
int omchat_projector_forward(omchat_ctx* ctx, const void* in, int rows, void* out, void* stream);
/* ---- encode_images (omchat_arch.py:50-53): tower (select_layer, patch features) then projector ------------------ */
int omchat_encode_images(omchat_ctx* ctx, const void* pixels, int n_tiles, int select_layer, void* out, void* stream);

/* ---- splice: prepare_inputs_labels_for_multimodal (omchat_arch.py:55-209) --------------------------------------- */
/* Host-side plan (integers only).  ids int64 [b,T] with -200 sentinels; mask uint8 [b,T] or NULL; n_tok rows per
 * tile; padding_side 0 = right, 1 = left; max_length <= 0 = none.  Writes src_index int32 [b * S_out] (>= 0: token
 * id, <= -1: feature row -1-k, OMCHAT_PAD_ROW: zero row), lengths int32 [b]; returns S_out via *S_out.
 * Call with src_index == NULL to size the output.  n_tiles_avail is checked like the reference's running index.
 * vocab > 0: an unmasked id outside [0, vocab) other than the -200 sentinel returns 4 (the reference raises IndexError from
 * embed_tokens, omchat_arch.py:139); vocab <= 0 skips the check. */
int omchat_splice_plan(const int64_t* ids, const uint8_t* mask, int b, int T, int n_tok, int n_tiles_avail,
                       int padding_side, int max_length, int32_t* src_index, int32_t* lengths, int* S_out, int vocab);
/* Device gather: embeds[r] = embed_tokens[idx] | feats[row] | 0.  src_index device int32 [rows]. */
int omchat_splice_gather(omchat_ctx* ctx, const int32_t* src_index, const void* feats, void* embeds, int rows, void* stream);

/* ---- decoder: OmChatQwen2ForCausalLM.forward (omchat_qwen2.py:45-89) -> Qwen2ForCausalLM.forward --------------- */
/* Prefill step 0: embeds [b, S, t_hidden] (right-padded rows), lengths host int32 [b].  Resets the KV cache of
 * sequences 0..b-1.  logits_last: device fp32 [b, t_vocab] for the last valid position of each sequence (or NULL).
 * hidden_out: optional [b, S, t_hidden] post-final-norm hidden states (test hook).  */
int omchat_prefill(omchat_ctx* ctx, const void* embeds, int b, int S, const int32_t* lengths, float* logits_last,
                   void* hidden_out, void* stream);
/* Prefill of a LEFT-padded batch (config.tokenizer_padding_side == "left", omchat_arch.py:176-184): row i holds its lengths[i] tokens at
 * [S - lengths[i], S).  As in the reference, position_ids are dropped (:206-207) so RoPE runs on arange(S) for every row, the padded
 * keys are masked, and logits_last is the position S - 1 of every row (what generate reads).  A padded query row sees no key; its
 * attention output is the uniform average of the sequence's V rows, as the reference's eager CPU attention computes it (every score at
 * finfo.min).  Decode steps after it go through omchat_decode_step_masked (omchat_decode_step would place the rows per sequence and is
 * refused). */
int omchat_prefill_left(omchat_ctx* ctx, const void* embeds, int b, int S, const int32_t* lengths, float* logits_last,
                        void* hidden_out, void* stream);
/* Decode step >= 1 (omchat_qwen2.py:92-111, omchat_arch.py:61-70): one token per sequence, appended at kv_len.
 * tokens device int32 [b]; logits device fp32 [b, t_vocab] or NULL; next_tokens device int32 [b] (greedy argmax,
 * first index wins) or NULL. */
int omchat_decode_step(omchat_ctx* ctx, const int32_t* tokens, int b, float* logits, int32_t* next_tokens, void* stream);
/* Decode step of a PADDED batch exactly as the reference computes it (omchat_arch.py:61-70 as HF generate drives it, `images` passed on
 * every step): the new token of EVERY row is appended at the common cache length (S of the padded prefill + the masked steps so far), is
 * rotated to positions[i] (host int32 [b]; the reference's sum(attention_mask) - 1) and attends the cache slots j <= slots with
 * key_mask[i * mask_ld + j] != 0 (host bytes [b][mask_ld], mask_ld >= slots + 1: the token-level mask padded with ones -- it hides real
 * prompt slots and exposes padded ones once images expanded the rows differently).  Valid after omchat_prefill (right padding) and
 * omchat_prefill_left, for all b rows of that prefill, on one GPU (16-bit or e4m3 KV cache); omchat_decode_step and this entry cannot be
 * mixed after one prefill (they place the cache rows differently).  Synchronises the stream. */
int omchat_decode_step_masked(omchat_ctx* ctx, const int32_t* tokens, int b, const int32_t* positions, const uint8_t* key_mask, int mask_ld,
                              float* logits, int32_t* next_tokens, void* stream);
/* The same step WITHOUT per-step host data, for the loop HF generate drives (single_inference.py:53-62): there the decode branch pads the
 * token-level mask with ones up to the cache length and every generated token appends another one (omchat_arch.py:63-69), so over the cache
 * slots the key mask of every step is [the prompt's token-level mask | ones] and position_ids = sum(mask) - 1 grows by one per step.
 * omchat_masked_decode_begin (once after the prefill; synchronises): key_mask host bytes [b][mask_ld], the first mask_cols columns are taken,
 * every slot behind them counts as visible; positions host int32 [b] = the FIRST step's position_ids.  omchat_decode_step_masked_next (every
 * step; no host buffer, no synchronisation): appends at the common slot, rotates to the device-resident positions and advances them.
 * omchat_kv_rewind takes the positions back with the slots.  A call of omchat_decode_step_masked in between needs a new begin. */
int omchat_masked_decode_begin(omchat_ctx* ctx, int b, const int32_t* positions, const uint8_t* key_mask, int mask_ld, int mask_cols, void* stream);
int omchat_decode_step_masked_next(omchat_ctx* ctx, const int32_t* tokens, int b, float* logits, int32_t* next_tokens, void* stream);
/* Experimental one-launch forms of the batch-1 decode layer (NOT in the product build since round 5: compile with -DOMCHAT_EXPERIMENTS=1;
 * measured slower than the six launches): with tuning key 23 a decoder layer is ONE launch with in-launch hand-offs (csrc/decode_layer.hip), with key 22 attention +
 * merge + o_proj are one launch (csrc/fused_decode.hip); same bits as the separate launches either way.  launches: how many such launches
 * this context has issued; timeout_bits: sticky bits of hand-offs that gave up after their wall-clock budget (0 = none; otherwise the
 * affected steps' results are wrong).  Synchronises. */
int omchat_fused_status(omchat_ctx* ctx, long* launches, unsigned* timeout_bits);
/* 1 when the library was built with -DOMCHAT_EXPERIMENTS=1 (those one-launch forms and the work-stealing gate|up GEMV compiled in), 0 for
 * the product build, in which tuning keys 22 / 23 / 24 select nothing. */
int omchat_has_experiments(void);
/* lm_head on arbitrary hidden rows (Qwen2ForCausalLM.forward :462-465): hidden [n, t_hidden] -> fp32 [n, t_vocab] */
int omchat_lm_head(omchat_ctx* ctx, const void* hidden, int n, float* logits, void* stream);
/* Teacher-forced scoring (Qwen2ForCausalLM.forward's shifted cross-entropy, modeling_qwen2.py): hidden [rows, t_hidden]
 * final-normed rows of b sequences of S slots each (what omchat_prefill's hidden_out holds), labels device int32 [rows], ALREADY SHIFTED
 * (labels[i * S + t] is the token that follows slot t; -100 = not scored; the caller keeps every other label inside [0, t_vocab) -- the
 * kernels stay in bounds and score a label outside it NaN).  logprob device fp32 [rows]: log_softmax(hidden[r] lm_head^T)[labels[r]] under
 * the raw fp32 distribution of omchat_lm_head, 0 where the label is -100.  out device fp32 [2 + 2 b]: loss_sum = -sum of the scored rows'
 * logprob, their count, then every sequence's sum of logprob and its count.  The [rows, t_vocab] logits are never stored: an MFMA GEMM on
 * the 16-bit lm_head whose epilogue keeps per-row (max, sum exp) partials (8 bytes a row and 64 vocabulary columns of workspace, owned
 * and grown by the context before anything is enqueued).  A pure function of `hidden`: cache, positions and pick state are untouched.
 * Deterministic (fixed reduction orders).  Errors, each before any work: a tensor-parallel context (the lm_head is vocabulary-parallel and
 * no exchange of the partials is built), missing weights, rows > max_prefill_rows, b * S != rows. */
int omchat_score_hidden(omchat_ctx* ctx, const void* hidden, int rows, const int32_t* labels, int b, int S, float* logprob, float* out,
                        void* stream);
/* greedy pick (HF generate with do_sample=False: argmax of the last position, first index wins): logits fp32
 * [b, t_vocab] (rank-local slice under tensor parallelism; the (max, index) pairs are exchanged) -> int32 [b] */
int omchat_greedy(omchat_ctx* ctx, const float* logits, int b, int32_t* next_tokens, void* stream);
/* ---- sampling (HF generate with do_sample=True) ----------------------------------------------- */
/* omchat_set_sampling: from now on every token pick of this context -- omchat_sample, omchat_decode_step, both masked steps, the captured
 * decode graph -- samples instead of taking the argmax.  Processing order as HF's sampling path: repetition penalty (rep_penalty; 1 = off),
 * temperature (> 0), top-k (0 = off; ties at the k-th value are kept; top_k == 1 is exactly the greedy pick), top-p (1 = off; the smallest set
 * of highest tokens whose mass reaches top_p, ties at the threshold kept), then a Gumbel-max draw keyed by (seed, row, step, global vocabulary
 * index): the same ids at every TP degree.  seen_ids host int32, the rows' seen ids one after another (n_seen_per_row host int32 [b]); ids
 * outside [0, vocab) -- the -200 image sentinel -- are ignored; each pick adds its id.  Resets the rows' step counters to 0.  b = 0 switches
 * sampling off (greedy again).  A parameter change drops the captured decode graphs.  Synchronises. */
int omchat_set_sampling(omchat_ctx* ctx, int b, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                        const int32_t* seen_ids, const int32_t* n_seen_per_row, void* stream);
/* omchat_set_sampling_filters: HF's four warpers behind top-p for the sampling state omchat_set_sampling just configured, in HF's order and
 * with min_tokens_to_keep = 1; each sees the softmax over the survivors of the ones before it.  min_p (negative = off): keeps p >= min_p *
 * p_max.  typical_p (>= 1 = off): keeps the tokens with the smallest |-log p - H| (H = the entropy) whose mass first reaches typical_p, ties
 * at the cut kept -- the top token can go.  epsilon_cutoff (>= 1 = off): keeps p >= epsilon.  eta_cutoff (>= 1 = off): keeps p >=
 * min(eta, sqrt(eta) * exp(-H)).  Epsilon and eta always keep the largest surviving logit and its ties.  The kept set is a key interval
 * [lo, hi] of the processed logits.  omchat_set_sampling alone leaves all four off, so call this after it.  top_k == 1 stays the greedy pick.
 * Other values than the captured decode graphs hold drop them in front of the next step.  Refused while sampling is off. */
int omchat_set_sampling_filters(omchat_ctx* ctx, double min_p, double typical_p, double epsilon_cutoff, double eta_cutoff, void* stream);
/* the sampled counterpart of omchat_greedy (the first token after the prefill); omchat_greedy itself when sampling is off */
int omchat_sample(omchat_ctx* ctx, const float* logits, int b, int32_t* next_tokens, void* stream);
/* ---- HF logits constraints (generate's no_repeat_ngram_size, bad_words_ids, min_new_tokens / min_length, suppress_tokens,
 * begin_suppress_tokens) ------------------------------------------------------------------------------------------ */
#define OMCHAT_CON_MAX_NGRAM 64          /* no_repeat_ngram_size */
#define OMCHAT_CON_MAX_EOS 16            /* eos ids */
#define OMCHAT_CON_MAX_SUPPRESS 1024     /* suppress ids, and begin-suppress ids */
#define OMCHAT_CON_MAX_BAD_WORDS 1024    /* bad words */
#define OMCHAT_CON_MAX_BAD_WORD_IDS 8192 /* ids of all bad words together */
/* omchat_set_constraints: from now on every token pick of rows 0..b-1 of this context -- omchat_greedy, omchat_sample, omchat_decode_step, both
 * masked steps, the captured decode graph -- excludes the ids HF 5.x's NoRepeatNGram, NoBadWords, MinLength, MinNewTokensLength, SuppressTokens
 * and SuppressTokensAtBegin processors would set to -inf, given the row's token history: the prompt row as passed (prompt_ids host int32, the
 * rows one after another, prompt_len host int32 [b]; the -200 image sentinel and pad ids are ordinary values for matching) plus the token every
 * decode step is fed, appended on the device before that step's pick.  The pick (argmax or sampler) runs on a context-owned copy of the logits
 * with the banned ids at -inf: logits handed in or returned stay raw.  no_repeat_ngram_size 0 = off; min_new_tokens / min_length 0 = off (they
 * ban eos_ids); bad words are flattened (bad_word_offsets host int32 [n_bad_words + 1] into bad_word_ids); a bad word equal to one eos id is
 * dropped; ids outside [0, t_vocab_total) are never banned.  max_new: the most decode steps that will follow (sizes the history; a step beyond
 * it is refused).  The history is grown on demand, never shrunk, and counted in omchat_device_bytes.  omchat_kv_rewind takes the history back
 * with the slots.  b = 0 switches constraints off.  Refused (before anything is enqueued): values above the caps, a beam search in progress;
 * omchat_decode_verify and omchat_beam_begin refuse while constraints are on.  A parameter change drops the captured decode graphs.
 * Synchronises. */
int omchat_set_constraints(omchat_ctx* ctx, int b, int no_repeat_ngram_size, int min_new_tokens, int min_length, const int32_t* eos_ids, int n_eos,
                           const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress,
                           const int32_t* bad_word_ids, const int32_t* bad_word_offsets, int n_bad_words, const int32_t* prompt_ids,
                           const int32_t* prompt_len, int max_new, void* stream);
/* ---- finite-state token constraints (generate(token_fsm=)) ----------------------------------------------------------- */
/* A token FSM has n_states states; state s owns the edges off[s] .. off[s + 1] - 1 of tok / nxt (host int32; CSR), sorted by token without
 * duplicates, every tok in [0, t_vocab_total), every nxt in [0, n_states).  The tokens of a state's edges are the ids allowed there; EOS ids are
 * ordinary tokens.  One extra state, OMCHAT_FSM_DEAD: a row goes there when the token it is fed has no edge from its state (the pad fed to an
 * ended row, an EOS without an edge), and in it the logits pass through unmasked -- no row is ever all -inf.
 * The caps keep every index in int32.  A table costs (n_states + 1 + 2 E) * 4 bytes of device memory, every rank holding all of it: 4 MiB of
 * offsets and 512 MiB of edges at the caps; 1.2 MB for one state with an edge for every id of a 152 064-id vocabulary. */
#define OMCHAT_FSM_MAX_STATES (1 << 20)
#define OMCHAT_FSM_MAX_EDGES (1 << 26)
#define OMCHAT_FSM_DEAD (-1)
/* omchat_fsm_load: validates and uploads a table; it stays until it is replaced or unloaded (n_states = 0, which also switches the stage off)
 * and counts in omchat_device_bytes.  Refused, with nothing changed: a table above the caps, unsorted or duplicate tokens, ids or targets
 * out of range, a state that some edge leads to and that has no edge (the message names it; add an EOS edge), a beam search in progress.  A
 * load drops the captured decode graphs and switches the stage off: omchat_fsm_begin follows.  Synchronises. */
int omchat_fsm_load(omchat_ctx* ctx, int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, void* stream);
/* omchat_fsm_begin: from now on every token pick of rows 0..b-1 of this context -- omchat_greedy, omchat_sample, omchat_decode_step, both masked
 * steps, the captured decode graph -- first advances the row's state over the token the decode step is fed (not at the first pick after the
 * prefill), then runs on the context-owned copy of the logits with every id that is no edge of the row's state at -inf (behind the bans of
 * omchat_set_constraints when both are on); logits handed in or returned stay raw.  A decode step that picks nothing only advances.
 * start_states host int32 [b], each in range and with an edge; max_new: the most decode steps that will follow (a step beyond it is refused
 * before it is enqueued).  The rows' states are kept as a trail of max_batch * (max_new + 1) * 4 bytes, grown on demand, never shrunk,
 * counted in omchat_device_bytes; omchat_kv_rewind takes the states back with the slots.  b = 0 switches the stage off: no launch, no graph
 * node remains.  Sticky like the sampler and the constraints.  Refused: no table, a beam search in progress; omchat_decode_verify and
 * omchat_beam_begin refuse while it is on.  Switching on or off, another b or a trail that had to grow drops the captured decode graphs.
 * Synchronises. */
int omchat_fsm_begin(omchat_ctx* ctx, int b, const int32_t* start_states, int max_new, void* stream);
/* the current states of rows 0..b-1 (host int32 [b]; OMCHAT_FSM_DEAD included).  Synchronises the device. */
int omchat_fsm_states(omchat_ctx* ctx, int b, int32_t* out, void* stream);
/* ---- classifier-free guidance (generate(guidance_scale=)) ------------------------------------------------------------- */
/* omchat_set_guidance: from now on rows 0..b-1 of this context are the conditional rows and rows b..2b-1 their twins, which hold the negative
 * prompt.  omchat_greedy, omchat_sample and omchat_decode_step then take exactly 2b rows (of logits / of tokens) and pick b ids from
 *   scores[r] = scale * (lc - lu) + lu,   lc = log_softmax(logits[r]), lu = log_softmax(logits[b + r])
 * (HF's UnbatchedClassifierFreeGuidanceLogitsProcessor), written to the context-owned copy in front of the bans of omchat_set_constraints and
 * the automaton of omchat_fsm_begin; where either logit is -inf the score is -inf (HF's formula has NaN there).  next_tokens has 2b entries:
 * the twins get their rows' ids, written on the device, and a decode step moves the positions of all 2b rows.  Sampling state, ban history,
 * automaton states and the log-prob record belong to the b conditional rows: their setters keep taking b.  The record's raw number is the
 * conditional row's raw log-softmax; the processed one is that of the guided scores as the pick saw them.  omchat_kv_rewind(ctx, 2b, n)
 * takes back 2b cache rows and b rows of pick state.  Any other row count is refused before anything is enqueued, as are, while guidance
 * is on, omchat_beam_begin, omchat_decode_verify, omchat_group_begin and the masked decode steps.  Refused here: a tensor-parallel context
 * (the exchange of the two log-sum-exps is not built), 2b > max_batch, a scale that is not finite, a beam search or a sampled group in
 * progress.  b = 0 switches the stage off: no launch, no graph node remains.  Sticky like the sampler's state.  b, the scale and the
 * buffers are kernel arguments of the captured decode graphs: a change drops them, the same b and scale keep them.  The workspace
 * (max_batch rows of tile partials) and the copy are context-owned and counted in omchat_device_bytes.  Deterministic: the same logits
 * give the same scores, bit for bit, eager or in a graph. */
int omchat_set_guidance(omchat_ctx* ctx, int b, float scale, void* stream);
/* ---- layer-contrastive decoding (generate(dola_layers=)) --------------------------------------------------------------- */
/* omchat_set_dola: from now on every pick of rows 0..b-1 of this context contrasts the final layer's next-token distribution with an early
 * layer's from the same forward pass (Chuang et al., "DoLa: Decoding by Contrasting Layers"; HF 4.4x's _dola_decoding).  layers: k host
 * indices into HF's hidden_states tuple -- 0 the embedding row of the fed token, i the residual stream behind decoder layer i, all below
 * num_hidden_layers --, 1 <= k <= OMCHAT_DOLA_MAX_LAYERS.  omchat_prefill (with logits_last) and omchat_decode_step then also keep each
 * sequence's last-position hidden row at those layers, push all (k + 1) b rows -- the final row through the final RMSNorm, the candidate rows
 * as they are, or normalised too with norm != 0 ("logit lens", this project's extension) -- through the 16-bit lm_head in one pass, and
 * leave the raw fp32 logits [(k + 1) b][V] in a context-owned buffer: rows [0, b) the final rows, row (1 + j) b + r candidate j of sequence
 * r.  The logits handed back to the caller stay the b final rows.  Every pick (omchat_greedy, omchat_sample, the step's own) runs on
 *   out[v] = lm[v] - lp[v] where lm[v] >= max lm + log(relative_top), -inf elsewhere;  lm = log_softmax(final), lp = log_softmax(candidate)
 * of the candidate with the largest Jensen-Shannon divergence from the final row (the first on ties; k == 1: that one), written to the
 * context's copy in front of the bans of omchat_set_constraints and the automaton of omchat_fsm_begin.  Every row picks its own layer (HF
 * averages the divergence over the batch; at b = 1 the two agree).  While it is on, omchat_greedy and omchat_sample read the context's rows of
 * the last prefill or step -- their `logits` argument must be what that call returned -- and a pick, a step or a rewind takes exactly b rows.
 * The log-prob record's raw number is the final row's raw log-softmax, the processed one what the pick saw.  One int32 per row and pick --
 * the HF index of the picked layer -- is recorded on the device (omchat_dola_read); omchat_kv_rewind takes its lines back with the slots.
 * Refused here, before anything changes: a tensor-parallel context, an active beam search, guidance, a sampled group, the fp8 or MXFP4
 * decode replicas (the head pass is 16-bit), (k + 1) b > min(max_batch, 32), an index outside [0, num_hidden_layers), a relative_top outside
 * (0, 1].  Refused while it is on, before anything is enqueued: omchat_beam_begin, omchat_set_guidance, omchat_group_begin,
 * omchat_prefill_suffixes, omchat_decode_verify, the masked steps, omchat_prefill_left, omchat_prefill_extend, the two replica switches.
 * b = 0 switches it off: no launch, no graph node remains.  Sticky; every parameter is a kernel argument of the captured decode graphs, which
 * a change drops.  Deterministic: the same logits give the same scores and the same layer, bit for bit, eager or in a graph. */
#define OMCHAT_DOLA_MAX_LAYERS 16
int omchat_set_dola(omchat_ctx* ctx, int b, const int32_t* layers, int k, float relative_top, int norm, void* stream);
/* the record: out host int32 [rows][steps], line t of row r = the HF index of the layer pick t of row r contrasted with, -1 where no such
 * pick was made (yet).  Synchronises the device. */
int omchat_dola_read(omchat_ctx* ctx, int32_t* out, int rows, int steps);
/* test hook: the raw rows of the last prefill or step, host fp32 [(k + 1) b][V].  Synchronises the device. */
int omchat_dola_rows(omchat_ctx* ctx, float* out);
/* ---- contrastive search (generate(penalty_alpha=, top_k=)) ----------------------------------------------------------- */
/* omchat_set_contrastive: HF 4.4x's _contrastive_search (Su et al., "A Contrastive Framework for Neural Text Generation") for ONE sequence.
 * 2 <= k <= min(OMCHAT_CS_MAX_K, max_batch) candidates per token, 0 < alpha <= 1, max_new emitted ids at most, share != 0: the k rows share
 * the prompt's cache slots (omchat_group_begin's share), eos_ids: up to 8 host ids.  k = 0 switches the mode off.  Call it BEFORE the
 * prefill: while it is on, omchat_prefill with b = 1 also keeps the post-final-norm hidden rows of all its P positions as the history
 * (16-bit rows [P + max_new][hidden] and one fp32 inverse L2 norm per row) and refuses P + max_new > max_seq before any work.
 * omchat_contrastive_step(logits, rows, next_tokens, done_word): the FIRST call after the prefill takes the prefill's logits with
 * rows = 1: the k largest ids of the row (ties to the lower id) with their fp32 softmax probabilities are the candidates, the prompt row is
 * forked or shared into rows 0..k-1 (omchat_group_begin), next_tokens[0..k) = the candidates, next_tokens[k] = -1.  The caller then runs
 * omchat_decode_step with those k tokens and b = k (eager or through the decode graph) and hands its logits [k][V] to the next call with
 * rows = k: pen_i = max_j cos(h_i, history_j) over the step's final-normed rows, pick = the first maximum of (1 - alpha) p_i - alpha pen_i,
 * next_tokens[k] = the emitted id, *done_word (device, or NULL) = 1 when that id is an EOS id or max_new ids are out, else 0; the picked
 * row's hidden state joins the history, the ONE new cache slot of the picked row is copied to the other rows, and next_tokens[0..k) are the
 * next candidates from logits row `pick`.  Nothing synchronises with the host.  One record per emitted id stays on the device
 * (omchat_contrastive_read).  Afterwards every row holds prompt + emitted ids; omchat_group_begin with b = 0 and omchat_set_contrastive
 * with k = 0 leave row 0 as a plain sequence.
 * Refused here, before anything changes: a tensor-parallel context, the e4m3 KV cache, fp8 prefill GEMMs, MXFP4 decode mode 1 (batch-1
 * steps only), an active beam search, guidance, layer-contrastive decoding, a token FSM, constraints, logprobs, sampling, a sampled group,
 * k or alpha out of range, a hidden size that is no multiple of 32.  Refused while it is on, before anything is enqueued: omchat_beam_begin,
 * omchat_decode_verify, omchat_set_guidance, omchat_set_dola, omchat_fsm_begin, omchat_set_constraints, omchat_set_logprobs,
 * omchat_set_sampling, both masked steps, omchat_prefill_left, omchat_prefill_extend, omchat_prefill_suffixes, a prefill of b > 1, a
 * foreign omchat_group_begin and a decode step of other than k rows.  Deterministic: no float atomics, fixed reduction orders. */
#define OMCHAT_CS_MAX_K 16
#define OMCHAT_CS_REC_WORDS 52
int omchat_set_contrastive(omchat_ctx* ctx, int k, double alpha, int max_new, int share, const int32_t* eos_ids, int n_eos, void* stream);
int omchat_contrastive_step(omchat_ctx* ctx, const float* logits, int rows, int32_t* next_tokens, int32_t* done_word, void* stream);
/* the record: out host int32 [steps][OMCHAT_CS_REC_WORDS] -- words [0, 16) the candidates' ids, [16, 32) their probabilities and [32, 48)
 * their penalties (fp32 bits), [48] the pick (the selected candidate's rank), [49] the emitted id, [50] the penalty launch's chunks, [51] the
 * history's rows at that pick.  steps <= the picks since the prefill.  Synchronises the device. */
int omchat_contrastive_read(omchat_ctx* ctx, int32_t* out, int steps);
/* test hook: rows [row0, row0 + n) of the history (host, 16-bit [n][hidden]; or NULL), their inverse norms (host fp32 [n]; or NULL) and
 * the final-normed rows of the last k-row step in row-major order (host, 16-bit [k][hidden]; or NULL).  Synchronises the device. */
int omchat_contrastive_rows(omchat_ctx* ctx, int row0, int n, void* hist_out, float* inv_out, void* cand_out);
/* ---- per-token log-probabilities of the picked ids (generate(output_logprobs=True)) ---------------------------------- */
/* omchat_set_logprobs: from now on every token pick of rows 0..b-1 of this context -- omchat_greedy, omchat_sample, omchat_decode_step, both
 * masked steps, the captured decode graph -- also records two fp32 numbers on the device, without a host sync: raw = log_softmax(logits)[id]
 * over the whole vocabulary (HF: compute_transition_scores(sequences, out.logits, normalize_logits=True)) and processed =
 * log_softmax(scores)[id], scores = what HF's processors leave of the row (banned ids at -inf, repetition penalty with the seen set from
 * before the pick, / temperature, ids outside the top-k / top-p kept set at -inf; HF: the same call on out.scores).  An id whose processed
 * value is -inf records -inf.  Greedy without constraints: processed is raw, bit for bit.  The record holds max_new picks per row (a pick
 * beyond it is refused before anything is enqueued), is grown on demand, never shrunk, and counted in omchat_device_bytes; every call resets
 * the rows' counters to 0.  omchat_kv_rewind takes the counters back with the slots.  b = 0 switches it off: no launch, allocation or graph
 * node remains.  Refused: a beam search in progress; omchat_decode_verify and omchat_beam_begin refuse while it is on, omchat_greedy while
 * it and sampling are both on.  Switching on or off, another b, or a max_new beyond the record's capacity drops the captured decode graphs; a max_new
 * within it keeps them.  While it is on, omchat_kv_rewind must cover all its rows (b >= the b given here).  Under tensor parallelism
 * the ranks' partial sums cross in one fp32 all-reduce and every rank records the same numbers. */
int omchat_set_logprobs(omchat_ctx* ctx, int b, int max_new, void* stream);
/* host copy of the record of rows 0..b-1: raw / processed host fp32 [b][max_len] (entries behind a row's count are left as they are),
 * counts host int32 [b] = picks recorded per row.  Synchronises the device. */
int omchat_read_logprobs(omchat_ctx* ctx, int b, float* raw, float* processed, int32_t* counts, int max_len);
/* omchat_set_logprobs_ex: omchat_set_logprobs, and next to the two numbers every pick also records, at the same device counter (so
 * omchat_kv_rewind, the step enqueued ahead and the captured graph treat all records as one):
 *   top alternatives  top_n pairs (global id, log-probability), 0 <= top_n <= OMCHAT_LP_MAX_TOP (0 = none), the top_n entries of
 *                     log_softmax(logits) over the whole vocabulary under the RAW distribution -- the caller's logits before bans, penalty
 *                     and temperature -- ordered by value descending, then by global id ascending.  -0.0 and +0.0 compare equal; an id whose
 *                     logit is -inf has log-probability -inf and ranks behind every finite one.  The selection is exact (comparisons only).
 *   scored ids        the raw log-probability of each of the n_score distinct global ids score_ids (host int32, 0 <= n_score <=
 *                     OMCHAT_LP_MAX_SCORED, one list for all rows, fixed until the next call).
 * Every value is x - (max + log sum) with the very (max, sum) of the picked id's raw value: where the picked id is among the alternatives or
 * the scored ids, its entry is bit-equal to the raw record.  Switching the extras on changes no bit of the raw / processed record.  Refused
 * before anything is enqueued: top_n outside 0..20 or beyond the whole vocabulary, more than 32 ids, a duplicate id, an id outside
 * [0, t_vocab_total), under tensor parallelism a vocabulary of 2^24 ids or more (ids cross the exchange as fp32; still one all-reduce).
 * top_n = 0 and n_score = 0 is omchat_set_logprobs: the same launches, no further allocation, no further graph node.  Another top_n or id
 * list drops the captured decode graphs.  The extras' record grows with max_new (max_batch * (2 top_n + n_score) * 4 bytes a pick) and is
 * counted in omchat_device_bytes.  Alternatives under the processed distribution, per-row id lists, beams and verify rows: not recorded. */
#define OMCHAT_LP_MAX_TOP 20
#define OMCHAT_LP_MAX_SCORED 32
int omchat_set_logprobs_ex(omchat_ctx* ctx, int b, int max_new, int top_n, const int32_t* score_ids, int n_score, void* stream);
/* host copy of the extras of rows 0..b-1: top_vals host fp32 [b][max_len][top_n], top_ids host int32 [b][max_len][top_n], scored host fp32
 * [b][max_len][n_score] (each may be NULL; entries behind a row's count are left as they are), counts host int32 [b].  Refused while the
 * extras are off.  Synchronises the device. */
int omchat_read_logprob_extras(omchat_ctx* ctx, int b, float* top_vals, int32_t* top_ids, float* scored, int32_t* counts, int max_len);
/* test accessor: the step counter of `row` and (seen_words host uint32 [(t_vocab + 31) / 32], may be NULL) its seen bitmap over this rank's
 * vocabulary slice, bit i of word w = local id 32 w + i.  Refused while sampling is off.  Synchronises the device. */
int omchat_read_sampling_state(omchat_ctx* ctx, int row, int* step, uint32_t* seen_words);
int omchat_kv_lengths(omchat_ctx* ctx, int32_t* out, int b);      /* host copy of the current KV lengths */
/* take back the last n decode steps of sequences 0..b-1 (generate() enqueues step k + 1 before it has read token k on the host, as the
 * reference's HF loop cannot; when token k ends the generation -- EOS, a stopping criterion -- that step is forgotten).  Synchronises. */
int omchat_kv_rewind(omchat_ctx* ctx, int b, int n, void* stream);

/* ---- beam search (HF generate with num_beams = N > 1, _beam_search) --------------------------------------------- */
/* omchat_beam_begin: after the prefill of b prompts into rows 0..b-1, every row prompt_tok_len cache slots long (equal lengths, no left
 * padding; the caller guarantees the lengths, the first step forks exactly prompt_tok_len slots).  early_stopping: 0 = False, 1 = True, 2 = "never"; eos_ids host int32 [n_eos] (n_eos <= 8); max(2, 1 + n_eos) * num_beams
 * <= 32; b * num_beams <= max_batch; prompt_tok_len + max_new - 1 <= max_seq.  Allocates the device state, the exchange table and the stash
 * of the KV gather (counted in omchat_device_bytes).  The stash has room for every beam row's generated slots -- any row can be both a
 * destination and a parent when parents form cycles --: layers * b*N * kv_heads * max_new * 512 bytes (776 with the e4m3 cache), e.g.
 * 1.9 GB at 28 layers, 4 kv heads, b*N = 32, max_new = 1024; it is kept (grown, never shrunk) until the context is destroyed.
 * Logits passed to omchat_beam_step must hold at least max(2, 1 + n_eos) * num_beams finite values per row.  Synchronises. */
int omchat_beam_begin(omchat_ctx* ctx, int b, int num_beams, float length_penalty, int early_stopping, const int32_t* eos_ids, int n_eos,
                      int max_new, int prompt_tok_len, void* stream);
/* One beam step on rank-local logits fp32 [rows, t_vocab].  The first call takes the prefill's logits (rows == b): it selects, then forks
 * prompt i's cache row into rows i*N .. i*N+N-1 (host and device lengths included).  Every later call takes the decode step's logits of
 * the b*N beam rows: it selects, then copies the generated slots of each row whose parent is another row.  next_tokens (device int32
 * [b*N]): the tokens to feed the next decode step.  done_word (device int32, may be NULL): 1 once every prompt's search is over -- a
 * prompt that is over is frozen, so a step enqueued ahead of reading the word changes nothing.  Under tensor parallelism the candidates
 * cross ranks through one fp32 all-reduce; every rank takes the same decisions.  No host sync. */
int omchat_beam_step(omchat_ctx* ctx, const float* logits, int rows, int32_t* next_tokens, int32_t* done_word, void* stream);
/* omchat_beam_processors: the search begun by omchat_beam_begin ranks processed scores, as HF's _beam_search does with a repetition penalty
 * and the token bans of omchat_set_constraints: per running row lp = log_softmax(logits) in fp32; for every id of the row's history in
 * [0, t_vocab_total) lp = lp < 0 ? lp * rep_penalty : lp / rep_penalty; the ids HF's NoRepeatNGram, NoBadWords, MinLength, MinNewTokensLength,
 * SuppressTokens and SuppressTokensAtBegin processors exclude become -inf; then + the running score and the finish of the plain search, with
 * the processed lp where the tie order names the raw logit.  The history of a row is its prompt row as passed (prompt_ids host int32
 * [b][prompt_len]; the -200 image sentinel is an ordinary value for matching and is ignored by the penalty) plus the ids along the beam's
 * own path: it follows the backpointers on the device.  The lists are those of omchat_set_constraints; the EOS ids of the two length
 * bounds and of dropped one-EOS bad words are the search's own.  Valid only between omchat_beam_begin and the first omchat_beam_step.
 * rep_penalty == 1 with nothing to ban leaves the search plain (the same launches).  Refused before anything is enqueued or changed:
 * rep_penalty <= 0, values above the caps, tensor-parallel contexts, and t_vocab_total - (n_suppress + n_begin_suppress + n_bad_words +
 * n_eos + prompt_len + max_new) < max(2, 1 + n_eos) * num_beams (the bans could leave a row fewer finite scores than a step keeps).  Every
 * fed id is in [0, t_vocab_total).  The histories and two bitmaps per row are grown on demand and counted in omchat_device_bytes.  The
 * pick's own constraint state stays off.  Synchronises. */
int omchat_beam_processors(omchat_ctx* ctx, float rep_penalty, int no_repeat_ngram_size, int min_new_tokens, int min_length,
                           const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress,
                           const int32_t* bad_word_ids, const int32_t* bad_word_offsets, int n_bad_words, const int32_t* prompt_ids,
                           int prompt_len, void* stream);
/* The best num_return (<= N) finished hypotheses of every prompt, best first: tokens host int32 [b*num_return][max_len] (generated ids
 * only), lengths host int32 [b*num_return], scores host fp32 [b*num_return] (HF's sequences_scores).  Synchronises the device.  After a
 * beam search the cache rows hold running beams, not the returned hypotheses; omchat_kv_rewind leaves the beam state alone. */
int omchat_beam_result(omchat_ctx* ctx, int num_return, int32_t* tokens, int32_t* lengths, float* scores, int max_len);

/* ---- sampled groups (HF generate with do_sample and num_return_sequences = N > 1) --------------------------------- */
/* omchat_group_begin: after the prefill of b prompts into rows 0..b-1, every row prompt_len cache slots long (equal lengths, no padding),
 * make them b * N rows, prompt-major (rows i*N .. i*N+N-1 belong to prompt i), every row prompt_len keys long on the host and the device.
 * share = 0: prompt i's slots [0, prompt_len) are copied into its N rows (the e4m3 bytes and scales too); from there the rows are an ordinary
 * batch for omchat_decode_step(b * N) in every mode it has, and no mode of the context is on.
 * share = 1: only row i*N receives the prompt (one row copy for i > 0); the other rows hold nothing below slot prompt_len.  While this
 * mode is on, omchat_decode_step takes exactly b * N rows -- of any lengths >= prompt_len (they differ after omchat_prefill_suffixes) -- and
 * its attention reads the prompt keys once per group (omchat_op_attn_shared, omchat_op_attn_shared_lens);
 * omchat_decode_verify, omchat_prefill_extend, the masked steps and omchat_beam_begin are refused.  Needs the 16-bit KV cache, tp_size == 1,
 * N <= 16 and N * (q heads per kv head) <= 128; any weight format of the batched step.  It ends with any prefill or with b = 0 (which
 * does nothing else).  A captured decode graph is bound to (b, N, prompt_len).
 * Refused before any state is touched: a beam search in progress, a left-padded or masked-decode state, rows of other lengths than
 * prompt_len, b * N > max_batch.  No host sync. */
int omchat_group_begin(omchat_ctx* ctx, int b, int N, int prompt_len, int share, void* stream);
/* 1 when omchat_group_begin(ctx, ., N, ., 1) is available on this context (the conditions above), else 0 */
int omchat_group_share_available(omchat_ctx* ctx, int N);

/* ---- prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)) -------------------------- */
#define OMCHAT_VERIFY_KEEP_ALL 1
#define OMCHAT_VERIFY_SAMPLE 2
/* T >= 2 tokens of sequence 0 on top of its cache (b = 1 context state, after omchat_prefill):
 * tokens device int32 [T] = the last emitted token (not yet cached) followed by T - 1 draft tokens.
 * Appends T slots at L..L+T-1.
 * logits: device fp32 [T, t_vocab] or NULL (rank-local under TP).
 * picks: device int32 [T], the greedy pick at each position.
 * *n_accept (host): n = the largest n <= T-1 with tokens[j+1] == picks[j] for all j < n.
 * The cache is then trimmed to L + 1 + n slots, device and host lengths both.
 * flags & OMCHAT_VERIFY_KEEP_ALL keeps all T slots (teacher forcing; n is still reported).
 * Refused while sampling or a beam search is active, with the e4m3 cache, and when L + T > max_seq.
 * T <= 16 and T * (t_heads / t_kv_heads) <= 128 (the query rows of one kv head in the attention kernel), checked before anything is enqueued.  The rows go through the batched decode path (packed-operand GEMVs: the first verify step builds the packed weight replica, as
 * the first batched omchat_decode_step does) and the multi-query attention of omchat_op_attn_verify; never captured in the decode graph.
 * Synchronises (the host needs n).
 * flags & OMCHAT_VERIFY_SAMPLE: the sampled form (HF's assisted decoding with do_sample=True and a drafter without logits).  Sampling must be
 * on (omchat_set_sampling; every parameter and the four filters of omchat_set_sampling_filters apply).  picks[j] is then the id a plain
 * omchat_decode_step of sequence 0 would sample at that position: drawn with row 0's key at step s + j (s = sequence 0's step counter) from
 * logits processed with the seen set of sequence 0 plus tokens[1..j].  n is computed as above.  The n + 1 emitted picks picks[0..n] are then
 * committed to sequence 0 on the device: their seen bits set, the step counter advanced by n + 1; a rejected draft leaves no trace.
 * omchat_kv_rewind(ctx, 1, r) straight after it takes back the last r <= n + 1 of these picks (slots, step counter and the seen bits they
 * newly set), also with the repetition penalty on; once a prefill or any decode step ran, the one-step rule of omchat_kv_rewind holds again.
 * Without the flag nothing changes: the call is still refused while sampling is on.  With it the call is refused while sampling is off,
 * together with OMCHAT_VERIFY_KEEP_ALL, and -- as without it -- while constraints, logprobs or a beam search are on and with the e4m3 cache.
 * The first sampled verify step with the penalty on allocates 16 seen bitmaps (counted in omchat_device_bytes). */
int omchat_decode_verify(omchat_ctx* ctx, const int32_t* tokens, int T, float* logits, int32_t* picks,
                         int* n_accept, int flags, void* stream);

/* ---- multi-turn: continue sequence 0's cache (generate(reuse_cache=True)) ---------------------- */
/* Sequence 0 of a context whose cache state is ONE right-aligned sequence (after omchat_prefill with b = 1, any number of omchat_decode_step /
 * omchat_decode_verify calls, or an earlier extend).  Sets the sequence's length to keep (0 <= keep <= current length: slots >= keep are
 * forgotten, slots < keep are not written), runs the decoder over the S_new rows embeds [S_new, t_hidden] at positions keep .. keep + S_new - 1,
 * appends their K / V and leaves device and host lengths / positions as an omchat_prefill of keep + S_new rows would, so decode steps, verify
 * steps, sampling and the decode graph continue unchanged.  logits_last: device fp32 [t_vocab] of the last row (or NULL); hidden_out: optional
 * [S_new, t_hidden] post-final-norm rows (test hook).  keep = 0 issues exactly omchat_prefill's launches (same bits).  The attention takes
 * the prefill kernel with q_pos0 = keep when the block alone fills the GPU and the split-KV block attention (omchat_op_attn_extend) otherwise
 * (omchat_extend_attn_form).  Refused before anything is enqueued: no live sequence-0 state, a b > 1 state, a left-padded or masked-decode
 * state, an active beam search, keep outside [0, length], S_new < 1, S_new > max_prefill_rows, keep + S_new > max_seq, the e4m3 KV cache,
 * fp8 x fp8 prefill GEMMs and tensor-parallel contexts.  Synchronises. */
int omchat_prefill_extend(omchat_ctx* ctx, const void* embeds, int S_new, int keep, float* logits_last, void* hidden_out, void* stream);
/* the attention form omchat_prefill_extend takes for S_new rows on top of keep cached ones with Hkv kv heads on the current device:
 * 0 = the prefill kernel with q_pos0, 1 = the split-KV block attention */
int omchat_extend_attn_form(int S_new, int keep, int Hkv);
/* test hook: rows [pos0, pos0 + n) of sequence 0's 16-bit K (which = 0) or V (which = 1) cache of decoder layer `layer`, copied to
 * out [t_kv_heads, n, 128] (device, context dtype) */
int omchat_kv_read(omchat_ctx* ctx, int layer, int which, int pos0, int n, void* out, void* stream);
/* the same for cache row `row` < max_batch (the sibling rows of a group) */
int omchat_kv_read_row(omchat_ctx* ctx, int row, int layer, int which, int pos0, int n, void* out, void* stream);

/* ---- shared-prefix batches: N suffixes over one prefilled prompt -------------------------------------------------- */
/* omchat_prefill_suffixes: rows 0 .. N - 1 each hold exactly `keep` slots of ONE prompt on the host and the device -- the ordinary rows that
 * omchat_group_begin(ctx, 1, N, keep, 0) leaves, the shared-prompt state of omchat_group_begin(ctx, 1, N, keep, 1), or for N == 1 simply the
 * b = 1 state with keep slots.  embeds [N, S_max, t_hidden] (device, context dtype), row j valid in [0, lengths[j]) (host lengths, 1 .. S_max);
 * the other rows are padding: they may be computed, and they write no cache slot.  Row (j, t) runs through the layers at position keep + t
 * over the prompt keys [0, keep) of row 0 and row j's own keys [keep, keep + t]; its K / V are appended at slot keep + t of row j's own cache.
 * No slot outside [keep, keep + lengths[j]) of any row is written, row 0's slots < keep never.  The lengths end as keep + lengths[j] on the
 * host and the device, positions and the pick state as omchat_prefill leaves them; a shared-prompt group stays on, and omchat_decode_step
 * then takes its N rows of different lengths.  logits_last: device fp32 [N, t_vocab], row j = the logits of (j, lengths[j] - 1) (or NULL);
 * hidden_out: optional [N, S_max, t_hidden] post-final-norm rows.  The attention is omchat_op_attn_suffix; over forked rows tuning key 51 = 0
 * takes the batched prefill kernel with q_pos0 = keep instead (omchat_suffix_attn_form).  Refused before anything is enqueued: no such
 * state (a row that does not hold keep slots, a group of another shape), keep < 1, lengths outside [1, S_max], N > max_batch,
 * N * S_max > max_prefill_rows or > 65535, keep + S_max > max_seq, an active beam search, a left-padded or masked-decode state, the e4m3 KV
 * cache, fp8 x fp8 prefill GEMMs, tensor-parallel contexts, and more than 8 query heads per kv head over a shared
 * prompt.  Synchronises. */
int omchat_prefill_suffixes(omchat_ctx* ctx, const void* embeds, int N, int S_max, const int32_t* lengths, int keep, float* logits_last,
                            void* hidden_out, void* stream);
/* the attention form omchat_prefill_suffixes takes (shared: over a shared prompt; n_rep = q heads per kv head): 1 = the suffix kernel,
 * 0 = the batched prefill kernel with q_pos0 = keep */
int omchat_suffix_attn_form(int shared, int n_rep);

/* ---- decode step as a hipGraph ------------------------------------------------------------------------------------ */
/* With on != 0, omchat_decode_step on a TP = 1 context (b <= 32) replays one captured graph per step instead of issuing its
 * ~230 kernel launches (same kernels, same results: tests compare bit for bit).  Captured on a context-owned stream that is
 * ordered after / before the caller's `stream` with events; re-captured when a sequence outgrows the captured split-KV grid
 * (every 1024 tokens) or the batch size / fp8 / MXFP4 mode changes.  While profiling is enabled every 8th step runs eagerly so the
 * HIP-event brackets still sample the timed region.
 * Measured on ROCm 7.2 / MI355X (bench.py --graph): replay is SLOWER than the eager stream (3.21 vs 2.96 ms per token at
 * TP = 1: graph nodes are dispatched with a barrier packet each), so it is opt-in -- useful when the host, not the GPU,
 * bounds the step (small per-rank kernels under tensor parallelism, a busy Python thread). */
int omchat_enable_decode_graph(omchat_ctx* ctx, int on);
int omchat_decode_graph_stats(omchat_ctx* ctx, long* steps, long* replays, long* captures);
/* bf16x12: *roles = the roles tuning key 50 selects now (bit 0 gate|up, 1 down_proj, 2 lm_head); launches[3] = coded launches
 * enqueued so far per role by eager steps and graph captures; coded[3] = tensors of the role that are coded (built, under the patch cap).
 * Any pointer may be NULL. */
int omchat_bf16x12_stats(omchat_ctx* ctx, int* roles, long* launches, int* coded);

/* ---- weight-only fp8 for decode (BASELINE configs[4]) -------------------------------------------- */
/* Builds (once) an OCP e4m3 replica of the decoder weights that a decode step streams (fused qkv, o, gate|up, down,
 * lm_head): per output row scale = absmax / 448, W8 = e4m3_rne(W / scale).  With on != 0, batch-1 decode steps on a
 * context (any tensor-parallel degree: each rank quantises its own shard, one scale per local output row) read these bytes (half the
 * HBM traffic of the 16-bit weights) and apply the scale after the fp32
 * row reduction; prefill and b > 1 steps keep the 16-bit weights.  Not part of the reference (it has no quantised
 * path): parity is against the oracle run on the de-quantised weights. */
int omchat_enable_fp8_decode(omchat_ctx* ctx, int on);

/* ---- weight-only MXFP4 for decode ----------------------------------------------------------- */
/* Builds (once) an MXFP4 replica (OCP Microscaling v1.0) of the same decode-streamed weights: per output row and per block of 32
 * consecutive k one e8m0 scale byte, e = floor(log2(absmax)) - 2 (stored e + 127; 127 for a zero block), and e2m1 codes of w / 2^e,
 * round to nearest, ties to the even code, saturating at 6; two codes per byte, the even k in the low nibble.  4.25 bits per weight:
 * 3.76 GB streamed per token at Qwen2-7B width against 14.1 GB (16-bit) and 7.1 GB (e4m3).
 * mode 0: off.
 * mode 1: batch-1 decode steps read the replica through gfx950's e2m1 -> 16-bit convert at scale 1 and apply 2^e to the lane's fp32
 *   partial sum; prefill, b > 1 steps, the verify step and beam search keep the 16-bit weights.
 * mode 2: as mode 1, and every decode-side pass with 2 <= b <= 32 rows -- batched steps, omchat_decode_step_masked*, beam steps,
 *   omchat_decode_verify -- reads a PACKED copy of the same codes and scales (a byte shuffle of the replica into the fragment order of
 *   the packed batched GEMVs; + N K (1/2 + 1/32) bytes per matrix, about + 3.8 GB at Qwen2-7B width) through MFMA forms: the codes are
 *   widened at scale 1, each 16-row x 32-k unit runs one MFMA from a zero accumulator, and 2^e of the row's block is applied to the
 *   fp32 result.  One weight format per generation: a step of more than 32 rows is refused while mode 2 is on, never run on 16 bits.
 *   The 16-bit packed replica of batched decode is not built for steps that stream the MXFP4 one.
 * After omchat_load_tensor the next step re-quantises (and re-packs) in place: the device pointers, and so a captured graph, stay valid.
 * Refused, with the mode left as it was: before the weights are loaded; while omchat_enable_fp8_decode is on (and the reverse: one
 * weight format per step); on a tensor-parallel context; when a streamed K (hidden_size, heads x 128, intermediate_size) is not a
 * multiple of 32; mode 2 also when one of those three is not a multiple of 64, when the qkv width, hidden_size or vocab_size is not a
 * multiple of 16, or when the packed copy does not fit in device memory.  The e4m3 KV cache and the fp8 x fp8 prefill GEMMs are
 * independent of it.  Not part of the reference: parity is against the oracle run on the de-quantised weights
 * (tests/test_gpu_mxfp4.py, tests/test_gpu_mxfp4_batched.py). */
int omchat_enable_mxfp4_decode(omchat_ctx* ctx, int mode);

/* ---- the weight format of a decode step ---------------------------------------------------------------------------- */
/* The formats a decode-side pass can stream its five projections in (qkv, o_proj, gate|up, down_proj, lm_head). */
enum omchat_weight_format {
  OMCHAT_WFMT_16 = 0,             /* the 16-bit weights, row-major */
  OMCHAT_WFMT_16_PACKED = 1,      /* their packed replica for batched steps */
  OMCHAT_WFMT_E4M3 = 2,           /* omchat_enable_fp8_decode */
  OMCHAT_WFMT_MXFP4 = 3,          /* omchat_enable_mxfp4_decode, row-major */
  OMCHAT_WFMT_MXFP4_PACKED = 4,   /* its packed copy (mode 2) */
  OMCHAT_WFMT_COUNT = 5
};
/* The one rule (host-only, no context): the format a step of `rows` rows streams, and in *x_pack_nb (may be NULL) the block count of the
 * packed activation layout its GEMVs run on (0 = row-major activations, 1, or 2 for rows > 16).  fp8_on / mxfp4_mode: what the two enable
 * calls set (never both); packed16_ready: the 16-bit packed replica is built and current; geometry_ok: hidden_size, heads x 128 and
 * intermediate_size are each a multiple of 64.
 *   rows == 1:        e4m3 if fp8_on, else MXFP4 if mxfp4_mode >= 1, else 16-bit
 *   2 <= rows <= 32:  packed activations when geometry_ok; the weights packed MXFP4 in mode 2, else 16-bit packed if that replica is
 *                     ready and the activations are packed, else 16-bit.  (Mode 2 without geometry_ok -- refused by the enable call --
 *                     answers packed MXFP4 with *x_pack_nb = 0, which every step refuses.)
 *   rows > 32:        16-bit, row-major activations (with mode 2 on, the step entries refuse such a step up front) */
int omchat_decode_weight_format(int rows, int fp8_on, int mxfp4_mode, int packed16_ready, int geometry_ok, int* x_pack_nb);

/* ---- fp8 KV cache and fp8 x fp8 prefill GEMMs (BASELINE configs[4]: long video context, "fp8 MFMA weights") ------ */
/* omchat_enable_fp8_kv: after the next prefill the decode steps read keys and values as OCP e4m3 bytes (57 344 -> 28 672 bytes per
 * cached token, + 2 x 4 kv heads x 28 layers fp32 scales) with one scale per (layer, sequence, kv head, position) = absmax / 448; the
 * token being decoded is rotated, appended and quantised before its attention.  The 16-bit cache stays (prefill attention reads it).
 * omchat_enable_fp8_prefill: the qkv and gate|up GEMMs of the prefill run as fp8 x fp8 MFMA: activations quantised per token by the
 * RMSNorm kernel, weights from the e4m3 replica (per output row); o_proj / down_proj keep 16-bit operands.
 * Neither is part of the reference: parity is stated against the oracle on de-quantised operands (tests/test_gpu_fp8.py). */
int omchat_enable_fp8_kv(omchat_ctx* ctx, int on);
int omchat_enable_fp8_prefill(omchat_ctx* ctx, int on);

/* ---- measurement: HIP-event timing of the dominant kernel classes, recorded on the launch stream ------------------ */
#define OMCHAT_PROF_DECODE_GATEUP 0   /* decode gate|up weight-streaming GEMV (+SwiGLU), one launch per layer per token */
#define OMCHAT_PROF_PREFILL_GATEUP 1  /* decoder prefill gate|up MFMA GEMM (+SwiGLU), one launch per layer */
#define OMCHAT_PROF_VIT_FC1 2         /* ViT fc1 MFMA GEMM (+bias+GELU), one launch per layer */
#define OMCHAT_PROF_CATS 3
int omchat_prof_enable(omchat_ctx* ctx, int on);
/* synchronises the device, folds the recorded event pairs into (total_ms, launches) for `cat`; reset != 0 clears. */
int omchat_prof_read(omchat_ctx* ctx, int cat, double* total_ms, long* launches, int reset);

/* ---- the one native op seam of the reference: FlashAttention.forward (intern_vit_6b/flash_attention.py:30-75) --- */
/* qkv packed [B, S, 3, H, 128] -> out [B, S, H, 128]; softmax_scale <= 0 means 1/sqrt(128). */
int omchat_mha_fwd(const void* qkv, int B, int S, int H, float softmax_scale, int causal, void* out, int dtype, void* stream);
/* same seam with head dim D = 128 | 64 and the key_padding_mask branch (:56-67) for right-padded batches: seqlens int32 [B] on the
 * device (NULL = all S); keys >= seqlens[b] are masked, rows of padded queries are left to the caller to zero (pad_input) */
int omchat_mha_fwd_varlen(const void* qkv, int B, int S, int H, int D, const int32_t* seqlens, float softmax_scale, int causal,
                          void* out, int dtype, void* stream);

/* ---- op-level entry points (unit parity tests, benches) --------------------------------------------------------- */
/* C[M, N] = epi(A[M, K] W[N, K]^T) on MFMA, fp32 accumulate.  Contract (checked, an error otherwise): K % 64 == 0; lda, ldw % 8 == 0 and
 * A, W 16-byte aligned; N % 4 == 0 (the epilogue owns four consecutive columns per lane); C and resid 8-byte aligned with ldc, ldr % 4 == 0
 * (8-byte epilogue accesses); bias and ls 8-byte aligned; EPI_SWIGLU: N % 32 == 0 and C is [M, N / 2]. */
int omchat_op_gemm(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                   const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, void* stream);
/* Round 6: the vision tower's norms folded into its GEMMs (csrc/model.hip vit_layer_fused; InternVisionEncoderLayer.forward,
 * modeling_intern_vit.py:210-222 with InternRMSNorm :39-44 and the joint-head q / k norm :143-148).  Op-level entries of its pieces:
 * omchat_op_gemm_fused = omchat_op_gemm with (a) a per-row factor on the fp32 accumulators, C = epi(s[m] * (A W^T) ...) -- the RMSNorm in front
 * of a projection -- given either finished (row_scale [M] fp32) or as the producer's statistics slots (rs_stats, s[m] = rsqrt(sum of slots
 * [0, rs_nslots) / rs_dim + rs_eps), finished per tile inside the launch); both null = no factor; (b) epi 7 (= 2, layer-scale + residual) /
 * 8 (= 0) that also leave stats fp32: per row and per wave-column block ("slot") the sum of squares of the 16-bit values stored.  ALL statistics
 * buffers are SLOT-MAJOR: element (slot s, row m) at [s * ld + m], ld >= M (the 16 rows of an MFMA fragment are one 64-byte run for the producer,
 * and a consumer's wave reads 64 consecutive rows of a slot); *nslots = the number of slots written (one per wave tile of the tile kernel(s) that
 * ran: 64 or 112 columns each; epi 8 runs on 64-column wave tiles only, so the thirds of a fused q | k | v output own whole slots).  omchat_op_stats_finish: for group g < ngroups, t_g = sum of slots
 * [slot0 + g * nslots, slot0 + (g + 1) * nslots) of a row; dim > 0: out[m * ngroups + g] = rsqrt(t_g / dim + eps), dim == 0: out = t_g (a
 * stand-alone finishing launch: tests and callers outside the fused layer).  omchat_op_row_sumsq: stats[m] = sum_c x[m][c]^2 (slot 0).
 * omchat_op_fold_cols: out[r][c] = T(W[r][c] * n[c]) (a norm weight folded into the columns of the linear map behind it).
 * omchat_op_vit_knorm_slots: the K half of the joint-head norm from the qkv GEMM's slots (q slots [0, nslots), k slots [nslots, 2 nslots),
 * nslots <= 64): k = T(w_k * T(k * rsqrt(sum k slots / C_total + eps))) in place on rows of stride ld, sumsq_q[m] = sum of the q slots.
 * omchat_op_mha_qnorm: omchat_mha_fwd on packed qkv [B, S, 3, H, 128] whose Q is RAW -- q = T(T(w_q * T(q * rstd_q)) * q_scale) is applied
 * where the kernel loads Q, rstd_q from sumsq[(b * S + s) * stride]. */
int omchat_op_gemm_fused(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                         const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, const float* row_scale,
                         const float* rs_stats, int rs_ld, int rs_nslots, int rs_dim, float rs_eps,
                         float* stats, int stats_ld, int* nslots, void* stream);
int omchat_op_stats_finish(const float* stats, int ld, int slot0, int nslots, int ngroups, int rows, int dim, float eps, float* out, void* stream);
int omchat_op_row_sumsq(int dtype, const void* x, int ldx, int rows, int H, float* stats, void* stream);
int omchat_op_fold_cols(int dtype, const void* W, const void* n, void* out, int rows, int cols, void* stream);
int omchat_op_vit_knorm_slots(int dtype, void* k, int ld, const void* wk, int rows, int C, int C_total, float eps, const float* stats, int stats_ld,
                              int nslots, float* sumsq_q, void* stream);
int omchat_op_mha_qnorm(int dtype, const void* qkv, int B, int Sq, int H, const float* sumsq, int stride, int dim, const void* wq,
                        float eps, float q_scale, void* out, void* stream);
/* same with the stream-K tail enabled: ws from omchat_op_gemm_sk_ws() bytes of device memory; stream_k 0 = auto, 1 = required */
/* experiment knobs -- PROCESS-GLOBAL test / measurement hooks shared by every context of the process: refused (error return) unless the
 * process environment has OMCHAT_ALLOW_TUNING=1; nothing in the product sets a key.  (key 0: start skew of the 256x256 GEMM workgroups, in units of ~1024 cycles; key 1: 1 = skinny GEMM
 * always takes the MFMA form, 0 = batch 1 takes the whole-row streaming form; key 4: row count from which a tensor-parallel
 * row-parallel projection is pipelined against its all-reduce in 2 chunks (3x: 4 chunks), default 1024; key 5: 0 = GEMM tile
 * shapes from the cost model instead of the first-use measurement; key 6: 0 = batched decode steps (2 <= b <= 32) read the
 * row-major weights instead of building the packed replica (+ one more copy of the decoder weights); key 8: 0 = first-generation
 * 16x16x32 prefill attention kernel; key 9: 0 = tensor-parallel decode over the peer transport keeps the all-reduce of the split-K
 * slices and the residual + RMSNorm as two launches instead of omchat_peer_resid_rmsnorm; key 10: key tiles (of 64) per wave of the
 * split-KV decode attention, 0 = chosen from the grid size (1 for single sequences, up to 4 for large batches); key 11: 1 = the batched
 * decode GEMV never takes its x-stationary persistent form; key 12: 1 = the batched decode attention loads its K tiles as whole rows
 * through LDS instead of fragment-shaped straight to registers (same bits; measured neutral); key 13: 1 = multi-round 256x256 GEMMs
 * take the persistent one-workgroup-per-CU form that overlaps the next tile's prologue with the epilogue (same bits; measured neutral);
 * key 14: batch-1 decode, bit 0 = the post-attention RMSNorm runs inside the gate|up GEMV, bit 1 = the input / final RMSNorm inside the
 * qkv / lm_head GEMV with down_proj un-split (default 3; 0 = both residual + RMSNorm launches stay); bit 2 (experiments build only; off by
 * default in BOTH builds, so the twin's batched decode is the product's) = batched steps (2 <= b <= 32) take the seven-launch layer -- o_proj
 * un-split with the residual in its epilogue, the post-attention norm in the x-stationary gate|up GEMV -- measured slower: 4.57-4.87 vs 4.28 ms;
 * key 16: which of those norm-in-GEMV launches take the loop form (one resident round of workgroups, three register buffers per wave):
 * bit 0 = gate|up, bit 1 = qkv, bit 2 = e4m3 gate|up, bit 3 = lm_head (default 0 since round 5 -- key 38; every form gives the same bits);
 * key 17: 1 (default) = batch-1 o_proj / qkv launches whose rows deal evenly to two workgroups per CU use N / (2 CUs) waves per workgroup;
 * key 19: split-KV merges with more partials per head than this take the 512-thread form (default 64: at 57 partials the 128-thread
 * one-batch form is faster, 4.9 vs 5.9 us);
 * key 21: column groups per head in the split-KV merge: 1 (default) = four workgroups per head beyond 256 partials (33 k keys: 21 -> ~7 us
 * per launch), 2 = also two workgroups per head for 65..256 partials (neutral), 0 = one workgroup per head;
 * key 22: 1 = a batch-1 decode step on one GPU (16-bit weights and cache, <= 4096 keys) runs attention + merge + o_proj as one launch
 * (fused_decode.hip), 0 (default) = as three launches (same bits);
 * key 23: 1 = such a step runs every decoder layer as ONE launch (decode_layer.hip: qkv, attention, merge, o_proj, gate|up, down
 * with in-launch hand-offs; measured slower: 98 vs 91.5 us per layer), 0 (default) = six launches per layer (same bits);
 * key 24: 1 = the batch-1 gate|up GEMV takes its shares from per-XCD work queues (gemv_rows_norm_dyn_kernel; eager steps only; same
 * bits; measured 80-331 us against 45: the returning atomic drains the wave's load ring), 0 (default) = equal static shares;
 * key 25: 1 (default) = decode attention launches with enough keys (>= 6 tiles of 32 keys per CU: b >= 4 at 3.7 k keys, b = 1 from ~12 k)
 * take the LDS-DMA ring form (attention.hip: attn_decode_dma_kernel; 16-bit cache), 0 = the register multi-tile / one-tile kernels;
 * key 26: low byte = resident waves per CU that form's split count is sized for (0 = by launch size: 2 or 4), next byte = ring stages 2..4;
 * key 27 / 28: experiments (rotated tile order of that form; per-(blockIdx % 8) share deltas of the batch-1 gate|up GEMV, eight nibbles
 * d + 8: measured 1 % at best, profiles/r04_n);
 * key 30: GQA prefill attention, heaviest causal query-block ranks issued as two workgroups of half the kv group's heads each: -1 (default) =
 * a quarter of the ranks while the launch is at most one workgroup per CU (S <= 2048 for one Qwen2-7B sequence: 61.2 -> 53.7 us), 0 = off,
 * n > 0 = n ranks whatever the size (same bits either way);
 * key 33: 1 (default) = MHA prefill attention launches (the ViT) use a one-dimensional grid that keeps the query blocks of a (head, sequence) pair on
 * one XCD (K / V fetched once: 355 -> 82 MB per launch at 3 tiles), 0 = (query block, head, sequence) grid (same bits);
 * key 29: tensor parallelism, 1 = the row-parallel projections of the ViT / the prefill are all-reduced as fp32 partial sums and the
 * epilogue (bias, layer scale, residual) is applied once to the sum, so TP = N differs from TP = 1 in fp32 summation order only (twice
 * the bytes on the links); 0 (default) = every rank applies the epilogue to its own partial and 16-bit results are summed.  TP = 8 f16
 * logit error against TP = 1: 4.97e-3 with, 5.32e-3 without (profiles/r04_w, r04_x));
 * key 34: launch shapes for the SHARD widths of a tensor-parallel rank's decode GEMVs (default 15): bit 0 = the x-stationary form, one tile per
 * workgroup, for the short qkv shard of a batched step; bit 1 = split-K slices of >= 16 chunks and one chunk per wave per step for short-K
 * o_proj / down_proj shards; bit 2 = one (gate, up) pair per wave for the short batch-1 gate|up shard; bit 3 = the x-stationary form, one
 * (gate, up) tile per workgroup, for a batched gate|up shard of at most one tile per CU (0 = the round-4 shapes; same sums up to fp32 order
 * where the slice count changes);
 * key 35 (experiments build): a rank context whose exchanges are no-ops takes the one-GPU launch structures on its shard widths (measurement);
 * key 36 (experiments build): 2 = the MHA prefill attention splits the keys between two wave groups of an eight-wave workgroup (measured slower);
 * key 43: 1 (default) = the MFMA GEMMs issue no operand reads and no MFMAs for 64-row blocks / waves that lie wholly beyond M (the 13th row tile of the
 * 3-tile ViT holds 3 valid rows of 256), 0 = full issue (same bits; in the model -0.7 % of the ViT, inside the noise: profiles/r06_a_gemm_dead_row_skip_ab.txt);
 * key 44: 1 (default) = the RMSNorm vision tower at TP = 1 runs the fused layer of round 6 (norm1 / norm2 as a row scale of the qkv / fc1 GEMM with the
 * norm weight folded into the GEMM weight, statistics from the producing GEMM's epilogue finished per tile inside the consuming GEMM, q norm on load in the
 * attention kernel, K norm from the qkv epilogue's statistics: six launches), 0 = the eight launches of round 5;
 * key 46: 1 (default) = MHA prefill attention whose key count is a whole number of 64-key tiles + 1 (the ViT: 1025) folds the odd key into the
 * online softmax's initial state (m = q . k_last, l = 1, O = v_last) instead of giving it a tile step of its own (-5.9 % of the launch), 0 = 17 tile steps;
 * key 47: 64-key tiles per wave of the decode attention over the e4m3 KV cache: 0 (default) = by the launch's size (one wave per tile below two
 * one-tile waves per CU; from there a wave walks 3 tiles with the next one prefetched into registers, and four such waves share a workgroup and
 * fold their states in LDS when that leaves <= 64 partials per head for the one-round-trip merge and still fills half the CUs: 33 k keys 21.1 ->
 * 14.9 us per attention + merge), 1 = always one wave per tile, 2 / 3 / 4 = tiles per wave forced, 11 = 3 tiles x 4 waves forced;
 * key 48: 1 (default) = that walking form also rotates q / k and appends + quantises the new token's k / v rows (no RoPE + append launch in front of
 * the attention of a long-context e4m3 decode step; the same bytes), 0 = separate launch;
 * key 52: the unmasked one-tile split-KV decode attention over the 16-bit cache (one workgroup per 64-key split, kv head, sequence): 1 (default) = a
 * single sequence's launch shares each tile among four waves (attn_decode_4w_kernel: K through an LDS image, S^T and the softmax in every wave, the PV
 * product and the partial's columns by quarters), 0 = one wave per tile (attn_decode_kernel), 2 = four waves at every batch size; the same partials,
 * output and appended cache bytes bit for bit;
 * key 45: 1 (default) = sequence-parallel norms under tensor parallelism (omchat_ctx_sp_stats), 0 = one all-reduce per sub-block and replicated norms;
 * key 37: 1 (default) = the GEMM epilogues store 16 bytes per lane (two column blocks exchanged between lane pairs), 0 = 8 bytes (same bits);
 * key 38: (gate, up) pairs per wave of the batch-1 gate|up GEMV's non-loop norm form: 1 (default: thousands of small workgroups that the dispatcher
 * re-balances over the XCDs; decode 2.650 -> 2.597 ms per token against the loop form), 2, 3 (same bits); 16 x n sets the e4m3 replica's form
 * (default 1: 1.700 -> 1.658 ms per token against 4);
 * key 39 (experiments build): n = 1 / 2 / 4: the batch-1 long-K GEMV (down_proj) loads x from L2 in every wave instead of staging it in LDS, as
 * workgroups of n waves (same bits; measured slower: 2.70 against 2.605 ms per token);
 * key 40 (experiments build): 1 = RMSNorm and ViT q / k norm launches of >= 256 rows (H <= 4096) take one wave per row -- all loads up front, no LDS,
 * no barrier; same bits, measured no faster -- 0 (default) = one workgroup per row;
 * key 41 (experiments build, TIMING PROBE: results are INVALID under it): 1 = every launch goes out with hipExtAnyOrderLaunch (consumers may overtake
 * producers): prices the launch boundaries of a step;
 * key 28 (the static-skew form < 256 exists in the experiments build only: the product build IGNORES values below 256): < 256: workgroups moved from every odd XCD's share of the batch-1 gate|up launch to every even XCD's (contiguous pair ranges per XCD; same bits;
 * -0.6 % of the step at 24); >= 256: eight nibbles of per-XCD share deltas of the loop form (round 4);
 * key 42 (experiments build, prototype): bit 0 = the batch-1 o_proj GEMV is launched out of order behind the split-KV merge and waits on its per-head completion
 * flags (gemv_rows_wait_kernel; bit-identical results); bit 1 = cache-bypassing loads of the row instead of an agent-scope acquire, bit 2 = write-through store
 * in the merge instead of a release, bit 3 = slower poll, bit 4 = collect in-kernel clock stamps of the six launches of a layer (printed by omchat_fused_status); measured not faster (7: 2.618 against 2.608 ms per token) */
/* batch-1 skinny GEMM with the RMSNorm that precedes it computed in the registers of every wave: y = epi(W RMSNorm(x; norm_w, eps)),
 * x the raw hidden row [K], K <= 4096, epi NONE / SWIGLU (transformers modeling_qwen2.py:247-252 + :46-48; the decode step uses it for
 * post_attention_layernorm + gate|up) */
int omchat_op_gemv_norm(int dtype, const void* X, const void* W, int ldw, void* Y, int N, int K, const void* norm_w, float eps,
                        const void* bias, int epi, int out_f32, void* stream);
int omchat_op_set_tuning(int key, int value);
/* GEMM tile choices are measured on first use of a (dtype, epilogue, ceil(M/256), N, K) class; load / dump persist them as text
 * (returns the number of entries, -1 when the file cannot be opened); omchat_gemm_tune_runs = measurements done by this process */
int omchat_gemm_tune_load(const char* path);
int omchat_gemm_tune_dump(const char* path);
long omchat_gemm_tune_runs(void);
size_t omchat_op_gemm_sk_ws(void);
int omchat_op_gemm_sk(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                      const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, void* ws,
                      size_t ws_bytes, int stream_k, void* stream);
int omchat_op_gemv(int dtype, const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int b, int N, int K,
                   const void* bias, const void* resid, int ldr, int epi, int out_f32, void* stream);
/* batched decode GEMV with packed operands (MFMA fragment order, csrc/common.h): packs X [b <= 32, K] (and W [N, K] when
 * w_packed) into scratch, then Y = epi(X W^T); epi EPI_NONE (T or fp32 out) | EPI_SWIGLU (y_packed: output in the packed x layout
 * of the consumer) | EPI_PARTIAL (fp32 [ksplit][b][ldy]).  omchat_op_pack_x: row-major -> packed x with NB = b > 16 ? 2 : 1. */
int omchat_op_gemv_packed(int dtype, const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int b, int N, int K,
                          const void* bias, int epi, int out_f32, int ksplit, int w_packed, int y_packed, void* stream);
int omchat_op_pack_x(int dtype, const void* X, int ldx, int b, int K, void* out, void* stream);
/* Test hook: the launch that the skinny-GEMM entry points above would make for these integers on the current tuning state, decided on the
 * host without a launch (dense operands).  flags: bit 0 x_packed, 1 w_packed, 2 y_packed, 3 norm_w given, 4 out_f32, 5 force_mfma, 6 resid given;
 * wf: weights 0 = 16-bit, 1 = e4m3 + row scales, 2 = MXFP4, 3 = bf16x12; n_cu: compute units to plan for (<= 0: the device's).
 * out[OMCHAT_GEMV_PLAN_INTS] (fields that the kernel family does not have are 0):
 *   [0] family: 0 gemv_kernel (MFMA), 1 gemv_pk, 2 gemv_xs, 3 gemv_xs_split, 4 gemv_rows, 5 gemv_rows_norm, 6 gemv_rows_norm_loop,
 *       7 gemv_rows_longk, and in -DOMCHAT_EXPERIMENTS=1 builds 8 gemv_rows_norm_dyn, 9 gemv_rows_longk_direct
 *   [1] weight form (as wf)  [2] packed W (gemv_pk)  [3] epilogue  [4] NTILE  [5] WAVES  [6] UNROLL  [7] NB  [8] RR  [9] NCH  [10] NORM (gemv_xs)
 *   [11] grid x  [12] grid y  [13] block  [14] dynamic LDS bytes  [15] per_wg  [16] skew (loop form)  [17] rows_per_wg (long-K form)
 *   [18] n5 (gemv_xs_split)  [19] xskew (experiments build)
 * A call that the entry points refuse returns 1 with their text in omchat_last_error.
 * The hook passes no work counters (GemvArgs::dyn_ctr), so tuning key 24 (family 8) does not show through it.
 * omchat_op_gemv_split_k: the K slices (ksplit) that a decode step of batch b and hidden size H gives its o_proj (down = 0, K = q width) or
 * down_proj (down = 1, K = mlp width) launch; packed: the step streams a packed weight replica. */
#define OMCHAT_GEMV_PLAN_INTS 20
int omchat_op_gemv_plan(int dtype, int b, int N, int K, int epi, int ksplit, int flags, int wf, int n_cu, int* out);
int omchat_op_gemv_split_k(int b, int K, int H, int packed, int down);
/* fp8 x fp8 MFMA GEMM (BASELINE configs[4] "fp8 MFMA weights"): A8 [M, K] and W8 [N, K] are OCP e4m3 bytes with one fp32 scale per row;
 * C (dtype) = epi(a_scale[m] * w_scale[n] * A8 W8^T), epilogues as omchat_op_gemm (ls unused).  K % 128 == 0.
 * omchat_op_quant_rows_fp8: per-row (per token) quantisation of activations, optionally behind an RMSNorm (norm_w != NULL). */
int omchat_op_gemm_fp8(int dtype, const void* A8, const float* a_scale, const void* W8, const float* w_scale, void* C, int ldc, int M, int N,
                       int K, const void* bias, const void* resid, int ldr, int epi, void* stream);
int omchat_op_quant_rows_fp8(int dtype, const void* x, const void* norm_w, float eps, void* y8, float* scale, int rows, int H, void* stream);
/* fp8 pieces: W [N][K] (dtype) -> W8 [N][K] e4m3 bytes + scale [N]; y[N] = (W8 . x) * scale (+ epilogue), batch 1;
 * epi EPI_PARTIAL writes fp32 slices [ksplit][N] */
int omchat_op_quant_fp8(int dtype, const void* W, int N, int K, void* W8, float* scale, void* stream);
int omchat_op_gemv_fp8(int dtype, const void* X, const void* W8, const float* scale, void* Y, int N, int K, const void* bias,
                       const void* resid, int epi, int out_f32, int ksplit, void* stream);
/* ... with the preceding RMSNorm in registers: x is the RAW row, as in omchat_op_gemv_norm (K <= 4096, epi NONE / SWIGLU) */
int omchat_op_gemv_fp8_norm(int dtype, const void* X, const void* W8, const float* scale, void* Y, int N, int K, const void* norm_w, float eps,
                            const void* bias, int epi, int out_f32, void* stream);
/* MXFP4 pieces (format: omchat_enable_mxfp4_decode above): W [N][K] (dtype), K % 32 == 0 -> W4 [N][K / 2] bytes + S [N][K / 32] e8m0 bytes;
 * y[N] = epi(sum over blocks of 2^e (codes . x)), batch 1, the epilogues and ksplit of omchat_op_gemv_fp8; _norm: x is the RAW row and the
 * RMSNorm runs in registers as in omchat_op_gemv_norm (K <= 4096, epi NONE / SWIGLU) */
int omchat_op_quant_mxfp4(int dtype, const void* W, int N, int K, void* W4, void* S, void* stream);
int omchat_op_gemv_mxfp4(int dtype, const void* X, const void* W4, const void* S, void* Y, int N, int K, const void* bias,
                         const void* resid, int epi, int out_f32, int ksplit, void* stream);
int omchat_op_gemv_mxfp4_norm(int dtype, const void* X, const void* W4, const void* S, void* Y, int N, int K, const void* norm_w, float eps,
                              const void* bias, int epi, int out_f32, void* stream);
/* MXFP4 under b rows.  _rows: row-major operands -- b == 1 is omchat_op_gemv_mxfp4 without a residual, b > 1 is refused (MXFP4 at b > 1
 * exists on the packed operands only).  _packed: omchat_op_gemv_packed on MXFP4 weights, 1 <= b <= 32, K % 64 == 0, N % 16 == 0: X [b, K]
 * row-major and the row-major replica W4 / S are packed into scratch, then Y = epi(X dequant(W)^T); epi EPI_NONE (T or fp32 out) |
 * EPI_SWIGLU (y_packed) | EPI_PARTIAL.  The packed layout itself is internal (csrc/common.h: packed_w4_index / packed_s4_index). */
int omchat_op_gemv_mxfp4_rows(int dtype, const void* X, int ldx, const void* W4, const void* S, void* Y, int ldy, int b, int N, int K,
                              const void* bias, int epi, int out_f32, int ksplit, void* stream);
int omchat_op_gemv_mxfp4_packed(int dtype, const void* X, int ldx, const void* W4, const void* S, void* Y, int ldy, int b, int N, int K,
                                const void* bias, int epi, int out_f32, int ksplit, int y_packed, void* stream);
/* bf16x12 pieces: the lossless 12-bit coding of bf16 rows that the long batch-1 decode GEMVs stream (DESIGN.md section 17;
 * tests/bf16x12_ref.py defines the format).  _encode: W bf16 [N][K], K % 512 == 0 -> coded [N][K * 3 / 2] bytes, top [N] bytes, cnt [N] bytes
 * (min(misses, 33)), patch [N][32] uint32; *over (device int, zeroed by the caller) becomes 1 when a row needs more than 32 patches -- such a
 * matrix is not coded.  _gemv: y = the bits of the 16-bit launch on the same matrix, batch 1, for norm_w != NULL with EPI_SWIGLU / EPI_NONE
 * (omchat_op_gemv_norm, K <= 4096) and for EPI_RESID with resid on 4096 < K <= 32768 (omchat_op_gemv) */
int omchat_op_encode_bf16x12(const void* W, int N, int K, void* coded, void* top, void* cnt, void* patch, void* over, void* stream);
int omchat_op_gemv_bf16x12(const void* X, const void* coded, const void* top, const void* cnt, const void* patch, void* Y, int N, int K,
                           const void* norm_w, float eps, const void* resid, int epi, int out_f32, void* stream);
/* pack once, launch many times (tools/bench_mxfp4.py): omchat_op_pack_w: W [N, K] -> packed 16-bit replica (N K elements);
 * omchat_op_pack_w4: W4 / S -> packed MXFP4 replica W4P (N K / 2 bytes), SP (N K / 32 bytes); omchat_op_gemv_prepacked: the launch alone on
 * XP (omchat_op_pack_x) and WP, with SP = NULL for 16-bit weights; no allocation, no synchronisation */
int omchat_op_pack_w(int dtype, const void* W, int ldw, int N, int K, void* out, void* stream);
int omchat_op_pack_w4(const void* W4, const void* S, int N, int K, void* W4P, void* SP, void* stream);
int omchat_op_gemv_prepacked(int dtype, const void* XP, const void* WP, const void* SP, void* Y, int ldy, int b, int N, int K, const void* bias,
                             int epi, int out_f32, int ksplit, int y_packed, void* stream);
int omchat_op_rmsnorm(int dtype, const void* x, const void* w, void* y, int rows, int H, float eps, void* stream);
/* the decode step's fused residual add + RMSNorm (modeling_qwen2.py:283-296 + 247-252): x[rows, H] = T(x + T(sum_s part[s])) in place,
 * part = fp32 split-K slices [ks][rows][H] of the projection, then xn = T(w * T(x * rsqrt(mean(x^2) + eps))) (w == NULL: skip);
 * pack_nb != 0 writes xn in the packed x layout of the batched GEMV */
int omchat_op_resid_rmsnorm(int dtype, void* x, int ldx, const float* part, int ks, const void* w, void* xn, int ldn, int rows, int H,
                            float eps, int pack_nb, void* stream);
int omchat_op_vit_qknorm(int dtype, void* qkv, int ld, const void* wq, const void* wk, int rows, int C, int C_total,
                         float eps, float q_scale, void* stream);
/* test hooks: omchat_op_vit_qknorm with the statistics given (sumsq_in [rows, 2] fp32: the q and the k sum of squares of a row over ALL C_total
 * channels, the tensor-parallel form; NULL = the row's own) and / or the K half alone (only_k != 0, needs sumsq_in); omchat_op_vit_qk_sumsq
 * writes those [rows, 2] sums for the q | k columns [0, C) | [C, 2C) of rows of stride ld */
int omchat_op_vit_qknorm_ex(int dtype, void* qkv, int ld, const void* wq, const void* wk, int rows, int C, int C_total,
                            float eps, float q_scale, const float* sumsq_in, int only_k, void* stream);
int omchat_op_vit_qk_sumsq(int dtype, const void* qkv, int ld, int rows, int C, float* sumsq_out, void* stream);
/* q [b,Sq,Hq,128], k/v [b,Hkv,Skv,128] (cache layout), out [b,Sq,Hq,128]; kv_len device int32 [b] or NULL */
int omchat_op_attn_prefill(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv,
                           int Hq, int Hkv, const int32_t* kv_len, int causal, int q_pos0, float scale, void* stream);
/* same with head dim D = 128 or 64 (InternViT-300M attention, intern_vit_300m/modeling_intern_vit.py:138-155) */
int omchat_op_attn_prefill_d(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv,
                             int Hq, int Hkv, int D, const int32_t* kv_len, int causal, int q_pos0, float scale, void* stream);
/* nn.LayerNorm over the last dim (weight + bias), fp32 statistics, one rounding */
int omchat_op_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, int rows, int H, float eps, void* stream);
/* q [b,Hq,128], k/v [b,Hkv,cap,128]; kv_len device int32 [b] or NULL (-> L); ws from omchat_op_attn_decode_ws */
size_t omchat_op_attn_decode_ws(int b, int Hq, int L);
int omchat_op_attn_decode(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Hq, int Hkv,
                          int cap, int L, const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream);
/* Multi-query decode attention of the verify step: T (1..16) consecutive new tokens of ONE sequence over its cache k / v [Hkv,cap,128];
 * query row t sits at position L + t and sees keys 0 .. L + t.  q [T,Hq,128] already rotated, the cache already holding L + T keys;
 * out [T,Hq,128]; ws of omchat_op_attn_decode_ws(T, Hq, L + T) bytes.  T * Hq / Hkv <= 128. */
int omchat_op_attn_verify(int dtype, const void* q, void* k, void* v, void* out, int T, int Hq, int Hkv, int cap, int L, float scale,
                          void* ws, size_t ws_bytes, void* stream);
/* 64-key tiles per split that omchat_op_attn_verify takes over `keys` (= L + T) keys with Hkv kv heads on the current device */
int omchat_op_attn_verify_tpw(int keys, int Hkv);
/* Split-KV block attention of omchat_prefill_extend: Sq >= 1 new query rows of ONE sequence at positions L .. L + Sq - 1
 * (q [Sq,Hq,128] already rotated) over k / v [Hkv,cap,128] that already hold L + Sq keys; row t sees keys 0 .. L + t.  out [Sq,Hq,128];
 * ws of omchat_op_attn_extend_ws(Sq, Hq, Hkv, L) bytes (never more than omchat_op_attn_decode_ws(Sq, Hq, L + Sq)).  Hq / Hkv <= 8. */
size_t omchat_op_attn_extend_ws(int Sq, int Hq, int Hkv, int L);
int omchat_op_attn_extend(int dtype, const void* q, const void* k, const void* v, void* out, int Sq, int Hq, int Hkv, int cap, int L,
                          float scale, void* ws, size_t ws_bytes, void* stream);
/* Shared-prompt decode attention of a sampled group (omchat_group_begin with share = 1): G groups of N consecutive rows,
 * one query token per row.  q [G*N,Hq,128] already rotated; k / v [G*N rows,Hkv,cap,128] complete: the keys [0, P) of a group are read from
 * its first row only (never its slots >= P), the keys [P, L) of every row from that row's own cache.  out [G*N,Hq,128]; ws of
 * omchat_op_attn_shared_ws(G, N, Hq, Hkv, P, L) bytes.  1 <= P < L <= cap, N <= 16, N * Hq / Hkv <= 128. */
size_t omchat_op_attn_shared_ws(int G, int N, int Hq, int Hkv, int P, int L);
int omchat_op_attn_shared(int dtype, const void* q, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap, int P, int L,
                          float scale, void* ws, size_t ws_bytes, void* stream);
/* the same over rows of different lengths: kv_len device int32 [G*N], row r holds kv_len[r] keys (P < kv_len[r] <= L) and its query sits at
 * position kv_len[r] - 1; L only sizes the grid and the workspace.  A suffix tile beyond a row's length leaves the neutral partial.  With
 * every kv_len[r] == L it gives the bits of omchat_op_attn_shared. */
int omchat_op_attn_shared_lens(int dtype, const void* q, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap, int P, int L,
                               const int* kv_len, float scale, void* ws, size_t ws_bytes, void* stream);
/* Suffix-pass attention of omchat_prefill_suffixes: N rows of S query tokens each, q / out [N,S,Hq,128] (q already
 * rotated), k / v [N rows,Hkv,cap,128] complete; lengths host int32 [N], 1 .. S: the valid tokens of row j.  Query (j, t) sees the keys
 * [0, P) of row 0 and the keys [P, P + t] of row j.  Only out rows t < lengths[j] are defined by the contract (the others are computed from
 * the row's valid keys).  Never read: row 0's slots >= P through the prefix, slots < P of rows j > 0, slots >= P + lengths[j] of any row.
 * kv_len_dev: N ints of device memory that receive P + lengths[j] (one synchronising copy); lengths == NULL: kv_len_dev already holds
 * them -- the lengths come from the device, nothing synchronises, and a value outside [P + 1, P + S] reads no slot beyond P + S (a row
 * without own keys gets the prompt's keys only).  ws of omchat_op_attn_suffix_ws(N, S, Hq, Hkv, P) bytes.  One attention launch and one
 * merge whatever N is.  P >= 1, P + S <= cap, Hq / Hkv <= 8, N * S <= 65535. */
size_t omchat_op_attn_suffix_ws(int N, int S, int Hq, int Hkv, int P);
int omchat_op_attn_suffix(int dtype, const void* q, const void* k, const void* v, void* out, int N, int S, int Hq, int Hkv, int cap, int P,
                          const int32_t* lengths, int* kv_len_dev, float scale, void* ws, size_t ws_bytes, void* stream);
/* the same with the RoPE + append fused in, as the verify step runs it: qkv [T][(Hq + 2 Hkv) * 128] raw projections (not modified);
 * q / k rotated at positions L .. L + T - 1 (table of omchat_op_rope_kv), k / v appended to rows L .. L + T - 1 of the cache
 * (the bytes omchat_op_rope_kv writes).  Synchronises. */
int omchat_op_attn_verify_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int T, int Hq, int Hkv, int cap,
                                 int L, float scale, void* ws, size_t ws_bytes, void* stream);
/* test hook (tests/test_gpu_attn_block_rows.py): omchat_op_attn_shared[_lens] with the RoPE + append fused in, as omchat_decode_step runs it over
 * a shared-prompt group: qkv [G*N][(Hq + 2 Hkv) * 128] raw projections (not modified); row r holds kv_len[r] keys counting the new one (device
 * int32 [G*N], or NULL: L for every row); q is rotated at kv_len[r] - 1, the rotated k and the raw v go to that slot of row r's own cache (the
 * bytes omchat_op_rope_kv_pos writes with slot = position).  No other cache byte is written.  Synchronises. */
int omchat_op_attn_shared_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap,
                                 int P, int L, const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream);
/* test hook: the plan of the split-KV block attention on the current device.  mode: 0 verify (S = T, L), 1 extend (S = Sq, L), 2 shared
 * (G, N, P, L), 3 suffix (N, S, P); the integers a mode does not name are ignored.  out[4] (host) = {tpw: 64-key tiles per split (shared / suffix:
 * per prefix split), nsp: such splits, nss: suffix splits per row, tps: tiles per suffix split}.  Pure: launches nothing. */
int omchat_op_attn_block_plan(int mode, int G, int N, int S, int Hq, int Hkv, int P, int L, int* out);
/* the same over an e4m3 KV cache (omchat_enable_fp8_kv; BASELINE configs[4]): k8 / v8 [b,Hkv,cap,128] OCP e4m3 bytes, ks / vs [b,Hkv,cap] fp32, one
 * scale per cached row (as omchat_op_rope_kv_q8 writes them): score = (q . k8) * ks in fp32, the value scale folded into the probabilities (f16:
 * divided by a power of two per 64-key tile first, so that the folded factor stays in f16's normal range for value rows of any finite size) */
int omchat_op_attn_decode_kv8(int dtype, const void* q, const void* k8, const void* v8, const float* ks, const float* vs, void* out, int b,
                              int Hq, int Hkv, int cap, int L, const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream);
/* test hooks (tests/test_gpu_kv8_attn.py).
 * omchat_op_attn_decode_kv8_masked: omchat_op_attn_decode_kv8 over a padded batch: every row holds L keys, key j of row i is visible iff
 * key_mask[i][j] != 0 (device bytes [b][mask_sb], mask_sb % 64 == 0, mask_sb >= L).
 * omchat_op_attn_merge: the split-KV merge every attention launch ends in, alone, over given partials ws [rows][q_heads][nsplit][132] floats (O at
 * 0..127, the split's score maximum at 128, its exponential sum at 129): row r merges its first min(nsplit, ceil(kv_len[r] / split_keys)) partials
 * (kv_len NULL: L for every row) with weights 2^((m_s - max m) * scale * log2(e)); out [rows][q_heads][128].  Tuning keys 19 / 21 pick the kernel.
 * omchat_op_kv_quant: rows [lo, min(lo + max_rows, len[i])) of k16 / v16 [b,Hkv,cap,128] quantised into k8 / v8 / ks / vs (s = absmax / 448, 1 for a
 * zero row; bytes = e4m3_rne(x / s)); lo = pos_lo[i] (device int32 [b]) or pos0 (pos_lo NULL); len device int32 [b] or NULL (no upper bound). */
int omchat_op_attn_decode_kv8_masked(int dtype, const void* q, const void* k8, const void* v8, const float* ks, const float* vs, void* out, int b,
                                     int Hq, int Hkv, int cap, int L, const unsigned char* key_mask, int64_t mask_sb, float scale, void* ws,
                                     size_t ws_bytes, void* stream);
int omchat_op_attn_merge(int dtype, const float* ws, int nsplit, int q_heads, int rows, const int32_t* kv_len, int L, float scale, void* out,
                         int split_keys, void* stream);
int omchat_op_kv_quant(int dtype, const void* k16, const void* v16, void* k8, void* v8, float* ks, float* vs, int b, int Hkv, int cap,
                       const int32_t* pos_lo, int pos0, const int32_t* len, int max_rows, void* stream);
/* one decode step's attention over the e4m3 cache INCLUDING the new token's RoPE + append + quantisation, as the decoder layer issues it: qkv
 * [b][(Hq + 2 Hkv) * 128] raw projections; sequence i holds kv_len[i] keys counting the new one (NULL: L), whose rows go to position kv_len[i] - 1
 * of k8 / v8 / ks / vs and of the 16-bit caches k16 / v16 [b,Hkv,cap,128]; pos = kv_len - 1 (device, NULL with kv_len).  Launches long enough for
 * the walking form (tuning key 47) do all of it in the attention launch (key 48; omchat_op_rope_kv_q8's bytes), the others run that launch in front */
int omchat_op_attn_decode_kv8_append(int dtype, void* qkv, float theta, void* k8, void* v8, float* ks, float* vs, void* k16, void* v16, void* out,
                                     int b, int Hq, int Hkv, int cap, int L, const int32_t* kv_len, const int32_t* pos, float scale, void* ws,
                                     size_t ws_bytes, void* stream);
/* qkv [rows, (Hq+2Hkv)*128]; rows = b*S; positions pos0 + s; caches [b,Hkv,cap,128]; theta: rope base */
int omchat_op_rope_kv(int dtype, void* qkv, int b, int S, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache,
                      int cap, void* stream);
/* the same with the appended rows ALSO quantised into an e4m3 KV cache (k8 / v8 [b, Hkv, cap, 128] bytes, ks / vs [b, Hkv, cap] fp32: per row
 * s = absmax / 448 (1 for a zero row), bytes = e4m3_rne(x / s) of the 16-bit values stored in kcache / vcache) -- the decode step of the fp8
 * KV cache mode (BASELINE configs[4]) */
int omchat_op_rope_kv_q8(int dtype, void* qkv, int b, int S, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache, int cap,
                         void* k8, void* v8, float* ks, float* vs, void* stream);
int omchat_op_argmax(const float* logits, int b, int V, int32_t* out, void* stream);
/* test hooks of the row / glue kernels (tests/test_gpu_glue_ops.py): the launchers the model loops call, with the arguments the entry points above
 * do not expose.
 * omchat_op_attn_prefill_left: omchat_op_attn_prefill of a LEFT-padded batch -- kv_start device int32 [b], keys j < kv_start[i] of sequence i are
 * masked; fill_uniform != 0 then writes the uniform average of all Skv value rows to the query rows i < kv_start (what omchat_prefill_left does). */
int omchat_op_attn_prefill_left(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv, int Hq, int Hkv,
                                const int32_t* kv_len, const int32_t* kv_start, int causal, int q_pos0, float scale, int fill_uniform, void* stream);
/* test hook: omchat_op_rope_kv with per-row positions (pos device int32 [b * S] or NULL -> pos0 + s) and the cache slot slot0 + s instead of the
 * position (slot0 = -1: the position itself); the cos / sin table holds max_pos positions.  A position >= max_pos or a slot >= cap is refused
 * before anything is launched.  Synchronises. */
int omchat_op_rope_kv_pos(int dtype, void* qkv, int b, int S, int Hq, int Hkv, const int32_t* pos, int pos0, int slot0, int max_pos, float theta,
                          void* kcache, void* vcache, int cap, void* stream);
/* test hook (tests/test_gpu_decode_append.py): one decode step's attention over the 16-bit cache INCLUDING the new token's RoPE + append, as the
 * decoder layer issues it.  qkv [b][(Hq + 2 Hkv) * 128] raw projections (not modified); sequence i holds kv_len[i] keys counting the new one
 * (NULL: L); the rotated k and v go to slot kv_len[i] - 1 of k / v [b,Hkv,cap,128] (the bytes omchat_op_rope_kv writes), and that slot is the RoPE
 * position.  key_mask (device bytes [b][mask_sb], mask_sb % 64 == 0, kv_len NULL): key j of row i is visible iff key_mask[i][j] != 0, the RoPE
 * position is pos[i] (device int32 [b]) and the slot L - 1 for every row.  pack_nb != 0: out in the packed x layout.  NULL pointers, L < 1,
 * L > cap, key_mask without pos or with kv_len are refused before anything is launched.  Synchronises. */
int omchat_op_attn_decode_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int b, int Hq, int Hkv, int cap, int L,
                                 const int32_t* kv_len, const int32_t* pos, const unsigned char* key_mask, int64_t mask_sb, int pack_nb,
                                 float scale, void* ws, size_t ws_bytes, void* stream);
/* test hook: omchat_op_argmax over rows of stride ld >= V; adv_pos / adv_len device int32 [b] or NULL: each advanced by one per row */
int omchat_op_argmax_ld(const float* logits, int ld, int b, int V, int32_t* out, int32_t* adv_pos, int32_t* adv_len, void* stream);
/* test hook: pixels [B,3,HW,HW] -> cols [B * (HW / patch)^2, Kpad], columns (channel, ky, kx), zero beyond 3 * patch^2 */
int omchat_op_im2col(int dtype, const void* pixels, void* cols, int B, int HW, int patch, int Kpad, void* stream);
/* test hook: x [B, np + 1, C]: x[b, 0] = cls + pos[0], x[b, 1 + p] = pe[b * np + p] + pos[1 + p] (fp32 sum, one rounding) */
int omchat_op_vit_assemble(int dtype, const void* pe, const void* cls, const void* pos, void* x, int B, int np, int C, void* stream);
/* test hook: out[r] = table[idx[r]] (idx >= 0) | feats[-1 - idx[r]] (idx < 0) | zeros (idx == INT_MIN); idx device int32 [rows] */
int omchat_op_gather_rows(int dtype, const int32_t* idx, const void* table, const void* feats, void* out, int rows, int H, void* stream);
/* test hook: dst[r] = src[(r / group) * (group + skip) + skip + r % group], rows of width H with strides src_ld / dst_ld (elements) */
int omchat_op_copy_rows(int dtype, const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int rows, int H, int group, int skip, void* stream);
/* test hook: out [M, N] = epi(sum [M, N] fp32, bias, ls, resid) with the rounding points of omchat_op_gemm's epilogues EPI_NONE / EPI_RESID / EPI_LS_RESID */
int omchat_op_tp_finish(int dtype, const float* sum, const void* bias, const void* ls, const void* resid, void* out, int M, int N, int epi, void* stream);
/* test hook: x = T(x + y) in place, then xn = RMSNorm(x) * w (b == NULL), LayerNorm(x) * w + b, or nothing (w == NULL) */
int omchat_op_resid16_norm(int dtype, void* x, int ldx, const void* y, int ldy, const void* w, const void* b, void* xn, int ldn, int rows, int H,
                           float eps, void* stream);
/* test hook: dst fp32 [n] = src (dtype) [n] */
int omchat_op_cast_f32(int dtype, const void* src, float* dst, int64_t n, void* stream);
/* test hooks: omchat_op_rmsnorm / omchat_op_layernorm with row strides ldx / ldy >= H; pack_nb != 0 writes y in the packed x layout */
int omchat_op_rmsnorm_ld(int dtype, const void* x, int ldx, const void* w, void* y, int ldy, int rows, int H, float eps, int pack_nb, void* stream);
int omchat_op_layernorm_ld(int dtype, const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int rows, int H, float eps, void* stream);
/* context-free ban pass of omchat_set_constraints (test hook): histories host int32, the rows one after another (hist_len host int32 [b]; prompt_len
 * host int32 [b] = how many of them are the prompt); V ids of the vocabulary slice of `rank` out of V_total; fed_last != 0 passes each row's last
 * id as the token a decode step is fed instead of as stored history (the same set either way).  ban_out device uint32 [b][(V + 31) / 32]: bit i
 * of a row = local id i is banned.  Synchronises. */
int omchat_op_constrain(const int32_t* hist_ids, const int32_t* hist_len, const int32_t* prompt_len, int b, int V, int V_total, int rank, int fed_last,
                        int no_repeat_ngram_size, int min_new_tokens, int min_length, const int32_t* eos_ids, int n_eos, const int32_t* suppress_ids,
                        int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress, const int32_t* bad_word_ids,
                        const int32_t* bad_word_offsets, int n_bad_words, uint32_t* ban_out, void* stream);
/* context-free mark + apply passes of omchat_fsm_begin (test hook): a table as omchat_fsm_load takes it (validated the same way), states host
 * int32 [b] (OMCHAT_FSM_DEAD allowed), fed host int32 [b] = the global ids a decode step is fed, or NULL (no advance); logits device fp32
 * [b][V] = the vocabulary slice of `rank` out of V_total (left as they are).  out device fp32 [b][V] = the masked copy, new_states host
 * int32 [b] = the rows' states after the advance.  Synchronises. */
int omchat_op_fsm(int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, const int32_t* states, const int32_t* fed, int b, int V,
                  int V_total, int rank, const float* logits, float* out, int32_t* new_states, void* stream);

/* context-free guidance stage of omchat_set_guidance (test hook): logits device fp32 [2b][ld], rows [0, b) conditional, rows [b, 2b) their
 * twins, V <= ld ids per row (any V; 16-byte accesses when ld % 4 == 0 and the base is aligned, scalar ones otherwise); out device fp32
 * [b][ld_out], ld_out >= V; ws device memory of omchat_op_guidance_ws(b, V) bytes, 8-byte aligned.  Enqueues two launches, does not
 * synchronise. */
size_t omchat_op_guidance_ws(int b, int V);
int omchat_op_guidance(const float* logits, int ld, int b, int V, float scale, void* ws, float* out, int ld_out, void* stream);

/* context-free launches of contrastive search (test hooks; the launchers omchat_contrastive_step calls).  dtype: OMCHAT_DTYPE of the 16-bit
 * rows.  None synchronises.
 * plan: the penalty launch's cut of L history rows on this device: chunk c covers rows [c * rows_per_chunk, min(L, (c + 1) * rows_per_chunk)).
 * penalty: hist device [L][H], inv device fp32 [L] (with compute_norms != 0 it is written first, by the launch the prefill uses), cand
 *   device k rows, row-major (cand_nb = 0) or in the packed x layout with cand_nb blocks of 16 rows; part device fp32 [chunks][16] receives
 *   the partial maxima, cand_inv device fp32 [16] the candidates' inverse norms.  H % 32 == 0.
 * topk: logits device fp32 rows of stride ld, row *row_sel (device int32; NULL = row 0), V <= ld ids (columns at or beyond V are never
 *   read); ids device int32 [k], probs device fp32 [k]; ws device memory of omchat_op_contrastive_topk_ws(V) bytes, 8-byte aligned.
 * select: folds part [chunks][16], scores, picks and commits: out device int32 [OMCHAT_CS_REC_WORDS] the record; hist / inv (or NULL, NULL):
 *   the picked row of cand and cand_inv[pick] are appended at row n_hist; parents device int32 [k], sel / token / done_word device int32
 *   (each may be NULL). */
int omchat_op_contrastive_plan(int L, int* chunks, int* rows_per_chunk);
int omchat_op_contrastive_penalty(int dtype, void* hist, float* inv, int compute_norms, int L, int H, const void* cand, int cand_nb, int k,
                                  float* part, float* cand_inv, void* stream);
size_t omchat_op_contrastive_topk_ws(int V);
int omchat_op_contrastive_topk(const float* logits, int ld, const int32_t* row_sel, int V, int k, int32_t* ids, float* probs, void* ws,
                               void* stream);
int omchat_op_contrastive_select(int dtype, const float* part, int chunks, int k, double alpha, const int32_t* ids, const float* probs,
                                 const float* cand_inv, const void* cand, int cand_nb, int H, void* hist, float* inv, int n_hist,
                                 const int32_t* eos_ids, int n_eos, int last, int32_t* rec, int32_t* parents, int32_t* sel, int32_t* token,
                                 int32_t* done_word, void* stream);

/* context-free stage of omchat_set_dola (test hook): logits device fp32 [(k + 1) b][ld] in the row order given there, V <= ld ids per row (any
 * V; 16-byte accesses when ld % 4 == 0 and the base is aligned, scalar ones otherwise); out device fp32 [b][ld_out], ld_out >= V; picked
 * device int32 [b] (or NULL): the chosen candidate's POSITION 0..k-1; ws device memory of ws_bytes >= omchat_op_dola_ws(b, k, V) bytes,
 * 8-byte aligned.  Enqueues three launches (two at k == 1), does not synchronise. */
size_t omchat_op_dola_ws(int b, int k, int V);
int omchat_op_dola(const float* logits, int ld, int V, int b, int k, float relative_top, float* out, int ld_out, int32_t* picked, void* ws,
                   size_t ws_bytes, void* stream);

/* context-free sampler over logits fp32 [b, V] with the parameters of omchat_set_sampling; every row at step `step`.  thr_out (device uint32 [b]
 * or NULL, test hook): the kept set's threshold -- the order-preserving key of the smallest kept processed logit (0 = everything kept). */
int omchat_op_sample(const float* logits, int b, int V, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                     const int32_t* seen_ids, const int32_t* n_seen_per_row, int step, int32_t* out, uint32_t* thr_out, void* stream);
/* omchat_op_sample with the four filters of omchat_set_sampling_filters (same "off" values).  thr_lo / thr_hi (device uint32 [b] or NULL, test
 * hooks): both ends of the kept key interval; thr_lo as omchat_op_sample's thr_out, thr_hi = 0xFFFFFFFF when the row's top token is kept. */
int omchat_op_sample_filtered(const float* logits, int b, int V, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                              double min_p, double typical_p, double epsilon_cutoff, double eta_cutoff, const int32_t* seen_ids,
                              const int32_t* n_seen_per_row, int step, int32_t* out, uint32_t* thr_lo, uint32_t* thr_hi, void* stream);
/* context-free verify form of the sampler (omchat_decode_verify with OMCHAT_VERIFY_SAMPLE; test hook): logits device fp32 [T][ld] (ld >= V)
 * of the vocabulary slice of `rank` (V ids out of V_total; rank = 0, V_total = V for the whole vocabulary), tokens device int32 [T] = the last
 * emitted id and the T - 1 drafts, 2 <= T <= 16.  Row j is drawn with row 0's key at step base_step + j; with rep_penalty != 1 it sees
 * seen_ids (host int32 [n_seen], GLOBAL ids of sequence 0's seen set) plus tokens[1..j]; ids outside [0, V_total) or the slice are ignored.
 * Parameters and filters as omchat_op_sample_filtered.  out device int32 [T] (global ids; the slice's winner, no exchange), thr_lo / thr_hi
 * as there.  Synchronises. */
int omchat_op_sample_verify(const float* logits, int T, int V, int ld, const int32_t* tokens, uint64_t seed, int base_step, float temperature,
                            int top_k, double top_p, float rep_penalty, double min_p, double typical_p, double epsilon_cutoff, double eta_cutoff,
                            const int32_t* seen_ids, int n_seen, int rank, int V_total, int32_t* out, uint32_t* thr_lo, uint32_t* thr_hi,
                            void* stream);
/* context-free log-probability stage of omchat_set_logprobs (test hook): logits device fp32 [b][ld] (ld >= V), ids host int32 [b] (the picked
 * ids), ban device uint32 [b][(V + 31) / 32] or NULL (set bit = processed value -inf), seen ids as omchat_op_sample takes them (read when
 * rep_penalty != 1), newly_seen host int32 [b] or NULL (!= 0: the pick set its id's seen bit, so the id counts as unseen), thr device uint32 [b]
 * or NULL (omchat_op_sample's thr_out; 0 = everything kept).  raw_out / processed_out device fp32 [b].  Synchronises. */
int omchat_op_token_logprob(const float* logits, int b, int V, int ld, const int32_t* ids, const uint32_t* ban, float temperature,
                            float rep_penalty, const int32_t* seen_ids, const int32_t* n_seen_per_row, const int32_t* newly_seen,
                            const uint32_t* thr, float* raw_out, float* processed_out, void* stream);
/* logprob[m] = log_softmax(A[m] W^T)[labels[m]] and lse[m] = logsumexp(A[m] W^T) over N columns WITHOUT storing the [M, N] products (DESIGN.md
 * section 18): the MFMA GEMM with the EPI_LSE epilogue -- fp32 accumulators used raw, per-row (max, sum exp) pairs per 64-column slot, the
 * label's accumulator -- then one wave per row folds the slots in a fixed order.  Contract of omchat_op_gemm: K % 64 == 0, N % 4 == 0,
 * lda / ldw % 8 == 0, A / W 16-byte aligned.  labels device int32 [M]: -100 (logprob 0) or an id in [0, N); anything else is an error,
 * checked on the host before the launch.  logprob device fp32 [M]; lse device fp32 [M] or NULL; ws: omchat_op_lse_label_ws(M, N) bytes,
 * 16-byte aligned.  Two runs give the same bits.  Synchronises (the label check). */
size_t omchat_op_lse_label_ws(int M, int N);
int omchat_op_lse_label(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int32_t* labels, float* logprob,
                        float* lse, void* ws, size_t ws_bytes, void* stream);
/* omchat_op_token_logprob over a kept interval: thr_lo / thr_hi device uint32 [b] or NULL (omchat_op_sample_filtered's; NULL = no bound on
 * that side).  An id outside the interval records -inf as its processed value. */
int omchat_op_token_logprob_interval(const float* logits, int b, int V, int ld, const int32_t* ids, const uint32_t* ban, float temperature,
                                     float rep_penalty, const int32_t* seen_ids, const int32_t* n_seen_per_row, const int32_t* newly_seen,
                                     const uint32_t* thr_lo, const uint32_t* thr_hi, float* raw_out, float* processed_out, void* stream);
/* context-free extras of omchat_set_logprobs_ex (test hook, TP = 1): logits device fp32 [b][ld] (ld >= V); score_ids host int32 [n_score]
 * or NULL; outputs device: top_vals fp32 [b][top_n], top_ids int32 [b][top_n], scored fp32 [b][n_score] (NULL where its count is 0).  The
 * contract, the caps and the tie rule (value descending, -0 == +0, then id ascending) are omchat_set_logprobs_ex's.  Synchronises. */
int omchat_op_top_logprobs(const float* logits, int b, int V, int ld, int top_n, const int32_t* score_ids, int n_score, float* top_vals,
                           int32_t* top_ids, float* scored, void* stream);
/* context-free beam step (test hook of omchat_beam_step's selection, TP = 1): logits fp32 [rows, V] (rows = b at t = 0, else b*N), step t
 * of max_new; state: device int32 [omchat_beam_state_words(b, N, max_new)] carried from call to call (initialised by the t = 0 call).
 * Outputs device int32: tokens [b*N], parents [b*N] (rows; a row's own index at t = 0 and for frozen prompts), done_word [1]. */
size_t omchat_beam_state_words(int b, int N, int max_new);
int omchat_op_beam_select(const float* logits, int rows, int V, int b, int N, int t, int max_new, float length_penalty, int early_stopping,
                          const int32_t* eos_ids, int n_eos, int32_t* state, int32_t* tokens, int32_t* parents, int32_t* done_word, void* stream);
/* the same step on processed scores (test hook of the selection behind omchat_beam_processors): omchat_op_beam_select's arguments, then the
 * rows' histories as omchat_op_constrain takes them (hist_ids host int32, the rows one after another, hist_len / prompt_len host int32
 * [rows]), the repetition penalty and the lists.  A penalty of 1 with nothing to ban runs omchat_op_beam_select itself.  Synchronises. */
int omchat_op_beam_select_processed(const float* logits, int rows, int V, int b, int N, int t, int max_new, float length_penalty,
                                    int early_stopping, const int32_t* eos_ids, int n_eos, int32_t* state, int32_t* tokens, int32_t* parents,
                                    int32_t* done_word, const int32_t* hist_ids, const int32_t* hist_len, const int32_t* prompt_len,
                                    float rep_penalty, int no_repeat_ngram_size, int min_new_tokens, int min_length, const int32_t* suppress_ids,
                                    int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress, const int32_t* bad_word_ids,
                                    const int32_t* bad_word_offsets, int n_bad_words, void* stream);
/* per-path histories (test hook of the beam step's history move; all pointers device): dst[r][P, P + g) = src[parents[r]][P, P + g),
 * dst[r][P + g] = tokens[r], len[r] = P + g + 1 for the rows [rows][ld] (N rows per prompt; a parent outside the row's prompt counts as the
 * row itself; P + g + 1 <= ld); bitmap_words words at bitmaps are zeroed.  No host sync. */
int omchat_op_beam_hist_move(const int32_t* src, int32_t* dst, int rows, int N, int ld, int P, int g, const int32_t* parents,
                             const int32_t* tokens, int32_t* len, uint32_t* bitmaps, size_t bitmap_words, void* stream);
/* KV-cache rows between sequences (test hook of the beam step's gather): k / v 16-bit [layers][rows_cap][kvh][max_seq][128]; k8 / v8 (e4m3
 * bytes, same layout) and ks / vs (fp32 [layers][rows_cap][kvh][max_seq]) or NULL.  Row r in [row0, row0 + nrows) becomes a copy of
 * parents[r] (device int32, values in [row0, row0 + nrows)) over slots [lo, hi), for any parent map (cycles, repeats); parents == NULL:
 * of row fork_src.  Synchronises. */
int omchat_op_kv_gather(int dtype, void* k, void* v, void* k8, void* v8, float* ks, float* vs, int layers, int rows_cap, int kvh, int max_seq,
                        const int32_t* parents, int row0, int nrows, int fork_src, int lo, int hi, void* stream);
int omchat_op_fill_uniform(int dtype, void* dst, int64_t n, uint64_t key, float scale, float offset, void* stream);

/* ---- image front-end: process_anyres_image (omchat/mm_utils.py:119-158) + CLIPImageProcessor ---- */
/* (internVIT_encoder.py:25-29) on the device, bit-identical to the reference's PIL/numpy result.
 * plan (host only): select_best_resolution (mm_utils.py:12-39) over `pinpoints` [n_pin][2] = (w, h); n_tiles = 1 thumbnail
 * + the tiles of the best resolution.  anyres: `rgb` uint8 [H][W][3] (host, or device when rgb_on_device) ->
 * pixels_out device [n_tiles][3][tile][tile] in `dtype` (OMCHAT_F16 / BF16 / F32): tile 0 = Image.resize((tile, tile)),
 * then the row-major tiles of resize_and_pad_image (mm_utils.py:42-74); every value = (u/255 - mean)/std with
 * transformers' rounding order.  Blocks until the staging copies are done (the kernels stay ordered on `stream`). */
int omchat_preproc_plan(int W, int H, const int* pinpoints, int n_pin, int tile, int* best_w, int* best_h, int* n_tiles);
int omchat_preproc_anyres(int dtype, const void* rgb, int rgb_on_device, int W, int H, int best_w, int best_h, int tile,
                          const float mean[3], const float std_[3], void* pixels_out, void* stream);
/* dynamic_preprocess + process_dynamic_image (mm_utils.py:276-323, the OmChat-2.1 / InternViT-300M tiling): plain resize to
 * (grid_w*tile, grid_h*tile) -- aspect not preserved --, row-major tiles, thumbnail FIRST when `thumbnail` (the reference
 * adds it when the grid has more than one block); pixels_out [thumbnail + grid_w*grid_h][3][tile][tile].  The grid choice
 * (find_closest_aspect_ratio, :326-339) is host integer/float logic in omchat_amd/mm_utils.py. */
int omchat_preproc_dynamic(int dtype, const void* rgb, int rgb_on_device, int W, int H, int grid_w, int grid_h, int tile, int thumbnail,
                           const float mean[3], const float std_[3], void* pixels_out, void* stream);
/* host-only pieces exposed for the CPU parity tests: Pillow's fixed-point resampling taps (Resample.c precompute_coeffs +
 * normalize_coeffs_8bpc, BICUBIC): bounds [out][2] = (first source index, taps), kk [out][*ksize]; and the 3 x 256
 * rescale+normalize table */
int omchat_resample_coeffs(int in_size, int out_size, int* ksize, int* bounds, int* kk, int kk_cap);
int omchat_normalize_lut(const float mean[3], const float std_[3], float lut[768]);

/* ---- tensor-parallel bootstrap (RCCL over xGMI; one process per GPU) -------------------------------------------- */
int omchat_comm_unique_id(char id[128]);
int omchat_comm_init(const char id[128], int rank, int size, void** comm_out);
/* the collective of the tensor-parallel data path, callable on its own: in-place sum over the ranks of `comm` */
int omchat_comm_allreduce(void* comm, void* buf, size_t count, int dtype, void* stream);
void omchat_comm_destroy(void* comm);

int omchat_comm_count(void* comm, int* nranks);                  /* ncclCommCount: ranks of the communicator */

/* ---- peer all-reduce over IPC-mapped buffers (xGMI P2P), csrc/comm.hip ------------------------------------------ */
/* The decode-sized collective of SURVEY.md 8e: one-shot (every rank reads every rank's slot and sums in rank order: all ranks
 * get identical bits) up to `oneshot_max` bytes, two-shot (reduce-scatter + all-gather by peer reads) above it.  One process
 * per GPU: omchat_peer_create allocates the rank's shared buffer (capacity `cap_bytes` per message piece; longer messages are
 * cut into pieces) and returns its 64-byte hipIpcMemHandle_t; the caller ships the handles of all ranks (any bootstrap channel;
 * tp.py uses torch.distributed) and passes the `size` x 64-byte table to omchat_peer_connect.  omchat_peer_connect_local is the
 * same-process variant (rank contexts in threads: pointers instead of IPC handles). */
typedef struct omchat_peer omchat_peer;
int omchat_peer_create(int rank, int size, size_t cap_bytes, omchat_peer** out, char handle_out[64]);
int omchat_peer_connect(omchat_peer* p, const char* all_handles);
void* omchat_peer_base(omchat_peer* p);
int omchat_peer_connect_local(omchat_peer* p, void* const* bases);
/* fast != 0: drop the one-lane system-scope release / acquire fences around the flag barrier (payload stays sc0 sc1);
 * oneshot_max_bytes != 0: one-shot / two-shot switch point (default 256 KiB); max_blocks != 0: workgroups per call (default 64,
 * <= 128; every workgroup of a call must be resident on every rank at once, so rank contexts that SHARE a GPU keep it small) */
int omchat_peer_set_mode(omchat_peer* p, int fast, size_t oneshot_max_bytes, int max_blocks);
size_t omchat_peer_capacity(omchat_peer* p);
/* in-place sum over the ranks, `count` elements of OMCHAT_F16 / BF16 / F32; buf 16-byte aligned, byte count % 16 == 0 */
int omchat_peer_allreduce(omchat_peer* p, void* buf, size_t count, int dtype, void* stream);
/* the two halves of that all-reduce as collectives of their own (round 6, sequence-parallel norms): buf = [size][blk_count] elements (dtype as
 * above; block bytes a multiple of 16).  reduce_scatter: block `rank` of buf becomes the sum over the ranks of their block `rank` (rank order,
 * fp32, one rounding: the bits of omchat_peer_allreduce), the other blocks are left unchanged.  all_gather: block `rank` of every rank is copied into
 * block `rank` of every other rank's buf.  Same stream / ordering rules as omchat_peer_allreduce. */
int omchat_peer_reduce_scatter(omchat_peer* p, void* buf, size_t blk_count, int dtype, void* stream);
int omchat_peer_all_gather(omchat_peer* p, void* buf, size_t blk_count, int dtype, void* stream);
/* Tensor-parallel decode, the all-reduce fused with its consumer: part = this rank's fp32 split-K slices [ks][rows][H] of a row-parallel
 * projection (ks <= 8, rows <= 128, ks * rows * H * 4 <= capacity).  On return (stream order) x[rows, H] = T(x + T(sum over ranks and
 * slices)) on every rank and, when w != NULL, xn = T(w * T(x * rsqrt(mean(x^2) + eps))) (pack_nb != 0: in the packed x layout of the
 * batched GEMV).  Same bits as omchat_peer_allreduce(part) followed by the local residual + RMSNorm launch, one launch instead of two.
 * (reference: the residual adds and RMSNorms of transformers modeling_qwen2.py:283-296, 247-252) */
int omchat_peer_resid_rmsnorm(omchat_peer* p, int dtype, void* x, int ldx, const float* part, int ks, const void* w, void* xn, int ldn,
                              int rows, int H, float eps, int pack_nb, void* stream);
/* synchronises the device; *err_out = 1 when a barrier spin timed out (a peer died or never arrived) since the last call */
int omchat_peer_error(omchat_peer* p, int* err_out);
void omchat_peer_destroy(omchat_peer* p);
/* use `peer` for the tensor-parallel sums of `ctx`: messages <= max_bytes (0 = keep 256 KiB), every size when all_sizes != 0
 * or when the context has no RCCL communicator */
int omchat_ctx_set_peer(omchat_ctx* ctx, omchat_peer* peer, size_t max_bytes, int all_sizes);
int omchat_ctx_comm_stats(omchat_ctx* ctx, long* peer_calls, long* rccl_calls);
/* Sequence-parallel norms under tensor parallelism (round 6; default on, tuning key 45 = 0 restores the all-reduce form): a row-parallel
 * projection of the vision tower / the prefill ends in a reduce-scatter over row blocks (rank r receives the summed rows it owns: block r of
 * ceil(rows / tp_size) rows per chunk), the owner adds the residual and normalises ITS rows, an all-gather hands every rank the normalised
 * activation; the residual stream stays row-sharded between sub-blocks and is gathered once at the end.  Same link bytes as the all-reduce, the
 * replicated RMSNorm / LayerNorm work divided by tp_size.  RCCL: ncclReduceScatter / ncclAllGather in place; hook / peer transports emulate both
 * with all-reduces.  The counters say which form ran. */
int omchat_ctx_sp_stats(omchat_ctx* ctx, long* reduce_scatters, long* all_gathers);
/* in-place sum of a caller buffer over the context's tensor-parallel group (same transports as the model's own all-reduces); used for
 * the data-parallel vision tower: every rank encodes its share of the tiles into a zero-filled feature buffer and the sum gathers them */
int omchat_ctx_allreduce(omchat_ctx* ctx, void* buf, size_t count, int dtype, void* stream);

/* Test seam: replace the RCCL all-reduce of a tensor-parallel context by a caller-supplied function (sum over ranks,
 * in place, `count` elements of dtype OMCHAT_F16/BF16/F32, ordered on `stream`).  Lets the whole TP dataflow be
 * verified with several rank contexts on ONE GPU; production contexts never set it. */
typedef int (*omchat_allreduce_fn)(void* user, void* buf, size_t count, int dtype, void* stream);
int omchat_set_allreduce_hook(omchat_ctx* ctx, omchat_allreduce_fn fn, void* user);
/* Measurement seam (bench.py --shard-of N): an omchat_allreduce_fn that does nothing.  A context created with tp_size = N and this
 * hook runs ONE rank's share of the tensor-parallel work (its GEMM / GEMV / attention shard shapes and launch sequence) on a single
 * GPU with the exchanges removed: kernel time per rank without an N-GPU node.  The results are NOT the model's outputs. */
int omchat_allreduce_noop(void* user, void* buf, size_t count, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
