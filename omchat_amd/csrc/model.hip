// Model-level loops of the OmChat hot path on one GPU (one tensor-parallel rank): context, weight routing, workspaces,
// KV cache, and the kernel sequences for the vision tower, projector, prefill and decode.  Host C++; every FLOP runs
// in the HIP kernels of this directory.
#include "ctx.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

static thread_local std::string g_err;
void omchat_set_error(const std::string& s) { g_err = s; }
extern "C" const char* omchat_last_error(void) { return g_err.c_str(); }
extern "C" const char* omchat_version(void) { return "omchat_hip 0.1 (gfx950)"; }

namespace {

__global__ void cast_from_f32_f16(const float* s, f16* d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (f16)s[i];
}
__global__ void cast_from_f32_bf16(const float* s, bf16* d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (bf16)s[i];
}
__global__ void add_positions_kernel(int* pos, int b, int d) {
  const int i = threadIdx.x;
  if (i < b) pos[i] += d;
}
__global__ void advance_lens_kernel(int* pos, int* len, int b) {
  const int i = threadIdx.x;
  if (i < b) { pos[i] += 1; len[i] += 1; }
}
// prompt-lookup verify (omchat_decode_verify): n = leading drafts equal to the picks; sequence 0 keeps L + 1 + n slots (all T with keep_all)
__global__ void verify_accept_kernel(const int32_t* tokens, const int32_t* picks, int T, int L, int keep_all, int* pos, int* len, int* n_out) {
  if (threadIdx.x != 0) return;
  int n = 0;
  while (n < T - 1 && tokens[n + 1] == picks[n]) ++n;
  const int kept = keep_all ? T : n + 1;
  pos[0] = L + kept; len[0] = L + kept + 1;
  n_out[0] = n;
}
// the sampled form (OMCHAT_VERIFY_SAMPLE): the same n, and the n + 1 emitted picks are committed to sequence 0's sampler state as n + 1 plain
// steps would have: seen bits in pick order (this rank's shard; bm = nullptr without the penalty), each newly set bit recorded in vlast
// [16] for omchat_kv_rewind, the step counter advanced by n + 1.  smp_last[0] no longer names the last pick's bit.
__global__ void verify_accept_sample_kernel(const int32_t* tokens, const int32_t* picks, int T, int L, int* pos, int* len, int* n_out,
                                            uint32_t* bm, int gbase, int V, int* vlast, int* last, int* step) {
  if (threadIdx.x != 0) return;
  int n = 0;
  while (n < T - 1 && tokens[n + 1] == picks[n]) ++n;
  for (int i = 0; i < VERIFY_MAX_T; ++i) {
    int set = -1;
    if (bm && i <= n) {
      const int id = picks[i];
      const int li = id >= gbase ? id - gbase : -1;
      if (id >= 0 && li >= 0 && li < V) {
        const uint32_t bit = 1u << (li & 31);
        if (!(bm[li >> 5] & bit)) { bm[li >> 5] |= bit; set = li; }
      }
    }
    vlast[i] = set;
  }
  last[0] = -1;
  step[0] += n + 1;
  pos[0] = L + n + 1; len[0] = L + n + 2;
  n_out[0] = n;
}
__global__ void last_row_index_kernel(const int* len, int S, int b, int* idx, int keep) {      // (keep: cached rows in front of the S prefilled ones)
  const int i = threadIdx.x;
  if (i < b) idx[i] = i * S + len[i] - keep - 1;
}

}  // namespace

#if !OMCHAT_EXPERIMENTS
// product build: the round-4 one-launch experiments are not compiled in (kernels.h); their entry points refuse
size_t fused_decode_ws_bytes(int) { return 0; }
bool attn_oproj_fused_ok(const AttnDecodeArgs&, int, int) { return false; }
int launch_attn_oproj_fused(int, const AttnDecodeArgs&, const FusedDecodeArgs&, hipStream_t) { omchat_set_error("fused decode launch: build with -DOMCHAT_EXPERIMENTS=1"); return 1; }
size_t decode_layer_ws_bytes(int, int, int, int, int) { return 0; }
bool decode_layer_ok(const DecodeLayerArgs&) { return false; }
int launch_decode_layer(int, const DecodeLayerArgs&, hipStream_t) { omchat_set_error("one-launch decode layer: build with -DOMCHAT_EXPERIMENTS=1"); return 1; }
#endif
extern "C" int omchat_has_experiments(void) { return OMCHAT_EXPERIMENTS; }
int g_shard_as_tp1 = 0;          // omchat_op_set_tuning key 35 (experiments build): see decode_body
void model_set_shard_as_tp1(int v) { g_shard_as_tp1 = v; }
int g_decode_layer = 0;          // omchat_op_set_tuning key 23: 1 = batch-1 decode on one GPU runs each decoder layer as ONE launch (decode_layer.hip); 0 = six launches (same bits)
void model_set_decode_layer(int v) { g_decode_layer = v; }
int g_fuse_attn_oproj = 0;      // omchat_op_set_tuning key 22: 1 = batch-1 decode on one GPU runs split-KV attention + merge + o_proj as ONE launch (fused_decode.hip); 0 = three launches (A/B, same bits)
void model_set_fuse_attn_oproj(int v) { g_fuse_attn_oproj = v; }
int g_ao_oproj = 0;            // omchat_op_set_tuning key 42 (experiments build, prototype): batch-1 o_proj launched out of order behind the split-KV merge (gemv_rows_wait_kernel)
void model_set_ao_oproj(int v) { g_ao_oproj = v; }
int g_fuse_peer_norm = 1;      // omchat_op_set_tuning key 9: 0 = tensor-parallel decode keeps the all-reduce and the residual + RMSNorm as two launches (A/B)
void model_set_fuse_peer_norm(int v) { g_fuse_peer_norm = v; }

namespace {

int add_route(omchat_ctx* ctx, const std::string& name, void** slot, int64_t rows, int64_t cols, float std_, float off,
              int kind = R_PLAIN, void* dst_override = nullptr, int64_t dst_ld = -1) {
  Route r;
  r.rows = rows; r.cols = cols; r.kind = kind; r.synth_std = std_; r.synth_off = off;
  if (dst_override) {
    r.dst = dst_override;
  } else {
    TRY(ctx->alloc(&r.dst, (size_t)rows * cols * 2));
    if (slot) *slot = r.dst;
  }
  r.dst_ld = dst_ld < 0 ? cols : dst_ld;
  ctx->routes[name] = r;
  return 0;
}

// the five projections a decode step streams, as W [N][K]: the only place their shapes are written
struct ProjShape { int N, K; };
ProjShape proj_shape(const omchat_ctx* ctx, int which) {
  const int H = ctx->c.t_hidden, It = ctx->c.t_mlp;
  switch (which) {
    case omchat_ctx::P_QKV: return {ctx->t_qkvdim, H};
    case omchat_ctx::P_O: return {H, ctx->t_qdim};
    case omchat_ctx::P_GU: return {2 * It, H};
    case omchat_ctx::P_DOWN: return {H, It};
    default: return {ctx->c.t_vocab, H};      // P_LM
  }
}
// entry j of a format's table (layers * 4 + 1 of them) is projection j % 4 of layer j / 4; the last one is the lm_head
ProjShape entry_shape(const omchat_ctx* ctx, size_t j) { return proj_shape(ctx, j == (size_t)ctx->c.t_layers * 4 ? omchat_ctx::P_LM : (int)(j % 4)); }

int build(omchat_ctx* ctx) {
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, I = c.v_mlp;
  ctx->v_np = (c.v_image / c.v_patch) * (c.v_image / c.v_patch);
  ctx->v_ntok = ctx->v_np + 1;
  ctx->v_hd = c.v_head_dim ? c.v_head_dim : 128;
  ctx->v_Cq = c.v_heads * ctx->v_hd;
  const int K = 3 * c.v_patch * c.v_patch;
  ctx->v_kpad = cdiv(K, 64) * 64;
  const std::string TW = "model.vision_tower.vision_tower.";

  // ---- vision tower weights
  if (c.v_layers > 0) {
    TRY(add_route(ctx, TW + "embeddings.class_embedding", &ctx->v_cls, 1, C, 0.02f, 0.f));
    TRY(add_route(ctx, TW + "embeddings.position_embedding", &ctx->v_pos, ctx->v_ntok, C, 0.02f, 0.f));
    TRY(ctx->alloc(&ctx->v_wpatch, (size_t)C * ctx->v_kpad * 2));
    OM_HIP(hipMemset(ctx->v_wpatch, 0, (size_t)C * ctx->v_kpad * 2));
    TRY(add_route(ctx, TW + "embeddings.patch_embedding.weight", nullptr, C, K, 0.02f, 0.f, R_PATCH, ctx->v_wpatch, ctx->v_kpad));
    TRY(add_route(ctx, TW + "embeddings.patch_embedding.bias", &ctx->v_bpatch, 1, C, 0.02f, 0.f));
    ctx->vl.resize(c.v_layers);
    for (int j = 0; j < c.v_layers; ++j) {
      const std::string P = TW + "encoder.layers." + std::to_string(j) + ".";
      auto& L = ctx->vl[j];
      TRY(add_route(ctx, P + "ls1", &L.ls1, 1, C, 0.02f, 0.1f));
      TRY(add_route(ctx, P + "ls2", &L.ls2, 1, C, 0.02f, 0.1f));
      TRY(add_route(ctx, P + "norm1.weight", &L.n1, 1, C, 0.05f, 1.f));
      TRY(add_route(ctx, P + "norm2.weight", &L.n2, 1, C, 0.05f, 1.f));
      L.n1b = L.n2b = L.qn = L.kn = nullptr;
      if (c.v_norm_type == 1) {
        TRY(add_route(ctx, P + "norm1.bias", &L.n1b, 1, C, 0.02f, 0.f));
        TRY(add_route(ctx, P + "norm2.bias", &L.n2b, 1, C, 0.02f, 0.f));
      }
      TRY(add_route(ctx, P + "attn.qkv.weight", &L.wqkv, 3 * ctx->v_Cq, C, 0.02f, 0.f));
      if (!c.v_no_qk_norm) {
        TRY(add_route(ctx, P + "attn.q_norm.weight", &L.qn, 1, ctx->v_Cq, 0.05f, 1.f));
        TRY(add_route(ctx, P + "attn.k_norm.weight", &L.kn, 1, ctx->v_Cq, 0.05f, 1.f));
      }
      TRY(add_route(ctx, P + "attn.proj.weight", &L.wproj, C, ctx->v_Cq, 0.02f, 0.f));
      TRY(add_route(ctx, P + "attn.proj.bias", &L.bproj, 1, C, 0.02f, 0.f));
      TRY(add_route(ctx, P + "mlp.fc1.weight", &L.w1, I, C, 0.02f, 0.f));
      TRY(add_route(ctx, P + "mlp.fc1.bias", &L.b1, 1, I, 0.02f, 0.f));
      TRY(add_route(ctx, P + "mlp.fc2.weight", &L.w2, C, I, 0.02f, 0.f));
      TRY(add_route(ctx, P + "mlp.fc2.bias", &L.b2, 1, C, 0.02f, 0.f));
    }
    const int H = c.t_hidden;
    TRY(add_route(ctx, "model.mm_projector.0.weight", &ctx->p_w0, H, C, 0.02f, 0.f));
    TRY(add_route(ctx, "model.mm_projector.0.bias", &ctx->p_b0, 1, H, 0.02f, 0.f));
    TRY(add_route(ctx, "model.mm_projector.2.weight", &ctx->p_w2, H, H, 0.02f, 0.f));
    TRY(add_route(ctx, "model.mm_projector.2.bias", &ctx->p_b2, 1, H, 0.02f, 0.f));
  }

  // ---- decoder weights (q/k/v fused; gate/up interleaved in 16-row blocks for the SwiGLU epilogue)
  const int H = c.t_hidden, It = c.t_mlp;
  ctx->t_qdim = c.t_heads * 128; ctx->t_kvdim = c.t_kv_heads * 128; ctx->t_qkvdim = ctx->t_qdim + 2 * ctx->t_kvdim;
  if (c.t_layers > 0) {
    OM_CHECK(It % 16 == 0, "t_mlp must be a multiple of 16");
    TRY(add_route(ctx, "model.embed_tokens.weight", &ctx->t_embed, c.t_vocab_total, H, 0.02f, 0.f));
    TRY(add_route(ctx, "model.norm.weight", &ctx->t_norm, 1, H, 0.05f, 1.f));
    TRY(add_route(ctx, "lm_head.weight", &ctx->t_lm, c.t_vocab, H, 0.02f, 0.f));
    ctx->dl.resize(c.t_layers);
    for (int i = 0; i < c.t_layers; ++i) {
      const std::string P = "model.layers." + std::to_string(i) + ".";
      auto& L = ctx->dl[i];
      TRY(ctx->alloc(&L.wqkv, (size_t)ctx->t_qkvdim * H * 2));
      TRY(ctx->alloc(&L.bqkv, (size_t)ctx->t_qkvdim * 2));
      TRY(ctx->alloc(&L.wgu, (size_t)2 * It * H * 2));
      char* wq = (char*)L.wqkv; char* bq = (char*)L.bqkv;
      TRY(add_route(ctx, P + "self_attn.q_proj.weight", nullptr, ctx->t_qdim, H, 0.02f, 0.f, R_PLAIN, wq));
      TRY(add_route(ctx, P + "self_attn.k_proj.weight", nullptr, ctx->t_kvdim, H, 0.02f, 0.f, R_PLAIN, wq + (size_t)ctx->t_qdim * H * 2));
      TRY(add_route(ctx, P + "self_attn.v_proj.weight", nullptr, ctx->t_kvdim, H, 0.02f, 0.f, R_PLAIN, wq + (size_t)(ctx->t_qdim + ctx->t_kvdim) * H * 2));
      TRY(add_route(ctx, P + "self_attn.q_proj.bias", nullptr, 1, ctx->t_qdim, 0.02f, 0.f, R_PLAIN, bq));
      TRY(add_route(ctx, P + "self_attn.k_proj.bias", nullptr, 1, ctx->t_kvdim, 0.02f, 0.f, R_PLAIN, bq + (size_t)ctx->t_qdim * 2));
      TRY(add_route(ctx, P + "self_attn.v_proj.bias", nullptr, 1, ctx->t_kvdim, 0.02f, 0.f, R_PLAIN, bq + (size_t)(ctx->t_qdim + ctx->t_kvdim) * 2));
      TRY(add_route(ctx, P + "self_attn.o_proj.weight", &L.wo, H, ctx->t_qdim, 0.02f, 0.f));
      TRY(add_route(ctx, P + "mlp.gate_proj.weight", nullptr, It, H, 0.02f, 0.f, R_GATE, L.wgu));
      TRY(add_route(ctx, P + "mlp.up_proj.weight", nullptr, It, H, 0.02f, 0.f, R_UP, L.wgu));
      TRY(add_route(ctx, P + "mlp.down_proj.weight", &L.wd, H, It, 0.02f, 0.f));
      TRY(add_route(ctx, P + "input_layernorm.weight", &L.ln1, 1, H, 0.05f, 1.f));
      TRY(add_route(ctx, P + "post_attention_layernorm.weight", &L.ln2, 1, H, 0.05f, 1.f));
    }
    // the 16-bit entry of the weight-format table: a view of the above
    omchat_ctx::WTable& w16 = ctx->wt[OMCHAT_WFMT_16];
    for (auto& L : ctx->dl) for (void* w : {L.wqkv, L.wo, L.wgu, L.wd}) w16.e.push_back({w});
    w16.e.push_back({ctx->t_lm});
    for (size_t j = 0; j < w16.e.size(); ++j) w16.e[j].ldw = entry_shape(ctx, j).K;
    w16.state = omchat_ctx::W_BUILT;
    // RoPE table: Qwen2RotaryEmbedding (modeling_qwen2.py:64-102): inv_freq and angles in fp32, cos/sin fp32
    std::vector<float> tab((size_t)c.max_seq * 128);
    for (int i = 0; i < 64; ++i) {
      const float inv = (float)(1.0 / pow((double)c.rope_theta, (double)((float)(2 * i) / 128.0f)));
      for (int pos = 0; pos < c.max_seq; ++pos) {
        const float ang = (float)pos * inv;
        tab[((size_t)pos * 64 + i) * 2] = (float)cos((double)ang);
        tab[((size_t)pos * 64 + i) * 2 + 1] = (float)sin((double)ang);
      }
    }
    TRY(ctx->alloc((void**)&ctx->rope, tab.size() * 4));
    OM_HIP(hipMemcpy(ctx->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  }

  // ---- workspaces
  if (c.v_layers > 0) {
    const size_t Bm = (size_t)c.max_tiles, M = Bm * ctx->v_ntok;
    TRY(ctx->alloc(&ctx->vw_cols, Bm * ctx->v_np * ctx->v_kpad * 2));
    TRY(ctx->alloc(&ctx->vw_pe, Bm * ctx->v_np * C * 2));
    const size_t SL = 64;      // row slack: the last row block of a sequence-parallel reduce-scatter reaches up to tp_size - 1 rows beyond M
    TRY(ctx->alloc(&ctx->vw_x, (M + SL) * C * 2));
    TRY(ctx->alloc(&ctx->vw_x2, (M + SL) * C * 2));
    TRY(ctx->alloc(&ctx->vw_xn, (M + SL) * C * 2));
    TRY(ctx->alloc(&ctx->vw_qkv, M * 3 * ctx->v_Cq * 2));
    TRY(ctx->alloc(&ctx->vw_ao, M * ctx->v_Cq * 2));
    TRY(ctx->alloc(&ctx->vw_h, M * I * 2));
    TRY(ctx->alloc(&ctx->vw_feat, M * C * 2));
    TRY(ctx->alloc(&ctx->vw_proj, M * c.t_hidden * 2));
    TRY(ctx->alloc((void**)&ctx->vw_sumsq, M * 2 * 4 + 64));
    // statistics slots (slot-major [slot][M]): one per wave-column block of the producing GEMM, at least 48 columns wide (gemm.hip launch_epi_stats)
    ctx->vw_stats_x_ld = ctx->vw_stats_qk_ld = (int)((M + 63) / 64 * 64);
    TRY(ctx->alloc((void**)&ctx->vw_stats_x, (size_t)(cdiv(C, 48) + 2) * ctx->vw_stats_x_ld * 4));            // one slot per wave tile (>= 48 columns)
    TRY(ctx->alloc((void**)&ctx->vw_stats_qk, (size_t)(cdiv(3 * ctx->v_Cq, 64) + 1) * ctx->vw_stats_qk_ld * 4));   // qkv: one per 64
    TRY(ctx->alloc((void**)&ctx->vw_rstd, M * 4 + 64));
  }
  if (c.t_layers > 0) {
    const size_t R = std::max<size_t>(32, (size_t)(c.max_prefill_rows > c.max_batch ? c.max_prefill_rows : c.max_batch));      // >= 32: packed decode operands
    TRY(ctx->alloc(&ctx->tw_x, (R + 64) * H * 2));       // (+ 64 rows: slack of the sequence-parallel row blocks, see vw_x)
    TRY(ctx->alloc(&ctx->tw_x2, (R + 64) * H * 2));
    TRY(ctx->alloc(&ctx->tw_xn, (R + 64) * H * 2));
    TRY(ctx->alloc(&ctx->tw_qkv, R * ctx->t_qkvdim * 2));
    TRY(ctx->alloc(&ctx->tw_ao, R * ctx->t_qdim * 2));
    TRY(ctx->alloc(&ctx->tw_act, R * It * 2));
    TRY(ctx->alloc(&ctx->tw_last, (size_t)c.max_batch * H * 2));
    // decode-step rows: max_batch sequences, or the up to VERIFY_MAX_T tokens of a prompt-lookup verify step (omchat_decode_verify)
    const size_t DR = std::max(c.max_batch, VERIFY_MAX_T);
    TRY(ctx->alloc((void**)&ctx->tw_logits, DR * c.t_vocab * 4));
    ctx->tw_attn_ws_bytes = attn_decode_ws_bytes((int)DR, c.t_heads, c.max_seq);
    TRY(ctx->alloc((void**)&ctx->tw_attn_ws, ctx->tw_attn_ws_bytes));
    TRY(ctx->alloc((void**)&ctx->tw_part, (size_t)DEC_KS_MAX * DR * H * 4));
    if (OMCHAT_EXPERIMENTS) {
      const size_t fb = fused_decode_ws_bytes(c.t_heads);
      TRY(ctx->alloc(&ctx->fd_ws, fb));
      TRY(ctx->alloc((void**)&ctx->fd_err, 64));
      OM_HIP(hipMemset(ctx->fd_ws, 0, fb));
      OM_HIP(hipMemset(ctx->fd_err, 0, 64));
      const size_t lb = decode_layer_ws_bytes(c.t_heads, H, ctx->t_qdim, ctx->t_kvdim, It);
      TRY(ctx->alloc(&ctx->dl_ws, lb));
      OM_HIP(hipMemset(ctx->dl_ws, 0, lb));
      TRY(ctx->alloc((void**)&ctx->dyn_ctr, (size_t)c.t_layers * 65 * 64 * 4));
      OM_HIP(hipMemset(ctx->dyn_ctr, 0, (size_t)c.t_layers * 65 * 64 * 4));
      TRY(ctx->alloc((void**)&ctx->dbg_stamps, (size_t)c.t_layers * 256));
      OM_HIP(hipMemset(ctx->dbg_stamps, 0, (size_t)c.t_layers * 256));
    }
    TRY(pick_alloc(ctx, (int)DR));
    TRY(ctx->alloc((void**)&ctx->d_verify_n, 16));
    TRY(ctx->alloc((void**)&ctx->d_pos, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&ctx->d_len, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&ctx->d_idx, (size_t)c.max_batch * 4));
    TRY(ctx->alloc((void**)&ctx->d_start, (size_t)c.max_batch * 4));
    const size_t cache = (size_t)c.t_layers * ctx->cache_layer_stride() * 2;
    TRY(ctx->alloc(&ctx->kcache, cache));
    TRY(ctx->alloc(&ctx->vcache, cache));
    OM_HIP(hipMemset(ctx->kcache, 0, cache));
    OM_HIP(hipMemset(ctx->vcache, 0, cache));
    ctx->h_len.assign(c.max_batch, 0);
  }
  return 0;
}

int ensure_stage(omchat_ctx* ctx, size_t f32_bytes, size_t t_bytes) {
  if (f32_bytes > ctx->stage_f32_bytes) {
    if (ctx->stage_f32) hipFree(ctx->stage_f32);
    OM_HIP(hipMalloc(&ctx->stage_f32, f32_bytes));
    ctx->stage_f32_bytes = f32_bytes;
  }
  if (t_bytes > ctx->stage_t_bytes) {
    if (ctx->stage_t) hipFree(ctx->stage_t);
    OM_HIP(hipMalloc(&ctx->stage_t, t_bytes));
    ctx->stage_t_bytes = t_bytes;
  }
  return 0;
}

// copy a contiguous [rows, cols] T tensor (host or device) into its routed destination
int place(omchat_ctx* ctx, Route& r, const void* src_t) {
  const size_t rowb = (size_t)r.cols * 2;
  if (r.kind == R_PLAIN || r.kind == R_PATCH) {
    OM_HIP(hipMemcpy2D(r.dst, (size_t)r.dst_ld * 2, src_t, rowb, rowb, (size_t)r.rows, hipMemcpyDefault));
  } else {
    // gate block j (16 rows) -> fused rows [32j, 32j+16); up block j -> [32j+16, 32j+32)
    char* d = (char*)r.dst + (r.kind == R_UP ? 16 * rowb : 0);
    OM_HIP(hipMemcpy2D(d, 32 * rowb, src_t, 16 * rowb, 16 * rowb, (size_t)r.rows / 16, hipMemcpyDefault));
  }
  r.loaded = true;
  ctx->vfold_stale = true;      // (any tensor: the folded qkv / fc1 copies of the vision tower are rebuilt before the next tower pass)
  return 0;
}

}  // namespace

extern "C" int omchat_ctx_create(const omchat_config* cfg, int tp_rank, int tp_size, void* rccl_comm, omchat_ctx** out) {
  OM_CHECK(cfg && out, "null argument");
  OM_CHECK(cfg->dtype == OMCHAT_F16 || cfg->dtype == OMCHAT_BF16, "dtype must be OMCHAT_F16 or OMCHAT_BF16");
  OM_CHECK(tp_size >= 1 && tp_rank >= 0 && tp_rank < tp_size, "bad tensor-parallel rank/size");
  OM_CHECK(cfg->v_head_dim == 0 || cfg->v_head_dim == 128 || cfg->v_head_dim == 64, "v_head_dim must be 128 or 64");
  OM_CHECK(cfg->v_norm_type == 0 || cfg->v_norm_type == 1, "v_norm_type must be 0 (RMSNorm) or 1 (LayerNorm)");
  OM_CHECK(cfg->v_layers == 0 || (cfg->v_hidden % 64 == 0 && cfg->v_mlp % 64 == 0 && cfg->v_image % cfg->v_patch == 0),
           "vision dims: hidden/mlp % 64, image % patch");
  OM_CHECK(cfg->t_layers == 0 || (cfg->t_hidden % 64 == 0 && cfg->t_mlp % 64 == 0 && cfg->t_heads % cfg->t_kv_heads == 0),
           "text dims: hidden/mlp % 64, heads % kv_heads");
  OM_CHECK(cfg->t_layers == 0 || cfg->t_heads / cfg->t_kv_heads <= 16, "GQA group must be <= 16");
  int dev_count = 0;
  if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
    omchat_set_error("omchat_ctx_create: no HIP device (the HIP path has no CPU fallback)");
    return 2;
  }
  omchat_ctx* ctx = new omchat_ctx();
  ctx->c = *cfg; ctx->dt = cfg->dtype; ctx->tp_rank = tp_rank; ctx->tp_size = tp_size; ctx->comm = (ncclComm_t)rccl_comm;
  int rc = build(ctx);
  if (rc == 0 && tp_size > 1) {      // communication stream + events of the pipelined all-reduce (gemm_allreduce)
    auto mk = [&]() -> int {
      OM_HIP(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
      for (auto& e : ctx->ev_chunk) OM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      for (auto& e : ctx->ev_ag) OM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      OM_HIP(hipEventCreateWithFlags(&ctx->ev_comm_done, hipEventDisableTiming));
      return 0;
    };
    rc = mk();
  }
  if (rc) { omchat_ctx_destroy(ctx); return rc; }
  *out = ctx;
  return 0;
}

extern "C" void omchat_ctx_destroy(omchat_ctx* ctx) {
  if (!ctx) return;
  for (void* p : ctx->allocs) hipFree(p);
  for (auto& pr : ctx->prof) for (hipEvent_t e : pr.ev) hipEventDestroy(e);
  drop_decode_graphs(ctx);
  if (ctx->graph_ev_in) (void)hipEventDestroy(ctx->graph_ev_in);
  if (ctx->graph_ev_out) (void)hipEventDestroy(ctx->graph_ev_out);
  if (ctx->graph_stream) (void)hipStreamDestroy(ctx->graph_stream);
  for (hipEvent_t e : ctx->ev_chunk) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_ag) if (e) (void)hipEventDestroy(e);
  if (ctx->ev_comm_done) (void)hipEventDestroy(ctx->ev_comm_done);
  if (ctx->tp_f32_ws) (void)hipFree(ctx->tp_f32_ws);
  if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
  if (ctx->stage_f32) hipFree(ctx->stage_f32);
  if (ctx->stage_t) hipFree(ctx->stage_t);
  ctx->beam.release(); ctx->group.release(); ctx->cs.release(); ctx->ext_ws.release(); ctx->score_ws.release(); ctx->pick.release();
  delete ctx;
}

extern "C" size_t omchat_device_bytes(omchat_ctx* ctx) { return ctx ? ctx->bytes : 0; }

extern "C" int omchat_load_tensor(omchat_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim, int src_dtype) {
  OM_CHECK(ctx && name && data && shape, "null argument");
  auto it = ctx->routes.find(name);
  OM_CHECK(it != ctx->routes.end(), std::string("unknown tensor name: ") + name);
  Route& r = it->second;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= shape[i];
  OM_CHECK(n == r.rows * r.cols, std::string("shape mismatch for ") + name + ": expected " + std::to_string(r.rows * r.cols) +
                                     " elements, got " + std::to_string(n));
  {   // the leading dims must multiply to the routed row count (catches a transposed [cols, rows] tensor of the right size)
    bool split_ok = r.rows == 1 || ndim == 1;
    int64_t lead = 1;
    for (int i = 0; i < ndim && !split_ok; ++i) { lead *= shape[i]; split_ok = lead == r.rows; }
    OM_CHECK(split_ok, std::string("shape mismatch for ") + name + ": expected [" + std::to_string(r.rows) + ", " + std::to_string(r.cols) + "]");
  }
  for (int f = 0; f < OMCHAT_WFMT_COUNT; ++f)      // no replica matches the 16-bit weights any more (the 16-bit entry is a view of them)
    if (f != OMCHAT_WFMT_16 && ctx->built(f)) ctx->wt[f].state = omchat_ctx::W_STALE;
  for (auto& t : ctx->x12) if (t.state == omchat_ctx::W_BUILT) t.state = omchat_ctx::W_STALE;      // ... nor does a bf16x12 coding
  if (src_dtype == ctx->dt) return place(ctx, r, data);
  OM_CHECK(src_dtype == OMCHAT_F32, "source dtype must be the context dtype or OMCHAT_F32");
  TRY(ensure_stage(ctx, (size_t)n * 4, (size_t)n * 2));
  OM_HIP(hipMemcpy(ctx->stage_f32, data, (size_t)n * 4, hipMemcpyDefault));
  const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  if (ctx->dt == OMCHAT_F16) hipLaunchKernelGGL(cast_from_f32_f16, dim3(grid), dim3(256), 0, 0, (const float*)ctx->stage_f32, (f16*)ctx->stage_t, n);
  else hipLaunchKernelGGL(cast_from_f32_bf16, dim3(grid), dim3(256), 0, 0, (const float*)ctx->stage_f32, (bf16*)ctx->stage_t, n);
  OM_LAUNCH_CHECK();
  OM_HIP(hipDeviceSynchronize());
  return place(ctx, r, ctx->stage_t);
}

static uint64_t fnv1a64(const std::string& s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (unsigned char ch : s) { h ^= ch; h *= 0x100000001B3ull; }
  return h;
}

extern "C" int omchat_fill_synthetic(omchat_ctx* ctx, uint64_t seed) {
  OM_CHECK(ctx, "null ctx");
  // tp_size > 1: every rank fills its LOCAL shapes (right geometry for benches; not a sharding of the TP=1 values)
  size_t maxn = 0;
  for (auto& kv : ctx->routes) maxn = std::max(maxn, (size_t)(kv.second.rows * kv.second.cols));
  TRY(ensure_stage(ctx, 16, maxn * 2));
  for (auto& kv : ctx->routes) {
    Route& r = kv.second;
    const int64_t n = r.rows * r.cols;
    const float scale = (float)((double)r.synth_std * sqrt(3.0));
    TRY(launch_fill_uniform(ctx->dt, ctx->stage_t, n, fnv1a64(kv.first) ^ seed, scale, r.synth_off, 0));
    OM_HIP(hipDeviceSynchronize());
    TRY(place(ctx, r, ctx->stage_t));
  }
  return 0;
}

extern "C" int omchat_weights_missing(omchat_ctx* ctx) {
  int miss = 0;
  std::string names;
  for (auto& kv : ctx->routes)
    if (!kv.second.loaded) { if (miss < 8) names += kv.first + " "; ++miss; }
  if (miss) omchat_set_error("missing tensors: " + names + (miss > 8 ? "..." : ""));
  return miss;
}

// ---------------------------------------------------------------------------------------------------------
// vision tower
// ---------------------------------------------------------------------------------------------------------
static int gemm(omchat_ctx* ctx, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias,
                const void* ls, const void* resid, int ldr, int epi, hipStream_t s) {
  GemmArgs g{A, lda, W, ldw, C, ldc, M, N, K, bias, ls, resid, ldr, epi, 0, nullptr, 0, -1};
  return launch_gemm(ctx->dt, g, s);
}

int g_norm_in_gemv = 3;       // omchat_op_set_tuning key 14: bit 0 = the post-attention RMSNorm runs inside the gate|up GEMV, bit 1 = the input / final norm
                              // inside qkv / lm_head with down_proj un-split (0 = batch-1 decode keeps both residual + RMSNorm launches: A/B);
                              // bit 2 (experiments build only, measured slower: 4.57-4.87 vs 4.28 ms per step) = the seven-launch batched layer
void model_set_norm_in_gemv(int v) { g_norm_in_gemv = v; }
int g_pack_replica = 1;       // omchat_op_set_tuning key 6: 0 = batched decode reads the row-major weights (packed x only)
void model_set_pack_replica(int v) { g_pack_replica = v; }
int g_ar_min_rows = 1024;      // rows from which a projection is pipelined in 2 (x3: 4) chunks; tests lower it (omchat_op_set_tuning key 4)
void model_set_ar_min_rows(int v) { g_ar_min_rows = v > 8 ? v : 8; }

// Row-parallel projection (proj / fc2 / o_proj / down_proj under tensor parallelism): Y = epi(A W^T) holds this rank's partial
// sums and is all-reduced in place.  The rows are cut into up to AR_CHUNKS chunks of whole 256-row tiles; the all-reduce of
// chunk i is enqueued on the communication stream behind an event and runs under the GEMM of chunk i + 1 (RCCL's ring kernels
// take a few CUs, the GEMM the rest).  The launch stream resumes after the last chunk's all-reduce.
int g_tp_f32 = 0;      // omchat_op_set_tuning key 29: 1 = row-parallel projections of the prefill / the ViT are all-reduced as fp32 partial sums and the
                       // epilogue (bias, layer scale, residual) is applied once to the sum (launch_tp_finish); 0 (default) = every rank applies the
                       // epilogue to its own partial and the 16-bit results are summed (half the bytes on the links)
void model_set_tp_f32(int v) { g_tp_f32 = v; }

// bias / resid: the true operands on EVERY rank (the 16-bit path hands them to rank 0 only)
static int gemm_allreduce(omchat_ctx* ctx, const void* A, int lda, const void* W, int ldw, void* Y, int N, int M, int K, const void* bias_all,
                          const void* ls, const void* resid_all, int epi, hipStream_t s) {
  const bool lead = ctx->tp_rank == 0;
  const void* bias = lead ? bias_all : nullptr;
  const void* resid = lead ? resid_all : nullptr;
  int nch = M >= 3 * g_ar_min_rows ? 4 : (M >= g_ar_min_rows ? 2 : 1);
  if (!ctx->comm_stream) nch = 1;
  // A chunk must still fill the GPU: cutting the 3-tile ViT (M = 3075: 169 tiles of 256^2) or the single-sequence prefill (S = 3584: 196
  // tiles) into 1024-row chunks ran every projection as 3-4 launches on 52-78 of the 256 CUs (bench.py --shard-of 8, profiles/r03_a:
  // 3 x 34 us for a projection that takes ~40 us in one launch).  The all-reduce of such a message is then exposed, but it is shorter
  // than the lost GEMM time.  (Tests lower g_ar_min_rows below one tile to force chunking on tiny shapes: the rule is skipped there.)
  if (g_ar_min_rows >= 256) {
    const int n_cu = device_cus();
    const long tiles = (long)cdiv(M, 256) * cdiv(N, 256);
    while (nch > 1 && tiles / nch < n_cu) nch >>= 1;
  }
  const int align = g_ar_min_rows >= 256 ? 256 : 8;
  const int rows_per = nch == 1 ? M : cdiv(cdiv(M, nch), align) * align;
  // fp32 partial sums (tuning key 29): GEMM -> raw accumulators, fp32 all-reduce, one epilogue on the sum
  const bool f32 = g_tp_f32 && N % 4 == 0 && (epi == EPI_NONE || epi == EPI_RESID || epi == EPI_LS_RESID);
  if (f32) {
    const size_t need = (size_t)M * N * 4;
    if (ctx->tp_f32_bytes < need) {
      OM_HIP(hipStreamSynchronize(s));
      if (ctx->comm_stream) OM_HIP(hipStreamSynchronize(ctx->comm_stream));
      if (ctx->tp_f32_ws) (void)hipFree(ctx->tp_f32_ws);
      ctx->tp_f32_ws = nullptr; ctx->tp_f32_bytes = 0;
      OM_HIP(hipMalloc((void**)&ctx->tp_f32_ws, need));
      ctx->tp_f32_bytes = need;
    }
  }
  if (nch == 1) {
    if (f32) {
      TRY(gemm(ctx, A, lda, W, ldw, ctx->tp_f32_ws, N, M, N, K, nullptr, nullptr, nullptr, 0, EPI_F32OUT, s));
      TRY(ctx->allreduce_f32(ctx->tp_f32_ws, (size_t)M * N, s));
      return launch_tp_finish(ctx->dt, ctx->tp_f32_ws, bias_all, ls, resid_all, Y, M, N, epi, s);
    }
    TRY(gemm(ctx, A, lda, W, ldw, Y, N, M, N, K, bias, ls, resid, N, epi, s));
    return ctx->allreduce(Y, (size_t)M * N, s);
  }
  int i = 0;
  for (int r0 = 0; r0 < M; r0 += rows_per, ++i) {
    const int rows = std::min(rows_per, M - r0);
    char* y = (char*)Y + (size_t)r0 * N * 2;
    if (f32) {
      float* part = ctx->tp_f32_ws + (size_t)r0 * N;
      TRY(gemm(ctx, (const char*)A + (size_t)r0 * lda * 2, lda, W, ldw, part, N, rows, N, K, nullptr, nullptr, nullptr, 0, EPI_F32OUT, s));
      OM_HIP(hipEventRecord(ctx->ev_chunk[i], s));
      OM_HIP(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_chunk[i], 0));
      TRY(ctx->allreduce_f32(part, (size_t)rows * N, ctx->comm_stream));
      TRY(launch_tp_finish(ctx->dt, part, bias_all, ls, resid_all ? (const char*)resid_all + (size_t)r0 * N * 2 : nullptr, y, rows, N, epi, ctx->comm_stream));
      continue;
    }
    TRY(gemm(ctx, (const char*)A + (size_t)r0 * lda * 2, lda, W, ldw, y, N, rows, N, K, bias, ls,
             resid ? (const char*)resid + (size_t)r0 * N * 2 : nullptr, N, epi, s));
    OM_HIP(hipEventRecord(ctx->ev_chunk[i], s));
    OM_HIP(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_chunk[i], 0));
    TRY(ctx->allreduce(y, (size_t)rows * N, ctx->comm_stream));
  }
  OM_HIP(hipEventRecord(ctx->ev_comm_done, ctx->comm_stream));
  OM_HIP(hipStreamWaitEvent(s, ctx->ev_comm_done, 0));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Sequence-parallel norms (round 6; tuning key 45, default on under tensor parallelism).  The all-reduce form above leaves the WHOLE residual
// stream on every rank, and every rank then normalises all M rows: RMSNorm (2 x 88 us per ViT layer at 24 tiles) does not shrink with the group
// size -- 16 % of a TP = 8 ViT layer (profiles/r03_a).  Here a row-parallel projection ends in a reduce-scatter over ROW BLOCKS: rank r receives the
// summed rows it owns, adds the residual and normalises THOSE rows (M / tp_size of them, one launch), and an all-gather hands every rank the
// normalised activation the next column-parallel GEMM needs.  Same bytes on the links as the all-reduce (reduce-scatter + all-gather ARE its two
// halves), the replicated norm work divided by the group size.  The residual stream itself stays row-sharded between sub-blocks (rank r's copy is
// current on its own rows only) and is gathered once at the end of the tower / the prefill.  Megatron-LM's sequence parallelism restricted to the
// norms: the GEMMs and the attention keep their head / column shards.  No reference counterpart (builder.py:22-25 is device_map="auto").
//   rows of a chunk [r0, r0 + rows): block = cdiv(rows, tp_size) rows per rank; rank r owns [r0 + r * block, r0 + min((r + 1) * block, rows))
//   partials: every rank T(T(acc + (rank 0 ? bias : 0)) * ls) (ViT) or T(acc) (decoder); the owner adds the residual AFTER the sum -- one rounding
//   point moved against the all-reduce form (rank 0 added it before), inside the evaluation-order noise of 16-bit TP
// ---------------------------------------------------------------------------------------------------------
int g_tp_sp = 1;
void model_set_tp_sp(int v) { g_tp_sp = v; }

struct SpPlan { int nch, rows_per; };
static SpPlan sp_plan(omchat_ctx* ctx, int M, int N) {      // the chunk rule of gemm_allreduce (a chunk must still fill the GPU)
  int nch = M >= 3 * g_ar_min_rows ? 4 : (M >= g_ar_min_rows ? 2 : 1);
  if (!ctx->comm_stream) nch = 1;
  if (g_ar_min_rows >= 256) {
    const int n_cu = device_cus();
    const long tiles = (long)cdiv(M, 256) * cdiv(N, 256);
    while (nch > 1 && tiles / nch < n_cu) nch >>= 1;
  }
  const int unit = 8 * ctx->tp_size;                                    // whole row blocks inside every chunk but the last
  const int align = g_ar_min_rows >= 256 ? cdiv(256, unit) * unit : unit;
  const int rows_per = nch == 1 ? M : cdiv(cdiv(M, nch), align) * align;
  return {nch, rows_per};
}

// x (the residual stream, current on this rank's rows) <- x + sum over ranks of epi'(A W^T);  xn <- norm(x) on every row of every rank (nw == null: none)
static int gemm_sp(omchat_ctx* ctx, const void* A, int lda, const void* W, int ldw, void* P, void* x, int N, int M, int K, const void* bias_all, const void* ls,
                   int epi, const void* nw, const void* nb, void* xn, float eps, hipStream_t s) {
  const bool lead = ctx->tp_rank == 0;
  const SpPlan pl = sp_plan(ctx, M, N);
  const bool pipe = pl.nch > 1;
  hipStream_t cs = pipe ? ctx->comm_stream : s;
  int i = 0;
  for (int r0 = 0; r0 < M; r0 += pl.rows_per, ++i) {
    const int rows = std::min(pl.rows_per, M - r0);
    const int blk = cdiv(rows, ctx->tp_size);
    char* p = (char*)P + (size_t)r0 * N * 2;
    // the partial: bias on rank 0 only, layer scale on every rank (it distributes over the sum), NO residual
    TRY(gemm(ctx, (const char*)A + (size_t)r0 * lda * 2, lda, W, ldw, p, N, rows, N, K, lead ? bias_all : nullptr, ls, nullptr, 0,
             epi == EPI_LS_RESID ? EPI_LS_RESID : EPI_NONE, s));
    if (pipe) {
      OM_HIP(hipEventRecord(ctx->ev_chunk[i], s));
      OM_HIP(hipStreamWaitEvent(cs, ctx->ev_chunk[i], 0));
    }
    TRY(ctx->reduce_scatter_rows(p, blk, N, cs));
    const int o0 = ctx->tp_rank * blk, on = std::max(0, std::min(blk, rows - o0));      // my rows of this chunk
    char* xo = (char*)x + (size_t)(r0 + o0) * N * 2;
    char* no = nw ? (char*)xn + (size_t)(r0 + o0) * N * 2 : nullptr;
    TRY(launch_resid16_norm(ctx->dt, xo, N, p + (size_t)o0 * N * 2, N, nw, nb, no, N, on, N, eps, cs));
    if (nw) TRY(ctx->all_gather_rows((char*)xn + (size_t)r0 * N * 2, blk, N, cs));
    if (pipe && nw) OM_HIP(hipEventRecord(ctx->ev_ag[i], cs));
  }
  if (pipe && nw) {
    // the launch stream does NOT wait here: the consumer of xn (the next column-parallel GEMM: gemm_after_sp) goes out per row chunk behind
    // ev_ag[i], so chunk i + 1's reduce-scatter / norm / all-gather also runs under the consumer's GEMM of chunk i
    ctx->sp_pend_nch = pl.nch; ctx->sp_pend_rows_per = pl.rows_per;
  } else if (pipe) {
    OM_HIP(hipEventRecord(ctx->ev_comm_done, cs));
    OM_HIP(hipStreamWaitEvent(s, ctx->ev_comm_done, 0));
  }
  return 0;
}

// every exchange of a pending sequence-parallel sub-block is behind the launch stream (no consumer took it chunk by chunk)
static int sp_drain(omchat_ctx* ctx, hipStream_t s) {
  for (int i = 0; i < ctx->sp_pend_nch; ++i) OM_HIP(hipStreamWaitEvent(s, ctx->ev_ag[i], 0));
  ctx->sp_pend_nch = 0;
  return 0;
}

// C = epi(A W^T + bias) where A [M, lda] is the normalised activation a sequence-parallel sub-block is still gathering: one GEMM per row chunk of
// its plan, each behind that chunk's all-gather (a chunk holds >= 256 tiles of the producer, so the consumer's chunk fills the GPU too)
static int gemm_after_sp(omchat_ctx* ctx, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias, int epi,
                         hipStream_t s) {
  // a consumer chunk must hold two whole rounds of tiles: below that the partial last round of every chunk costs more than the exchange it hides
  // (bench.py --shard-of 4, configs[2]: the ViT's fc1 as four chunks of 312 tiles 380 ms per rank against 372 with one launch)
  const long chunk_tiles = (long)cdiv(ctx->sp_pend_rows_per, 256) * cdiv(N, 256);
  if (ctx->sp_pend_nch <= 1 || (g_ar_min_rows >= 256 && chunk_tiles < 2L * device_cus())) {      // (tests lower g_ar_min_rows: the rule is skipped there)
    TRY(sp_drain(ctx, s));
    return gemm(ctx, A, lda, W, ldw, C, ldc, M, N, K, bias, nullptr, nullptr, 0, epi, s);
  }
  const int nch = ctx->sp_pend_nch, rows_per = ctx->sp_pend_rows_per;
  ctx->sp_pend_nch = 0;
  int i = 0;
  for (int r0 = 0; r0 < M; r0 += rows_per, ++i) {
    const int rows = std::min(rows_per, M - r0);
    OM_HIP(hipStreamWaitEvent(s, ctx->ev_ag[i < nch ? i : nch - 1], 0));
    TRY(gemm(ctx, (const char*)A + (size_t)r0 * lda * 2, lda, W, ldw, (char*)C + (size_t)r0 * ldc * 2, ldc, rows, N, K, bias, nullptr, nullptr, 0, epi, s));
  }
  return 0;
}

// the row-sharded residual stream made whole on every rank (end of the tower / of the prefill): one all-gather per chunk of the same plan
static int sp_gather_x(omchat_ctx* ctx, void* x, int N, int M, hipStream_t s) {
  const SpPlan pl = sp_plan(ctx, M, N);
  for (int r0 = 0; r0 < M; r0 += pl.rows_per) {
    const int rows = std::min(pl.rows_per, M - r0);
    TRY(ctx->all_gather_rows((char*)x + (size_t)r0 * N * 2, cdiv(rows, ctx->tp_size), N, s));
  }
  return 0;
}

int g_vit_fused = 1;      // omchat_op_set_tuning key 44: 1 = the ViT layer with its norms folded into the GEMMs (round 6), 0 = the round-5 launches
void model_set_vit_fused(int v) { g_vit_fused = v; }

// The fused ViT layer needs norm1 / norm2's WEIGHT inside the qkv / fc1 weights: y = w * (x * rstd) feeds a linear map, so
// (w * x * rstd) W^T = rstd * (x (W diag(w))^T): W' = T(W * w) column-wise, once per load; rstd becomes the GEMM's row scale.
static int ensure_vit_folded(omchat_ctx* ctx, hipStream_t s) {
  if (!ctx->vfold_stale && !ctx->vfold.empty()) return 0;
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, I = c.v_mlp, Cq = ctx->v_Cq;
  if (ctx->vfold.empty()) {
    ctx->vfold.resize(c.v_layers);
    for (auto& f : ctx->vfold) {
      TRY(ctx->alloc(&f.wqkv, (size_t)3 * Cq * C * 2));
      TRY(ctx->alloc(&f.w1, (size_t)I * C * 2));
    }
  }
  for (int j = 0; j < c.v_layers; ++j) {
    TRY(launch_fold_cols(ctx->dt, ctx->vl[j].wqkv, ctx->vl[j].n1, ctx->vfold[j].wqkv, 3 * Cq, C, s));
    TRY(launch_fold_cols(ctx->dt, ctx->vl[j].w1, ctx->vl[j].n2, ctx->vfold[j].w1, I, C, s));
  }
  ctx->vfold_stale = false;
  return 0;
}

static int gemm_x(omchat_ctx* ctx, GemmArgs g, hipStream_t s) { return launch_gemm(ctx->dt, g, s); }

// One InternVisionEncoderLayer (modeling_intern_vit.py:210-222) as SIX launches (round 6; TP = 1, RMSNorm tower):
//   qkv GEMM (A = raw x, W' = Wqkv diag(norm1.w), row scale rstd1 finished per tile from x's slots, epilogue leaves the q / k sum-of-squares slots)
//   K norm (from its slots; leaves the q sums)   attention (Q normed + scaled where it is loaded)   proj GEMM (+b, *ls1, +x; leaves x's slots)
//   fc1 GEMM (A = raw x, W' = W1 diag(norm2.w), row scale rstd2 from x's slots, +b, GELU)   fc2 GEMM (+b, *ls2, +x; leaves x's slots)
// against the round-5 layer's rmsnorm, qkv, q/k norm, attention, proj, rmsnorm, fc1, fc2: two 39 MB norm passes and half of the 79 MB
// q / k pass are gone, and nothing was added between the GEMMs (a first form with three statistics-finishing launches of 4.8 us each gave
// the whole gain back: profiles/r06_c).  Numerics: x * rstd is no longer rounded to 16 bits before the product (one rounding FEWER than the reference,
// N2) and the norm weight is rounded into W' instead of into the activation; the q / k norm keeps the reference's rounding points, its
// statistics are summed per 64-column block first (fp32 order).  Guarded by the reference goldens and the full-depth oracle fixture.
static int vit_layer_fused(omchat_ctx* ctx, int j, void* x, int B, bool last, hipStream_t s) {
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, I = c.v_mlp, Cq = ctx->v_Cq, ntok = ctx->v_ntok, M = B * ntok, hd = ctx->v_hd;
  auto& L = ctx->vl[j];
  auto& F = ctx->vfold[j];
  const float qscale = 0.08838834764831845f;      // head_dim ** -0.5 (modeling_intern_vit.py:118), head dim 128
  int ns_x = 0;
  if (j == 0) {      // the embeddings came from vit_assemble: one slot
    TRY(launch_row_sumsq(ctx->dt, x, C, M, C, ctx->vw_stats_x, s));
    ctx->vw_stats_x_ld_used = 1;
  }
  {
    GemmArgs g{x, C, F.wqkv, C, ctx->vw_qkv, 3 * Cq, M, 3 * Cq, C, nullptr, nullptr, nullptr, 0, EPI_NONE_STATS, 2, nullptr, 0, -1};
    // norm1 as the row scale, finished per tile from the slots x's producer left
    g.rs_stats = ctx->vw_stats_x; g.rs_ld = ctx->vw_stats_x_ld; g.rs_nslots = ctx->vw_stats_x_ld_used; g.rs_dim = C; g.rs_eps = c.v_eps;
    g.stats = ctx->vw_stats_qk; g.stats_ld = ctx->vw_stats_qk_ld;
    TRY(gemm_x(ctx, g, s));      // (tile 2: 64-column slots, so q = slots [0, Cq / 64), k = [Cq / 64, 2 Cq / 64))
  }
  // K is normalised in place from its slots; the q slots' sum goes to vw_sumsq [M] for the attention kernel's q norm on load
  const int qs = Cq / 64;
  TRY(launch_vit_knorm_slots(ctx->dt, (char*)ctx->vw_qkv + (size_t)Cq * 2, 3 * Cq, L.kn, M, Cq, c.v_qk_channels, c.v_eps, ctx->vw_stats_qk, ctx->vw_stats_qk_ld, qs,
                             ctx->vw_sumsq, s));
  AttnArgs a{};
  a.scale = 1.0f;
  a.Q = ctx->vw_qkv; a.q_sb = (int64_t)ntok * 3 * Cq; a.q_sh = hd; a.q_sr = 3 * Cq;
  a.K = (const char*)ctx->vw_qkv + (size_t)Cq * 2; a.k_sb = a.q_sb; a.k_sh = hd; a.k_sr = 3 * Cq;
  a.V = (const char*)ctx->vw_qkv + (size_t)2 * Cq * 2; a.v_sb = a.q_sb; a.v_sh = hd; a.v_sr = 3 * Cq;
  a.O = ctx->vw_ao; a.o_sb = (int64_t)ntok * Cq; a.o_sh = hd; a.o_sr = Cq;
  a.batch = B; a.q_heads = c.v_heads; a.kv_heads = c.v_heads; a.Sq = ntok; a.Skv = ntok; a.kv_len = nullptr; a.causal = 0; a.q_pos0 = 0;
  a.head_dim = hd;
  a.qn_sumsq = ctx->vw_sumsq; a.qn_stride = 1; a.qn_dim = c.v_qk_channels; a.qn_w = L.qn; a.qn_eps = c.v_eps; a.qn_scale = qscale;
  TRY(launch_attn_prefill(ctx->dt, a, s));
  {
    GemmArgs g{ctx->vw_ao, Cq, L.wproj, Cq, x, C, M, C, Cq, L.bproj, L.ls1, x, C, EPI_LS_RESID_STATS, 0, nullptr, 0, -1};
    g.stats = ctx->vw_stats_x; g.stats_ld = ctx->vw_stats_x_ld; g.stats_nslots = &ns_x;
    TRY(gemm_x(ctx, g, s));
  }
  ctx->prof_mark(OMCHAT_PROF_VIT_FC1, s);
  {
    GemmArgs g{x, C, F.w1, C, ctx->vw_h, I, M, I, C, L.b1, nullptr, nullptr, 0, EPI_GELU, 0, nullptr, 0, -1};
    g.rs_stats = ctx->vw_stats_x; g.rs_ld = ctx->vw_stats_x_ld; g.rs_nslots = ns_x; g.rs_dim = C; g.rs_eps = c.v_eps;      // norm2
    TRY(gemm_x(ctx, g, s));
  }
  ctx->prof_mark(OMCHAT_PROF_VIT_FC1, s);
  {
    GemmArgs g{ctx->vw_h, I, L.w2, I, x, C, M, C, I, L.b2, L.ls2, x, C, last ? EPI_LS_RESID : EPI_LS_RESID_STATS, 0, nullptr, 0, -1};
    if (!last) { g.stats = ctx->vw_stats_x; g.stats_ld = ctx->vw_stats_x_ld; g.stats_nslots = &ns_x; }
    TRY(gemm_x(ctx, g, s));
    if (!last) ctx->vw_stats_x_ld_used = ns_x;
  }
  return 0;
}

static int vit_run(omchat_ctx* ctx, const void* pixels, int B, int n_layers, hipStream_t s, void** x_out) {
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, I = c.v_mlp, Cq = ctx->v_Cq, np = ctx->v_np, ntok = ctx->v_ntok, M = B * ntok;
  const bool lead = ctx->tp_rank == 0;
  // (Cq / 64 <= 64: vit_knorm_slots sums the q / k slots one per lane of a wave -- up to 32 heads of 128; a wider tower takes the round-5 layer)
  const bool fused = g_vit_fused && ctx->tp_size == 1 && c.v_norm_type == 0 && !c.v_no_qk_norm && ctx->v_hd == 128 && Cq % 64 == 0 && Cq / 64 <= 64;
  if (fused) TRY(ensure_vit_folded(ctx, s));
  // InternVisionEmbeddings.forward (modeling_intern_vit.py:90-102)
  TRY(launch_im2col(ctx->dt, pixels, ctx->vw_cols, B, c.v_image, c.v_patch, ctx->v_kpad, s));
  TRY(gemm(ctx, ctx->vw_cols, ctx->v_kpad, ctx->v_wpatch, ctx->v_kpad, ctx->vw_pe, C, B * np, C, ctx->v_kpad, ctx->v_bpatch, nullptr, nullptr, 0, EPI_NONE, s));
  TRY(launch_vit_assemble(ctx->dt, ctx->vw_pe, ctx->v_cls, ctx->v_pos, ctx->vw_x, B, np, C, s));
  void* x = ctx->vw_x;
  void* y = ctx->vw_x2;
  const bool sp = g_tp_sp && ctx->tp_size > 1 && !g_tp_f32;      // sequence-parallel norms: gemm_sp
  for (int j = 0; j < n_layers; ++j) {
    if (fused) { TRY(vit_layer_fused(ctx, j, x, B, j + 1 == n_layers, s)); continue; }
    auto& L = ctx->vl[j];
    // InternVisionEncoderLayer.forward (modeling_intern_vit.py:210-222)
    const int hd = ctx->v_hd;
    const float qscale = hd == 128 ? 0.08838834764831845f : 0.125f;      // head_dim ** -0.5 (modeling_intern_vit.py:118)
    auto norm = [&](const void* w, const void* b) -> int {      // InternRMSNorm, or nn.LayerNorm for the 300M tower (NORM2FN)
      if (c.v_norm_type == 1) return launch_layernorm(ctx->dt, x, C, w, b, ctx->vw_xn, C, M, C, c.v_eps, s);
      return launch_rmsnorm(ctx->dt, x, C, w, ctx->vw_xn, C, M, C, c.v_eps, s);
    };
    if (!sp || j == 0) TRY(norm(L.n1, L.n1b));      // (sequence-parallel: the previous layer's fc2 left norm1(x) in vw_xn)
    if (sp) TRY(gemm_after_sp(ctx, ctx->vw_xn, C, L.wqkv, C, ctx->vw_qkv, 3 * Cq, M, 3 * Cq, C, nullptr, EPI_NONE, s));
    else TRY(gemm(ctx, ctx->vw_xn, C, L.wqkv, C, ctx->vw_qkv, 3 * Cq, M, 3 * Cq, C, nullptr, nullptr, nullptr, 0, EPI_NONE, s));
    AttnArgs a{};
    if (!c.v_no_qk_norm) {
      const float* sumsq = nullptr;
      if (ctx->tp_size > 1) {     // joint-head norm: sum of squares over ALL ranks' heads
        TRY(launch_vit_qk_sumsq(ctx->dt, ctx->vw_qkv, 3 * Cq, M, Cq, ctx->vw_sumsq, s));
        TRY(ctx->allreduce_f32(ctx->vw_sumsq, (size_t)M * 2, s));
        sumsq = ctx->vw_sumsq;
      }
      TRY(launch_vit_qknorm(ctx->dt, ctx->vw_qkv, 3 * Cq, L.qn, L.kn, M, Cq, c.v_qk_channels, c.v_eps, qscale, sumsq, s));
      a.scale = 1.0f;     // q was pre-scaled by the q/k norm kernel (reference order, modeling_intern_vit.py:148)
    } else {
      a.scale = qscale;     // q * scale is exact for head_dim 64 (2^-3), so scaling the fp32 scores is the same value
    }
    a.Q = ctx->vw_qkv; a.q_sb = (int64_t)ntok * 3 * Cq; a.q_sh = hd; a.q_sr = 3 * Cq;
    a.K = (const char*)ctx->vw_qkv + (size_t)Cq * 2; a.k_sb = a.q_sb; a.k_sh = hd; a.k_sr = 3 * Cq;
    a.V = (const char*)ctx->vw_qkv + (size_t)2 * Cq * 2; a.v_sb = a.q_sb; a.v_sh = hd; a.v_sr = 3 * Cq;
    a.O = ctx->vw_ao; a.o_sb = (int64_t)ntok * Cq; a.o_sh = hd; a.o_sr = Cq;
    a.batch = B; a.q_heads = c.v_heads; a.kv_heads = c.v_heads; a.Sq = ntok; a.Skv = ntok; a.kv_len = nullptr; a.causal = 0; a.q_pos0 = 0;
    a.head_dim = hd;
    TRY(launch_attn_prefill(ctx->dt, a, s));
    if (ctx->tp_size == 1) {
      TRY(gemm(ctx, ctx->vw_ao, Cq, L.wproj, Cq, x, C, M, C, Cq, L.bproj, L.ls1, x, C, EPI_LS_RESID, s));
    } else if (sp) {
      TRY(gemm_sp(ctx, ctx->vw_ao, Cq, L.wproj, Cq, y, x, C, M, Cq, L.bproj, L.ls1, EPI_LS_RESID, L.n2, L.n2b, ctx->vw_xn, c.v_eps, s));
    } else {
      TRY(gemm_allreduce(ctx, ctx->vw_ao, Cq, L.wproj, Cq, y, C, M, Cq, L.bproj, L.ls1, x, EPI_LS_RESID, s));
      std::swap(x, y);
    }
    if (!sp) TRY(norm(L.n2, L.n2b));
    ctx->prof_mark(OMCHAT_PROF_VIT_FC1, s);
    if (sp) TRY(gemm_after_sp(ctx, ctx->vw_xn, C, L.w1, C, ctx->vw_h, I, M, I, C, L.b1, EPI_GELU, s));
    else TRY(gemm(ctx, ctx->vw_xn, C, L.w1, C, ctx->vw_h, I, M, I, C, L.b1, nullptr, nullptr, 0, EPI_GELU, s));
    ctx->prof_mark(OMCHAT_PROF_VIT_FC1, s);
    if (ctx->tp_size == 1) {
      TRY(gemm(ctx, ctx->vw_h, I, L.w2, I, x, C, M, C, I, L.b2, L.ls2, x, C, EPI_LS_RESID, s));
    } else if (sp) {
      const bool more = j + 1 < n_layers;      // the next layer's norm1 on the owned rows; after the last layer the stream is gathered instead
      TRY(gemm_sp(ctx, ctx->vw_h, I, L.w2, I, y, x, C, M, I, L.b2, L.ls2, EPI_LS_RESID, more ? ctx->vl[j + 1].n1 : nullptr, more ? ctx->vl[j + 1].n1b : nullptr,
                  ctx->vw_xn, c.v_eps, s));
      if (!more) TRY(sp_gather_x(ctx, x, C, M, s));
    } else {
      TRY(gemm_allreduce(ctx, ctx->vw_h, I, L.w2, I, y, C, M, I, L.b2, L.ls2, x, EPI_LS_RESID, s));
      std::swap(x, y);
    }
  }
  TRY(sp_drain(ctx, s));
  *x_out = x;
  return 0;
}

static int resolve_layer(omchat_ctx* ctx, int select_layer, int* idx) {
  const int L = ctx->c.v_layers;
  const int i = select_layer >= 0 ? select_layer : L + 1 + select_layer;
  OM_CHECK(i >= 0 && i <= L, "select_layer out of range");
  *idx = i;
  return 0;
}

extern "C" int omchat_vit_forward(omchat_ctx* ctx, const void* pixels, int n_tiles, int select_layer, int keep_cls, void* out, void* stream) {
  OM_CHECK(ctx && pixels && out, "null argument");
  OM_CHECK(ctx->c.v_layers > 0, "context has no vision tower");
  OM_CHECK(n_tiles >= 0, "negative tile count");
  OM_CHECK(omchat_weights_missing(ctx) == 0, std::string(omchat_last_error()));
  int idx; TRY(resolve_layer(ctx, select_layer, &idx));
  hipStream_t s = (hipStream_t)stream;
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, np = ctx->v_np, ntok = ctx->v_ntok;
  const size_t px_tile = (size_t)3 * c.v_image * c.v_image * 2;
  const int out_tok = keep_cls ? ntok : np;
  for (int t0 = 0; t0 < n_tiles; t0 += c.max_tiles) {
    const int B = std::min(c.max_tiles, n_tiles - t0);
    void* x;
    TRY(vit_run(ctx, (const char*)pixels + t0 * px_tile, B, idx, s, &x));
    // feature_select (internVIT_encoder.py:35-43): 'patch' drops CLS, 'cls_patch' keeps it
    char* o = (char*)out + (size_t)t0 * out_tok * C * 2;
    if (keep_cls) TRY(launch_copy_rows(ctx->dt, x, C, o, C, B * ntok, C, ntok, 0, s));
    else TRY(launch_copy_rows(ctx->dt, x, C, o, C, B * np, C, np, 1, s));
  }
  return 0;
}

extern "C" int omchat_projector_forward(omchat_ctx* ctx, const void* in, int rows, void* out, void* stream) {
  OM_CHECK(ctx && in && out, "null argument");
  OM_CHECK(ctx->c.v_layers > 0, "context has no projector");
  hipStream_t s = (hipStream_t)stream;
  const int C = ctx->c.v_hidden, H = ctx->c.t_hidden;
  const int cap = ctx->c.max_tiles * ctx->v_ntok;
  for (int r0 = 0; r0 < rows; r0 += cap) {
    const int R = std::min(cap, rows - r0);
    const char* a = (const char*)in + (size_t)r0 * C * 2;
    char* o = (char*)out + (size_t)r0 * H * 2;
    // Linear + GELU + Linear (multimodal_projector/builder.py:57-61)
    TRY(gemm(ctx, a, C, ctx->p_w0, C, ctx->vw_proj, H, R, H, C, ctx->p_b0, nullptr, nullptr, 0, EPI_GELU, s));
    TRY(gemm(ctx, ctx->vw_proj, H, ctx->p_w2, H, o, H, R, H, H, ctx->p_b2, nullptr, nullptr, 0, EPI_NONE, s));
  }
  return 0;
}

extern "C" int omchat_encode_images(omchat_ctx* ctx, const void* pixels, int n_tiles, int select_layer, void* out, void* stream) {
  OM_CHECK(ctx && pixels && out, "null argument");
  OM_CHECK(ctx->c.v_layers > 0, "context has no vision tower");
  OM_CHECK(omchat_weights_missing(ctx) == 0, std::string(omchat_last_error()));
  int idx; TRY(resolve_layer(ctx, select_layer, &idx));
  hipStream_t s = (hipStream_t)stream;
  const omchat_config& c = ctx->c;
  const int C = c.v_hidden, H = c.t_hidden, np = ctx->v_np;
  const size_t px_tile = (size_t)3 * c.v_image * c.v_image * 2;
  for (int t0 = 0; t0 < n_tiles; t0 += c.max_tiles) {
    const int B = std::min(c.max_tiles, n_tiles - t0);
    void* x;
    TRY(vit_run(ctx, (const char*)pixels + t0 * px_tile, B, idx, s, &x));
    TRY(launch_copy_rows(ctx->dt, x, C, ctx->vw_feat, C, B * np, C, np, 1, s));
    TRY(omchat_projector_forward(ctx, ctx->vw_feat, B * np, (char*)out + (size_t)t0 * np * H * 2, s));
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// splice
// ---------------------------------------------------------------------------------------------------------
extern "C" int omchat_splice_plan(const int64_t* ids, const uint8_t* mask, int b, int T, int n_tok, int n_tiles_avail, int padding_side,
                                  int max_length, int32_t* src_index, int32_t* lengths, int* S_out, int vocab) {
  OM_CHECK(ids && S_out && b > 0 && T > 0 && n_tok >= 0, "bad argument");
  // embed_tokens raises IndexError for an id outside [0, vocab) (omchat_arch.py:139); the device gather would read out of bounds
  if (vocab > 0)
    for (size_t i = 0; i < (size_t)b * T; ++i) {
      if (mask && !mask[i]) continue;
      if (ids[i] != -200 && (ids[i] < 0 || ids[i] >= vocab)) {
        omchat_set_error("omchat_splice_plan: token id " + std::to_string(ids[i]) + " out of range [0, " + std::to_string(vocab) + ") (index out of range in embed_tokens)");
        return 4;
      }
    }
  // pass 1: lengths (omchat_arch.py:115-164); a row without sentinels still consumes one tile slot (:122-129)
  std::vector<int> len(b);
  int cur = 0, S = 0, total_img = 0;
  for (int i = 0; i < b; ++i) {
    int n = 0, n_img = 0;
    for (int t = 0; t < T; ++t) {
      if (mask && !mask[(size_t)i * T + t]) continue;
      if (ids[(size_t)i * T + t] == -200) { n += n_tok; ++n_img; } else ++n;
    }
    cur += n_img == 0 ? 1 : n_img;
    total_img += n_img;
    if (max_length > 0 && n > max_length) n = max_length;
    len[i] = n;
    S = std::max(S, n);
  }
  // text-only call (no tiles, no sentinels) = plain embed_tokens lookup (the reference short-circuits before the splice, :59-70)
  OM_CHECK(cur <= n_tiles_avail || n_tok == 0 || (n_tiles_avail == 0 && total_img == 0), "more <image> sentinels than image tiles (reference: IndexError on image_features)");
  *S_out = S;
  if (lengths) for (int i = 0; i < b; ++i) lengths[i] = len[i];
  if (!src_index) return 0;
  cur = 0;
  for (int i = 0; i < b; ++i) {
    int32_t* row = src_index + (size_t)i * S;
    const int off = padding_side == 1 ? S - len[i] : 0;       // left padding (:176-184) vs right (:185-193)
    for (int s = 0; s < S; ++s) row[s] = INT32_MIN;
    int w = 0, n_img = 0;
    for (int t = 0; t < T; ++t) {
      if (mask && !mask[(size_t)i * T + t]) continue;
      const int64_t id = ids[(size_t)i * T + t];
      if (id == -200) {
        for (int k = 0; k < n_tok; ++k, ++w)
          if (w < len[i]) row[off + w] = -1 - (cur * n_tok + k);
        ++cur; ++n_img;
      } else {
        if (w < len[i]) row[off + w] = (int32_t)id;
        ++w;
      }
    }
    if (n_img == 0) ++cur;
  }
  return 0;
}

extern "C" int omchat_splice_gather(omchat_ctx* ctx, const int32_t* src_index, const void* feats, void* embeds, int rows, void* stream) {
  OM_CHECK(ctx && src_index && embeds, "null argument");
  OM_CHECK(ctx->t_embed, "context has no decoder");
  return launch_gather_rows(ctx->dt, src_index, ctx->t_embed, feats, embeds, rows, ctx->c.t_hidden, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------------------------------------
// hidden [n][H] -> logits through the lm_head reference of the caller's format; x_packed: hidden is in the packed x layout (n <= 32)
static int lm_head_rows(omchat_ctx* ctx, const void* hidden, int n, float* logits, hipStream_t s, const omchat_ctx::WRef& lm, bool x_packed = false) {
  const int H = ctx->c.t_hidden, V = ctx->c.t_vocab;
  for (int r0 = 0; r0 < n; r0 += 32) {
    const int R = std::min(32, n - r0);
    GemvArgs g{(const char*)hidden + (size_t)r0 * H * 2, H, nullptr, 0, logits + (size_t)r0 * V, V, R, V, H, nullptr, nullptr, 0, EPI_NONE, 1};
    use_weight(g, lm);
    g.x_packed = x_packed;
    TRY(launch_gemv(ctx->dt, g, s));
  }
  return 0;
}

// Layer-contrastive decoding (omchat_set_dola): the head pass of a prefill or step.  dola_hid holds the candidate rows at
// (1 + j) * b + r; xf = the b last-position rows of the residual stream behind the last layer.  They go to rows [0, b) and through the final
// RMSNorm (with `norm` the candidate rows too: the same launch over more rows), then all (k + 1) b rows through the 16-bit head in one pass
// into the context's rows; the caller's logits (or NULL) get the b final rows.
static int dola_head(omchat_ctx* ctx, const void* xf, float* logits, hipStream_t s) {
  PickState& P = ctx->pick;
  const omchat_config& c = ctx->c;
  const int H = c.t_hidden, b = P.dola.b, n = P.dola.rows();
  OM_HIP(hipMemcpyAsync(P.dola_hid, xf, (size_t)b * H * 2, hipMemcpyDeviceToDevice, s));
  TRY(launch_rmsnorm(ctx->dt, P.dola_hid, H, ctx->t_norm, P.dola_hid, H, P.dola.norm ? n : b, H, c.t_eps, s));
  TRY(lm_head_rows(ctx, P.dola_hid, n, P.dola_logits, s, ctx->lm_w(OMCHAT_WFMT_16)));
  if (logits) OM_HIP(hipMemcpyAsync(logits, P.dola_logits, (size_t)b * c.t_vocab * 4, hipMemcpyDeviceToDevice, s));
  P.dola_fresh = true;
  return 0;
}
// ... and the rows a candidate layer keeps: dst = row block (1 + j) of dola_hid
static void* dola_slot(omchat_ctx* ctx, int j) { return (char*)ctx->pick.dola_hid + (size_t)(1 + j) * ctx->pick.dola.b * ctx->c.t_hidden * 2; }

// (Re)build one replica of the decode-streamed weights: the layers * 4 + 1 entries of its table, by proj_shape.  The first build takes every
// buffer or none and commits the table only then (a half-built table must never reach a launch); a rebuild after omchat_load_tensor fills
// the same buffers in place (same device pointers: a captured graph stays valid).  Synchronous, never inside a graph capture.
// The packed MXFP4 replica is a byte shuffle of the row-major one, which is therefore brought up to date first.
static int build_replica(omchat_ctx* ctx, int fmt) {
  omchat_ctx::WTable& T = ctx->wt[fmt];
  if (T.state == omchat_ctx::W_BUILT) return 0;
  const bool f8 = fmt == OMCHAT_WFMT_E4M3, mx = fmt == OMCHAT_WFMT_MXFP4, mxp = fmt == OMCHAT_WFMT_MXFP4_PACKED, p16 = fmt == OMCHAT_WFMT_16_PACKED;
  if (f8 || mx) OM_CHECK(omchat_weights_missing(ctx) == 0, "load the weights before quantising them");
  if (mx) OM_CHECK(ctx->c.t_hidden % 32 == 0 && ctx->t_qdim % 32 == 0 && ctx->c.t_mlp % 32 == 0,
                   "MXFP4 decode: every streamed K (hidden_size, heads x 128, intermediate_size) must be a multiple of 32");
  if (mxp) TRY(build_replica(ctx, OMCHAT_WFMT_MXFP4));
  const std::vector<omchat_ctx::WRef>& src = ctx->wt[mxp ? OMCHAT_WFMT_MXFP4 : OMCHAT_WFMT_16].e;
  if (T.e.empty()) {
    std::vector<omchat_ctx::WRef> fresh(src.size());
    std::vector<void**> slots;
    std::vector<size_t> sizes;
    for (size_t j = 0; j < fresh.size(); ++j) {
      const size_t N = entry_shape(ctx, j).N, K = entry_shape(ctx, j).K;
      omchat_ctx::WRef& r = fresh[j];
      r.ldw = (int)(mx || mxp ? K / 2 : K);
      r.packed = p16 || mxp;
      slots.push_back(&r.W); sizes.push_back(p16 ? N * K * 2 : f8 ? N * K : N * (K / 2));
      if (f8) { slots.push_back((void**)&r.w_scale); sizes.push_back(N * 4); }
      if (mx || mxp) { slots.push_back((void**)&r.mx_scale); sizes.push_back(N * (K / 32)); }
    }
    if (ctx->alloc_group(slots, sizes)) {
      if (p16) { T.state = omchat_ctx::W_UNAVAILABLE; return 0; }      // optional: batched steps keep streaming the row-major weights
      if (mxp) omchat_set_error("omchat_enable_mxfp4_decode: the packed MXFP4 replica of mode 2 does not fit in device memory (hipMalloc failed)");
      return 2;
    }
    T.e.swap(fresh);
  }
  for (size_t j = 0; j < T.e.size(); ++j) {
    const int N = entry_shape(ctx, j).N, K = entry_shape(ctx, j).K;
    const omchat_ctx::WRef& w = src[j]; const omchat_ctx::WRef& r = T.e[j];
    if (f8) TRY(launch_quant_fp8_rows(ctx->dt, w.W, K, N, K, r.W, K, r.w_scale, nullptr));
    else if (mx) TRY(launch_quant_mxfp4_rows(ctx->dt, w.W, K, N, K, r.W, K / 2, r.mx_scale, nullptr));
    else if (mxp) TRY(launch_pack_w4(w.W, w.mx_scale, N, K, r.W, r.mx_scale, nullptr));
    else TRY(launch_pack_w(ctx->dt, w.W, K, N, K, r.W, nullptr));
  }
  OM_HIP(hipDeviceSynchronize());
  T.state = omchat_ctx::W_BUILT;
  return 0;
}

// omchat_op_set_tuning key 50: the roles of a batch-1 step that stream the bf16x12 coding of their bf16 rows: bit 0 = gate|up, bit 1 =
// down_proj, bit 2 = lm_head; 0 = the 16-bit launches exactly (A/B: the same bits either way).  The default is what tools/bench_bf16x12.py measured:
// gate|up 41.1 -> 33.7 us, lm_head 160.3 -> 126.0 us, and the long-K down_proj form in passes of four chunks (68 VGPRs: both workgroups of
// a CU resident) 22.8 -> 21.9 us; in the 16-bit form's passes of eight it took 136 VGPRs and measured 27.3 us (LOG.md)
int g_x12_roles = 7;
void model_set_x12_roles(int v) { g_x12_roles = v & 7; }

// The roles a step of `rows` rows would stream coded, by everything but the state of the copies: the step's format is 16-bit at b == 1 on one
// GPU in bf16, and the role's 16-bit launch is in its default form
static int x12_step_mask(const omchat_ctx* ctx, int rows, int fmt) {
  if (rows != 1 || fmt != OMCHAT_WFMT_16 || ctx->dt != OMCHAT_BF16 || ctx->tp_size != 1) return 0;
  return g_x12_roles & gemv_x12_default_forms();
}

// (Re)build the bf16x12 coding of one role (ctx.h): every buffer of the role or none; an allocation that fails or a K outside the forms leaves
// the role on 16 bits for good.  A rebuild after omchat_load_tensor encodes into the same buffers (a captured graph stays valid); if that
// moves a tensor over or under the patch cap, the launch it needs is another one and the captured graphs are dropped.
static int build_x12(omchat_ctx* ctx, int role) {
  omchat_ctx::X12Table& T = ctx->x12[role];
  if (T.state == omchat_ctx::W_BUILT || T.state == omchat_ctx::W_UNAVAILABLE) return 0;
  const omchat_config& c = ctx->c;
  const int H = c.t_hidden, It = c.t_mlp, L = c.t_layers;
  const bool lm = role == omchat_ctx::X12_LM, down = role == omchat_ctx::X12_DOWN;
  const size_t N = lm ? c.t_vocab : down ? H : 2 * (size_t)It, K = down ? It : H, n = lm ? 1 : L;
  const bool k_ok = K % 512 == 0 && (down ? (K > 4096 && K <= 32768) : K <= 4096);
  if (!k_ok || omchat_weights_missing(ctx) != 0) { if (!k_ok) T.state = omchat_ctx::W_UNAVAILABLE; return 0; }
  if (T.e.empty()) {
    std::vector<omchat_ctx::X12Ref> fresh(n);
    std::vector<void**> slots;
    std::vector<size_t> sizes;
    for (auto& r : fresh) {
      slots.push_back(&r.W); sizes.push_back(N * (K / 2 * 3));
      slots.push_back((void**)&r.top); sizes.push_back(N);
      slots.push_back((void**)&r.cnt); sizes.push_back(N);
      slots.push_back((void**)&r.patch); sizes.push_back(N * 32 * 4);
    }
    int* over = nullptr;
    if (!ctx->x12_over) { slots.push_back((void**)&over); sizes.push_back((size_t)std::max(L, 1) * 4); }
    if (ctx->alloc_group(slots, sizes)) { T.state = omchat_ctx::W_UNAVAILABLE; return 0; }      // stays 16-bit; nothing is retried
    if (over) ctx->x12_over = over;
    T.e.swap(fresh);
  }
  OM_HIP(hipDeviceSynchronize());      // as build_replica: whatever still writes the 16-bit weights, on any stream, is done before they are read
  OM_HIP(hipMemset(ctx->x12_over, 0, n * 4));
  for (size_t j = 0; j < n; ++j) {
    const void* W = lm ? ctx->lm_w(OMCHAT_WFMT_16).W : ctx->layer_w(OMCHAT_WFMT_16, (int)j)[down ? omchat_ctx::P_DOWN : omchat_ctx::P_GU].W;
    const omchat_ctx::X12Ref& r = T.e[j];
    TRY(launch_encode_bf16x12(W, (int)K, (int)N, (int)K, r.W, r.top, r.cnt, r.patch, ctx->x12_over + j, nullptr));
  }
  OM_HIP(hipDeviceSynchronize());      // (never inside a graph capture)
  std::vector<int> over(n);
  OM_HIP(hipMemcpy(over.data(), ctx->x12_over, n * 4, hipMemcpyDeviceToHost));
  bool moved = false;
  for (size_t j = 0; j < n; ++j) { moved = moved || (T.state == omchat_ctx::W_STALE && T.e[j].ok != !over[j]); T.e[j].ok = !over[j]; }
  if (moved) drop_decode_graphs(ctx);
  T.state = omchat_ctx::W_BUILT;
  return 0;
}

extern "C" int omchat_enable_fp8_decode(omchat_ctx* ctx, int on) {
  OM_CHECK(ctx, "null context");
  OM_CHECK(ctx->c.t_layers > 0, "context has no decoder");
  if (!on) { ctx->fp8_decode = false; return 0; }
  OM_CHECK(!ctx->mxfp4_mode, "MXFP4 decode is on: one weight format per step (omchat_enable_mxfp4_decode(ctx, 0) first)");
  OM_CHECK(!on || !ctx->pick.dola_on(), "fp8 decode: layer-contrastive decoding is on, and its head pass is 16-bit only (omchat_set_dola with b = 0 first)");
  TRY(build_replica(ctx, OMCHAT_WFMT_E4M3));
  ctx->fp8_decode = true;
  return 0;
}

// mode: 0 = off, 1 = batch-1 steps stream the MXFP4 replica, 2 = steps of 2 <= b <= 32 rows as well (the packed replica)
extern "C" int omchat_enable_mxfp4_decode(omchat_ctx* ctx, int mode) {
  OM_CHECK(ctx, "null context");
  OM_CHECK(ctx->c.t_layers > 0, "context has no decoder");
  OM_CHECK(mode >= 0 && mode <= 2, "mode: 0 = off, 1 = batch-1 steps, 2 = steps of up to 32 rows as well");
  if (!mode) { ctx->mxfp4_mode = 0; return 0; }
  OM_CHECK(!ctx->fp8_decode, "fp8 decode is on: one weight format per step (omchat_enable_fp8_decode(ctx, 0) first)");
  OM_CHECK(!mode || !ctx->pick.dola_on(), "MXFP4 decode: layer-contrastive decoding is on, and its head pass is 16-bit only (omchat_set_dola with b = 0 first)");
  OM_CHECK(ctx->tp_size == 1, "MXFP4 decode under tensor parallelism is not implemented");
  if (mode == 2) {
    const omchat_config& c = ctx->c;
    OM_CHECK(c.t_hidden % 64 == 0 && ctx->t_qdim % 64 == 0 && c.t_mlp % 64 == 0,
             "MXFP4 decode mode 2: the packed path needs hidden_size, heads x 128 and intermediate_size each a multiple of 64");
    OM_CHECK(ctx->t_qkvdim % 16 == 0 && c.t_hidden % 16 == 0 && c.t_vocab % 16 == 0,
             "MXFP4 decode mode 2: the packed path needs the qkv width, hidden_size and vocab_size each a multiple of 16");
  }
  TRY(build_replica(ctx, mode == 2 ? OMCHAT_WFMT_MXFP4_PACKED : OMCHAT_WFMT_MXFP4));
  ctx->mxfp4_mode = mode;
  return 0;
}

extern "C" int omchat_enable_fp8_kv(omchat_ctx* ctx, int on) {
  OM_CHECK(ctx, "null context");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  ctx->kv8_valid = false;            // takes effect with the next prefill
  if (!on) { ctx->fp8_kv = false; return 0; }
  if (!ctx->k8cache) {
    const size_t bytes = (size_t)c.t_layers * ctx->cache_layer_stride();
    const size_t sc = (size_t)c.t_layers * ctx->scale_layer_stride() * 4;
    TRY(ctx->alloc(&ctx->k8cache, bytes)); TRY(ctx->alloc(&ctx->v8cache, bytes));
    TRY(ctx->alloc((void**)&ctx->ks8, sc)); TRY(ctx->alloc((void**)&ctx->vs8, sc));
  }
  ctx->fp8_kv = true;
  return 0;
}

extern "C" int omchat_enable_fp8_prefill(omchat_ctx* ctx, int on) {
  OM_CHECK(ctx, "null context");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  if (!on) { ctx->fp8_prefill = false; return 0; }
  OM_CHECK(c.t_hidden % 128 == 0, "fp8 x fp8 prefill GEMMs need hidden_size % 128 == 0");
  TRY(build_replica(ctx, OMCHAT_WFMT_E4M3));
  if (!ctx->tw_q8) {
    const size_t R = std::max<size_t>(32, (size_t)(c.max_prefill_rows > c.max_batch ? c.max_prefill_rows : c.max_batch));
    TRY(ctx->alloc(&ctx->tw_q8, R * c.t_hidden));
    TRY(ctx->alloc((void**)&ctx->tw_q8s, R * 4));
  }
  ctx->fp8_prefill = true;
  return 0;
}


extern "C" int omchat_lm_head(omchat_ctx* ctx, const void* hidden, int n, float* logits, void* stream) {
  OM_CHECK(ctx && hidden && logits, "null argument");
  OM_CHECK(ctx->c.t_layers > 0, "context has no decoder");
  return lm_head_rows(ctx, hidden, n, logits, (hipStream_t)stream, ctx->lm_w(OMCHAT_WFMT_16));
}
// Teacher-forced scoring: a pure function of `hidden` -- no cache, position or pick state is read or written
extern "C" int omchat_score_hidden(omchat_ctx* ctx, const void* hidden, int rows, const int32_t* labels, int b, int S, float* logprob, float* out,
                                   void* stream) {
  OM_CHECK(ctx && hidden && labels && logprob && out, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(ctx->tp_size == 1, "scoring under tensor parallelism is not implemented: the lm_head is vocabulary-parallel and no exchange of the (max, sum) partials is built");
  OM_CHECK(omchat_weights_missing(ctx) == 0, "scoring needs the weights: " + std::string(omchat_last_error()));
  OM_CHECK(rows >= 1 && rows <= c.max_prefill_rows, "rows exceeds max_prefill_rows");
  OM_CHECK(b >= 1 && S >= 1 && (int64_t)b * S == rows, "b * S != rows");
  TRY(ctx->grow(ctx->score_ws, score_ws_bytes(rows, c.t_vocab)));      // before anything is enqueued
  hipStream_t s = (hipStream_t)stream;
  const omchat_ctx::WRef& lm = ctx->lm_w(OMCHAT_WFMT_16);
  TRY(launch_score(ctx->dt, hidden, c.t_hidden, lm.W, lm.ldw, rows, c.t_vocab, c.t_hidden, labels, logprob, nullptr, ctx->score_ws.p, ctx->score_ws.cap, s));
  return launch_score_reduce(logprob, labels, b, S, out, s);
}

// Attention form of omchat_prefill_extend (measured with tools/bench_extend.py, LOG.md).  The prefill kernel issues
// wgs = cdiv(S, 32) * kv_heads workgroups, each walking all keys serially: its time does not fall with S while wgs <= CUs (28 / 4 heads, bf16,
// S = 16 .. 1024: 99 us at 3.6 k keys, 212 at 8 k, 838 at 33 k).  The split-KV block attention reads the keys once per 16-row chunk and grows
// with S (3.6 k keys: 18 / 28 / 50 / 122 us at S = 16 / 64 / 256 / 1024; 33 k keys: 39 / 76 / 237 / 738): it wins by 2 - 20 x up to a quarter
// of the CUs' worth of query blocks, at half of them only where the key range is long enough to amortise its partials (S = 1024: 122 vs 97 us
// at 3.6 k keys, 217 vs 212 at 8 k, 738 vs 838 at 33 k), and loses beyond (S = 4096: 671 vs 365 us at 8 k keys).  keep = 0 is omchat_prefill's
// launch, always.
int g_extend_attn = -1;      // omchat_op_set_tuning key 49: attention form of omchat_prefill_extend for keep > 0: -1 = by the rule below, 0 = prefill kernel, 1 = split-KV (A/B)
void model_set_extend_attn(int v) { g_extend_attn = v; }
static bool extend_attn_split(int S, int keep, int kv_heads) {
  if (keep <= 0 || kv_heads <= 0) return false;
  if (g_extend_attn >= 0) return g_extend_attn != 0;
  const long wgs = (long)cdiv(S, 32) * kv_heads;
  if (4 * wgs <= device_cus()) return true;
  return 2 * wgs <= device_cus() && keep + S >= 16384;
}
extern "C" int omchat_extend_attn_form(int S_new, int keep, int Hkv) { return extend_attn_split(S_new, keep, Hkv) ? 1 : 0; }

// Attention form of omchat_prefill_suffixes.  Over forked rows both the suffix kernel (launch_attn_block ATTN_SUFFIX: the leader's
// prompt keys once per 16 flat query rows) and the batched prefill kernel with q_pos0 = keep (every row walks its own copy) are correct; over
// a shared prompt only the first is.  Measured alone with tools/bench_suffix.py (28 / 4 heads, bf16, 3584 prompt keys, 32-token suffixes; LOG.md): the
// suffix kernel + merge 34 / 59 / 97 us at N = 4 / 8 / 16, the prefill kernel 103 - 104 us at all three (its cdiv(S, 32) kv_heads N workgroups walk
// every key serially and fit the GPU) -- so the suffix kernel is the default at every N; longer suffixes and N > 16 were not measured.
int g_suffix_attn = -1;      // omchat_op_set_tuning key 51: attention form of omchat_prefill_suffixes over forked rows: -1 = by the rule, 0 = prefill kernel, 1 = suffix kernel (A/B)
void model_set_suffix_attn(int v) { g_suffix_attn = v; }
static bool suffix_attn_kernel(bool shared, int n_rep) {
  if (shared) return true;
  if (n_rep > 8) return false;
  return g_suffix_attn != 0;
}

// keep > 0 (omchat_prefill_extend, b = 1, right-aligned): the S rows sit at positions keep .. keep + S - 1 on top of keep cached slots
// sfx (omchat_prefill_suffixes): b sibling rows that each hold keep slots of one prompt (forked copies, or shared: only row 0 holds them);
// row i's lengths[i] suffix rows sit at positions keep .. on top of them, its padding rows leave the cache alone, and a group stays on
static int prefill_impl(omchat_ctx* ctx, const void* embeds, int b, int S, const int32_t* lengths, float* logits_last, void* hidden_out,
                        void* stream, bool left, int keep = 0, bool sfx = false) {
  OM_CHECK(ctx && embeds && lengths, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(b >= 1 && b <= c.max_batch, "batch exceeds max_batch");
  OM_CHECK(S >= 1 && keep + S <= c.max_seq, "sequence exceeds max_seq");
  OM_CHECK((int64_t)b * S <= c.max_prefill_rows, "b * S exceeds max_prefill_rows");
  OM_CHECK(omchat_weights_missing(ctx) == 0, std::string(omchat_last_error()));
  for (int i = 0; i < b; ++i) OM_CHECK(lengths[i] >= 1 && lengths[i] <= S, "lengths must be in [1, S]");
  // layer-contrastive decoding: the first generated id comes from this prefill, so it keeps the candidate layers' last rows too
  const PickState::Dola& D = ctx->pick.dola;
  const bool dola = D.on && logits_last;
  if (dola) {
    OM_CHECK(!left, "layer-contrastive decoding is on: a left-padded batch decodes with the masked step, which has no candidate rows (omchat_set_dola with b = 0 first)");
    OM_CHECK(keep == 0 && !sfx, "layer-contrastive decoding is on: prefill_extend and the suffix pass are not implemented with it (omchat_set_dola with b = 0 first)");
    OM_CHECK(b == D.b, "layer-contrastive decoding is on: a prefill takes exactly the b rows omchat_set_dola was given");
    if (const char* why = dola_state_refusal(ctx)) OM_CHECK(false, why);
  }
  // contrastive search: the b = 1 prefill keeps the post-final-norm rows of all its positions as the history
  const bool cs = ctx->contrastive_on();
  if (cs) {
    OM_CHECK(!left && keep == 0 && !sfx, "contrastive search is on: a left-padded prefill, prefill_extend and the suffix pass are not implemented with it (omchat_set_contrastive with k = 0 first)");
    OM_CHECK(b == 1, "contrastive search is on: a prefill takes exactly one row (omchat_set_contrastive with k = 0 first)");
    TRY(contrastive_prefill_admit(ctx, lengths[0]));
  }
  hipStream_t s = (hipStream_t)stream;
  if (ctx->fp8_prefill) TRY(build_replica(ctx, OMCHAT_WFMT_E4M3));      // weights were reloaded: re-quantise in place
  const int H = c.t_hidden, It = c.t_mlp, rows = b * S, qkvd = ctx->t_qkvdim, qd = ctx->t_qdim;
  const bool lead = ctx->tp_rank == 0;

  const bool split_attn = !sfx && extend_attn_split(S, keep, c.t_kv_heads) && c.t_heads / c.t_kv_heads <= 8;
  const bool sfx_attn = sfx && suffix_attn_kernel(ctx->group.on(), c.t_heads / c.t_kv_heads);
  if (sfx_attn) TRY(ctx->grow(ctx->ext_ws, attn_suffix_ws_bytes(b, S, c.t_heads, c.t_kv_heads, keep)));      // before anything is enqueued
  if (split_attn) TRY(ctx->grow(ctx->ext_ws, attn_extend_ws_bytes(S, c.t_heads, c.t_kv_heads, keep)));      // before anything is enqueued
  std::vector<int> pos(b), len1(b), klen(b), kstart(b);
  // left-padded batch (omchat_arch.py:176-184): row i holds its n_i tokens at [S - n_i, S); the reference drops position_ids
  // (:206-207), so RoPE runs on arange(S) for every row, the padded keys are masked, and every row's last token sits at S - 1
  for (int i = 0; i < b; ++i) {
    ctx->h_len[i] = left ? 0 : keep + lengths[i];            // 0 = no decode after a left-padded prefill (see omchat_decode_step)
    pos[i] = keep + lengths[i]; len1[i] = keep + lengths[i] + 1;
    klen[i] = left ? S : keep + lengths[i]; kstart[i] = left ? S - lengths[i] : 0;
  }
  ctx->left_padded = left;
  ctx->pre_S = keep + S; ctx->pre_b = b; ctx->masked_steps = 0; ctx->dec_mode = 0; ctx->mask_on_device = false;
  ctx->pick.smp_vcommit = 0;      // the slots of a sampled verify step's picks are gone: omchat_kv_rewind's one-step rule holds again
  // d_len holds the valid key range end during prefill; switched to (len + 1, pos = len) for the decode steps at the end
  OM_HIP(hipMemcpyAsync(ctx->d_len, klen.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));
  if (left) OM_HIP(hipMemcpyAsync(ctx->d_start, kstart.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));

  void* x = ctx->tw_x;
  void* y = ctx->tw_x2;
  OM_HIP(hipMemcpyAsync(x, embeds, (size_t)rows * H * 2, hipMemcpyDeviceToDevice, s));
  // HF's hidden_states index h (0 = the embeddings, h = behind decoder layer h) is a candidate: keep the rows' last positions
  auto dola_keep = [&](int h) -> int {
    const int j = dola ? D.slot(h) : -1;
    return j < 0 ? 0 : launch_gather_rows(ctx->dt, ctx->d_idx, x, nullptr, dola_slot(ctx, j), b, H, s);
  };
  if (dola) {
    hipLaunchKernelGGL(last_row_index_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, ctx->d_len, S, b, ctx->d_idx, keep);
    TRY(dola_keep(0));
  }
  // sequence-parallel norms (gemm_sp): not with the fp8 prefill (its norm writes e4m3 + scales) nor with fp32 partial sums (tuning key 29)
  const bool sp = g_tp_sp && ctx->tp_size > 1 && !g_tp_f32 && !(ctx->fp8_prefill && ctx->built(OMCHAT_WFMT_E4M3));
  for (int i = 0; i < c.t_layers; ++i) {
    auto& L = ctx->dl[i];
    char* kc = (char*)ctx->kcache + (size_t)i * ctx->cache_layer_stride() * 2;
    char* vc = (char*)ctx->vcache + (size_t)i * ctx->cache_layer_stride() * 2;
    // Qwen2DecoderLayer.forward (modeling_qwen2.py:269-298)
    const bool f8p = ctx->fp8_prefill && ctx->built(OMCHAT_WFMT_E4M3);
    const omchat_ctx::WRef* W8 = f8p ? ctx->layer_w(OMCHAT_WFMT_E4M3, i) : nullptr;
    // fp8 x fp8 MFMA for the two column-parallel GEMMs (BASELINE configs[4]): the RMSNorm writes e4m3 + one scale per token, the
    // weights are the e4m3 replica with one scale per output row; o_proj / down_proj keep the 16-bit operands
    auto gemm_f8 = [&](const omchat_ctx::WRef& w, void* Cb, int ldc, int N, const void* bias, int epi) -> int {
      GemmArgs g{ctx->tw_q8, H, w.W, H, Cb, ldc, rows, N, H, bias, nullptr, nullptr, 0, epi, 0, nullptr, 0, -1, 1, ctx->tw_q8s, w.w_scale};
      return launch_gemm(ctx->dt, g, s);
    };
    if (f8p) {
      TRY(launch_rmsnorm_q8(ctx->dt, x, H, L.ln1, ctx->tw_q8, H, ctx->tw_q8s, rows, H, c.t_eps, s));
      TRY(gemm_f8(W8[omchat_ctx::P_QKV], ctx->tw_qkv, qkvd, qkvd, L.bqkv, EPI_NONE));
    } else {
      if (!sp || i == 0) TRY(launch_rmsnorm(ctx->dt, x, H, L.ln1, ctx->tw_xn, H, rows, H, c.t_eps, s));      // (sequence-parallel: down_proj of layer i - 1 left it)
      if (sp) TRY(gemm_after_sp(ctx, ctx->tw_xn, H, L.wqkv, H, ctx->tw_qkv, qkvd, rows, qkvd, H, L.bqkv, EPI_NONE, s));
      else TRY(gemm(ctx, ctx->tw_xn, H, L.wqkv, H, ctx->tw_qkv, qkvd, rows, qkvd, H, L.bqkv, nullptr, nullptr, 0, EPI_NONE, s));
    }
    RopeArgs r{ctx->tw_qkv, qkvd, rows, S, c.t_heads, c.t_kv_heads, nullptr, keep, ctx->rope, c.max_seq, kc, vc, ctx->cache_sb(), ctx->cache_sh()};
    if (sfx) r.kv_end = ctx->d_len;      // (keep + lengths[i] at this point)
    TRY(launch_rope_kv(ctx->dt, r, s));
    if (sfx_attn || split_attn) {      // split_attn: few new rows over many cached keys, the keys split across workgroups (ATTN_EXTEND)
      AttnBlockArgs e{};
      ctx->bind_attn(e, i, false);
      e.ws = (float*)ctx->ext_ws.p; e.ws_bytes = ctx->ext_ws.cap;
      e.S = S;
      if (sfx_attn) { e.mode = ATTN_SUFFIX; e.N = b; e.P = keep; e.kv_len = ctx->d_len; }
      else { e.mode = ATTN_EXTEND; e.L = keep; }
      TRY(launch_attn_block(ctx->dt, e, s));
    }
    AttnArgs a{};
    a.Q = ctx->tw_qkv; a.q_sb = (int64_t)S * qkvd; a.q_sh = 128; a.q_sr = qkvd;
    a.K = kc; a.k_sb = ctx->cache_sb(); a.k_sh = ctx->cache_sh(); a.k_sr = 128;
    a.V = vc; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = 128;
    a.O = ctx->tw_ao; a.o_sb = (int64_t)S * qd; a.o_sh = 128; a.o_sr = qd;
    a.batch = b; a.q_heads = c.t_heads; a.kv_heads = c.t_kv_heads; a.Sq = S; a.Skv = keep + S; a.kv_len = ctx->d_len; a.causal = 1; a.q_pos0 = keep;
    a.kv_start = left ? ctx->d_start : nullptr;
    a.scale = omchat_ctx::T_ATTN_SCALE;
    if (!split_attn && !sfx_attn) TRY(launch_attn_prefill(ctx->dt, a, s));
    // left-padded batch: a padded query row sees no key at all; the reference's eager attention (the CPU path) then attends EVERY key of
    // the sequence with weight 1 / S (all scores are finfo.min -> softmax uniform, future keys included), and these rows' K / V in the
    // next layers are what a masked decode step exposes (omchat_arch.py:61-70).  The flash kernel leaves exactly 0 there; fill them.
    if (left && ctx->tp_size == 1) TRY(launch_attn_uniform_rows(ctx->dt, a, s));
    if (ctx->tp_size == 1) {
      TRY(gemm(ctx, ctx->tw_ao, qd, L.wo, qd, x, H, rows, H, qd, nullptr, nullptr, x, H, EPI_RESID, s));
    } else if (sp) {
      TRY(gemm_sp(ctx, ctx->tw_ao, qd, L.wo, qd, y, x, H, rows, qd, nullptr, nullptr, EPI_RESID, L.ln2, nullptr, ctx->tw_xn, c.t_eps, s));
    } else {
      TRY(gemm_allreduce(ctx, ctx->tw_ao, qd, L.wo, qd, y, H, rows, qd, nullptr, nullptr, x, EPI_RESID, s));
      std::swap(x, y);
    }
    if (f8p) TRY(launch_rmsnorm_q8(ctx->dt, x, H, L.ln2, ctx->tw_q8, H, ctx->tw_q8s, rows, H, c.t_eps, s));
    else if (!sp) TRY(launch_rmsnorm(ctx->dt, x, H, L.ln2, ctx->tw_xn, H, rows, H, c.t_eps, s));
    ctx->prof_mark(OMCHAT_PROF_PREFILL_GATEUP, s);
    if (f8p) TRY(gemm_f8(W8[omchat_ctx::P_GU], ctx->tw_act, It, 2 * It, nullptr, EPI_SWIGLU));
    else if (sp) TRY(gemm_after_sp(ctx, ctx->tw_xn, H, L.wgu, H, ctx->tw_act, It, rows, 2 * It, H, nullptr, EPI_SWIGLU, s));
    else TRY(gemm(ctx, ctx->tw_xn, H, L.wgu, H, ctx->tw_act, It, rows, 2 * It, H, nullptr, nullptr, nullptr, 0, EPI_SWIGLU, s));
    ctx->prof_mark(OMCHAT_PROF_PREFILL_GATEUP, s);
    if (ctx->tp_size == 1) {
      TRY(gemm(ctx, ctx->tw_act, It, L.wd, It, x, H, rows, H, It, nullptr, nullptr, x, H, EPI_RESID, s));
    } else if (sp) {
      const bool more = i + 1 < c.t_layers;
      TRY(gemm_sp(ctx, ctx->tw_act, It, L.wd, It, y, x, H, rows, It, nullptr, nullptr, EPI_RESID, more ? ctx->dl[i + 1].ln1 : nullptr, nullptr, ctx->tw_xn, c.t_eps, s));
      if (!more) TRY(sp_gather_x(ctx, x, H, rows, s));
    } else {
      TRY(gemm_allreduce(ctx, ctx->tw_act, It, L.wd, It, y, H, rows, It, nullptr, nullptr, x, EPI_RESID, s));
      std::swap(x, y);
    }
    TRY(dola_keep(i + 1));
  }
  TRY(sp_drain(ctx, s));
  if (hidden_out) TRY(launch_rmsnorm(ctx->dt, x, H, ctx->t_norm, hidden_out, H, rows, H, c.t_eps, s));
  if (cs) TRY(contrastive_prefill_keep(ctx, x, lengths[0], s));
  if (dola) {
    TRY(launch_gather_rows(ctx->dt, ctx->d_idx, x, nullptr, ctx->tw_last, b, H, s));
    TRY(dola_head(ctx, ctx->tw_last, logits_last, s));
  } else if (logits_last) {
    // only the last valid position feeds generation (Qwen2ForCausalLM.forward :462-465 projects all; same values)
    hipLaunchKernelGGL(last_row_index_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, ctx->d_len, S, b, ctx->d_idx, keep);
    TRY(launch_gather_rows(ctx->dt, ctx->d_idx, x, nullptr, ctx->tw_last, b, H, s));
    TRY(launch_rmsnorm(ctx->dt, ctx->tw_last, H, ctx->t_norm, ctx->tw_last, H, b, H, c.t_eps, s));
    TRY(lm_head_rows(ctx, ctx->tw_last, b, logits_last, s, ctx->lm_w(OMCHAT_WFMT_16)));
  }
  ctx->kv8_valid = false;
  ctx->beam.end();         // a prefill ends any beam search
  if (!sfx) ctx->group.end();        // ... and the shared-prompt mode of a sampled group (the suffix pass runs inside it)
  if (ctx->fp8_kv) {      // fp8 KV cache for the decode steps: quantise what this prefill wrote -- ALL S slots of every row: the masked decode
                          // of a padded batch exposes padded slots too (omchat_arch.py:61-70), and the per-sequence step overwrites them as it appends
    for (int i = 0; i < c.t_layers; ++i) {
      const size_t off = (size_t)i * ctx->cache_layer_stride(), so = (size_t)i * ctx->scale_layer_stride();
      TRY(launch_kv_quant(ctx->dt, (char*)ctx->kcache + off * 2, (char*)ctx->vcache + off * 2, (char*)ctx->k8cache + off, (char*)ctx->v8cache + off,
                          ctx->ks8 + so, ctx->vs8 + so, b, c.t_kv_heads, ctx->cache_sb(), ctx->cache_sh(), (int64_t)c.t_kv_heads * c.max_seq, c.max_seq,
                          nullptr, 0, nullptr, S, s));
    }
    ctx->kv8_valid = true;
  }
  OM_HIP(hipMemcpyAsync(ctx->d_pos, pos.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(ctx->d_len, len1.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipStreamSynchronize(s));     // pos/len1 are stack vectors
  return 0;
}

extern "C" int omchat_prefill(omchat_ctx* ctx, const void* embeds, int b, int S, const int32_t* lengths, float* logits_last, void* hidden_out,
                              void* stream) {
  return prefill_impl(ctx, embeds, b, S, lengths, logits_last, hidden_out, stream, false);
}

extern "C" int omchat_prefill_left(omchat_ctx* ctx, const void* embeds, int b, int S, const int32_t* lengths, float* logits_last,
                                   void* hidden_out, void* stream) {
  return prefill_impl(ctx, embeds, b, S, lengths, logits_last, hidden_out, stream, true);
}

extern "C" int omchat_prefill_extend(omchat_ctx* ctx, const void* embeds, int S_new, int keep, float* logits_last, void* hidden_out, void* stream) {
  OM_CHECK(ctx, "null argument");
  OM_CHECK(S_new >= 1, "prefill_extend: S_new < 1");
  OM_CHECK(embeds, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(ctx->tp_size == 1, "prefill_extend: tensor-parallel contexts are not implemented (DESIGN.md section 7)");
  OM_CHECK(!ctx->pick.dola_on(), "prefill_extend: layer-contrastive decoding is on (omchat_set_dola with b = 0 first); the kept slots' candidate rows are gone");
  OM_CHECK(!ctx->contrastive_on(), "prefill_extend: contrastive search is on (omchat_set_contrastive with k = 0 first); the kept slots' hidden rows are gone");
  OM_CHECK(!ctx->fp8_kv, "prefill_extend: the e4m3 KV cache is not implemented (DESIGN.md section 7): omchat_enable_fp8_kv(ctx, 0)");
  OM_CHECK(!ctx->fp8_prefill, "prefill_extend: fp8 x fp8 prefill GEMMs are not implemented (DESIGN.md section 7): omchat_enable_fp8_prefill(ctx, 0)");
  OM_CHECK(!ctx->left_padded, "prefill_extend: the cache holds a left-padded batch");
  OM_CHECK(ctx->dec_mode != 2, "prefill_extend: the cache holds a masked-decode (padded batch) state");
  OM_CHECK(!ctx->beam.on(), "prefill_extend: a beam search is active");
  OM_CHECK(!ctx->group.on(), "prefill_extend: a sampled group shares its prompt (omchat_group_begin with b = 0 first): sequence 0 has sibling rows");
  OM_CHECK(ctx->pre_b >= 1 && ctx->h_len[0] >= 1, "prefill_extend: no live sequence-0 state (omchat_prefill with b = 1 first)");
  OM_CHECK(ctx->pre_b == 1, "prefill_extend: the cache holds a b > 1 state");
  OM_CHECK(keep >= 0 && keep <= ctx->h_len[0], "prefill_extend: keep outside [0, current length]");
  OM_CHECK(S_new <= c.max_prefill_rows, "prefill_extend: S_new > max_prefill_rows");
  OM_CHECK((int64_t)keep + S_new <= c.max_seq, "prefill_extend: keep + S_new > max_seq");
  const int32_t len = S_new;
  return prefill_impl(ctx, embeds, 1, S_new, &len, logits_last, hidden_out, stream, false, keep);
}

extern "C" int omchat_suffix_attn_form(int shared, int n_rep) { return suffix_attn_kernel(shared != 0, n_rep) ? 1 : 0; }

extern "C" int omchat_prefill_suffixes(omchat_ctx* ctx, const void* embeds, int N, int S_max, const int32_t* lengths, int keep, float* logits_last,
                                       void* hidden_out, void* stream) {
  OM_CHECK(ctx && embeds && lengths, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(ctx->tp_size == 1, "prefill_suffixes: tensor-parallel contexts are not implemented (DESIGN.md section 7)");
  OM_CHECK(!ctx->pick.dola_on(), "prefill_suffixes: layer-contrastive decoding is on (omchat_set_dola with b = 0 first); the suffix pass keeps no candidate rows");
  OM_CHECK(!ctx->contrastive_on(), "prefill_suffixes: contrastive search is on (omchat_set_contrastive with k = 0 first); the suffix pass keeps no history rows");
  OM_CHECK(!ctx->fp8_kv, "prefill_suffixes: the e4m3 KV cache is not implemented (DESIGN.md section 7): omchat_enable_fp8_kv(ctx, 0)");
  OM_CHECK(!ctx->fp8_prefill, "prefill_suffixes: fp8 x fp8 prefill GEMMs are not implemented (DESIGN.md section 7): omchat_enable_fp8_prefill(ctx, 0)");
  OM_CHECK(!ctx->left_padded && ctx->dec_mode != 2, "prefill_suffixes: the cache holds a left-padded or masked-decode (padded batch) state");
  OM_CHECK(!ctx->beam.on(), "prefill_suffixes: a beam search is active");
  OM_CHECK(N >= 1 && N <= c.max_batch, "prefill_suffixes: N outside [1, max_batch]");
  OM_CHECK(S_max >= 1, "prefill_suffixes: S_max < 1");
  for (int j = 0; j < N; ++j) OM_CHECK(lengths[j] >= 1 && lengths[j] <= S_max, "prefill_suffixes: lengths must be in [1, S_max]");
  OM_CHECK((int64_t)N * S_max <= c.max_prefill_rows, "prefill_suffixes: N * S_max > max_prefill_rows");
  OM_CHECK((int64_t)N * S_max <= 65535, "prefill_suffixes: N * S_max > 65535 query rows");
  OM_CHECK(keep >= 1, "prefill_suffixes: keep < 1 (no prompt to share: omchat_prefill)");
  OM_CHECK((int64_t)keep + S_max <= c.max_seq, "prefill_suffixes: keep + S_max > max_seq");
  const GroupState& G = ctx->group;
  OM_CHECK(ctx->pre_b >= 1, "prefill_suffixes: no live state (omchat_prefill with b = 1, then omchat_group_begin(ctx, 1, N, keep, share))");
  for (int j = 0; j < N; ++j)
    OM_CHECK(ctx->h_len[j] == keep, "prefill_suffixes: rows 0 .. N - 1 must each hold exactly keep slots (omchat_group_begin(ctx, 1, N, keep, share) first)");
  OM_CHECK(!G.on() || (G.b == 1 && G.N == N && G.P == keep), "prefill_suffixes: the shared-prompt group is not one prompt of keep slots with N rows");
  OM_CHECK(!G.on() || c.t_heads / c.t_kv_heads <= 8, "prefill_suffixes: the suffix attention takes at most 8 query heads per kv head (share = 0)");
  return prefill_impl(ctx, embeds, N, S_max, lengths, logits_last, hidden_out, stream, false, keep, true);
}

// omchat_kv_read for a cache row other than 0 (tests of the sibling rows of a group)
extern "C" int omchat_kv_read_row(omchat_ctx* ctx, int row, int layer, int which, int pos0, int n, void* out, void* stream) {
  OM_CHECK(ctx && out, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(row >= 0 && row < c.max_batch && layer >= 0 && layer < c.t_layers && (which == 0 || which == 1) && pos0 >= 0 && n >= 1 && pos0 + n <= c.max_seq,
           "bad argument");
  const char* src = (const char*)(which ? ctx->vcache : ctx->kcache) +
                    ((size_t)layer * ctx->cache_layer_stride() + (size_t)row * ctx->cache_sb() + (size_t)pos0 * 128) * 2;
  OM_HIP(hipMemcpy2DAsync(out, (size_t)n * 256, src, (size_t)ctx->cache_sh() * 2, (size_t)n * 256, (size_t)c.t_kv_heads, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  return 0;
}

extern "C" int omchat_kv_read(omchat_ctx* ctx, int layer, int which, int pos0, int n, void* out, void* stream) {
  OM_CHECK(ctx && out, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(layer >= 0 && layer < c.t_layers && (which == 0 || which == 1) && pos0 >= 0 && n >= 1 && pos0 + n <= c.max_seq, "bad argument");
  const char* src = (const char*)(which ? ctx->vcache : ctx->kcache) + ((size_t)layer * ctx->cache_layer_stride() + (size_t)pos0 * 128) * 2;
  OM_HIP(hipMemcpy2DAsync(out, (size_t)n * 256, src, (size_t)ctx->cache_sh() * 2, (size_t)n * 256, (size_t)c.t_kv_heads, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  return 0;
}

// The weight format of a decode step and the packed-x block count of its GEMVs: the whole rule (include/omchat_hip.h states it)
extern "C" int omchat_decode_weight_format(int rows, int fp8_on, int mxfp4_mode, int packed16_ready, int geometry_ok, int* x_pack_nb) {
  const bool batched = rows >= 2 && rows <= 32;
  const int nb = batched && geometry_ok ? (rows > 16 ? 2 : 1) : 0;
  if (x_pack_nb) *x_pack_nb = nb;
  if (rows == 1) return fp8_on ? OMCHAT_WFMT_E4M3 : mxfp4_mode >= 1 ? OMCHAT_WFMT_MXFP4 : OMCHAT_WFMT_16;
  if (batched && mxfp4_mode == 2) return OMCHAT_WFMT_MXFP4_PACKED;      // (nb == 0: refused at enable time, and by the step)
  return nb && packed16_ready ? OMCHAT_WFMT_16_PACKED : OMCHAT_WFMT_16;
}
// ... of a step of `rows` rows on this context; assume_packed16: as if the 16-bit packed replica were ready (does the step want it built?)
static int step_format(const omchat_ctx* ctx, int rows, int* x_pack_nb = nullptr, bool assume_packed16 = false) {
  const omchat_config& c = ctx->c;
  return omchat_decode_weight_format(rows, ctx->fp8_decode, ctx->mxfp4_mode, assume_packed16 || ctx->built(OMCHAT_WFMT_16_PACKED),
                                     c.t_hidden % 64 == 0 && ctx->t_qdim % 64 == 0 && c.t_mlp % 64 == 0, x_pack_nb);
}
int decode_x_pack_nb(const omchat_ctx* ctx, int rows) { int nb = 0; (void)step_format(ctx, rows, &nb); return nb; }
static bool is_mxfp4(int fmt) { return fmt == OMCHAT_WFMT_MXFP4 || fmt == OMCHAT_WFMT_MXFP4_PACKED; }

// Every replica a step of `rows` rows may stream is built and current -- called by the step entries before pick_admit, before any
// host-to-device copy and before anything is enqueued (a failure must leave nothing in flight).
//  - the 16-bit packed replica is built by the first step whose format wants it (and re-packed after a weight reload), unless tuning key 6 = 0,
//    the geometry is odd (stay on the row-major weights) or it did not fit before
//  - an enabled replica that omchat_load_tensor left stale is rebuilt IN PLACE (same device pointers: a captured graph replays the fresh bytes)
static int step_weights_ready(omchat_ctx* ctx, int rows) {
  const omchat_config& c = ctx->c;
  if (step_format(ctx, rows, nullptr, true) == OMCHAT_WFMT_16_PACKED && g_pack_replica && ctx->wt[OMCHAT_WFMT_16_PACKED].state != omchat_ctx::W_UNAVAILABLE &&
      !(ctx->t_qkvdim % 16 || c.t_hidden % 16 || c.t_vocab % 16))
    TRY(build_replica(ctx, OMCHAT_WFMT_16_PACKED));
  if (ctx->fp8_decode) TRY(build_replica(ctx, OMCHAT_WFMT_E4M3));
  if (ctx->mxfp4_mode) TRY(build_replica(ctx, ctx->mxfp4_mode == 2 ? OMCHAT_WFMT_MXFP4_PACKED : OMCHAT_WFMT_MXFP4));
  const int x12m = x12_step_mask(ctx, rows, step_format(ctx, rows));      // built by the first batch-1 step that will use it
  for (int role = 0; role < omchat_ctx::X12_ROLES; ++role) if (x12m >> role & 1) TRY(build_x12(ctx, role));
  return 0;
}

// mode 2 of the MXFP4 decode: one weight format per generation, so a step that the packed forms cannot take (b > 32) is refused by the step
// entries before they touch any state or enqueue anything, never run on 16 bits
static const char* const MX4_ROWS_MSG = "MXFP4 decode mode 2 streams steps of at most 32 rows (omchat_enable_mxfp4_decode(ctx, 0 or 1) first)";
static bool mx4_rows_ok(const omchat_ctx* ctx, int rows) { return ctx->mxfp4_mode != 2 || is_mxfp4(step_format(ctx, rows)); }

// One decode step on stream s.  Lmax = upper bound of the key count (sizes the split-KV grid; the kernels read the true
// lengths from d_len).  Every argument is a context pointer or a step-invariant scalar when called for graph capture.
// exact_len: every sequence holds exactly Lmax keys after this step (eager launches only): the attention launches then take the length
// as a kernel argument instead of loading d_len first -- one dependent memory round trip less in two latency-bound launches per layer.
// vL >= 0: prompt-lookup verify step (omchat_decode_verify) -- the b rows are consecutive tokens of sequence 0 at positions vL .. vL + b - 1
// (multi-query attention, launch_attn_block ATTN_VERIFY), and next_tokens receives the greedy pick of every row without moving any position.
static int decode_body(omchat_ctx* ctx, const int32_t* tokens, int b, int Lmax, float* logits, int32_t* next_tokens, hipStream_t s, bool allow_prof,
                       bool exact_len = false, bool masked = false, int vL = -1, bool vsample = false) {
  const omchat_config& c = ctx->c;
  const int H = c.t_hidden, It = c.t_mlp, qkvd = ctx->t_qkvdim, qd = ctx->t_qdim;
  const bool lead = ctx->tp_rank == 0;
  void* x = ctx->tw_x;
  void* y = ctx->tw_x2;
  TRY(launch_gather_rows(ctx->dt, tokens, ctx->t_embed, nullptr, x, b, H, s));      // embed_tokens
  // layer-contrastive decoding (the step entries refused every other mode): the step's rows of the residual stream are kept at the candidate
  // layers -- HF's hidden_states index h: 0 = the embeddings, h = behind decoder layer h -- with a device-to-device copy, which a graph captures
  const PickState::Dola& D = ctx->pick.dola;
  const bool dola = D.on && vL < 0 && !masked;
  auto dola_keep = [&](int h) -> int {
    const int j = dola ? D.slot(h) : -1;
    if (j >= 0) OM_HIP(hipMemcpyAsync(dola_slot(ctx, j), x, (size_t)b * H * 2, hipMemcpyDeviceToDevice, s));
    return 0;
  };
  TRY(dola_keep(0));
  // One weight format per step (omchat_decode_weight_format): e4m3 or MXFP4 at b == 1 (under tensor parallelism every rank streams the e4m3
  // replica of its own shard), and on batched steps (2 <= b <= 32) the packed MXFP4 replica in mode 2, else the 16-bit packed one once it
  // exists.  pk: the activations that feed a GEMV of a batched step (tw_xn, tw_ao, tw_act) are produced in the packed x layout (common.h)
  // by their producers, in pk blocks of 16 rows.
  int pk = 0;
  const int fmt = step_format(ctx, b, &pk);
  OM_CHECK(fmt != OMCHAT_WFMT_MXFP4_PACKED || pk, "MXFP4 decode mode 2: geometry outside the packed path");
  const bool wq = fmt == OMCHAT_WFMT_E4M3 || is_mxfp4(fmt);      // a quantised replica is streamed: the launches that exist for 16-bit weights only stay out
  const bool wpk = fmt == OMCHAT_WFMT_16_PACKED, mpk = fmt == OMCHAT_WFMT_MXFP4_PACKED;
  using WRef = omchat_ctx::WRef;
  enum { QKV = omchat_ctx::P_QKV, O = omchat_ctx::P_O, GU = omchat_ctx::P_GU, DOWN = omchat_ctx::P_DOWN };
  auto gemv_args = [&](const void* X, int ldx, const WRef& W, int K, void* Y, int ldy, int R, int N, const void* bias, const void* resid, int epi,
                       int ks, bool ypk) {
    GemvArgs g{X, ldx, nullptr, 0, Y, ldy, R, N, K, bias, resid, H, epi, 0, ks};
    use_weight(g, W);
    if (pk) { g.x_packed = 1; g.y_packed = ypk && epi == EPI_SWIGLU; }
    return g;
  };
  auto gemv = [&](const void* X, int ldx, const WRef& W, int K, void* Y, int ldy, int N, const void* bias, const void* resid, int epi,
                  bool ypk = false) -> int {
    for (int r0 = 0; r0 < b; r0 += 32) {
      const int R = std::min(32, b - r0);
      const GemvArgs g = gemv_args((const char*)X + (size_t)r0 * ldx * 2, ldx, W, K, (char*)Y + (size_t)r0 * ldy * 2, ldy, R, N, bias,
                                   resid ? (const char*)resid + (size_t)r0 * H * 2 : nullptr, epi, 0, ypk);
      TRY(launch_gemv(ctx->dt, g, s));
    }
    return 0;
  };
  // split-K over workgroups: fp32 slices [ks][b][H], summed by the fused residual + RMSNorm kernel
  auto gemv_partial = [&](const void* X, int ldx, const WRef& W, int K, int ks) -> int {
    OM_CHECK(b <= 32, "split-K decode path handles b <= 32");
    const GemvArgs g = gemv_args(X, ldx, W, K, ctx->tw_part, H, b, H, nullptr, nullptr, EPI_PARTIAL, ks, false);
    TRY(launch_gemv(ctx->dt, g, s));
    // tensor parallelism: the slices hold this rank's partial sums; reduce_resid_rmsnorm sums them over the ranks in fp32 (<= 3 x 3584
    // floats at batch 1, latency-bound like any small message) together with the residual + RMSNorm, identically on every rank
    return 0;
  };
  const bool fused = b <= 32;
  // K slices of the two split-K projections (gemv_split_k, next to the launch plan they belong with)
  const int ks_o = gemv_split_k(b, qd, H, wpk || mpk, false, gemv_tuning()), ks_d = gemv_split_k(b, It, H, wpk || mpk, true, gemv_tuning());
  // batch 1, one GPU (round 3): the two residual + RMSNorm launches of a layer disappear.  o_proj and down_proj run without split-K and
  // write x + attn / x + mlp themselves (EPI_RESID, in place; down_proj's K = 18944 through gemv_rows_longk_kernel), and each RMSNorm runs
  // inside the projection that consumes it (gemv_rows_norm_kernel: qkv, gate|up, lm_head): six dependent launches per layer instead of
  // eight.  n2 = the post-attention norm (tuning key 14 bit 0), n1 = the input norm of the next layer / the final norm (bit 1).
  // (only while the whole-row GEMV form is in use: with tuning key 1 -- force the MFMA form -- the norm has no registers to live in and
  // the step keeps its residual + RMSNorm launches)
  // measurement only (experiments build, bench.py --shard-of N --tuning 35=1): a rank context whose exchanges are no-ops takes the ONE-GPU launch
  // structures on its shard widths -- what removing launches could buy a tensor-parallel rank if its two exchanges per layer were free
  const bool tp1_like = ctx->tp_size == 1 || (OMCHAT_EXPERIMENTS && g_shard_as_tp1 && ctx->hook == omchat_allreduce_noop);
  const bool n2 = (g_norm_in_gemv & 1) && fused && b == 1 && tp1_like && qd <= 4096 && H <= 4096 && !gemv_get_force_mfma();
  const bool n1 = n2 && (g_norm_in_gemv & 2) && It <= 32768 && It % 8 == 0;
  // batched steps on one GPU (round 5, key 14 bit 2; -DOMCHAT_EXPERIMENTS=1 builds only: measured slower, gemv.hip): o_proj un-split in the x-stationary form writes x + attn itself (row-major in place AND the
  // packed raw copy), and the post-attention RMSNorm runs in the registers of the gate|up GEMV: seven launches per layer instead of eight
  const bool nb2 = OMCHAT_EXPERIMENTS && (g_norm_in_gemv & 4) && fused && wpk && ctx->tp_size == 1 && !wq && (qd >> 6) == 56 && (H >> 6) == 56 && qd % 64 == 0 &&
                   H / 16 <= device_cus() && (2 * It) / 32 >= 4 * device_cus();
  // bf16x12 (tuning key 50): the three long launches of the six-launch layer stream the 12-bit coding of their rows where it is built and the
  // tensor is coded -- the same bits as the 16-bit launch, three quarters of the bytes
  const int x12m = n1 ? x12_step_mask(ctx, b, fmt) : 0;
  auto x12_of = [&](int role, size_t j) -> const omchat_ctx::X12Ref* {
    const omchat_ctx::X12Table& T = ctx->x12[role];
    return ((x12m >> role) & 1) && T.state == omchat_ctx::W_BUILT && T.e[j].ok ? &T.e[j] : nullptr;
  };
  if (fused && !n1) TRY(launch_rmsnorm(ctx->dt, x, H, ctx->dl[0].ln1, ctx->tw_xn, H, b, H, c.t_eps, s, pk));
#if OMCHAT_EXPERIMENTS
  if ((g_ao_oproj & 16) && ctx->dbg_stamps) OM_HIP(hipMemsetAsync(ctx->dbg_stamps, 0, (size_t)c.t_layers * 256, s));      // measurement: the stamps of THIS step only
#endif
  for (int i = 0; i < c.t_layers; ++i) {
    auto& L = ctx->dl[i];      // the norms and the bias
    const WRef* W = ctx->layer_w(fmt, i);                    // the four projections in the step's format
    const WRef* W16 = ctx->layer_w(OMCHAT_WFMT_16, i);       // ... and as 16-bit row-major, for the launches that exist for those only (!wq, b == 1)
    char* kc = (char*)ctx->kcache + (size_t)i * ctx->cache_layer_stride() * 2;
    char* vc = (char*)ctx->vcache + (size_t)i * ctx->cache_layer_stride() * 2;
    if (!fused) TRY(launch_rmsnorm(ctx->dt, x, H, L.ln1, ctx->tw_xn, H, b, H, c.t_eps, s));
    // batch 1, one GPU (round 4): the whole layer as ONE launch with in-launch hand-offs (decode_layer.hip; the same bits as the six
    // launches below).  Eager steps only: the launch is tagged with a per-launch counter, which a captured graph would freeze.
    if (g_decode_layer && !dola && n1 && exact_len && !masked && !wq && !(ctx->fp8_kv && ctx->kv8_valid) && ctx->dl_ws) {      // (the layer kernel has no key mask)
      DecodeLayerArgs d{L.ln1, L.ln2, W16[QKV].W, L.bqkv, W16[O].W, W16[GU].W, W16[DOWN].W, kc, vc, ctx->cache_sh(), x, H, qd, ctx->t_kvdim, It, c.t_heads, c.t_kv_heads, Lmax,
                        ctx->rope, c.max_seq, c.t_eps, omchat_ctx::T_ATTN_SCALE, ctx->dl_ws, ++ctx->fd_epoch, ctx->fd_err, 2000};
      if (decode_layer_ok(d)) {
        const bool mark_l = allow_prof && i == c.t_layers / 2;      // HIP-event bracket on one layer per token (bench.py roofline)
        if (mark_l) ctx->prof_mark(OMCHAT_PROF_DECODE_GATEUP, s);
        TRY(launch_decode_layer(ctx->dt, d, s));
        if (mark_l) ctx->prof_mark(OMCHAT_PROF_DECODE_GATEUP, s);
        ++ctx->n_layer_launches;
        continue;
      }
      --ctx->fd_epoch;
    }
    if (n1) {
      GemvArgs g = gemv_args(x, H, W[QKV], H, ctx->tw_qkv, qkvd, 1, qkvd, L.bqkv, nullptr, EPI_NONE, 0, false);
      g.norm_w = L.ln1; g.norm_eps = c.t_eps;
      if (OMCHAT_EXPERIMENTS && (g_ao_oproj & 16) && ctx->dbg_stamps) g.dbg = ctx->dbg_stamps + (size_t)i * 32;
      TRY(launch_gemv(ctx->dt, g, s));
    } else {
      TRY(gemv(ctx->tw_xn, H, W[QKV], H, ctx->tw_qkv, qkvd, qkvd, L.bqkv, nullptr, EPI_NONE));
    }
    // RoPE + KV append are fused into the attention kernel (q rotated in registers, the split that owns the new
    // position rotates k and appends k / v)
    AttnDecodeArgs a{};
    ctx->bind_attn(a, i, true);
    a.ws = ctx->tw_attn_ws; a.ws_bytes = ctx->tw_attn_ws_bytes;
    a.o_pack_nb = fused ? pk : 0;
    a.batch = b; a.L = Lmax; a.kv_len = exact_len ? nullptr : ctx->d_len; a.pos = ctx->d_pos;
    if (masked) { a.key_mask = ctx->d_mask; a.mask_sb = ctx->mask_sb; }      // d_pos holds the given RoPE positions, every row has Lmax keys
    if (ctx->fp8_kv && ctx->kv8_valid) {
      // fp8 KV cache: rotate q / k and append to the 16-bit cache with the prefill's kernel, quantise the new row, then attend over e4m3
      // keys and values (two small launches more per layer than the fused 16-bit path; this mode is for long contexts)
      // (round 3: the new row is quantised inside the RoPE + append launch -- one launch less per layer than rope_kv + kv_quant)
      const size_t off = (size_t)i * ctx->cache_layer_stride(), so = (size_t)i * ctx->scale_layer_stride();
      RopeArgs r{ctx->tw_qkv, qkvd, b, 1, c.t_heads, c.t_kv_heads, ctx->d_pos, 0, ctx->rope, c.max_seq, kc, vc, ctx->cache_sb(), ctx->cache_sh()};
      r.k8 = (char*)ctx->k8cache + off; r.v8 = (char*)ctx->v8cache + off; r.ks = ctx->ks8 + so; r.vs = ctx->vs8 + so;
      r.s_sb = (int64_t)c.t_kv_heads * c.max_seq; r.s_sh = c.max_seq;
      if (masked) r.slot0 = Lmax - 1;                              // padded batch: common cache slot, per-row RoPE positions from d_pos
      else if (exact_len) { r.pos = nullptr; r.pos0 = Lmax - 1; }      // the position by value: one dependent load less in front of the table read
      // round 6: from ~9 k keys on the attention launch walks its tiles and rotates / appends / quantises the new rows itself (the same bytes)
      if (attn_decode_kv8_fuses_rope(b, c.t_kv_heads, Lmax, masked)) { a.k16_w = kc; a.v16_w = vc; a.pos = nullptr; }
      else {
        TRY(launch_rope_kv(ctx->dt, r, s));
        a.rope = nullptr; a.pos = nullptr; a.k_new = nullptr; a.v_new = nullptr;
      }
      a.K = (char*)ctx->k8cache + off; a.V = (char*)ctx->v8cache + off;
      a.k_scale = ctx->ks8 + so; a.v_scale = ctx->vs8 + so; a.scale_sb = (int64_t)c.t_kv_heads * c.max_seq; a.scale_sh = c.max_seq;
    }
    // batch 1, one GPU (round 4): attention + merge + o_proj (+ residual) as ONE launch with in-launch hand-offs (fused_decode.hip; the same
    // bits as the three launches).  Eager steps only: the launch is tagged with a per-launch counter, which a captured graph would freeze.
    bool ao_oproj = false;
    const bool fuse_ao = g_fuse_attn_oproj && !dola && n2 && exact_len && !wq && a.rope && ctx->fd_ws && attn_oproj_fused_ok(a, H, qd);
    if (vL < 0 && ctx->group.on()) {
      // sampled group sharing its prompt (omchat_group_begin): the prompt keys once per group, each row's own keys per row; the lengths come
      // from the device, Lmax (the suffix bucket, omchat_decode_step) sizes the grid -- the same launch eager and captured
      const GroupState& G = ctx->group;
      AttnBlockArgs sa{};
      static_cast<AttnOperands&>(sa) = a;      // the step's binding (16-bit cache: omchat_decode_step refuses this mode over the e4m3 one)
      sa.ws = (float*)G.ws.p; sa.ws_bytes = G.ws.cap;
      sa.mode = ATTN_SHARED; sa.G = G.b; sa.N = G.N; sa.P = G.P; sa.L = Lmax; sa.kv_len = ctx->d_len;
      TRY(launch_attn_block(ctx->dt, sa, s));
    } else if (vL >= 0) {
      AttnBlockArgs va{};
      static_cast<AttnOperands&>(va) = a;      // ... as does omchat_decode_verify
      va.mode = ATTN_VERIFY; va.S = b; va.L = vL;
      TRY(launch_attn_block(ctx->dt, va, s));
    } else if (fuse_ao) {
      FusedDecodeArgs fa{W16[O].W, qd, x, H, qd, ctx->fd_ws, ++ctx->fd_epoch, ctx->fd_err, 2000};
      TRY(launch_attn_oproj_fused(ctx->dt, a, fa, s));
      ++ctx->n_fused_launches;
    } else {
#if OMCHAT_EXPERIMENTS
      // tuning key 42 (prototype): o_proj out of order behind the merge, which publishes per-head completion flags (fd_ws doubles as the flag words:
      // key 22 and key 42 are not meant to be on together)
      ao_oproj = (g_ao_oproj & 1) && n2 && !wq && !masked && ctx->fd_ws && Lmax <= 4096 && H == 3584 && qd == 3584 && c.t_heads <= 64 && !ctx->graph_on;
      if (ao_oproj) { a.done_flags = (unsigned*)ctx->fd_ws; a.done_epoch = ++ctx->fd_epoch; a.done_mode = g_ao_oproj; }
      if ((g_ao_oproj & 16) && n2 && ctx->dbg_stamps) a.done_dbg = ctx->dbg_stamps + (size_t)i * 32;
#endif
      TRY(launch_attn_decode(ctx->dt, a, s));
    }
    // batch 1, one GPU (round 3): o_proj without split-K writes x + attn itself (EPI_RESID, in place) and the post-attention RMSNorm runs
    // in the registers of the gate|up GEMV's waves (gemv.hip: norm_w): seven dependent launches per layer instead of eight
    if (fuse_ao) {
      // x + attn is already in place
    } else if (ao_oproj) {
      GemvArgs g = gemv_args(ctx->tw_ao, qd, W16[O], qd, x, H, 1, H, nullptr, x, EPI_RESID, 0, false);
      if ((g_ao_oproj & 16) && ctx->dbg_stamps) g.dbg = ctx->dbg_stamps + (size_t)i * 32;
      TRY(launch_gemv_wait(ctx->dt, g, (const unsigned*)ctx->fd_ws, ctx->fd_epoch, c.t_heads, ctx->fd_err, g_ao_oproj, s));
    } else if (n2 && OMCHAT_EXPERIMENTS && (g_ao_oproj & 16) && ctx->dbg_stamps && !wq) {
      GemvArgs g = gemv_args(ctx->tw_ao, qd, W16[O], qd, x, H, 1, H, nullptr, x, EPI_RESID, 0, false);
      g.dbg = ctx->dbg_stamps + (size_t)i * 32;
      TRY(launch_gemv(ctx->dt, g, s));
    } else if (n2) {
      TRY(gemv(ctx->tw_ao, qd, W[O], qd, x, H, H, nullptr, x, EPI_RESID));
    } else if (nb2) {
      GemvArgs g = gemv_args(ctx->tw_ao, qd, W[O], qd, x, H, b, H, nullptr, x, EPI_RESID, 0, false);      // (nb2 holds wpk: the 16-bit packed reference)
      g.y_pack = ctx->tw_xn;
      TRY(launch_gemv(ctx->dt, g, s));
    } else if (fused) {
      TRY(gemv_partial(ctx->tw_ao, qd, W[O], qd, ks_o));
      TRY(ctx->reduce_resid_rmsnorm(x, H, ctx->tw_part, ks_o, L.ln2, ctx->tw_xn, H, b, H, c.t_eps, pk, s));
    } else if (ctx->tp_size == 1) {
      TRY(gemv(ctx->tw_ao, qd, W[O], qd, x, H, H, nullptr, x, EPI_RESID));
    } else {
      TRY(gemv(ctx->tw_ao, qd, W[O], qd, y, H, H, nullptr, lead ? x : nullptr, lead ? EPI_RESID : EPI_NONE));
      TRY(ctx->allreduce(y, (size_t)b * H, s));
      std::swap(x, y);
    }
    if (!fused) TRY(launch_rmsnorm(ctx->dt, x, H, L.ln2, ctx->tw_xn, H, b, H, c.t_eps, s));
    // HIP-event bracket on ONE layer per token only: each event record costs ~1-2 us of launch-stream time, and 56 of them
    // per token would themselves slow the measured decode by a few per cent
    const bool mark = allow_prof && i == c.t_layers / 2;
    if (mark) ctx->prof_mark(OMCHAT_PROF_DECODE_GATEUP, s);
    if (n2) {
      GemvArgs g = gemv_args(x, H, W[GU], H, ctx->tw_act, It, 1, 2 * It, nullptr, nullptr, EPI_SWIGLU, 0, false);
      g.norm_w = L.ln2; g.norm_eps = c.t_eps;
      if (const auto* r = x12_of(omchat_ctx::X12_GU, i)) { use_weight_x12(g, *r, H); ++ctx->x12_launches[omchat_ctx::X12_GU]; }
      if (ctx->dyn_ctr && !ctx->graph_on) g.dyn_ctr = ctx->dyn_ctr + (size_t)i * 65 * 64;
      if (OMCHAT_EXPERIMENTS && (g_ao_oproj & 16) && ctx->dbg_stamps) g.dbg = ctx->dbg_stamps + (size_t)i * 32;
      TRY(launch_gemv(ctx->dt, g, s));
    } else if (nb2) {
      GemvArgs g = gemv_args(ctx->tw_xn, H, W[GU], H, ctx->tw_act, It, b, 2 * It, nullptr, nullptr, EPI_SWIGLU, 0, true);
      g.norm_w = L.ln2; g.norm_eps = c.t_eps;
      TRY(launch_gemv(ctx->dt, g, s));
    } else {
      TRY(gemv(ctx->tw_xn, H, W[GU], H, ctx->tw_act, It, 2 * It, nullptr, nullptr, EPI_SWIGLU, true));
    }
    if (mark) ctx->prof_mark(OMCHAT_PROF_DECODE_GATEUP, s);
    if (n1 && OMCHAT_EXPERIMENTS && (g_ao_oproj & 16) && ctx->dbg_stamps && !wq) {
      GemvArgs g = gemv_args(ctx->tw_act, It, W16[DOWN], It, x, H, 1, H, nullptr, x, EPI_RESID, 0, false);
      g.dbg = ctx->dbg_stamps + (size_t)i * 32;
      TRY(launch_gemv(ctx->dt, g, s));
    } else if (n1 && x12_of(omchat_ctx::X12_DOWN, i)) {
      GemvArgs g = gemv_args(ctx->tw_act, It, W[DOWN], It, x, H, 1, H, nullptr, x, EPI_RESID, 0, false);
      use_weight_x12(g, *x12_of(omchat_ctx::X12_DOWN, i), It);
      ++ctx->x12_launches[omchat_ctx::X12_DOWN];
      TRY(launch_gemv(ctx->dt, g, s));
    } else if (n1) {
      TRY(gemv(ctx->tw_act, It, W[DOWN], It, x, H, H, nullptr, x, EPI_RESID));
    } else if (fused) {
      TRY(gemv_partial(ctx->tw_act, It, W[DOWN], It, ks_d));
      const void* nw = i + 1 < c.t_layers ? ctx->dl[i + 1].ln1 : ctx->t_norm;      // next layer's input norm, or the final norm
      TRY(ctx->reduce_resid_rmsnorm(x, H, ctx->tw_part, ks_d, nw, ctx->tw_xn, H, b, H, c.t_eps, pk, s));
    } else if (ctx->tp_size == 1) {
      TRY(gemv(ctx->tw_act, It, W[DOWN], It, x, H, H, nullptr, x, EPI_RESID));
    } else {
      TRY(gemv(ctx->tw_act, It, W[DOWN], It, y, H, H, nullptr, lead ? x : nullptr, lead ? EPI_RESID : EPI_NONE));
      TRY(ctx->allreduce(y, (size_t)b * H, s));
      std::swap(x, y);
    }
    TRY(dola_keep(i + 1));
  }
  if (!fused)   TRY(launch_rmsnorm(ctx->dt, x, H, ctx->t_norm, ctx->tw_xn, H, b, H, c.t_eps, s));
  float* lg = logits ? logits : ctx->tw_logits;
  int pick_b = b;
  if (dola) {
    // in place of the batch-1 head with its fused norm and coded stream: the final norm as a launch, one 16-bit pass over (k + 1) b rows
    TRY(dola_head(ctx, x, logits, s));
    lg = ctx->pick.dola_logits; pick_b = D.rows();
  } else if (n1) {
    GemvArgs g{x, H, nullptr, 0, lg, c.t_vocab, 1, c.t_vocab, H, nullptr, nullptr, 0, EPI_NONE, 1};
    use_weight(g, ctx->lm_w(fmt));
    if (const auto* r = x12_of(omchat_ctx::X12_LM, 0)) { use_weight_x12(g, *r, H); ++ctx->x12_launches[omchat_ctx::X12_LM]; }
    g.norm_w = ctx->t_norm; g.norm_eps = c.t_eps;
    TRY(launch_gemv(ctx->dt, g, s));
  } else {
    TRY(lm_head_rows(ctx, ctx->tw_xn, b, lg, s, ctx->lm_w(fmt), fused && pk));
  }
  // the position bookkeeping (pos += 1, len += 1) rides in the argmax's second stage when the step picks a token (one launch less per token)
  if (vL >= 0) TRY(pick_verify(ctx, lg, b, tokens, next_tokens, s, vsample));
  else if (next_tokens) TRY(pick_run(ctx, lg, pick_b, next_tokens, s, true, tokens));
  else {
    hipLaunchKernelGGL(advance_lens_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, ctx->d_pos, ctx->d_len, b);
    TRY(pick_feed(ctx, tokens, b, s));
  }
  OM_LAUNCH_CHECK();
  return 0;
}

static void destroy_graph(omchat_ctx::DecodeGraph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g = omchat_ctx::DecodeGraph{};
}

void drop_decode_graphs(omchat_ctx* ctx) {
  for (auto& kv : ctx->graphs) destroy_graph(kv.second);
  ctx->graphs.clear();
}


extern "C" int omchat_enable_decode_graph(omchat_ctx* ctx, int on) {
  OM_CHECK(ctx, "null ctx");
  OM_CHECK(ctx->c.t_layers > 0, "context has no decoder");
  if (on && !ctx->graph_stream) {
    OM_HIP(hipStreamCreateWithFlags(&ctx->graph_stream, hipStreamNonBlocking));
    OM_HIP(hipEventCreateWithFlags(&ctx->graph_ev_in, hipEventDisableTiming));
    OM_HIP(hipEventCreateWithFlags(&ctx->graph_ev_out, hipEventDisableTiming));
    TRY(ctx->alloc((void**)&ctx->d_tok_in, (size_t)ctx->c.max_batch * 4));
    TRY(ctx->alloc((void**)&ctx->d_tok_out, (size_t)ctx->c.max_batch * 4));
  }
  ctx->graph_on = on != 0;
  return 0;
}

// bf16x12, for tests and tools: the roles tuning key 50 selects at the moment, and per role (gate|up, down_proj, lm_head)
// the coded launches enqueued so far by eager steps and graph captures and the number of its tensors that are coded (built and under the patch cap)
extern "C" int omchat_bf16x12_stats(omchat_ctx* ctx, int* roles, long* launches, int* coded) {
  OM_CHECK(ctx, "null context");
  if (roles) *roles = g_x12_roles;
  for (int r = 0; r < omchat_ctx::X12_ROLES; ++r) {
    if (launches) launches[r] = ctx->x12_launches[r];
    int n = 0;
    if (ctx->x12[r].state == omchat_ctx::W_BUILT) for (const auto& e : ctx->x12[r].e) n += e.ok ? 1 : 0;
    if (coded) coded[r] = n;
  }
  return 0;
}

extern "C" int omchat_decode_graph_stats(omchat_ctx* ctx, long* steps, long* replays, long* captures) {
  OM_CHECK(ctx, "null ctx");
  if (steps) *steps = ctx->graph_steps;
  if (replays) *replays = ctx->graph_replays;
  if (captures) *captures = ctx->graph_captures;
  return 0;
}

extern "C" int omchat_decode_step(omchat_ctx* ctx, const int32_t* tokens, int b, float* logits, int32_t* next_tokens, void* stream) {
  OM_CHECK(ctx && tokens, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(b >= 1 && b <= c.max_batch, "batch exceeds max_batch");
  OM_CHECK(mx4_rows_ok(ctx, b), MX4_ROWS_MSG);
  if (const char* why = pick_rows_refusal(ctx, b)) OM_CHECK(false, why);
  if (ctx->pick.dola_on())
    if (const char* why = dola_state_refusal(ctx)) OM_CHECK(false, why);
  if (ctx->contrastive_on()) {
    OM_CHECK(ctx->cs.forked && b == ctx->cs.k, "contrastive search is on: a step takes the top_k candidate rows the first omchat_contrastive_step handed back (omchat_set_contrastive with k = 0 first)");
    if (const char* why = contrastive_state_refusal(ctx)) OM_CHECK(false, why);
  }
  int Lmax = 0;
  OM_CHECK(!ctx->left_padded, "per-sequence decode after a left-padded prefill: use omchat_decode_step_masked (the reference positions such a "
                              "batch with sum(mask) - 1 and a per-row key mask, omchat_arch.py:61-70; DESIGN.md section 7)");
  OM_CHECK(ctx->dec_mode != 2, "omchat_decode_step after omchat_decode_step_masked on the same prefill: the two place the cache rows differently");
  bool same_len = true;
  int Lmin = c.max_seq;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(ctx->h_len[i] >= 1, "decode before prefill");
    Lmax = std::max(Lmax, ctx->h_len[i] + 1);
    Lmin = std::min(Lmin, ctx->h_len[i]);
    same_len = same_len && ctx->h_len[i] == ctx->h_len[0];
  }
  OM_CHECK(Lmax <= c.max_seq, "KV cache full (max_seq)");
  hipStream_t s = (hipStream_t)stream;
  GroupState& G = ctx->group;
  const bool grp = G.on();
  if (grp) {
    // the rows may differ in length (omchat_prefill_suffixes): the shared attention reads each row's own length from the device
    OM_CHECK(b == G.b * G.N && Lmin >= G.P, "a sampled group shares its prompt: a step takes all its b * N rows, none shorter than the prompt (omchat_group_begin with b = 0 first)");
    OM_CHECK(ctx->tp_size == 1 && !(ctx->fp8_kv && ctx->kv8_valid), "shared-prompt mode: one GPU, 16-bit KV cache");
    // the suffix grid in buckets of 256 keys: eager and captured steps issue the same launches, and a graph lasts 256 steps
    Lmax = std::min(c.max_seq, G.P + (Lmax - G.P + 255) / 256 * 256);
    const size_t need = attn_shared_ws_bytes(G.b, G.N, c.t_heads, c.t_kv_heads, G.P, Lmax);
    if (need > G.ws.cap) TRY(ctx->grow(G.ws, attn_shared_ws_bytes(G.b, G.N, c.t_heads, c.t_kv_heads, G.P, std::min(c.max_seq, Lmax + 768))));
  }
  TRY(step_weights_ready(ctx, b));
  TRY(pick_admit(ctx, next_tokens != nullptr, true));
  ctx->graph_steps++;
  // graph replay needs replay-invariant arguments: single-GPU fused path only; with profiling on, every 8th step runs eagerly
  // so that the HIP-event brackets of the dominant kernel are still recorded inside the timed region
  const bool graph = ctx->graph_on && ctx->tp_size == 1 && b <= 32 && !(ctx->prof_on && ctx->graph_steps % 8 == 0);
  if (!graph) {
    TRY(decode_body(ctx, tokens, b, Lmax, logits, next_tokens, s, true, same_len && !grp));
  } else {
    const int fmt = step_format(ctx, b);
    omchat_ctx::DecodeGraph& g = ctx->graphs[b * 8 + (is_mxfp4(fmt) ? 4 : 0) + (fmt == OMCHAT_WFMT_E4M3 ? 2 : 0) + ((ctx->fp8_kv && ctx->kv8_valid) ? 1 : 0) +
                                             (ctx->pick.dola_on() ? (1 << 19) : 0) + (grp ? (1 << 20) : 0) +
                                             (x12_step_mask(ctx, b, fmt) << 21)];      // (+ the bf16x12 roles of tuning key 50: switching captures again)
    hipStream_t gs = ctx->graph_stream;
    OM_HIP(hipEventRecord(ctx->graph_ev_in, s));
    OM_HIP(hipStreamWaitEvent(gs, ctx->graph_ev_in, 0));
    OM_HIP(hipMemcpyAsync(ctx->d_tok_in, tokens, (size_t)b * 4, hipMemcpyDeviceToDevice, gs));
    if (!g.exec || Lmax > g.cap_len || (grp && (Lmax != g.cap_len || G.N != g.grp_N || G.P != g.grp_P || G.ws.p != g.grp_ws))) {
      destroy_graph(g);
      const int cap = grp ? Lmax : std::min(c.max_seq, (Lmax + 1024 + 63) / 64 * 64);
      OM_HIP(hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal));
      const int rc = decode_body(ctx, ctx->d_tok_in, b, cap, ctx->tw_logits, ctx->d_tok_out, gs, false);
      hipGraph_t graph_h = nullptr;
      const hipError_t e = hipStreamEndCapture(gs, &graph_h);
      if (rc) { if (graph_h) (void)hipGraphDestroy(graph_h); return rc; }
      OM_HIP(e);
      g.graph = graph_h;
      OM_HIP(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
      g.cap_len = cap;
      if (grp) { g.grp_N = G.N; g.grp_P = G.P; g.grp_ws = G.ws.p; }
      ctx->graph_captures++;
    }
    OM_HIP(hipGraphLaunch(g.exec, gs));
    ctx->graph_replays++;
    if (next_tokens) OM_HIP(hipMemcpyAsync(next_tokens, ctx->d_tok_out, (size_t)b * 4, hipMemcpyDeviceToDevice, gs));
    if (logits) OM_HIP(hipMemcpyAsync(logits, ctx->tw_logits, (size_t)b * c.t_vocab * 4, hipMemcpyDeviceToDevice, gs));
    OM_HIP(hipEventRecord(ctx->graph_ev_out, gs));
    OM_HIP(hipStreamWaitEvent(s, ctx->graph_ev_out, 0));
  }
  for (int i = 0; i < b; ++i) ctx->h_len[i] += 1;
  ctx->dec_mode = 1;
  return 0;
}

// Prompt-lookup verify (include/omchat_hip.h): T tokens of sequence 0 through every layer as the batched decode step
// runs T sequences, with the multi-query attention in place of the per-sequence one, then the acceptance of the drafts on the device.
extern "C" int omchat_decode_verify(omchat_ctx* ctx, const int32_t* tokens, int T, float* logits, int32_t* picks, int* n_accept, int flags,
                                    void* stream) {
  OM_CHECK(ctx && tokens && picks && n_accept, "null argument");
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(T >= 2 && T <= VERIFY_MAX_T, "2 <= T <= 16 tokens (T = 1 is omchat_decode_step)");
  OM_CHECK(c.t_kv_heads > 0 && T * (c.t_heads / c.t_kv_heads) <= 128, "T * (q heads per kv head) must be <= 128 (the verify attention's query rows)");
  OM_CHECK(!ctx->left_padded && ctx->dec_mode != 2, "after a padded-batch prefill or masked decode steps");
  const bool vsample = (flags & OMCHAT_VERIFY_SAMPLE) != 0;
  const char* why = pick_verify_refusal(ctx, flags);
  OM_CHECK(!why, why);
  OM_CHECK(!ctx->pick.constraints_on(), "constraints are on: each verify row would need its own ban set (omchat_set_constraints with b = 0 first)");
  OM_CHECK(!ctx->pick.fsm_on(), "a token FSM is on: each verify row would need its own state (omchat_fsm_begin with b = 0 first)");
  OM_CHECK(!ctx->pick.guidance_on(), "guidance is on: each verify row would need its twin (omchat_set_guidance with b = 0 first)");
  OM_CHECK(!ctx->pick.dola_on(), "layer-contrastive decoding is on: each verify row would need its candidate rows (omchat_set_dola with b = 0 first)");
  OM_CHECK(!ctx->beam.on(), "a beam search is active");
  OM_CHECK(!ctx->contrastive_on(), "contrastive search is on: its k rows are one sequence's candidates (omchat_set_contrastive with k = 0 first)");
  OM_CHECK(!ctx->group.on(), "a sampled group shares its prompt: a verify step runs one sequence (omchat_group_begin with b = 0 first)");
  OM_CHECK(!ctx->pick.logprobs_on(), "logprobs are on: a verify step's picks are not recorded (omchat_set_logprobs with b = 0 first)");
  OM_CHECK(!(ctx->fp8_kv && ctx->kv8_valid), "the e4m3 KV cache is not implemented");
  const int L = ctx->h_len[0];
  OM_CHECK(L >= 1, "decode before prefill");
  OM_CHECK(L + T <= c.max_seq, "KV cache full (max_seq)");
  hipStream_t s = (hipStream_t)stream;
  TRY(step_weights_ready(ctx, T));      // (the first verify step, like the first batched step, builds the packed weight replica)
  if (vsample) TRY(pick_verify_prepare(ctx));
  TRY(decode_body(ctx, tokens, T, L + T, logits, picks, s, false, false, false, L, vsample));
  if (vsample) {
    const PickState& P = ctx->pick;
    hipLaunchKernelGGL(verify_accept_sample_kernel, dim3(1), dim3(64), 0, s, tokens, picks, T, L, ctx->d_pos, ctx->d_len, ctx->d_verify_n,
                       P.smp.penalty != 1.f ? P.smp_bm : nullptr, ctx->tp_rank * c.t_vocab, c.t_vocab, P.smp_vlast, P.smp_last, P.smp_step);
  } else {
    hipLaunchKernelGGL(verify_accept_kernel, dim3(1), dim3(64), 0, s, tokens, picks, T, L, (flags & OMCHAT_VERIFY_KEEP_ALL) ? 1 : 0,
                       ctx->d_pos, ctx->d_len, ctx->d_verify_n);
  }
  OM_LAUNCH_CHECK();
  int n = 0;
  OM_HIP(hipMemcpyAsync(&n, ctx->d_verify_n, 4, hipMemcpyDeviceToHost, s));
  OM_HIP(hipStreamSynchronize(s));
  *n_accept = n;
  if (vsample) pick_verify_committed(ctx, n + 1);
  ctx->h_len[0] = L + ((flags & OMCHAT_VERIFY_KEEP_ALL) ? T : n + 1);
  ctx->dec_mode = 1;
  return 0;
}

// Decode step of a PADDED batch exactly as the reference computes it (omchat_arch.py:61-70 as HF generate drives it with `images` passed
// on every step): the new token of EVERY row is appended at the common cache length (S of the padded prefill + the steps so far), rotated
// to positions[i] = sum(mask_i) - 1, and attends the cache slots whose mask byte is non-zero -- the token-level mask padded with ones,
// which hides real prompt slots and exposes padded ones once images expanded the rows differently.  After a right-padded prefill the
// padded slots hold the K / V of causally un-masked padded query rows (what every backend of the reference computes); after a
// left-padded one those of fully masked rows, which the prefill filled as the reference's eager (CPU) attention does.
static int masked_common_checks(omchat_ctx* ctx, int b) {
  const omchat_config& c = ctx->c;
  OM_CHECK(c.t_layers > 0, "context has no decoder");
  OM_CHECK(ctx->pre_S >= 1 && b == ctx->pre_b, "masked decode: the batch of the last prefill, all rows");
  OM_CHECK(mx4_rows_ok(ctx, b), MX4_ROWS_MSG);
  OM_CHECK(ctx->dec_mode != 1, "omchat_decode_step_masked after omchat_decode_step on the same prefill: the two place the cache rows differently");
  OM_CHECK(ctx->tp_size == 1, "masked decode: one GPU (under tensor parallelism right-padded batches take the per-sequence step)");
  OM_CHECK(!ctx->pick.guidance_on(), "masked decode: guidance is on, and its twin rows run at their own lengths (omchat_set_guidance with b = 0 first)");
  OM_CHECK(!ctx->pick.dola_on(), "masked decode: layer-contrastive decoding is on, and the padded-batch step keeps no candidate rows (omchat_set_dola with b = 0 first)");
  OM_CHECK(!ctx->contrastive_on(), "masked decode: contrastive search is on, and its k rows run one unpadded sequence (omchat_set_contrastive with k = 0 first)");
  OM_CHECK(!ctx->group.on(), "masked decode: a sampled group shares its prompt, and the shared attention has no key mask (omchat_group_begin with b = 0 first)");
  OM_CHECK(ctx->pre_S + ctx->masked_steps + 1 <= c.max_seq, "KV cache full (max_seq)");
  if (!ctx->d_mask) {
    ctx->mask_sb = (int64_t)cdiv(c.max_seq, 64) * 64;
    TRY(ctx->alloc((void**)&ctx->d_mask, (size_t)c.max_batch * ctx->mask_sb));
  }
  // replicas first: a failure here must not leave host-to-device copies of caller / stack memory in flight
  TRY(step_weights_ready(ctx, b));
  return 0;
}

extern "C" int omchat_decode_step_masked(omchat_ctx* ctx, const int32_t* tokens, int b, const int32_t* positions, const uint8_t* key_mask,
                                         int mask_ld, float* logits, int32_t* next_tokens, void* stream) {
  OM_CHECK(ctx && tokens && positions && key_mask, "null argument");
  const omchat_config& c = ctx->c;
  TRY(masked_common_checks(ctx, b));
  const int Lc = ctx->pre_S + ctx->masked_steps;          // slots every row holds; the new token goes to slot Lc
  OM_CHECK(mask_ld >= Lc + 1, "key_mask rows must cover the cache and the new token (slots + 1 columns)");
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(positions[i] >= 0 && positions[i] < c.max_seq, "position outside the RoPE table");
    OM_CHECK(key_mask[(size_t)i * mask_ld + Lc] != 0, "the new token must see itself");
  }
  TRY(pick_admit(ctx, next_tokens != nullptr, true));
  ctx->mask_on_device = false;      // the device copy holds THIS step's mask, zero-padded: omchat_decode_step_masked_next needs a new begin
  OM_HIP(hipMemsetAsync(ctx->d_mask, 0, (size_t)b * ctx->mask_sb, s));
  OM_HIP(hipMemcpy2DAsync(ctx->d_mask, (size_t)ctx->mask_sb, key_mask, (size_t)mask_ld, (size_t)Lc + 1, (size_t)b, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(ctx->d_pos, positions, (size_t)b * 4, hipMemcpyHostToDevice, s));
  const int rc = decode_body(ctx, tokens, b, Lc + 1, logits, next_tokens, s, false, true, true);
  OM_HIP(hipStreamSynchronize(s));     // the caller's mask / positions may be reused as soon as this returns
  if (rc) return rc;
  ctx->masked_steps += 1;
  ctx->dec_mode = 2;
  return 0;
}

// The same step without per-step host data (round 5).  In the loop HF generate drives (single_inference.py:53-62 on a padded batch) the decode
// branch of prepare_inputs_labels_for_multimodal (omchat_arch.py:61-70) pads the token-level mask with ONES up to the cache length, and every
// generated token appends another one: over the cache slots the key mask of step k is [token-level mask of the PROMPT | ones], the same for
// every k, and position_ids = sum(mask) - 1 grows by one per step.  So the mask goes to the device once (begin: `mask_cols` columns from the
// caller, ones behind them) with the first step's positions, and every following step (next) takes its positions from the device, where the
// greedy pick of the previous step advanced them: no host buffer, no stream synchronisation, and the caller may enqueue step k + 1 before it
// has read token k (OmChatQwen2ForCausalLM.generate).  Arbitrary per-step masks keep omchat_decode_step_masked.
extern "C" int omchat_masked_decode_begin(omchat_ctx* ctx, int b, const int32_t* positions, const uint8_t* key_mask, int mask_ld, int mask_cols,
                                          void* stream) {
  OM_CHECK(ctx && positions && key_mask, "null argument");
  const omchat_config& c = ctx->c;
  TRY(masked_common_checks(ctx, b));
  OM_CHECK(mask_cols >= 1 && mask_cols <= mask_ld && mask_cols <= c.max_seq, "mask_cols: 1 .. min(mask_ld, max_seq)");
  // Only the slots that exist at the first step carry caller data: [0, Lc) the cache, Lc the new token's own slot.  Everything behind is a
  // generated token's slot and must read as visible whatever a zero-padded caller buffer holds there (zeros at or beyond Lc hid
  // the new token and every later one without an error); a caller mask that hides slot Lc itself is refused like the host-mask entry does.
  const int Lc = ctx->pre_S + ctx->masked_steps;
  const int cols = mask_cols < Lc + 1 ? mask_cols : Lc + 1;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(positions[i] >= 0 && positions[i] < c.max_seq, "position outside the RoPE table");
    OM_CHECK(mask_cols <= Lc || key_mask[(size_t)i * mask_ld + Lc] != 0, "the new token must see itself (key_mask column pre_S + steps)");
  }
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemsetAsync(ctx->d_mask, 1, (size_t)b * ctx->mask_sb, s));
  OM_HIP(hipMemcpy2DAsync(ctx->d_mask, (size_t)ctx->mask_sb, key_mask, (size_t)mask_ld, (size_t)cols, (size_t)b, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(ctx->d_pos, positions, (size_t)b * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipStreamSynchronize(s));     // once per generation: the caller's buffers are free again
  ctx->mask_on_device = true;
  return 0;
}

extern "C" int omchat_decode_step_masked_next(omchat_ctx* ctx, const int32_t* tokens, int b, float* logits, int32_t* next_tokens, void* stream) {
  OM_CHECK(ctx && tokens, "null argument");
  TRY(masked_common_checks(ctx, b));
  OM_CHECK(ctx->mask_on_device, "omchat_decode_step_masked_next: call omchat_masked_decode_begin after the prefill (and after any omchat_decode_step_masked)");
  const int Lc = ctx->pre_S + ctx->masked_steps;
  TRY(pick_admit(ctx, next_tokens != nullptr, true));
  const int rc = decode_body(ctx, tokens, b, Lc + 1, logits, next_tokens, (hipStream_t)stream, false, true, true);
  if (rc) return rc;
  ctx->masked_steps += 1;
  ctx->dec_mode = 2;
  return 0;
}

extern "C" int omchat_ctx_set_peer(omchat_ctx* ctx, omchat_peer* peer, size_t max_bytes, int all_sizes) {
  OM_CHECK(ctx, "null ctx");
  ctx->peer = peer;
  if (max_bytes) ctx->peer_max = max_bytes;
  ctx->peer_all = all_sizes != 0;
  return 0;
}

// in-place sum over the tensor-parallel group of a caller buffer, through the context's transports (peer kernels / RCCL); the buffer
// must be 16-byte aligned with >= 16 bytes of slack after `count` elements when the byte count is not a multiple of 16
extern "C" int omchat_ctx_allreduce(omchat_ctx* ctx, void* buf, size_t count, int dtype, void* stream) {
  OM_CHECK(ctx && buf, "null argument");
  OM_CHECK(dtype == OMCHAT_F16 || dtype == OMCHAT_BF16 || dtype == OMCHAT_F32, "bad dtype");
  return ctx->allreduce_any(buf, count, dtype, (hipStream_t)stream);
}

extern "C" int omchat_ctx_comm_stats(omchat_ctx* ctx, long* peer_calls, long* rccl_calls) {
  OM_CHECK(ctx, "null ctx");
  if (peer_calls) *peer_calls = ctx->n_ar_peer + ctx->n_fused_norm;
  if (rccl_calls) *rccl_calls = ctx->n_ar_rccl;
  return 0;
}

// sequence-parallel exchanges so far: reduce-scatters and all-gathers over row blocks (model.hip gemm_sp; 0 / 0 = the all-reduce form ran)
extern "C" int omchat_ctx_sp_stats(omchat_ctx* ctx, long* reduce_scatters, long* all_gathers) {
  OM_CHECK(ctx, "null ctx");
  if (reduce_scatters) *reduce_scatters = ctx->n_rs;
  if (all_gathers) *all_gathers = ctx->n_ag;
  return 0;
}

extern "C" int omchat_set_allreduce_hook(omchat_ctx* ctx, omchat_allreduce_fn fn, void* user) {
  OM_CHECK(ctx, "null ctx");
  ctx->hook = fn; ctx->hook_user = user;
  return 0;
}

extern "C" int omchat_prof_enable(omchat_ctx* ctx, int on) {
  OM_CHECK(ctx, "null ctx");
  ctx->prof_on = on != 0;
  return 0;
}

extern "C" int omchat_prof_read(omchat_ctx* ctx, int cat, double* total_ms, long* launches, int reset) {
  OM_CHECK(ctx && cat >= 0 && cat < OMCHAT_PROF_CATS && total_ms && launches, "bad argument");
  omchat_ctx::Prof& p = ctx->prof[cat];
  OM_HIP(hipDeviceSynchronize());
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    float ms = 0.f;
    OM_HIP(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
    p.ms += ms; p.count += 1;
  }
  p.used = 0;
  *total_ms = p.ms; *launches = p.count;
  if (reset) { p.ms = 0; p.count = 0; }
  return 0;
}

// Fused decode launches (fused_decode.hip): how many ran, and the sticky time-out bits of their in-launch hand-offs (0 = every hand-off
// completed; bit 0 = a merge sweep, bit 1 = a row sweep gave up after its wall-clock budget -- the step's results are then wrong and the
// caller must not use them).  Synchronises the device.
extern "C" int omchat_fused_status(omchat_ctx* ctx, long* launches, unsigned* timeout_bits) {
  OM_CHECK(ctx, "null ctx");
  if (launches) *launches = ctx->n_fused_launches + ctx->n_layer_launches;
  if (timeout_bits) {
    *timeout_bits = 0;
    if (ctx->fd_err) OM_HIP(hipMemcpy(timeout_bits, ctx->fd_err, 4, hipMemcpyDeviceToHost));
  }
#if OMCHAT_EXPERIMENTS
  if ((g_ao_oproj & 16) && ctx->dbg_stamps) {
    // measurement: clock stamps (100 MHz) of the LAST decode step, averaged over the layers: every kernel of the six-launch layer from its first wave's
    // start to its last wave's end, and the boundary in front of it (first start - the previous kernel's end)
    const int nl = ctx->c.t_layers;
    std::vector<unsigned long long> st((size_t)nl * 32);
    OM_HIP(hipMemcpy(st.data(), ctx->dbg_stamps, (size_t)nl * 256, hipMemcpyDeviceToHost));
    // order in the layer: qkv (8, 9), attention (10, 11), merge (12, 0), o_proj (1, 3), gate|up (4, 5), down_proj (6, 7)
    static const int S0[6] = {8, 10, 12, 1, 4, 6}, S1[6] = {9, 11, 0, 3, 5, 7};
    static const char* NM[6] = {"qkv", "attention", "merge", "o_proj", "gate|up", "down_proj"};
    double dur[6] = {0, 0, 0, 0, 0, 0}, gap[6] = {0, 0, 0, 0, 0, 0}, seen = 0, xcd_end[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xcd_raw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n = 0, ngap0 = 0, nx = 0, xcd_slowest[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nl; ++i) {
      const unsigned long long* t = &st[(size_t)i * 32];
      bool ok = true;
      for (int k = 0; k < 6; ++k) ok = ok && t[S0[k]] && t[S1[k]];
      if (!ok) continue;
      for (int k = 0; k < 6; ++k) {
        dur[k] += ((double)t[S1[k]] - (double)~t[S0[k]]) / 100.0;
        if (k > 0) gap[k] += ((double)~t[S0[k]] - (double)t[S1[k - 1]]) / 100.0;
      }
      if (i > 0 && st[(size_t)(i - 1) * 32 + 7]) { gap[0] += ((double)~t[8] - (double)st[(size_t)(i - 1) * 32 + 7]) / 100.0; ++ngap0; }
      if (t[2]) seen += ((double)t[2] - (double)t[0]) / 100.0;
      {      // gate|up: the end per XCD relative to the launch's first start, sorted within the layer (which XCD is slow changes from launch to launch)
        double e[8]; bool all = true;
        for (int x = 0; x < 8; ++x) { all = all && t[16 + x]; e[x] = ((double)t[16 + x] - (double)~t[4]) / 100.0; }
        if (all) {
          int slow = 0;
          for (int x = 0; x < 8; ++x) { xcd_raw[x] += e[x]; if (e[x] > e[slow]) slow = x; }
          ++xcd_slowest[slow];
          std::sort(e, e + 8); for (int x = 0; x < 8; ++x) xcd_end[x] += e[x]; ++nx;
        }
      }
      ++n;
    }
    if (n) {
      fprintf(stderr, "[omchat dbg] key 42 = %d, last decode step, mean over %d layers, us (boundary in front | first start -> last end):", g_ao_oproj, n);
      double sd = 0, sg = 0;
      for (int k = 0; k < 6; ++k) {
        const double g = k == 0 ? (ngap0 ? gap[0] / ngap0 : 0.0) : gap[k] / n;
        fprintf(stderr, " %s %.2f | %.2f;", NM[k], g, dur[k] / n);
        sd += dur[k] / n; sg += g;
      }
      fprintf(stderr, " kernels %.2f + boundaries %.2f = %.2f per layer", sd, sg, sd + sg);
      if (seen > 0) fprintf(stderr, "; flags seen %.2f after the merge's end", seen / n);
      if (nx) {
        fprintf(stderr, "; gate|up end per XCD after its first start, fastest to slowest:");
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %.2f", xcd_end[x] / nx);
        fprintf(stderr, "; by XCD id 0..7:");
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %.2f", xcd_raw[x] / nx);
        fprintf(stderr, "; layers in which XCD x ended last:");
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %d", xcd_slowest[x]);
      }
      fprintf(stderr, "\n");
    }
  }
#endif
  return 0;
}

// Forget the last n decode steps of sequences 0..b-1 (their cache rows stay in memory and are overwritten by the next steps): the drop-in
// generate() enqueues step k + 1 before it has looked at token k on the host, and takes the step back when token k ends the generation.
extern "C" int omchat_kv_rewind(omchat_ctx* ctx, int b, int n, void* stream) {
  OM_CHECK(ctx && b >= 1 && b <= (int)ctx->h_len.size() && n >= 0, "bad argument");
  if (n == 0) return 0;
  // every refusal before anything is enqueued or changed: the sampler's counters, the constraint history and the KV lengths stay in step
  OM_CHECK(!ctx->contrastive_on(), "contrastive search is on: its history and record have no rewind (omchat_set_contrastive with k = 0 first)");
  const char* why = pick_rewind_refusal(ctx, b, n);
  OM_CHECK(!why, why);
  if (ctx->dec_mode == 2) {
    OM_CHECK(n <= ctx->masked_steps, "rewind beyond the prefill");
  } else {
    for (int i = 0; i < b; ++i) OM_CHECK(ctx->h_len[i] - n >= 1, "rewind beyond the prefill");
  }
  TRY(pick_rewind(ctx, b, n, (hipStream_t)stream));
  if (ctx->dec_mode == 2) {
    ctx->masked_steps -= n;
    // the device-resident positions (omchat_decode_step_masked_next) go back with the slots; the host-mask form passes its positions every step
    hipLaunchKernelGGL(add_positions_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, (hipStream_t)stream, ctx->d_pos, b, -n);
    OM_LAUNCH_CHECK();
    return 0;
  }
  std::vector<int> pos(b), len1(b);
  for (int i = 0; i < b; ++i) {
    ctx->h_len[i] -= n;
    pos[i] = ctx->h_len[i]; len1[i] = ctx->h_len[i] + 1;
  }
  hipStream_t s = (hipStream_t)stream;
  OM_HIP(hipMemcpyAsync(ctx->d_pos, pos.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipMemcpyAsync(ctx->d_len, len1.data(), (size_t)b * 4, hipMemcpyHostToDevice, s));
  OM_HIP(hipStreamSynchronize(s));     // stack vectors
  return 0;
}

extern "C" int omchat_kv_lengths(omchat_ctx* ctx, int32_t* out, int b) {
  OM_CHECK(ctx && out && b <= (int)ctx->h_len.size(), "bad argument");
  // after a left-padded prefill, and once a masked decode step ran, every row holds the same number of cache slots
  for (int i = 0; i < b; ++i) out[i] = (ctx->left_padded || ctx->dec_mode == 2) ? ctx->pre_S + ctx->masked_steps : ctx->h_len[i];
  return 0;
}
