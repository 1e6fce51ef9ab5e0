// Op-level C ABI entry points (unit parity tests / micro benches) and the FlashAttention-shaped seam.
#include "kernels.h"
#include <stdlib.h>
#include "../../include/omchat_hip.h"
#include <math.h>
#include <vector>

#define S(x) ((hipStream_t)(x))
#if OMCHAT_EXPERIMENTS
int g_launch_any_order = 0;      // tuning key 41: timing probe, see kernels.h
#endif

extern "C" int omchat_op_gemm(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                              const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, void* stream) {
  GemmArgs g{A, lda, W, ldw, C, ldc, M, N, K, bias, ls, resid, ldr, epi, force_tile, nullptr, 0, -1};
  return launch_gemm(dtype, g, S(stream));
}

// round 6: the GEMM with the folded-norm row scale and / or the statistics epilogues (epi 7 = LS_RESID + stats, 8 = NONE + stats);
// *nslots (host int, may be null) receives the number of statistics slots the launch wrote (one per wave tile of the tile kernel that ran)
extern "C" int omchat_op_gemm_fused(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                                    const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, const float* row_scale,
                                    const float* rs_stats, int rs_ld, int rs_nslots, int rs_dim, float rs_eps,
                                    float* stats, int stats_ld, int* nslots, void* stream) {
  GemmArgs g{A, lda, W, ldw, C, ldc, M, N, K, bias, ls, resid, ldr, epi, force_tile, nullptr, 0, -1};
  g.row_scale = row_scale; g.stats = stats; g.stats_ld = stats_ld; g.stats_nslots = nslots;
  g.rs_stats = rs_stats; g.rs_ld = rs_ld; g.rs_nslots = rs_nslots; g.rs_dim = rs_dim; g.rs_eps = rs_eps;
  return launch_gemm(dtype, g, S(stream));
}
extern "C" int omchat_op_stats_finish(const float* stats, int ld, int slot0, int nslots, int ngroups, int rows, int dim, float eps, float* out, void* stream) {
  return launch_stats_finish(stats, ld, slot0, nslots, ngroups, rows, dim, eps, out, S(stream));
}
extern "C" int omchat_op_row_sumsq(int dtype, const void* x, int ldx, int rows, int H, float* stats, void* stream) {
  return launch_row_sumsq(dtype, x, ldx, rows, H, stats, S(stream));
}
extern "C" int omchat_op_fold_cols(int dtype, const void* W, const void* n, void* out, int rows, int cols, void* stream) {
  return launch_fold_cols(dtype, W, n, out, rows, cols, S(stream));
}
// the K half of the joint-head q / k norm straight from the qkv GEMM's statistics slots (q slots [0, nslots), k slots [nslots, 2 nslots)); leaves the q sums
extern "C" int omchat_op_vit_knorm_slots(int dtype, void* k, int ld, const void* wk, int rows, int C, int C_total, float eps, const float* stats, int stats_ld,
                                         int nslots, float* sumsq_q, void* stream) {
  return launch_vit_knorm_slots(dtype, k, ld, wk, rows, C, C_total, eps, stats, stats_ld, nslots, sumsq_q, S(stream));
}
// omchat_mha_fwd on a packed qkv [B, S, 3, H, 128] whose Q is still RAW: the Q half of InternAttention's joint-head norm is applied on load from
// sumsq [B * S][stride] (element 0 of a row: the sum of squares of its q channels; K must already be normalised: omchat_op_vit_knorm_slots)
extern "C" int omchat_op_mha_qnorm(int dtype, const void* qkv, int B, int Sq, int H, const float* sumsq, int stride, int dim, const void* wq,
                                   float eps, float q_scale, void* out, void* stream) {
  OM_CHECK(qkv && out && sumsq && wq, "null argument");
  AttnArgs a{};
  const int64_t row = (int64_t)3 * H * 128;
  a.Q = qkv; a.q_sb = Sq * row; a.q_sh = 128; a.q_sr = row;
  a.K = (const char*)qkv + (size_t)H * 128 * 2; a.k_sb = a.q_sb; a.k_sh = 128; a.k_sr = row;
  a.V = (const char*)qkv + (size_t)2 * H * 128 * 2; a.v_sb = a.q_sb; a.v_sh = 128; a.v_sr = row;
  a.O = out; a.o_sb = (int64_t)Sq * H * 128; a.o_sh = 128; a.o_sr = (int64_t)H * 128;
  a.batch = B; a.q_heads = H; a.kv_heads = H; a.Sq = Sq; a.Skv = Sq; a.kv_len = nullptr; a.causal = 0; a.q_pos0 = 0;
  a.scale = 1.0f;
  a.qn_sumsq = sumsq; a.qn_stride = stride; a.qn_dim = dim; a.qn_w = wq; a.qn_eps = eps; a.qn_scale = q_scale;
  return launch_attn_prefill(dtype, a, S(stream));
}

// The tuning keys are PROCESS-GLOBAL switches for tests and measurements (A/B of kernel forms, launch shapes): they mutate state shared by
// every context of the process, so production callers must not touch them -- the call is refused unless the process opted in with
// OMCHAT_ALLOW_TUNING=1 in its environment (tests/conftest.py, bench.py --tuning and tools/gpu_job.sh set it).  Nothing in omchat_amd/ sets a key.
extern "C" int omchat_op_set_tuning(int key, int value) {
  const char* allow = getenv("OMCHAT_ALLOW_TUNING");
  if (!allow || allow[0] != '1') {
    omchat_set_error("omchat_op_set_tuning: process-global test / measurement hook; set OMCHAT_ALLOW_TUNING=1 to use it (see include/omchat_hip.h)");
    return 1;
  }
  if (key == 0) { gemm_set_skew(value); return 0; }
  if (key == 1) { gemv_set_force_mfma(value); return 0; }
  if (key == 5) { gemm_set_autotune(value); return 0; }
  if (key == 4) { model_set_ar_min_rows(value); return 0; }
  if (key == 6) { model_set_pack_replica(value); return 0; }
  if (key == 8) { attn_set_v2(value); return 0; }
  if (key == 9) { model_set_fuse_peer_norm(value); return 0; }
  if (key == 10) { attn_set_tpw(value); return 0; }
  if (key == 11) { gemv_set_no_xs(value); return 0; }
  if (key == 12) { attn_set_klds(value); return 0; }
  if (key == 25) { attn_set_dma(value); return 0; }
  if (key == 26) { attn_set_dma_slots(value); return 0; }
  if (key == 27) { attn_set_dma_rot(value); return 0; }
  if (key == 28) { gemv_set_skew(value); return 0; }
  if (key == 29) { model_set_tp_f32(value); return 0; }
  if (key == 30) { attn_set_hsplit(value); return 0; }
  if (key == 33) { attn_set_mha_xcd(value); return 0; }
  if (key == 16) { gemv_set_norm_loop(value); return 0; }
  if (key == 17) { gemv_set_rows_balance(value); return 0; }
  if (key == 19) { attn_set_merge_mid_min(value); return 0; }
  if (key == 21) { attn_set_merge_dg(value); return 0; }
  if (key == 13) { gemm_set_persist(value); return 0; }
  if (key == 14) { model_set_norm_in_gemv(value); return 0; }
  if (key == 22) { model_set_fuse_attn_oproj(value); return 0; }
  if (key == 23) { model_set_decode_layer(value); return 0; }
  if (key == 24) { gemv_set_dyn(value); return 0; }
  if (key == 34) { gemv_set_shard_shapes(value); return 0; }
  if (key == 35) { model_set_shard_as_tp1(value); return 0; }
  if (key == 36) { attn_set_kg(value); return 0; }
  if (key == 37) { gemm_set_wide_store(value); return 0; }
  if (key == 43) { gemm_set_skip_dead(value); return 0; }
  if (key == 44) { model_set_vit_fused(value); return 0; }
  if (key == 45) { model_set_tp_sp(value); return 0; }
  if (key == 46) { attn_set_peel(value); return 0; }
  if (key == 47) { attn_set_kv8_tpw(value); return 0; }
  if (key == 48) { attn_set_kv8_fuse(value); return 0; }
  if (key == 49) { model_set_extend_attn(value); return 0; }
  if (key == 50) { model_set_x12_roles(value); return 0; }
  if (key == 51) { model_set_suffix_attn(value); return 0; }
  if (key == 52) { attn_set_4w(value); return 0; }
  if (key == 38) { gemv_set_gu_rr(value); return 0; }
  if (key == 39) { gemv_set_longk_direct(value); return 0; }
  if (key == 40) { norm_set_wave(value); return 0; }
#if OMCHAT_EXPERIMENTS
  if (key == 41) { g_launch_any_order = value; return 0; }
  if (key == 42) { model_set_ao_oproj(value); return 0; }
#endif
  omchat_set_error("omchat_op_set_tuning: unknown key");
  return 1;
}

extern "C" int omchat_allreduce_noop(void*, void*, size_t, int, void*) { return 0; }

extern "C" int omchat_gemm_tune_load(const char* path) { OM_CHECK(path, "null path"); return gemm_tune_load(path); }
extern "C" int omchat_gemm_tune_dump(const char* path) { OM_CHECK(path, "null path"); return gemm_tune_dump(path); }
extern "C" long omchat_gemm_tune_runs(void) { return gemm_tune_runs(); }

extern "C" size_t omchat_op_gemm_sk_ws(void) { return gemm_sk_ws_bytes(); }

extern "C" int omchat_op_gemm_sk(int dtype, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                                 const void* bias, const void* ls, const void* resid, int ldr, int epi, int force_tile, void* ws,
                                 size_t ws_bytes, int stream_k, void* stream) {
  GemmArgs g{A, lda, W, ldw, C, ldc, M, N, K, bias, ls, resid, ldr, epi, force_tile, ws, ws_bytes, stream_k};
  return launch_gemm(dtype, g, S(stream));
}

extern "C" int omchat_op_gemv(int dtype, const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int b, int N, int K,
                              const void* bias, const void* resid, int ldr, int epi, int out_f32, void* stream) {
  GemvArgs g{X, ldx, W, ldw, Y, ldy, b, N, K, bias, resid, ldr, epi, out_f32};
  return launch_gemv(dtype, g, S(stream));
}

// batch-1 GEMV with the preceding RMSNorm in registers: y = epi(W RMSNorm(x; norm_w, eps)), x the RAW row [K] (K <= 4096)
extern "C" int omchat_op_gemv_norm(int dtype, const void* X, const void* W, int ldw, void* Y, int N, int K, const void* norm_w, float eps,
                                   const void* bias, int epi, int out_f32, void* stream) {
  OM_CHECK(X && W && Y && norm_w, "null argument");
  GemvArgs g{X, K, W, ldw, Y, N, 1, N, K, bias, nullptr, 0, epi, out_f32};
  g.norm_w = norm_w; g.norm_eps = eps;
  return launch_gemv(dtype, g, S(stream));
}

// packed-operand batched GEMV (gemv.hip: gemv_pk_kernel): X row-major [b, K] and W row-major [N, K] are packed into scratch here
// (launch_pack_x / launch_pack_w), then Y = epi(X W^T); y_packed != 0 returns the SwiGLU output in the packed x layout
extern "C" int omchat_op_gemv_packed(int dtype, const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int b, int N, int K,
                                     const void* bias, int epi, int out_f32, int ksplit, int w_packed, int y_packed, void* stream) {
  OM_CHECK(b >= 1 && b <= 32 && K % 64 == 0, "1 <= b <= 32, K % 64 == 0");
  const int NB = b > 16 ? 2 : 1;
  void *xp = nullptr, *wp = nullptr;
  OM_HIP(hipMalloc(&xp, (size_t)NB * 16 * K * 2));
  int rc = launch_pack_x(dtype, X, ldx, b, K, xp, S(stream));
  if (rc == 0 && w_packed) {
    if (hipMalloc(&wp, (size_t)N * K * 2) != hipSuccess) { hipFree(xp); omchat_set_error("hipMalloc failed"); return 2; }
    rc = launch_pack_w(dtype, W, ldw, N, K, wp, S(stream));
  }
  if (rc == 0) {
    GemvArgs g{xp, K, w_packed ? wp : W, ldw, Y, ldy, b, N, K, bias, nullptr, 0, epi, out_f32, ksplit, 0, nullptr, 1, w_packed, y_packed};
    rc = launch_gemv(dtype, g, S(stream));
  }
  hipStreamSynchronize(S(stream));
  hipFree(xp); if (wp) hipFree(wp);
  return rc;
}
extern "C" int omchat_op_pack_x(int dtype, const void* X, int ldx, int b, int K, void* out, void* stream) { return launch_pack_x(dtype, X, ldx, b, K, out, S(stream)); }

// What launch_gemv decides for a call of these integers on the current tuning state, without launching (gemv_plan; fields and flag bits:
// include/omchat_hip.h).  The operands are dense (ldx = K, ldw = a row of the weight form); n_cu <= 0 = the device's compute units.
extern "C" int omchat_op_gemv_plan(int dtype, int b, int N, int K, int epi, int ksplit, int flags, int wf, int n_cu, int* out) {
  OM_CHECK(out && wf >= WF_16 && wf <= WF_X12, "null out or weight form outside 0..3");
  static const unsigned set[1] = {0};      // what the plan reads of a pointer is whether it is null (dyn_ctr stays null: key 24 does not show here)
  GemvArgs a{};
  a.b = b; a.N = N; a.K = K; a.epi = epi; a.ksplit = ksplit;
  a.ldx = K; a.ldy = a.ldr = N; a.ldw = wf == WF_MX4 ? K / 2 : wf == WF_X12 ? K / 2 * 3 : K;
  a.x_packed = flags & 1; a.w_packed = flags >> 1 & 1; a.y_packed = flags >> 2 & 1; a.out_f32 = flags >> 4 & 1; a.force_mfma = flags >> 5 & 1;
  if (flags & 8) a.norm_w = set;
  if (flags & 64) a.resid = set;
  if (wf == WF_E4M3) a.w_scale = (const float*)set;
  if (wf == WF_MX4) a.mx_scale = (const unsigned char*)set;
  if (wf == WF_X12) { a.x12_top = a.x12_cnt = (const unsigned char*)set; a.x12_patch = set; }
  const GemvPlan g = gemv_plan(dtype, a, gemv_tuning(), n_cu > 0 ? n_cu : device_cus());
  if (g.refusal) { omchat_set_error(g.refusal); return 1; }
  const int f[OMCHAT_GEMV_PLAN_INTS] = {g.family, g.wf, g.wpack, g.epi, g.ntile, g.waves, g.unroll, g.nb, g.rr, g.nch, g.norm, g.gx, g.gy, g.block, g.lds,
                                        g.per_wg, (int)g.skew, g.rows_per_wg, g.n5, g.xskew};
  for (int i = 0; i < OMCHAT_GEMV_PLAN_INTS; ++i) out[i] = f[i];
  return 0;
}
// ... and the K slices a decode step gives its o_proj (down = 0, K = q width) or down_proj (down = 1, K = mlp width) launch (gemv_split_k)
extern "C" int omchat_op_gemv_split_k(int b, int K, int H, int packed, int down) { return gemv_split_k(b, K, H, packed != 0, down != 0, gemv_tuning()); }

// fp8 x fp8 GEMM (BASELINE configs[4]): A8 [M, K], W8 [N, K] e4m3 bytes with per-row fp32 scales -> C (dtype) = epi(sa[m] sw[n] A8 W8^T)
extern "C" int omchat_op_gemm_fp8(int dtype, const void* A8, const float* a_scale, const void* W8, const float* w_scale, void* C, int ldc, int M,
                                  int N, int K, const void* bias, const void* resid, int ldr, int epi, void* stream) {
  GemmArgs g{A8, K, W8, K, C, ldc, M, N, K, bias, nullptr, resid, ldr, epi, 0, nullptr, 0, -1, 1, a_scale, w_scale};
  return launch_gemm(dtype, g, S(stream));
}
// per-row e4m3 quantisation of activations [rows, H]: norm_w != NULL applies the RMSNorm first (launch_rmsnorm_q8)
extern "C" int omchat_op_quant_rows_fp8(int dtype, const void* x, const void* norm_w, float eps, void* y8, float* scale, int rows, int H, void* stream) {
  if (norm_w) return launch_rmsnorm_q8(dtype, x, H, norm_w, y8, H, scale, rows, H, eps, S(stream));
  return launch_quant_rows_q8(dtype, x, H, y8, H, scale, rows, H, S(stream));
}

// decode: x = T(x + T(sum_s part[s])) in place, xn = RMSNorm(x) * w; part fp32 [ks][rows][H] (the split-K slices of the skinny GEMM)
extern "C" int omchat_op_resid_rmsnorm(int dtype, void* x, int ldx, const float* part, int ks, const void* w, void* xn, int ldn, int rows, int H,
                                       float eps, int pack_nb, void* stream) {
  OM_CHECK(x && part, "null argument");
  return launch_resid_rmsnorm(dtype, x, ldx, part, ks, w, xn, ldn, rows, H, eps, S(stream), pack_nb);
}
extern "C" int omchat_op_rmsnorm(int dtype, const void* x, const void* w, void* y, int rows, int H, float eps, void* stream) {
  return launch_rmsnorm(dtype, x, H, w, y, H, rows, H, eps, S(stream));
}

extern "C" int omchat_op_vit_qknorm(int dtype, void* qkv, int ld, const void* wq, const void* wk, int rows, int C, int C_total, float eps,
                                    float q_scale, void* stream) {
  return launch_vit_qknorm(dtype, qkv, ld, wq, wk, rows, C, C_total, eps, q_scale, nullptr, S(stream));
}
// test hooks: the same launch with externally reduced statistics (sumsq_in [rows, 2], the tensor-parallel form) and / or the K half alone,
// and the [rows, 2] sums of squares that form all-reduces
extern "C" int omchat_op_vit_qknorm_ex(int dtype, void* qkv, int ld, const void* wq, const void* wk, int rows, int C, int C_total, float eps,
                                       float q_scale, const float* sumsq_in, int only_k, void* stream) {
  return launch_vit_qknorm(dtype, qkv, ld, wq, wk, rows, C, C_total, eps, q_scale, sumsq_in, S(stream), only_k);
}
extern "C" int omchat_op_vit_qk_sumsq(int dtype, const void* qkv, int ld, int rows, int C, float* sumsq_out, void* stream) {
  OM_CHECK(qkv && sumsq_out, "null argument");
  return launch_vit_qk_sumsq(dtype, qkv, ld, rows, C, sumsq_out, S(stream));
}

extern "C" int omchat_op_attn_prefill(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv, int Hq,
                                      int Hkv, const int32_t* kv_len, int causal, int q_pos0, float scale, void* stream) {
  AttnArgs a{};
  a.Q = q; a.q_sb = (int64_t)Sq * Hq * 128; a.q_sh = 128; a.q_sr = (int64_t)Hq * 128;
  a.K = k; a.k_sb = (int64_t)Hkv * Skv * 128; a.k_sh = (int64_t)Skv * 128; a.k_sr = 128;
  a.V = v; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = 128;
  a.O = out; a.o_sb = a.q_sb; a.o_sh = 128; a.o_sr = a.q_sr;
  a.batch = b; a.q_heads = Hq; a.kv_heads = Hkv; a.Sq = Sq; a.Skv = Skv; a.kv_len = kv_len; a.causal = causal; a.q_pos0 = q_pos0; a.scale = scale;
  return launch_attn_prefill(dtype, a, S(stream));
}

extern "C" size_t omchat_op_attn_decode_ws(int b, int Hq, int L) { return attn_decode_ws_bytes(b, Hq, L); }

// The dense layout of the split-KV attention hooks: q / out [rows, Hq, 128] and caches [b, Hkv, cap, 128] (strides in cache elements; = bytes
// for the e4m3 cache).  qkv_rows: q is the q columns of rows of raw [q | k | v] projections (the _append hooks).
static void bind_dense(AttnOperands& a, const void* q, bool qkv_rows, const void* k, const void* v, void* out, int Hq, int Hkv, int cap, float scale,
                       void* ws, size_t ws_bytes) {
  a.Q = q; a.q_sb = (int64_t)(qkv_rows ? Hq + 2 * Hkv : Hq) * 128; a.q_sh = 128;
  a.K = k; a.k_sb = (int64_t)Hkv * cap * 128; a.k_sh = (int64_t)cap * 128; a.k_sr = 128;
  a.V = v; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = 128;
  a.O = out; a.o_sb = (int64_t)Hq * 128; a.o_sh = 128;
  a.q_heads = Hq; a.kv_heads = Hkv; a.scale = scale; a.ws = (float*)ws; a.ws_bytes = ws_bytes;
}
// ... and the fused-append view of such qkv rows: the raw k / v columns behind q's, rotated by the table `tab` of rope_max positions
static void bind_new_rows(AttnOperands& a, const float* tab, int rope_max) {
  a.rope = tab; a.rope_max = rope_max; a.new_sb = a.q_sb;
  a.k_new = (const char*)a.Q + (size_t)a.q_heads * 128 * 2; a.v_new = (const char*)a.Q + (size_t)(a.q_heads + a.kv_heads) * 128 * 2;
}

extern "C" int omchat_op_attn_decode(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Hq, int Hkv, int cap, int L,
                                     const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream) {
  AttnDecodeArgs a{};
  bind_dense(a, q, false, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.batch = b; a.L = L; a.kv_len = kv_len;
  return launch_attn_decode(dtype, a, S(stream));
}

extern "C" int omchat_op_attn_decode_kv8(int dtype, const void* q, const void* k8, const void* v8, const float* ks, const float* vs, void* out, int b,
                                         int Hq, int Hkv, int cap, int L, const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream) {
  if (!k8 || !v8 || !ks || !vs) { omchat_set_error("omchat_op_attn_decode_kv8: null cache or scale pointer"); return 1; }
  AttnDecodeArgs a{};
  bind_dense(a, q, false, k8, v8, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.k_scale = ks; a.v_scale = vs; a.scale_sb = (int64_t)Hkv * cap; a.scale_sh = cap;
  a.batch = b; a.L = L; a.kv_len = kv_len;
  return launch_attn_decode(dtype, a, S(stream));
}

// test hook: the same over a padded batch -- key j of row i is visible iff key_mask[i][j] != 0 (rows of mask_sb bytes), every row holds L keys
extern "C" int omchat_op_attn_decode_kv8_masked(int dtype, const void* q, const void* k8, const void* v8, const float* ks, const float* vs, void* out,
                                                int b, int Hq, int Hkv, int cap, int L, const unsigned char* key_mask, int64_t mask_sb, float scale,
                                                void* ws, size_t ws_bytes, void* stream) {
  if (!k8 || !v8 || !ks || !vs || !key_mask) { omchat_set_error("omchat_op_attn_decode_kv8_masked: null cache, scale or mask pointer"); return 1; }
  AttnDecodeArgs a{};
  bind_dense(a, q, false, k8, v8, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.k_scale = ks; a.v_scale = vs; a.scale_sb = (int64_t)Hkv * cap; a.scale_sh = cap;
  a.batch = b; a.L = L; a.key_mask = key_mask; a.mask_sb = mask_sb;
  return launch_attn_decode(dtype, a, S(stream));
}

// test hook: the split-KV merge alone over hand-made partials (tests/test_gpu_kv8_attn.py)
extern "C" int omchat_op_attn_merge(int dtype, const float* ws, int nsplit, int q_heads, int rows, const int32_t* kv_len, int L, float scale, void* out,
                                    int split_keys, void* stream) {
  return launch_attn_merge(dtype, ws, nsplit, q_heads, rows, kv_len, L, scale, out, split_keys, S(stream));
}

// test hook: the e4m3 cache quantiser over dense caches k16 / v16 / k8 / v8 [b, Hkv, cap, 128] and scales [b, Hkv, cap]
extern "C" int omchat_op_kv_quant(int dtype, const void* k16, const void* v16, void* k8, void* v8, float* ks, float* vs, int b, int Hkv, int cap,
                                  const int32_t* pos_lo, int pos0, const int32_t* len, int max_rows, void* stream) {
  if (!k16 || !v16 || !k8 || !v8 || !ks || !vs) { omchat_set_error("omchat_op_kv_quant: null argument"); return 1; }
  if (!pos_lo && (pos0 < 0 || (int64_t)pos0 + max_rows > cap)) { omchat_set_error("omchat_op_kv_quant: rows exceed the cache capacity"); return 1; }
  return launch_kv_quant(dtype, k16, v16, k8, v8, ks, vs, b, Hkv, (int64_t)Hkv * cap * 128, (int64_t)cap * 128, (int64_t)Hkv * cap, cap, pos_lo, pos0, len,
                         max_rows, S(stream));
}

static float* rope_table_device(int max_pos, float theta) {
  std::vector<float> tab((size_t)max_pos * 128);
  for (int i = 0; i < 64; ++i) {
    const float inv = (float)(1.0 / pow((double)theta, (double)((float)(2 * i) / 128.0f)));
    for (int p = 0; p < max_pos; ++p) {
      const float ang = (float)p * inv;
      tab[((size_t)p * 64 + i) * 2] = (float)cos((double)ang);
      tab[((size_t)p * 64 + i) * 2 + 1] = (float)sin((double)ang);
    }
  }
  float* d = nullptr;
  if (hipMalloc(&d, tab.size() * 4) != hipSuccess) return nullptr;
  if (hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return nullptr; }
  return d;
}

extern "C" int omchat_op_attn_verify_tpw(int keys, int Hkv) { return attn_verify_tpw(keys, Hkv); }

extern "C" int omchat_op_attn_verify(int dtype, const void* q, void* k, void* v, void* out, int T, int Hq, int Hkv, int cap, int L, float scale,
                                     void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(q && k && v && out && ws, "null argument");
  OM_CHECK(Hkv > 0 && L >= 0 && L + T <= cap, "L + T exceeds the cache capacity");
  AttnBlockArgs a{};
  bind_dense(a, q, false, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.mode = ATTN_VERIFY; a.S = T; a.L = L;
  return launch_attn_block(dtype, a, S(stream));
}

extern "C" size_t omchat_op_attn_extend_ws(int Sq, int Hq, int Hkv, int L) { return attn_extend_ws_bytes(Sq, Hq, Hkv, L); }

extern "C" int omchat_op_attn_extend(int dtype, const void* q, const void* k, const void* v, void* out, int Sq, int Hq, int Hkv, int cap, int L,
                                     float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(q && k && v && out && ws, "null argument");
  OM_CHECK(Hkv > 0 && L >= 0 && Sq >= 1 && L + Sq <= cap, "L + Sq exceeds the cache capacity");
  AttnBlockArgs a{};
  bind_dense(a, q, false, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.mode = ATTN_EXTEND; a.S = Sq; a.L = L;
  return launch_attn_block(dtype, a, S(stream));
}

extern "C" size_t omchat_op_attn_shared_ws(int G, int N, int Hq, int Hkv, int P, int L) { return attn_shared_ws_bytes(G, N, Hq, Hkv, P, L); }

// the two shared-prompt hooks behind their own checks: kv_len = null, every row holds exactly L keys
static int op_attn_shared(int dtype, const void* q, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap, int P, int L, const int* kv_len,
                          float scale, void* ws, size_t ws_bytes, void* stream) {
  AttnBlockArgs a{};
  bind_dense(a, q, false, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.mode = ATTN_SHARED; a.G = G; a.N = N; a.P = P; a.L = L; a.kv_len = kv_len;
  return launch_attn_block(dtype, a, S(stream));
}

extern "C" int omchat_op_attn_shared(int dtype, const void* q, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap, int P, int L,
                                     float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(q && k && v && out && ws, "null argument");
  OM_CHECK(Hkv > 0 && P >= 1 && L > P && L <= cap, "1 <= P < L <= cap");
  return op_attn_shared(dtype, q, k, v, out, G, N, Hq, Hkv, cap, P, L, nullptr, scale, ws, ws_bytes, stream);
}

// omchat_op_attn_shared with the rows' true lengths (device [G N], each in [P + 1, L]): L only sizes the grid and the workspace
extern "C" int omchat_op_attn_shared_lens(int dtype, const void* q, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap, int P, int L,
                                          const int* kv_len, float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(q && k && v && out && ws && kv_len, "null argument");
  OM_CHECK(Hkv > 0 && P >= 1 && L > P && L <= cap, "1 <= P < L <= cap");
  return op_attn_shared(dtype, q, k, v, out, G, N, Hq, Hkv, cap, P, L, kv_len, scale, ws, ws_bytes, stream);
}

extern "C" size_t omchat_op_attn_suffix_ws(int N, int S, int Hq, int Hkv, int P) { return attn_suffix_ws_bytes(N, S, Hq, Hkv, P); }

// Suffix-pass attention: q / out [N, S, Hq, 128] (q rotated), complete caches [N, Hkv, cap, 128], host lengths[N] of the
// suffixes (1 .. S); kv_len_dev is N ints of device scratch that receive P + lengths[j] for the kernel
extern "C" int omchat_op_attn_suffix(int dtype, const void* q, const void* k, const void* v, void* out, int N, int S, int Hq, int Hkv, int cap, int P,
                                     const int32_t* lengths, int* kv_len_dev, float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(q && k && v && out && ws && kv_len_dev, "null argument");
  OM_CHECK(Hkv > 0 && N >= 1 && S >= 1 && P >= 1 && (int64_t)P + S <= cap, "P + S exceeds the cache capacity");
  if (lengths) {      // host lengths: checked and uploaded; null = kv_len_dev already holds P + lengths[j] (the kernel clamps them to P + S)
    std::vector<int> kl(N);
    for (int j = 0; j < N; ++j) {
      OM_CHECK(lengths[j] >= 1 && lengths[j] <= S, "suffix attention: lengths must be in [1, S]");
      kl[j] = P + lengths[j];
    }
    OM_HIP(hipMemcpyAsync(kv_len_dev, kl.data(), (size_t)N * 4, hipMemcpyHostToDevice, S(stream)));
    OM_HIP(hipStreamSynchronize(S(stream)));      // host vector
  }
  AttnBlockArgs a{};
  bind_dense(a, q, false, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.mode = ATTN_SUFFIX; a.N = N; a.S = S; a.P = P; a.kv_len = kv_len_dev;
  return launch_attn_block(dtype, a, S(stream));
}

extern "C" int omchat_op_attn_verify_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int T, int Hq, int Hkv, int cap,
                                            int L, float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(qkv && k && v && out && ws, "null argument");
  OM_CHECK(Hkv > 0 && L >= 0 && T >= 1 && L + T <= cap, "L + T exceeds the cache capacity");
  float* tab = rope_table_device(L + T, theta);
  OM_CHECK(tab, "rope table allocation failed");
  AttnBlockArgs a{};
  bind_dense(a, qkv, true, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  bind_new_rows(a, tab, L + T);
  a.mode = ATTN_VERIFY; a.S = T; a.L = L;
  const int rc = launch_attn_block(dtype, a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(tab);
  return rc;
}

// test hook (tests/test_gpu_attn_block_rows.py): the shared-prompt decode attention WITH its fused RoPE + append, as omchat_decode_step issues it over
// a sampled group: qkv [G N][(Hq + 2 Hkv) * 128] raw projections (read-only); row r holds kv_len[r] keys counting the new one (NULL: L), q is rotated
// at kv_len[r] - 1 and the rotated k / raw v go to that slot of row r's own cache (omchat_op_rope_kv_pos's bytes).  Synchronises.
extern "C" int omchat_op_attn_shared_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int G, int N, int Hq, int Hkv, int cap,
                                            int P, int L, const int32_t* kv_len, float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(qkv && k && v && out && ws, "null argument");
  OM_CHECK(Hkv > 0 && G >= 1 && N >= 1 && P >= 1 && L > P && L <= cap, "1 <= P < L <= cap");
  float* tab = rope_table_device(L, theta);
  OM_CHECK(tab, "rope table allocation failed");
  AttnBlockArgs a{};
  bind_dense(a, qkv, true, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  bind_new_rows(a, tab, L);
  a.mode = ATTN_SHARED; a.G = G; a.N = N; a.P = P; a.L = L; a.kv_len = kv_len;
  const int rc = launch_attn_block(dtype, a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(tab);
  return rc;
}

// test hook: the plan launch_attn_block takes on the current device for a mode (0 verify, 1 extend, 2 shared, 3 suffix) and its integers (those the
// mode does not name are ignored): out = {tpw, nsp, nss, tps}.  Pure: launches nothing.
extern "C" int omchat_op_attn_block_plan(int mode, int G, int N, int S, int Hq, int Hkv, int P, int L, int* out) {
  OM_CHECK(out && mode >= ATTN_VERIFY && mode <= ATTN_SUFFIX && Hq >= 1 && Hkv >= 1, "bad mode, heads or null output");
  return attn_block_plan_query(mode, G, N, S, Hq, Hkv, P, L, out);
}

// One decode step's attention over the e4m3 cache INCLUDING the new token's RoPE + append, as the decoder layer issues it (model.hip): qkv
// [b][(Hq + 2 Hkv) * 128] raw projections of the new token; sequence i holds kv_len[i] keys counting the new one (NULL: L for every sequence), the
// new row goes to position kv_len[i] - 1 of k8 / v8 / ks / vs and of the 16-bit caches k16 / v16.  Long launches take the walking form, which does
// the rotation, the append and the quantisation itself (tuning keys 47 / 48); the others run omchat_op_rope_kv_q8's launch in front (q rotated in
// place in qkv then).  pos = kv_len - 1 as a device array (needed by that launch when kv_len != NULL).
extern "C" int omchat_op_attn_decode_kv8_append(int dtype, void* qkv, float theta, void* k8, void* v8, float* ks, float* vs, void* k16, void* v16,
                                                void* out, int b, int Hq, int Hkv, int cap, int L, const int32_t* kv_len, const int32_t* pos, float scale,
                                                void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(qkv && k8 && v8 && ks && vs && k16 && v16 && out, "null argument");
  OM_CHECK(L >= 1 && L <= cap, "L exceeds the cache capacity");
  OM_CHECK((kv_len == nullptr) == (pos == nullptr), "kv_len and pos come together");
  float* tab = rope_table_device(L, theta);
  OM_CHECK(tab, "rope table allocation failed");
  const int qkvd = (Hq + 2 * Hkv) * 128;
  AttnDecodeArgs a{};
  bind_dense(a, qkv, true, k8, v8, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  a.k_scale = ks; a.v_scale = vs; a.scale_sb = (int64_t)Hkv * cap; a.scale_sh = cap;
  a.batch = b; a.L = L; a.kv_len = kv_len;
  int rc = 0;
  if (attn_decode_kv8_fuses_rope(b, Hkv, L, false)) {
    bind_new_rows(a, tab, L);
    a.k16_w = k16; a.v16_w = v16;
  } else {
    RopeArgs r{qkv, qkvd, b, 1, Hq, Hkv, pos, L - 1, tab, L, k16, v16, (int64_t)Hkv * cap * 128, (int64_t)cap * 128};
    r.k8 = k8; r.v8 = v8; r.ks = ks; r.vs = vs; r.s_sb = (int64_t)Hkv * cap; r.s_sh = cap;
    rc = launch_rope_kv(dtype, r, S(stream));
  }
  if (!rc) rc = launch_attn_decode(dtype, a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(tab);
  return rc;
}

// The same step over the 16-bit cache, as the decoder layer issues it (model.hip, ctx.h bind_attn): q rotated in registers, the split that owns
// the new position rotates the fresh key and appends k / v (rope_kv_kernel's bytes, slot kv_len[i] - 1, which is also the RoPE position).  With
// key_mask (device bytes [b][mask_sb], the padded batch; kv_len must be NULL) the RoPE position of row i is pos[i] and the slot L - 1 for every
// row.  pack_nb != 0: out in the packed x layout (common.h).  qkv is read-only.  Synchronises.
extern "C" int omchat_op_attn_decode_append(int dtype, const void* qkv, float theta, void* k, void* v, void* out, int b, int Hq, int Hkv, int cap,
                                            int L, const int32_t* kv_len, const int32_t* pos, const unsigned char* key_mask, int64_t mask_sb,
                                            int pack_nb, float scale, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(qkv && k && v && out && ws, "null argument");
  OM_CHECK(b >= 1 && Hq >= 1 && Hkv >= 1, "empty attention");
  OM_CHECK(L >= 1 && L <= cap, "L exceeds the cache capacity");
  OM_CHECK(!key_mask || pos, "key_mask needs the RoPE positions (pos)");
  OM_CHECK(!key_mask || !kv_len, "key_mask: every row holds L keys (kv_len must be null)");
  float* tab = rope_table_device(L, theta);
  OM_CHECK(tab, "rope table allocation failed");
  AttnDecodeArgs a{};
  bind_dense(a, qkv, true, k, v, out, Hq, Hkv, cap, scale, ws, ws_bytes);
  bind_new_rows(a, tab, L);
  a.batch = b; a.L = L; a.kv_len = kv_len; a.pos = pos; a.key_mask = key_mask; a.mask_sb = mask_sb; a.o_pack_nb = pack_nb;
  const int rc = launch_attn_decode(dtype, a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(tab);
  return rc;
}

static int op_rope_kv_impl(int dtype, void* qkv, int b, int Sq, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache, int cap,
                           void* k8, void* v8, float* ks, float* vs, void* stream);
extern "C" int omchat_op_rope_kv(int dtype, void* qkv, int b, int Sq, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache, int cap,
                                 void* stream) {
  return op_rope_kv_impl(dtype, qkv, b, Sq, Hq, Hkv, pos0, theta, kcache, vcache, cap, nullptr, nullptr, nullptr, nullptr, stream);
}
// the same with the appended rows also quantised to the e4m3 cache (k8 / v8 [b, Hkv, cap, 128] bytes, ks / vs [b, Hkv, cap] fp32 scales):
// what a decode step with the fp8 KV cache launches (round 3; before: RoPE + append, then a quantiser launch over the new rows)
extern "C" int omchat_op_rope_kv_q8(int dtype, void* qkv, int b, int Sq, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache, int cap,
                                    void* k8, void* v8, float* ks, float* vs, void* stream) {
  OM_CHECK(k8 && v8 && ks && vs, "null fp8 cache argument");
  return op_rope_kv_impl(dtype, qkv, b, Sq, Hq, Hkv, pos0, theta, kcache, vcache, cap, k8, v8, ks, vs, stream);
}
static int op_rope_kv_impl(int dtype, void* qkv, int b, int Sq, int Hq, int Hkv, int pos0, float theta, void* kcache, void* vcache, int cap,
                           void* k8, void* v8, float* ks, float* vs, void* stream) {
  OM_CHECK(pos0 + Sq <= cap, "positions exceed cache capacity");
  const int max_pos = pos0 + Sq;
  float* d = rope_table_device(max_pos, theta);
  OM_CHECK(d, "rope table allocation failed");
  RopeArgs r{qkv, (Hq + 2 * Hkv) * 128, b * Sq, Sq, Hq, Hkv, nullptr, pos0, d, max_pos, kcache, vcache, (int64_t)Hkv * cap * 128, (int64_t)cap * 128};
  r.k8 = k8; r.v8 = v8; r.ks = ks; r.vs = vs; r.s_sb = (int64_t)Hkv * cap; r.s_sh = cap;
  int rc = launch_rope_kv(dtype, r, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(d);
  return rc;
}

extern "C" int omchat_op_argmax(const float* logits, int b, int V, int32_t* out, void* stream) {
  void* scratch = nullptr;
  OM_HIP(hipMalloc(&scratch, argmax_scratch_bytes(b)));
  int rc = launch_argmax(logits, V, b, V, out, scratch, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(scratch);
  return rc;
}

static int op_sample(const float* logits, int b, int V, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                     const SampleFilters& flt, const int32_t* seen_ids, const int32_t* n_seen_per_row, int step, int32_t* out, uint32_t* thr_out,
                     uint32_t* hi_out, void* stream) {
  OM_CHECK(logits && out && b >= 1 && V >= 1, "bad argument");
  OM_CHECK(temperature > 0.f && top_k >= 0 && top_p > 0.0 && top_p <= 1.0 && rep_penalty > 0.f, "sampling parameters out of range");
  const int bmw = (V + 31) / 32;
  std::vector<uint32_t> bm((size_t)b * bmw, 0u);
  if (rep_penalty != 1.f && seen_ids && n_seen_per_row) {
    size_t off = 0;
    for (int i = 0; i < b; ++i) {
      for (int j = 0; j < n_seen_per_row[i]; ++j) {
        const int id = seen_ids[off + j];
        if (id >= 0 && id < V) bm[(size_t)i * bmw + (id >> 5)] |= 1u << (id & 31);
      }
      off += (size_t)n_seen_per_row[i];
    }
  }
  std::vector<int> steps(b, step);
  const size_t ws_bytes = sample_ws_bytes(b);
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, ws_bytes + bm.size() * 4 + (size_t)b * 8));
  uint32_t* d_bm = (uint32_t*)(mem + ws_bytes);
  int* d_last = (int*)(mem + ws_bytes + bm.size() * 4);
  int* d_step = d_last + b;
  hipMemcpyAsync(d_bm, bm.data(), bm.size() * 4, hipMemcpyHostToDevice, S(stream));
  hipMemcpyAsync(d_step, steps.data(), (size_t)b * 4, hipMemcpyHostToDevice, S(stream));
  SampleArgs a;
  a.logits = logits; a.ld = V; a.b = b; a.V = V; a.V_total = V;
  a.seed = seed; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.penalty = rep_penalty;
  if (rep_penalty != 1.f) { a.bitmap = d_bm; a.bm_words = bmw; }
  a.last_set = d_last; a.step = d_step; a.out = out; a.thr_out = thr_out; a.hi_out = hi_out; a.ws = mem;
  a.f = flt;
  int rc = launch_sample(a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(mem);
  return rc;
}

extern "C" int omchat_op_sample(const float* logits, int b, int V, uint64_t seed, float temperature, int top_k, double top_p, float rep_penalty,
                                const int32_t* seen_ids, const int32_t* n_seen_per_row, int step, int32_t* out, uint32_t* thr_out, void* stream) {
  return op_sample(logits, b, V, seed, temperature, top_k, top_p, rep_penalty, SampleFilters{}, seen_ids, n_seen_per_row, step, out, thr_out,
                   nullptr, stream);
}

extern "C" int omchat_op_sample_filtered(const float* logits, int b, int V, uint64_t seed, float temperature, int top_k, double top_p,
                                         float rep_penalty, double min_p, double typical_p, double epsilon_cutoff, double eta_cutoff,
                                         const int32_t* seen_ids, const int32_t* n_seen_per_row, int step, int32_t* out, uint32_t* thr_lo,
                                         uint32_t* thr_hi, void* stream) {
  OM_CHECK(!(min_p > 1.0) && min_p == min_p && typical_p > 0.0 && epsilon_cutoff > 0.0 && eta_cutoff > 0.0, "sampling filter parameters out of range");
  SampleFilters f;
  f.min_p = min_p < 0.0 ? -1.0 : min_p;
  f.typical_p = typical_p < 1.0 ? typical_p : 1.0;
  f.epsilon = epsilon_cutoff < 1.0 ? epsilon_cutoff : 1.0;
  f.eta = eta_cutoff < 1.0 ? eta_cutoff : 1.0;
  return op_sample(logits, b, V, seed, temperature, top_k, top_p, rep_penalty, f, seen_ids, n_seen_per_row, step, out, thr_lo, thr_hi, stream);
}

extern "C" int omchat_op_sample_verify(const float* logits, int T, int V, int ld, const int32_t* tokens, uint64_t seed, int base_step,
                                       float temperature, int top_k, double top_p, float rep_penalty, double min_p, double typical_p,
                                       double epsilon_cutoff, double eta_cutoff, const int32_t* seen_ids, int n_seen, int rank, int V_total,
                                       int32_t* out, uint32_t* thr_lo, uint32_t* thr_hi, void* stream) {
  OM_CHECK(logits && tokens && out && T >= 2 && T <= SMP_VERIFY_ROWS && V >= 1 && ld >= V, "bad argument");
  OM_CHECK(rank >= 0 && V_total >= V && (int64_t)rank * V + V <= (int64_t)V_total, "the slice must lie inside the vocabulary");
  OM_CHECK(temperature > 0.f && top_k >= 0 && top_p > 0.0 && top_p <= 1.0 && rep_penalty > 0.f, "sampling parameters out of range");
  OM_CHECK(!(min_p > 1.0) && min_p == min_p && typical_p > 0.0 && epsilon_cutoff > 0.0 && eta_cutoff > 0.0, "sampling filter parameters out of range");
  OM_CHECK(n_seen >= 0 && (n_seen == 0 || seen_ids), "bad argument");
  SampleFilters f;
  f.min_p = min_p < 0.0 ? -1.0 : min_p;
  f.typical_p = typical_p < 1.0 ? typical_p : 1.0;
  f.epsilon = epsilon_cutoff < 1.0 ? epsilon_cutoff : 1.0;
  f.eta = eta_cutoff < 1.0 ? eta_cutoff : 1.0;
  const int bmw = (V + 31) / 32;
  std::vector<uint32_t> bm(bmw, 0u);
  const int64_t lo = (int64_t)rank * V;
  for (int j = 0; j < n_seen; ++j) {
    const int64_t li = (int64_t)seen_ids[j] - lo;
    if (seen_ids[j] >= 0 && seen_ids[j] < V_total && li >= 0 && li < V) bm[li >> 5] |= 1u << (li & 31);
  }
  const size_t ws_bytes = sample_ws_bytes(T), bmb = (size_t)bmw * 4;
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, ws_bytes + bmb * (1 + SMP_VERIFY_ROWS) + 16));
  uint32_t* d_bm = (uint32_t*)(mem + ws_bytes);
  uint32_t* d_vseen = d_bm + bmw;
  int* d_step = (int*)(d_vseen + (size_t)SMP_VERIFY_ROWS * bmw);
  hipMemcpyAsync(d_bm, bm.data(), bmb, hipMemcpyHostToDevice, S(stream));
  hipMemcpyAsync(d_step, &base_step, 4, hipMemcpyHostToDevice, S(stream));
  SampleArgs a;
  a.logits = logits; a.ld = ld; a.b = T; a.V = V; a.V_total = V_total; a.rank = rank;
  a.seed = seed; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.penalty = rep_penalty;
  if (rep_penalty != 1.f) { a.bitmap = d_bm; a.bm_words = bmw; a.vseen = d_vseen; }
  a.step = d_step; a.vtokens = tokens; a.out = out; a.thr_out = thr_lo; a.hi_out = thr_hi; a.ws = mem;
  a.f = f;
  int rc = launch_sample(a, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(mem);
  return rc;
}

static int op_token_logprob(const float* logits, int b, int V, int ld, const int32_t* ids, const uint32_t* ban, float temperature,
                            float rep_penalty, const int32_t* seen_ids, const int32_t* n_seen_per_row, const int32_t* newly_seen,
                            const uint32_t* thr, const uint32_t* thr_hi, float* raw_out, float* processed_out, void* stream) {
  OM_CHECK(logits && ids && raw_out && processed_out && b >= 1 && V >= 1 && ld >= V, "bad argument");
  OM_CHECK(temperature > 0.f && rep_penalty > 0.f, "sampling parameters out of range");
  const int bmw = (V + 31) / 32;
  std::vector<uint32_t> bm((size_t)b * bmw, 0u);
  std::vector<int> last(b, -1);
  const bool pen = rep_penalty != 1.f && seen_ids && n_seen_per_row;
  size_t off = 0;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(ids[i] >= 0 && ids[i] < V, "picked id outside the vocabulary");
    if (!pen) continue;
    for (int j = 0; j < n_seen_per_row[i]; ++j) {
      const int id = seen_ids[off + j];
      if (id >= 0 && id < V) bm[(size_t)i * bmw + (id >> 5)] |= 1u << (id & 31);
    }
    off += (size_t)n_seen_per_row[i];
    if (newly_seen && newly_seen[i]) {      // as smp_commit leaves it: the bit set, its index remembered
      bm[(size_t)i * bmw + (ids[i] >> 5)] |= 1u << (ids[i] & 31);
      last[i] = ids[i];
    }
  }
  hipStream_t s = S(stream);
  const size_t wsb = logprob_ws_bytes(b), bmb = bm.size() * 4, rb = ((size_t)b * 4 + 15) / 16 * 16;
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, wsb + bmb + 5 * rb));
  uint32_t* d_bm = (uint32_t*)(mem + wsb);
  int* d_ids = (int*)(mem + wsb + bmb);
  int* d_last = (int*)(mem + wsb + bmb + rb);
  int* d_cnt = (int*)(mem + wsb + bmb + 2 * rb);
  float* d_rec = (float*)(mem + wsb + bmb + 3 * rb);      // [2][1][b]
  hipMemcpyAsync(d_bm, bm.data(), bmb, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_ids, ids, (size_t)b * 4, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_last, last.data(), (size_t)b * 4, hipMemcpyHostToDevice, s);
  hipMemsetAsync(d_cnt, 0, (size_t)b * 4, s);
  LogprobArgs a;
  a.raw = logits; a.raw_ld = ld; a.b = b; a.V = V; a.ids = d_ids; a.ban = ban; a.bm_words = bmw;
  if (pen) { a.seen = d_bm; a.last_set = d_last; }
  a.temperature = temperature; a.penalty = rep_penalty; a.thr = thr; a.thr_hi = thr_hi; a.thr_stride = 1;
  a.ws = mem; a.rec = d_rec; a.cnt = d_cnt; a.max_new = 1; a.rec_ld = b;
  int rc = launch_logprob(a, s);
  if (!rc) {
    hipMemcpyAsync(raw_out, d_rec, (size_t)b * 4, hipMemcpyDeviceToDevice, s);
    hipMemcpyAsync(processed_out, d_rec + b, (size_t)b * 4, hipMemcpyDeviceToDevice, s);
  }
  hipStreamSynchronize(s);
  hipFree(mem);
  return rc;
}

extern "C" int omchat_op_token_logprob(const float* logits, int b, int V, int ld, const int32_t* ids, const uint32_t* ban, float temperature,
                                       float rep_penalty, const int32_t* seen_ids, const int32_t* n_seen_per_row, const int32_t* newly_seen,
                                       const uint32_t* thr, float* raw_out, float* processed_out, void* stream) {
  return op_token_logprob(logits, b, V, ld, ids, ban, temperature, rep_penalty, seen_ids, n_seen_per_row, newly_seen, thr, nullptr, raw_out,
                          processed_out, stream);
}

extern "C" size_t omchat_op_lse_label_ws(int M, int N) { return M >= 1 && N >= 1 ? score_ws_bytes(M, N) : 0; }

extern "C" int omchat_op_lse_label(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int32_t* labels,
                                   float* logprob, float* lse, void* ws, size_t ws_bytes, void* stream) {
  OM_CHECK(A && W && labels && logprob && ws, "null argument");
  OM_CHECK(M >= 1 && N >= 1 && K >= 1, "empty problem");
  OM_CHECK(N % 4 == 0 && K % 64 == 0, "N must be a multiple of 4 and K a multiple of 64 (omchat_op_gemm's contract)");
  std::vector<int32_t> h((size_t)M);
  OM_HIP(hipMemcpyAsync(h.data(), labels, (size_t)M * 4, hipMemcpyDeviceToHost, S(stream)));
  OM_HIP(hipStreamSynchronize(S(stream)));
  for (int i = 0; i < M; ++i) OM_CHECK(h[i] == -100 || (h[i] >= 0 && h[i] < N), "label outside {-100} and [0, N)");
  return launch_score(dtype, A, lda, W, ldw, M, N, K, labels, logprob, lse, ws, ws_bytes, S(stream));
}

extern "C" int omchat_op_token_logprob_interval(const float* logits, int b, int V, int ld, const int32_t* ids, const uint32_t* ban,
                                                float temperature, float rep_penalty, const int32_t* seen_ids, const int32_t* n_seen_per_row,
                                                const int32_t* newly_seen, const uint32_t* thr_lo, const uint32_t* thr_hi, float* raw_out,
                                                float* processed_out, void* stream) {
  return op_token_logprob(logits, b, V, ld, ids, ban, temperature, rep_penalty, seen_ids, n_seen_per_row, newly_seen, thr_lo, thr_hi, raw_out,
                          processed_out, stream);
}

extern "C" int omchat_op_top_logprobs(const float* logits, int b, int V, int ld, int top_n, const int32_t* score_ids, int n_score, float* top_vals,
                                      int32_t* top_ids, float* scored, void* stream) {
  OM_CHECK(logits && b >= 1 && V >= 1 && ld >= V, "bad argument");
  OM_CHECK(top_n >= 0 && top_n <= OMCHAT_LP_MAX_TOP && top_n <= V, "0 <= top_n <= 20, at most the vocabulary");
  OM_CHECK(n_score >= 0 && n_score <= OMCHAT_LP_MAX_SCORED && (top_n > 0 || n_score > 0), "0 <= n_score <= 32, and one of the two extras");
  OM_CHECK((!top_n || (top_vals && top_ids)) && (!n_score || (score_ids && scored)), "an extra without its output");
  for (int i = 0; i < n_score; ++i) {
    OM_CHECK(score_ids[i] >= 0 && score_ids[i] < V, "scored id outside the vocabulary");
    for (int j = 0; j < i; ++j) OM_CHECK(score_ids[j] != score_ids[i], "scored ids must be distinct");
  }
  hipStream_t s = S(stream);
  const size_t wsb = logprob_ws_bytes(b), xwb = (logprob_top_ws_bytes(b, top_n) + 15) / 16 * 16, rb = ((size_t)b * 4 + 15) / 16 * 16;
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, wsb + xwb + 4 * rb + (size_t)OMCHAT_LP_MAX_SCORED * 4));
  int* d_ids = (int*)(mem + wsb + xwb);      // the picked id of every row: 0 (its record is not read)
  int* d_cnt = (int*)(mem + wsb + xwb + rb);
  float* d_rec = (float*)(mem + wsb + xwb + 2 * rb);      // [2][1][b]
  int* d_sid = (int*)(mem + wsb + xwb + 4 * rb);
  hipMemsetAsync(d_ids, 0, 2 * rb, s);
  if (n_score) hipMemcpyAsync(d_sid, score_ids, (size_t)n_score * 4, hipMemcpyHostToDevice, s);
  LogprobArgs a;
  a.raw = logits; a.raw_ld = ld; a.b = b; a.V = V; a.ids = d_ids;
  a.ws = mem; a.rec = d_rec; a.cnt = d_cnt; a.max_new = 1; a.rec_ld = b;
  a.top_n = top_n; a.n_score = n_score; a.score_ids = d_sid; a.top_ws = mem + wsb;
  a.top_vals = top_vals; a.top_ids = top_ids; a.scored = scored;      // line 0 of a one-line record is the output's layout
  int rc = launch_logprob(a, s);
  hipStreamSynchronize(s);
  hipFree(mem);
  return rc;
}

static_assert(DOLA_MAX_LAYERS == OMCHAT_DOLA_MAX_LAYERS, "layer-contrastive decoding cap: kernels.h and omchat_hip.h");
static_assert(LP_MAX_TOP == OMCHAT_LP_MAX_TOP && LP_MAX_SCORED == OMCHAT_LP_MAX_SCORED, "log-prob extras caps: kernels.h and omchat_hip.h");
static_assert(CON_NGRAM_MAX == OMCHAT_CON_MAX_NGRAM && CON_EOS_MAX == OMCHAT_CON_MAX_EOS && CON_SUPPRESS_MAX == OMCHAT_CON_MAX_SUPPRESS &&
              CON_BAD_WORDS_MAX == OMCHAT_CON_MAX_BAD_WORDS && CON_BAD_WORD_IDS_MAX == OMCHAT_CON_MAX_BAD_WORD_IDS, "constraint caps: kernels.h and omchat_hip.h");

extern "C" int omchat_op_constrain(const int32_t* hist_ids, const int32_t* hist_len, const int32_t* prompt_len, int b, int V, int V_total, int rank,
                                   int fed_last, int no_repeat_ngram_size, int min_new_tokens, int min_length, const int32_t* eos_ids, int n_eos,
                                   const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids, int n_begin_suppress,
                                   const int32_t* bad_word_ids, const int32_t* bad_word_offsets, int n_bad_words, uint32_t* ban_out, void* stream) {
  OM_CHECK(hist_ids && hist_len && prompt_len && ban_out && b >= 1 && V >= 1 && V_total >= V && rank >= 0, "bad argument");
  OM_CHECK(no_repeat_ngram_size >= 0 && no_repeat_ngram_size <= CON_NGRAM_MAX && min_new_tokens >= 0 && min_length >= 0, "constraint parameters out of range");
  int maxL = 0;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(hist_len[i] >= (fed_last ? 1 : 0) && prompt_len[i] >= 0, "history lengths out of range");
    maxL = std::max(maxL, hist_len[i]);
  }
  ConstrainArgs a;
  std::vector<int32_t> lists(CON_LIST_WORDS);
  if (int rc = constrain_pack_lists(eos_ids, n_eos, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_word_ids, bad_word_offsets,
                                    n_bad_words, lists.data(), a)) return rc;
  const int ld = (maxL + 4) / 4 * 4, bmw = (V + 31) / 32;
  // the rows as the context keeps them: fed_last holds each row's last id back as the token the step is fed
  std::vector<int32_t> h((size_t)b * ld, 0), len(b), tok(b, 0);
  size_t off = 0;
  for (int i = 0; i < b; ++i) {
    len[i] = hist_len[i] - (fed_last ? 1 : 0);
    std::copy(hist_ids + off, hist_ids + off + len[i], h.begin() + (size_t)i * ld);
    if (fed_last) tok[i] = hist_ids[off + len[i]];
    off += (size_t)hist_len[i];
  }
  hipStream_t s = S(stream);
  char* mem = nullptr;
  const size_t hb = h.size() * 4, lb = lists.size() * 4, rb = ((size_t)b * 4 + 15) / 16 * 16;
  OM_HIP(hipMalloc(&mem, hb + lb + 3 * rb));
  int32_t* d_h = (int32_t*)mem;
  int32_t* d_lists = (int32_t*)(mem + hb);
  int* d_len = (int*)(mem + hb + lb);
  int* d_plen = (int*)(mem + hb + lb + rb);
  int32_t* d_tok = (int32_t*)(mem + hb + lb + 2 * rb);
  hipMemcpyAsync(d_h, h.data(), hb, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_lists, lists.data(), lb, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_len, len.data(), (size_t)b * 4, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_plen, prompt_len, (size_t)b * 4, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_tok, tok.data(), (size_t)b * 4, hipMemcpyHostToDevice, s);
  hipMemsetAsync(ban_out, 0, (size_t)b * bmw * 4, s);
  a.hist = d_h; a.hist_ld = ld; a.len = d_len; a.plen = d_plen; a.tok = fed_last ? d_tok : nullptr;
  a.b = b; a.V = V; a.V_total = V_total; a.gbase = rank * V;
  a.ngram = no_repeat_ngram_size; a.min_new = min_new_tokens; a.min_len = min_length;
  constrain_bind_lists(d_lists, a);
  a.ban = ban_out; a.bmw = bmw;
  int rc = launch_constrain_ban(a, s);
  hipStreamSynchronize(s);
  hipFree(mem);
  return rc;
}

static_assert(FSM_MAX_STATES == OMCHAT_FSM_MAX_STATES && FSM_MAX_EDGES == OMCHAT_FSM_MAX_EDGES && FSM_DEAD == OMCHAT_FSM_DEAD, "token FSM caps: kernels.h and omchat_hip.h");

extern "C" int omchat_op_fsm(int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, const int32_t* states, const int32_t* fed,
                             int b, int V, int V_total, int rank, const float* logits, float* out, int32_t* new_states, void* stream) {
  OM_CHECK(states && logits && out && new_states && b >= 1 && V >= 1 && V_total >= V && rank >= 0 && (int64_t)(rank + 1) * V <= V_total, "bad argument");
  if (int rc = fsm_validate(n_states, off, tok, nxt, V_total)) return rc;
  for (int i = 0; i < b; ++i) {
    OM_CHECK(states[i] == FSM_DEAD || (states[i] >= 0 && states[i] < n_states), "state outside the table");
    OM_CHECK(states[i] == FSM_DEAD || off[states[i] + 1] > off[states[i]], "state without an edge: every id would be -inf; add an EOS edge");
  }
  const size_t E = (size_t)off[n_states];
  const size_t n_off = ((size_t)n_states + 1 + 3) / 4 * 4, n_tok = (E + 3) / 4 * 4 + 4, rb = ((size_t)b + 3) / 4 * 4;
  const int bmw = (V + 31) / 32;
  // the rows as the context keeps them: a trail of two slots, the given state in slot 0
  std::vector<int32_t> trail((size_t)b * 2, 0);
  for (int i = 0; i < b; ++i) trail[(size_t)i * 2] = states[i];
  hipStream_t s = S(stream);
  int32_t* mem = nullptr;
  const size_t words = n_off + n_tok + E + 4 + 2 * rb + 3 * rb + (size_t)b * bmw;
  OM_HIP(hipMalloc(&mem, words * 4));
  int32_t* d_off = mem;
  int32_t* d_tok = mem + n_off;
  int32_t* d_nxt = d_tok + n_tok;
  int32_t* d_trail = d_nxt + E + 4;
  int32_t* d_cnt = d_trail + 2 * rb;
  int32_t* d_cur = d_cnt + rb;
  int32_t* d_fed = d_cur + rb;
  uint32_t* d_bm = (uint32_t*)(d_fed + rb);
  hipMemsetAsync(mem, 0, words * 4, s);
  hipMemcpyAsync(d_off, off, ((size_t)n_states + 1) * 4, hipMemcpyHostToDevice, s);
  if (E) {
    hipMemcpyAsync(d_tok, tok, E * 4, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(d_nxt, nxt, E * 4, hipMemcpyHostToDevice, s);
  }
  hipMemcpyAsync(d_trail, trail.data(), trail.size() * 4, hipMemcpyHostToDevice, s);
  if (fed) hipMemcpyAsync(d_fed, fed, (size_t)b * 4, hipMemcpyHostToDevice, s);
  FsmTable T;
  T.off = d_off; T.tok = d_tok; T.nxt = d_nxt; T.n_states = n_states;
  FsmArgs a;
  a.trail = d_trail; a.cap = 2; a.cnt = d_cnt; a.cur = d_cur; a.fed = fed ? d_fed : nullptr;
  a.b = b; a.V = V; a.gbase = rank * V; a.bm = d_bm; a.bmw = bmw;
  int rc = launch_fsm_mark(T, a, s);
  if (!rc) rc = launch_fsm_apply(logits, V, a, out, fed != nullptr, s);
  // the states as omchat_fsm_states reads them: trail[cnt]
  std::vector<int32_t> cnt(b, 0);
  if (!rc && hipMemcpyAsync(cnt.data(), d_cnt, (size_t)b * 4, hipMemcpyDeviceToHost, s) != hipSuccess) rc = 2;
  if (!rc && hipMemcpyAsync(trail.data(), d_trail, trail.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess) rc = 2;
  hipStreamSynchronize(s);
  hipFree(mem);
  if (!rc)
    for (int i = 0; i < b; ++i) {
      OM_CHECK(cnt[i] == (fed ? 1 : 0), "omchat_op_fsm: the count did not follow the fed token");
      new_states[i] = trail[(size_t)i * 2 + cnt[i]];
    }
  return rc;
}

extern "C" size_t omchat_op_guidance_ws(int b, int V) { return b >= 1 && V >= 1 ? guidance_ws_bytes(b, V) : 0; }

extern "C" int omchat_op_guidance(const float* logits, int ld, int b, int V, float scale, void* ws, float* out, int ld_out, void* stream) {
  return launch_guidance(logits, ld, b, V, scale, ws, out, ld_out, S(stream));
}

static_assert(OMCHAT_CS_MAX_K == CS_KMAX && OMCHAT_CS_REC_WORDS == CS_REC_WORDS, "contrastive search: the public header's caps");
extern "C" int omchat_op_contrastive_plan(int L, int* chunks, int* rows_per_chunk) {
  OM_CHECK(L >= 1 && chunks && rows_per_chunk, "contrastive plan: L >= 1");
  cs_plan(L, device_cus(), chunks, rows_per_chunk);
  return 0;
}
extern "C" int omchat_op_contrastive_penalty(int dtype, void* hist, float* inv, int compute_norms, int L, int H, const void* cand, int cand_nb, int k,
                                             float* part, float* cand_inv, void* stream) {
  if (compute_norms) { const int rc = launch_cs_norms(dtype, hist, L, H, inv, S(stream)); if (rc) return rc; }
  return launch_cs_penalty(dtype, hist, inv, L, H, cand, cand_nb, k, part, cand_inv, S(stream));
}
extern "C" size_t omchat_op_contrastive_topk_ws(int V) { return V >= 1 ? cs_topk_ws_bytes(V) : 0; }
extern "C" int omchat_op_contrastive_topk(const float* logits, int ld, const int32_t* row_sel, int V, int k, int32_t* ids, float* probs, void* ws,
                                          void* stream) {
  return launch_cs_topk(logits, ld, row_sel, V, k, ids, probs, ws, S(stream));
}
extern "C" int omchat_op_contrastive_select(int dtype, const float* part, int chunks, int k, double alpha, const int32_t* ids, const float* probs,
                                            const float* cand_inv, const void* cand, int cand_nb, int H, void* hist, float* inv, int n_hist,
                                            const int32_t* eos_ids, int n_eos, int last, int32_t* rec, int32_t* parents, int32_t* sel, int32_t* token,
                                            int32_t* done_word, void* stream) {
  OM_CHECK(n_eos >= 0 && n_eos <= CS_EOS_MAX && (n_eos == 0 || eos_ids), "contrastive select: at most 8 eos ids");
  CsSelectArgs a;
  a.part = part; a.chunks = chunks; a.k = k; a.alpha = (float)alpha; a.one_minus_alpha = (float)(1.0 - alpha);
  a.ids = ids; a.probs = probs; a.cand_inv = cand_inv; a.cand = cand; a.cand_nb = cand_nb; a.H = H;
  a.hist = hist; a.inv = inv; a.n_hist = n_hist;
  a.n_eos = n_eos;
  for (int q = 0; q < n_eos; ++q) a.eos[q] = eos_ids[q];
  a.last = last; a.rec = rec; a.parents = parents; a.sel = sel; a.token = token; a.done_word = done_word;
  return launch_cs_select(dtype, a, S(stream));
}

extern "C" size_t omchat_op_dola_ws(int b, int k, int V) { return b >= 1 && k >= 1 && V >= 1 ? dola_ws_bytes(b, k, V) : 0; }

extern "C" int omchat_op_dola(const float* logits, int ld, int V, int b, int k, float relative_top, float* out, int ld_out, int32_t* picked, void* ws,
                              size_t ws_bytes, void* stream) {
  DolaArgs a;
  a.logits = logits; a.ld = ld; a.V = V; a.b = b; a.k = k; a.relative_top = relative_top;
  a.out = out; a.ld_out = ld_out; a.picked = picked; a.ws = ws; a.ws_bytes = ws_bytes;
  return launch_dola(a, S(stream));
}

extern "C" size_t omchat_beam_state_words(int b, int N, int max_new) { return beam_state_words(b, N, max_new); }

extern "C" int omchat_op_beam_select(const float* logits, int rows, int V, int b, int N, int t, int max_new, float length_penalty,
                                     int early_stopping, const int32_t* eos_ids, int n_eos, int32_t* state, int32_t* tokens, int32_t* parents,
                                     int32_t* done_word, void* stream) {
  OM_CHECK(logits && state && tokens && parents && b >= 1 && N >= 2 && N <= BEAM_NMAX, "bad argument");
  OM_CHECK(n_eos >= 0 && n_eos <= BEAM_EOS_MAX && (n_eos == 0 || eos_ids), "at most 8 eos ids");
  const int KB = std::max(2, 1 + n_eos) * N;
  OM_CHECK(KB <= BEAM_KMAX && V >= KB, "max(2, 1 + n_eos) * N must not exceed 32 (nor V)");
  OM_CHECK(t >= 0 && t < max_new && rows == (t == 0 ? b : b * N), "rows = b at t = 0, b * N afterwards");
  OM_CHECK(early_stopping >= 0 && early_stopping <= 2, "early_stopping 0, 1 or 2");
  const int ns = beam_slices(V, 1);
  OM_CHECK(ns >= 1, "vocabulary cannot be sliced");
  const size_t TS = (size_t)ns * (4 + 2 * KB);
  std::vector<float> dn(max_new + 1, 1.f);
  for (int g = 1; g <= max_new; ++g) dn[g] = (float)pow((double)g, (double)length_penalty);
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, rows * TS * 4 + dn.size() * 4));
  float* table = (float*)mem;
  float* d_dn = table + rows * TS;
  hipStream_t s = S(stream);
  hipMemcpyAsync(d_dn, dn.data(), dn.size() * 4, hipMemcpyHostToDevice, s);
  int rc = launch_beam_select(logits, V, rows, V, 0, 1, ns, KB, table, s);
  if (!rc) {
    BeamFinishArgs a;
    a.table = table; a.ns = ns; a.K = a.KB = KB; a.V_total = V;
    a.b = b; a.N = N; a.t = t; a.max_new = max_new; a.es = early_stopping; a.lp_pos = length_penalty > 0.f;
    a.dn = d_dn; a.n_eos = n_eos;
    for (int q = 0; q < n_eos; ++q) a.eos[q] = eos_ids[q];
    a.state = state; a.tokens = tokens; a.parents = parents; a.done_word = done_word;
    rc = launch_beam_finish(a, s);
  }
  hipStreamSynchronize(s);
  hipFree(mem);
  return rc;
}

extern "C" int omchat_op_beam_select_processed(const float* logits, int rows, int V, int b, int N, int t, int max_new, float length_penalty,
                                               int early_stopping, const int32_t* eos_ids, int n_eos, int32_t* state, int32_t* tokens,
                                               int32_t* parents, int32_t* done_word, const int32_t* hist_ids, const int32_t* hist_len,
                                               const int32_t* prompt_len, float rep_penalty, int no_repeat_ngram_size, int min_new_tokens,
                                               int min_length, const int32_t* suppress_ids, int n_suppress, const int32_t* begin_suppress_ids,
                                               int n_begin_suppress, const int32_t* bad_word_ids, const int32_t* bad_word_offsets,
                                               int n_bad_words, void* stream) {
  OM_CHECK(logits && state && tokens && parents && b >= 1 && N >= 2 && N <= BEAM_NMAX, "bad argument");
  OM_CHECK(n_eos >= 0 && n_eos <= BEAM_EOS_MAX && (n_eos == 0 || eos_ids), "at most 8 eos ids");
  const int KB = std::max(2, 1 + n_eos) * N;
  OM_CHECK(KB <= BEAM_KMAX && V >= KB, "max(2, 1 + n_eos) * N must not exceed 32 (nor V)");
  OM_CHECK(t >= 0 && t < max_new && rows == (t == 0 ? b : b * N), "rows = b at t = 0, b * N afterwards");
  OM_CHECK(early_stopping >= 0 && early_stopping <= 2, "early_stopping 0, 1 or 2");
  OM_CHECK(hist_ids && hist_len && prompt_len, "the rows' histories, their lengths and the prompts' lengths");
  OM_CHECK(isfinite(rep_penalty) && rep_penalty > 0.f, "repetition_penalty must be a finite float > 0");
  OM_CHECK(no_repeat_ngram_size >= 0 && no_repeat_ngram_size <= CON_NGRAM_MAX && min_new_tokens >= 0 && min_length >= 0, "constraint parameters out of range");
  ConstrainArgs ca;
  std::vector<int32_t> lists(CON_LIST_WORDS);
  if (int rc = constrain_pack_lists(eos_ids, n_eos, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_word_ids, bad_word_offsets,
                                    n_bad_words, lists.data(), ca)) return rc;
  ca.ngram = no_repeat_ngram_size; ca.min_new = n_eos ? min_new_tokens : 0; ca.min_len = n_eos ? min_length : 0;
  if (rep_penalty == 1.f && !ca.ngram && !ca.min_new && !ca.min_len && !ca.n_sup && !ca.n_bsup && !ca.n_bw)      // the plain search
    return omchat_op_beam_select(logits, rows, V, b, N, t, max_new, length_penalty, early_stopping, eos_ids, n_eos, state, tokens, parents,
                                 done_word, stream);
  int maxL = 0; int64_t can_ban = (int64_t)ca.n_sup + ca.n_bsup + ca.n_bw + ca.n_eos;
  for (int i = 0; i < rows; ++i) {
    OM_CHECK(hist_len[i] >= 0 && prompt_len[i] >= 0, "history lengths out of range");
    maxL = std::max(maxL, hist_len[i]);
  }
  OM_CHECK(V - (can_ban + maxL) >= KB, "the bans could leave a row fewer finite scores than the candidates kept per step");
  const int ns = beam_slices(V, 1);
  OM_CHECK(ns >= 1, "vocabulary cannot be sliced");
  const size_t TS = (size_t)ns * (4 + 2 * KB);
  std::vector<float> dn(max_new + 1, 1.f);
  for (int g = 1; g <= max_new; ++g) dn[g] = (float)pow((double)g, (double)length_penalty);
  const int ld = (maxL + 4) / 4 * 4, bmw = (V + 31) / 32;
  std::vector<int32_t> h((size_t)rows * ld, 0);
  size_t off = 0;
  for (int i = 0; i < rows; ++i) {
    std::copy(hist_ids + off, hist_ids + off + hist_len[i], h.begin() + (size_t)i * ld);
    off += (size_t)hist_len[i];
  }
  const size_t tb = (rows * TS * 4 + 15) / 16 * 16, db = (dn.size() * 4 + 15) / 16 * 16, hb = h.size() * 4, lb = lists.size() * 4;
  const size_t rb = ((size_t)rows * 4 + 15) / 16 * 16, bb = (size_t)2 * rows * bmw * 4;
  char* mem = nullptr;
  OM_HIP(hipMalloc(&mem, tb + db + hb + lb + 2 * rb + bb));
  float* table = (float*)mem;
  float* d_dn = (float*)(mem + tb);
  int32_t* d_h = (int32_t*)(mem + tb + db);
  int32_t* d_lists = (int32_t*)(mem + tb + db + hb);
  int* d_len = (int*)(mem + tb + db + hb + lb);
  int* d_plen = (int*)(mem + tb + db + hb + lb + rb);
  uint32_t* d_bm = (uint32_t*)(mem + tb + db + hb + lb + 2 * rb);
  hipStream_t s = S(stream);
  hipMemcpyAsync(d_dn, dn.data(), dn.size() * 4, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_h, h.data(), hb, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_lists, lists.data(), lb, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_len, hist_len, (size_t)rows * 4, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_plen, prompt_len, (size_t)rows * 4, hipMemcpyHostToDevice, s);
  hipMemsetAsync(d_bm, 0, bb, s);
  ca.hist = d_h; ca.hist_ld = ld; ca.len = d_len; ca.plen = d_plen; ca.tok = nullptr;
  ca.b = rows; ca.V = ca.V_total = V; ca.gbase = 0;
  constrain_bind_lists(d_lists, ca);
  ca.ban = d_bm; ca.bmw = bmw; ca.seen = rep_penalty != 1.f ? d_bm + (size_t)rows * bmw : nullptr;
  int rc = launch_constrain_ban(ca, s);
  if (!rc) rc = launch_beam_stats(logits, V, rows, V, ns, KB, table, s);
  if (!rc) rc = launch_beam_select_processed(logits, V, rows, V, ns, KB, table, ca.ban, ca.seen, bmw, rep_penalty, s);
  if (!rc) {
    BeamFinishArgs a;
    a.table = table; a.ns = ns; a.K = a.KB = KB; a.V_total = V; a.proc = true;
    a.b = b; a.N = N; a.t = t; a.max_new = max_new; a.es = early_stopping; a.lp_pos = length_penalty > 0.f;
    a.dn = d_dn; a.n_eos = n_eos;
    for (int q = 0; q < n_eos; ++q) a.eos[q] = eos_ids[q];
    a.state = state; a.tokens = tokens; a.parents = parents; a.done_word = done_word;
    rc = launch_beam_finish(a, s);
  }
  hipStreamSynchronize(s);
  hipFree(mem);
  return rc;
}

extern "C" int omchat_op_beam_hist_move(const int32_t* src, int32_t* dst, int rows, int N, int ld, int P, int g, const int32_t* parents,
                                        const int32_t* tokens, int32_t* len, uint32_t* bitmaps, size_t bitmap_words, void* stream) {
  return launch_beam_hist_move(src, dst, rows, N, ld, P, g, parents, tokens, len, bitmaps, bitmap_words, S(stream));
}

extern "C" int omchat_op_kv_gather(int dtype, void* k, void* v, void* k8, void* v8, float* ks, float* vs, int layers, int rows_cap, int kvh,
                                   int max_seq, const int32_t* parents, int row0, int nrows, int fork_src, int lo, int hi, void* stream) {
  OM_CHECK(k && v && (dtype == OMCHAT_F16 || dtype == OMCHAT_BF16) && layers >= 1 && kvh >= 1 && max_seq >= 1, "bad argument");
  OM_CHECK(row0 >= 0 && nrows >= 1 && row0 + nrows <= rows_cap && lo >= 0 && hi <= max_seq, "rows / slots out of range");
  const bool f8 = k8 || v8 || ks || vs;
  OM_CHECK(!f8 || (k8 && v8 && ks && vs), "e4m3 cache: k8, v8, ks and vs together");
  hipStream_t s = S(stream);
  KvGatherArgs g;
  g.k = (char*)k; g.v = (char*)v; g.layers = layers; g.kvh = kvh; g.max_seq = max_seq; g.rows_cap = rows_cap;
  if (f8) { g.k8 = (char*)k8; g.v8 = (char*)v8; g.ks = ks; g.vs = vs; }
  char* mem = nullptr;
  if (parents) {
    std::vector<int32_t> hp(rows_cap);
    OM_HIP(hipMemcpy(hp.data() + row0, parents + row0, (size_t)nrows * 4, hipMemcpyDeviceToHost));
    for (int r = row0; r < row0 + nrows; ++r) OM_CHECK(hp[r] >= row0 && hp[r] < row0 + nrows, "parents out of [row0, row0 + nrows)");
    const int n = std::max(hi - lo, 1);
    const size_t slots = (size_t)layers * (row0 + nrows) * kvh * n;
    OM_HIP(hipMalloc(&mem, slots * (f8 ? 776 : 512)));
    g.sk = mem; g.sv = mem + slots * 256;
    if (f8) { g.sk8 = mem + slots * 512; g.sv8 = mem + slots * 640; g.sks = (float*)(mem + slots * 768); g.svs = (float*)(mem + slots * 772); }
    g.st_rows = row0 + nrows; g.st_slots = n;
  }
  int rc = launch_kv_gather(g, parents, row0, nrows, fork_src, lo, hi, s);
  hipStreamSynchronize(s);
  if (mem) hipFree(mem);
  return rc;
}

extern "C" int omchat_op_fill_uniform(int dtype, void* dst, int64_t n, uint64_t key, float scale, float offset, void* stream) {
  return launch_fill_uniform(dtype, dst, n, key, scale, offset, S(stream));
}

// FlashAttention.forward(qkv[B,S,3,H,D]) -> out[B,S,H,D]  (intern_vit_6b/flash_attention.py:30-75); D = 128 only.
extern "C" int omchat_mha_fwd(const void* qkv, int B, int Sq, int H, float softmax_scale, int causal, void* out, int dtype, void* stream) {
  OM_CHECK(qkv && out, "null argument");
  AttnArgs a{};
  const int64_t row = (int64_t)3 * H * 128;
  a.Q = qkv; a.q_sb = Sq * row; a.q_sh = 128; a.q_sr = row;
  a.K = (const char*)qkv + (size_t)H * 128 * 2; a.k_sb = a.q_sb; a.k_sh = 128; a.k_sr = row;
  a.V = (const char*)qkv + (size_t)2 * H * 128 * 2; a.v_sb = a.q_sb; a.v_sh = 128; a.v_sr = row;
  a.O = out; a.o_sb = (int64_t)Sq * H * 128; a.o_sh = 128; a.o_sr = (int64_t)H * 128;
  a.batch = B; a.q_heads = H; a.kv_heads = H; a.Sq = Sq; a.Skv = Sq; a.kv_len = nullptr; a.causal = causal; a.q_pos0 = 0;
  a.scale = softmax_scale > 0.f ? softmax_scale : 0.08838834764831845f;
  return launch_attn_prefill(dtype, a, S(stream));
}

// packed qkv [B, S, 3, H, D] (D = 128 or 64) with optional per-sequence valid lengths (keys >= seqlens[b] masked; the caller zeroes
// the rows of padded queries, as flash-attn's pad_input does)
extern "C" int omchat_mha_fwd_varlen(const void* qkv, int B, int Sq, int H, int D, const int32_t* seqlens, float softmax_scale, int causal,
                                     void* out, int dtype, void* stream) {
  OM_CHECK(qkv && out, "null argument");
  OM_CHECK(D == 128 || D == 64, "head_dim must be 128 or 64");
  AttnArgs a{};
  const int64_t row = (int64_t)3 * H * D;
  a.Q = qkv; a.q_sb = Sq * row; a.q_sh = D; a.q_sr = row;
  a.K = (const char*)qkv + (size_t)H * D * 2; a.k_sb = a.q_sb; a.k_sh = D; a.k_sr = row;
  a.V = (const char*)qkv + (size_t)2 * H * D * 2; a.v_sb = a.q_sb; a.v_sh = D; a.v_sr = row;
  a.O = out; a.o_sb = (int64_t)Sq * H * D; a.o_sh = D; a.o_sr = (int64_t)H * D;
  a.batch = B; a.q_heads = H; a.kv_heads = H; a.Sq = Sq; a.Skv = Sq; a.kv_len = seqlens; a.causal = causal; a.q_pos0 = 0;
  a.scale = softmax_scale > 0.f ? softmax_scale : (D == 128 ? 0.08838834764831845f : 0.125f);
  a.head_dim = D;
  return launch_attn_prefill(dtype, a, S(stream));
}

extern "C" int omchat_op_quant_fp8(int dtype, const void* W, int N, int K, void* W8, float* scale, void* stream) {
  return launch_quant_fp8_rows(dtype, W, K, N, K, W8, K, scale, S(stream));
}

extern "C" int omchat_op_gemv_fp8(int dtype, const void* X, const void* W8, const float* scale, void* Y, int N, int K, const void* bias,
                                  const void* resid, int epi, int out_f32, int ksplit, void* stream) {
  OM_CHECK(scale, "scale missing");
  GemvArgs g{X, K, W8, K, Y, N, 1, N, K, bias, resid, N, epi, out_f32, ksplit, 0, scale};
  return launch_gemv(dtype, g, S(stream));
}

// MXFP4 pieces (include/omchat_hip.h): W4 [N][K / 2] bytes, S [N][K / 32] e8m0 bytes
extern "C" int omchat_op_quant_mxfp4(int dtype, const void* W, int N, int K, void* W4, void* S_, void* stream) {
  OM_CHECK(K % 32 == 0, "MXFP4: K must be a multiple of 32 (one e8m0 scale per 32 consecutive k)");
  return launch_quant_mxfp4_rows(dtype, W, K, N, K, W4, K / 2, (unsigned char*)S_, S(stream));
}

extern "C" int omchat_op_gemv_mxfp4(int dtype, const void* X, const void* W4, const void* S_, void* Y, int N, int K, const void* bias,
                                    const void* resid, int epi, int out_f32, int ksplit, void* stream) {
  OM_CHECK(X && W4 && S_ && Y, "null argument");
  OM_CHECK(K % 32 == 0, "MXFP4: K must be a multiple of 32 (one e8m0 scale per 32 consecutive k)");
  GemvArgs g{X, K, W4, K / 2, Y, N, 1, N, K, bias, resid, N, epi, out_f32, ksplit};
  g.mx_scale = (const unsigned char*)S_;
  return launch_gemv(dtype, g, S(stream));
}

// the same weights under b rows of row-major x (no packed operands): b == 1 runs as omchat_op_gemv_mxfp4 does, b > 1 is refused by launch_gemv --
// MXFP4 at b > 1 exists on the packed operands only (omchat_op_gemv_mxfp4_packed)
extern "C" int omchat_op_gemv_mxfp4_rows(int dtype, const void* X, int ldx, const void* W4, const void* S_, void* Y, int ldy, int b, int N, int K,
                                         const void* bias, int epi, int out_f32, int ksplit, void* stream) {
  OM_CHECK(X && W4 && S_ && Y, "null argument");
  OM_CHECK(K % 32 == 0, "MXFP4: K must be a multiple of 32 (one e8m0 scale per 32 consecutive k)");
  GemvArgs g{X, ldx, W4, K / 2, Y, ldy, b, N, K, bias, nullptr, 0, epi, out_f32, ksplit};
  g.mx_scale = (const unsigned char*)S_;
  return launch_gemv(dtype, g, S(stream));
}

// packed-operand batched GEMV on MXFP4 weights (gemv.hip: gemv_pk_mx4_kernel / gemv_xs_mx4_kernel / gemv_xs_split_mx4_kernel): X row-major [b, K]
// and the row-major replica W4 [N][K / 2], S [N][K / 32] are packed into scratch here (launch_pack_x / launch_pack_w4), then Y = epi(X dequant(W)^T)
// as omchat_op_gemv_packed computes it on 16-bit weights.  Every refusal comes before anything is enqueued.
extern "C" int omchat_op_gemv_mxfp4_packed(int dtype, const void* X, int ldx, const void* W4, const void* S_, void* Y, int ldy, int b, int N, int K,
                                           const void* bias, int epi, int out_f32, int ksplit, int y_packed, void* stream) {
  OM_CHECK(X && W4 && S_ && Y, "null argument");
  OM_CHECK(b >= 1 && b <= 32, "packed MXFP4 GEMV: 1 <= b <= 32 rows per call");
  OM_CHECK(K >= 64 && K % 64 == 0, "packed MXFP4 GEMV: K % 64 == 0 (64-wide K chunks of the packed layout)");
  OM_CHECK(N >= 16 && N % 16 == 0, "packed MXFP4 GEMV: N % 16 == 0 (16-row weight tiles of the packed layout)");
  OM_CHECK(epi == EPI_NONE || epi == EPI_SWIGLU || epi == EPI_PARTIAL, "packed MXFP4 GEMV: epilogue NONE / SWIGLU / PARTIAL");
  OM_CHECK(dtype == OMCHAT_F16 || dtype == OMCHAT_BF16, "bad dtype");
  const int NB = b > 16 ? 2 : 1;
  void *xp = nullptr, *wp = nullptr, *sp = nullptr;
  auto drop = [&]() { if (xp) hipFree(xp); if (wp) hipFree(wp); if (sp) hipFree(sp); };
  if (hipMalloc(&xp, (size_t)NB * 16 * K * 2) != hipSuccess || hipMalloc(&wp, (size_t)N * (K / 2)) != hipSuccess ||
      hipMalloc(&sp, (size_t)N * (K / 32)) != hipSuccess) {
    (void)hipGetLastError(); drop(); omchat_set_error("hipMalloc failed"); return 2;
  }
  int rc = launch_pack_x(dtype, X, ldx, b, K, xp, S(stream));
  if (rc == 0) rc = launch_pack_w4(W4, (const unsigned char*)S_, N, K, wp, (unsigned char*)sp, S(stream));
  if (rc == 0) {
    GemvArgs g{xp, K, wp, K / 2, Y, ldy, b, N, K, bias, nullptr, 0, epi, out_f32, ksplit, 0, nullptr, 1, 1, y_packed};
    g.mx_scale = (const unsigned char*)sp;
    rc = launch_gemv(dtype, g, S(stream));
  }
  hipStreamSynchronize(S(stream));
  drop();
  return rc;
}

// The pieces of the two packed entries for callers that pack once and launch many times (tools/bench_mxfp4.py times the launch alone): the packers,
// and the launch on PRE-PACKED operands -- XP from omchat_op_pack_x; WP from omchat_op_pack_w with SP = NULL (16-bit weights), or WP / SP from
// omchat_op_pack_w4 (MXFP4).  Nothing is allocated or synchronised here.
extern "C" int omchat_op_pack_w(int dtype, const void* W, int ldw, int N, int K, void* out, void* stream) { return launch_pack_w(dtype, W, ldw, N, K, out, S(stream)); }
extern "C" int omchat_op_pack_w4(const void* W4, const void* S_, int N, int K, void* W4P, void* SP, void* stream) {
  return launch_pack_w4(W4, (const unsigned char*)S_, N, K, W4P, (unsigned char*)SP, S(stream));
}
extern "C" int omchat_op_gemv_prepacked(int dtype, const void* XP, const void* WP, const void* SP, void* Y, int ldy, int b, int N, int K, const void* bias,
                                        int epi, int out_f32, int ksplit, int y_packed, void* stream) {
  OM_CHECK(XP && WP && Y, "null argument");
  OM_CHECK(b >= 1 && b <= 32 && K >= 64 && K % 64 == 0 && N >= 16 && N % 16 == 0, "pre-packed GEMV: 1 <= b <= 32, K % 64 == 0, N % 16 == 0");
  GemvArgs g{XP, K, WP, SP ? K / 2 : K, Y, ldy, b, N, K, bias, nullptr, 0, epi, out_f32, ksplit, 0, nullptr, 1, 1, y_packed};
  g.mx_scale = (const unsigned char*)SP;
  return launch_gemv(dtype, g, S(stream));
}

// ... with the preceding RMSNorm in registers (omchat_op_gemv_norm on MXFP4 weights; K <= 4096, epilogue NONE / SWIGLU)
extern "C" int omchat_op_gemv_mxfp4_norm(int dtype, const void* X, const void* W4, const void* S_, void* Y, int N, int K, const void* norm_w,
                                         float eps, const void* bias, int epi, int out_f32, void* stream) {
  OM_CHECK(X && W4 && S_ && Y && norm_w, "null argument");
  OM_CHECK(K % 32 == 0, "MXFP4: K must be a multiple of 32 (one e8m0 scale per 32 consecutive k)");
  GemvArgs g{X, K, W4, K / 2, Y, N, 1, N, K, bias, nullptr, 0, epi, out_f32};
  g.norm_w = norm_w; g.norm_eps = eps;
  g.mx_scale = (const unsigned char*)S_;
  return launch_gemv(dtype, g, S(stream));
}

// ... and the same on e4m3 rows with one fp32 scale per row (omchat_op_gemv_fp8 with the RMSNorm in registers)
extern "C" int omchat_op_gemv_fp8_norm(int dtype, const void* X, const void* W8, const float* scale, void* Y, int N, int K, const void* norm_w,
                                       float eps, const void* bias, int epi, int out_f32, void* stream) {
  OM_CHECK(X && W8 && scale && Y && norm_w, "null argument");
  GemvArgs g{X, K, W8, K, Y, N, 1, N, K, bias, nullptr, 0, epi, out_f32, 0, 0, scale};
  g.norm_w = norm_w; g.norm_eps = eps;
  return launch_gemv(dtype, g, S(stream));
}

// bf16x12 pieces (include/omchat_hip.h): the encoder into caller-provided buffers, and the three batch-1 roles on coded operands --
// norm_w with EPI_SWIGLU (gate|up) or EPI_NONE (lm_head form), or EPI_RESID with resid (down_proj, long K)
extern "C" int omchat_op_encode_bf16x12(const void* W, int N, int K, void* coded, void* top, void* cnt, void* patch, void* over, void* stream) {
  return launch_encode_bf16x12(W, K, N, K, coded, (unsigned char*)top, (unsigned char*)cnt, (unsigned*)patch, (int*)over, S(stream));
}
extern "C" int omchat_op_gemv_bf16x12(const void* X, const void* coded, const void* top, const void* cnt, const void* patch, void* Y, int N, int K,
                                      const void* norm_w, float eps, const void* resid, int epi, int out_f32, void* stream) {
  OM_CHECK(X && coded && top && cnt && patch && Y, "null argument");
  GemvArgs g{X, K, coded, K / 2 * 3, Y, N, 1, N, K, nullptr, resid, N, epi, out_f32};
  g.norm_w = norm_w; g.norm_eps = eps;
  g.x12_top = (const unsigned char*)top; g.x12_cnt = (const unsigned char*)cnt; g.x12_patch = (const unsigned*)patch;
  return launch_gemv(OMCHAT_BF16, g, S(stream));
}

extern "C" int omchat_op_attn_prefill_d(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv, int Hq,
                                        int Hkv, int D, const int32_t* kv_len, int causal, int q_pos0, float scale, void* stream) {
  AttnArgs a{};
  a.Q = q; a.q_sb = (int64_t)Sq * Hq * D; a.q_sh = D; a.q_sr = (int64_t)Hq * D;
  a.K = k; a.k_sb = (int64_t)Hkv * Skv * D; a.k_sh = (int64_t)Skv * D; a.k_sr = D;
  a.V = v; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = D;
  a.O = out; a.o_sb = a.q_sb; a.o_sh = D; a.o_sr = a.q_sr;
  a.batch = b; a.q_heads = Hq; a.kv_heads = Hkv; a.Sq = Sq; a.Skv = Skv; a.kv_len = kv_len; a.causal = causal; a.q_pos0 = q_pos0; a.scale = scale;
  a.head_dim = D;
  return launch_attn_prefill(dtype, a, S(stream));
}

extern "C" int omchat_op_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, int rows, int H, float eps, void* stream) {
  return launch_layernorm(dtype, x, H, w, b, y, H, rows, H, eps, S(stream));
}

// ---------------------------------------------------------------------------------------------------------
// Test hooks of the row / glue kernels (tests/test_gpu_glue_ops.py): thin wrappers over the launchers the model loops call, with the arguments
// the product entry points above do not expose (kv_start, per-row RoPE positions and cache slots, row strides, the argmax's position words).
// ---------------------------------------------------------------------------------------------------------
extern "C" int omchat_op_attn_prefill_left(int dtype, const void* q, const void* k, const void* v, void* out, int b, int Sq, int Skv, int Hq,
                                           int Hkv, const int32_t* kv_len, const int32_t* kv_start, int causal, int q_pos0, float scale,
                                           int fill_uniform, void* stream) {
  OM_CHECK(q && k && v && out && kv_start, "null argument");
  AttnArgs a{};
  a.Q = q; a.q_sb = (int64_t)Sq * Hq * 128; a.q_sh = 128; a.q_sr = (int64_t)Hq * 128;
  a.K = k; a.k_sb = (int64_t)Hkv * Skv * 128; a.k_sh = (int64_t)Skv * 128; a.k_sr = 128;
  a.V = v; a.v_sb = a.k_sb; a.v_sh = a.k_sh; a.v_sr = 128;
  a.O = out; a.o_sb = a.q_sb; a.o_sh = 128; a.o_sr = a.q_sr;
  a.batch = b; a.q_heads = Hq; a.kv_heads = Hkv; a.Sq = Sq; a.Skv = Skv; a.kv_len = kv_len; a.kv_start = kv_start; a.causal = causal;
  a.q_pos0 = q_pos0; a.scale = scale;
  int rc = launch_attn_prefill(dtype, a, S(stream));
  if (!rc && fill_uniform) rc = launch_attn_uniform_rows(dtype, a, S(stream));      // the order of the decoder layer (model.hip)
  return rc;
}

// RoPE + KV append with the per-row position array and / or a cache slot that differs from the position (RopeArgs.pos / slot0): pos device int32
// [b * S] or NULL (-> pos0 + s), slot0 = -1: the slot is the position.  The table holds max_pos positions.  Every position must be < max_pos and
// every slot < cap: checked on the host (pos is copied back) before anything is launched.  Synchronises.
extern "C" int omchat_op_rope_kv_pos(int dtype, void* qkv, int b, int Sq, int Hq, int Hkv, const int32_t* pos, int pos0, int slot0, int max_pos,
                                     float theta, void* kcache, void* vcache, int cap, void* stream) {
  OM_CHECK(qkv && kcache && vcache && b >= 1 && Sq >= 1 && Hq >= 1 && Hkv >= 1 && max_pos >= 1 && cap >= 1 && slot0 >= -1, "bad argument");
  if (pos) {
    std::vector<int32_t> hp((size_t)b * Sq);
    OM_HIP(hipStreamSynchronize(S(stream)));
    OM_HIP(hipMemcpy(hp.data(), pos, hp.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t p : hp) {
      OM_CHECK(p >= 0 && p < max_pos, "position outside the RoPE table");
      OM_CHECK(slot0 >= 0 || p < cap, "cache slot exceeds the capacity");
    }
  } else {
    OM_CHECK(pos0 >= 0 && pos0 + Sq <= max_pos, "position outside the RoPE table");
    OM_CHECK(slot0 >= 0 || pos0 + Sq <= cap, "cache slot exceeds the capacity");
  }
  OM_CHECK(slot0 < 0 || slot0 + Sq <= cap, "cache slot exceeds the capacity");
  float* d = rope_table_device(max_pos, theta);
  OM_CHECK(d, "rope table allocation failed");
  RopeArgs r{qkv, (Hq + 2 * Hkv) * 128, b * Sq, Sq, Hq, Hkv, pos, pos0, d, max_pos, kcache, vcache, (int64_t)Hkv * cap * 128, (int64_t)cap * 128};
  r.slot0 = slot0;
  int rc = launch_rope_kv(dtype, r, S(stream));
  hipStreamSynchronize(S(stream));
  hipFree(d);
  return rc;
}

// argmax over rows of stride ld >= V, with the optional position words of the decode step (adv_pos / adv_len device int32 [b] or NULL).  Synchronises.
extern "C" int omchat_op_argmax_ld(const float* logits, int ld, int b, int V, int32_t* out, int32_t* adv_pos, int32_t* adv_len, void* stream) {
  OM_CHECK(logits && out && b >= 1 && V >= 1 && ld >= V, "bad argument");
  void* scratch = nullptr;
  OM_HIP(hipMalloc(&scratch, argmax_scratch_bytes(b)));
  int rc = launch_argmax(logits, ld, b, V, out, scratch, S(stream), adv_pos, adv_len);
  hipStreamSynchronize(S(stream));
  hipFree(scratch);
  return rc;
}

extern "C" int omchat_op_im2col(int dtype, const void* pixels, void* cols, int B, int HW, int patch, int Kpad, void* stream) {
  OM_CHECK(pixels && cols && B >= 0 && HW >= 1 && patch >= 1, "bad argument");
  return launch_im2col(dtype, pixels, cols, B, HW, patch, Kpad, S(stream));
}
extern "C" int omchat_op_vit_assemble(int dtype, const void* pe, const void* cls, const void* pos, void* x, int B, int np, int C, void* stream) {
  OM_CHECK(pe && cls && pos && x && B >= 0 && np >= 0, "bad argument");
  return launch_vit_assemble(dtype, pe, cls, pos, x, B, np, C, S(stream));
}
extern "C" int omchat_op_gather_rows(int dtype, const int32_t* idx, const void* table, const void* feats, void* out, int rows, int H, void* stream) {
  OM_CHECK(idx && out && rows >= 0, "bad argument");
  return launch_gather_rows(dtype, idx, table, feats, out, rows, H, S(stream));
}
extern "C" int omchat_op_copy_rows(int dtype, const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int rows, int H, int group, int skip,
                                   void* stream) {
  OM_CHECK(src && dst && rows >= 0 && skip >= 0 && src_ld >= H && dst_ld >= H, "bad argument");
  return launch_copy_rows(dtype, src, src_ld, dst, dst_ld, rows, H, group, skip, S(stream));
}
extern "C" int omchat_op_tp_finish(int dtype, const float* sum, const void* bias, const void* ls, const void* resid, void* out, int M, int N, int epi,
                                   void* stream) {
  return launch_tp_finish(dtype, sum, bias, ls, resid, out, M, N, epi, S(stream));
}
extern "C" int omchat_op_resid16_norm(int dtype, void* x, int ldx, const void* y, int ldy, const void* w, const void* b, void* xn, int ldn, int rows,
                                      int H, float eps, void* stream) {
  OM_CHECK(rows <= 0 || (x && y), "null argument");
  return launch_resid16_norm(dtype, x, ldx, y, ldy, w, b, xn, ldn, rows, H, eps, S(stream));
}
extern "C" int omchat_op_cast_f32(int dtype, const void* src, float* dst, int64_t n, void* stream) {
  OM_CHECK(n == 0 || (src && dst && n > 0), "bad argument");
  return launch_cast_f32(dtype, src, dst, n, S(stream));
}
extern "C" int omchat_op_rmsnorm_ld(int dtype, const void* x, int ldx, const void* w, void* y, int ldy, int rows, int H, float eps, int pack_nb,
                                    void* stream) {
  OM_CHECK(x && w && y && rows >= 0 && ldx >= H && (pack_nb != 0 || ldy >= H), "bad argument");
  return launch_rmsnorm(dtype, x, ldx, w, y, ldy, rows, H, eps, S(stream), pack_nb);
}
extern "C" int omchat_op_layernorm_ld(int dtype, const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int rows, int H, float eps,
                                      void* stream) {
  OM_CHECK(x && y && rows >= 0 && ldx >= H && ldy >= H, "bad argument");
  return launch_layernorm(dtype, x, ldx, w, b, y, ldy, rows, H, eps, S(stream));
}
