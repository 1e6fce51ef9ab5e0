// Internal launcher interface (C++) shared by the op-level C ABI (capi.cpp) and the model loops (model.cpp).
// Every launcher enqueues on `stream` and returns 0 / sets omchat_last_error().  dtype: OMCHAT_F16 | OMCHAT_BF16.
#pragma once
// Round-4 one-launch forms of the batch-1 decode layer (decode_layer.hip, fused_decode.hip) and the work-stealing gate|up GEMV: measured
// SLOWER than the launches they replace and kept for the record only.  They are compiled in with
// -DOMCHAT_EXPERIMENTS=1 (`python -m omchat_amd.build --twin ab_lib/experiments -DOMCHAT_EXPERIMENTS=1`); the product library has stubs
// that refuse, tuning keys 22 / 23 / 24 then do nothing, and omchat_has_experiments() reports which build is loaded.
#ifndef OMCHAT_EXPERIMENTS
#define OMCHAT_EXPERIMENTS 0
#endif
#include "common.h"
#if OMCHAT_EXPERIMENTS
// TIMING PROBE ONLY (tuning key 41, experiments build): every kernel launch of the library goes out with hipExtAnyOrderLaunch.  On this GPU the flag does not
// let a kernel overtake its predecessor (tools/experiments/tune_anyorder.hip: it still starts after the predecessor's last wave) but the boundary shrinks from 2.5 to
// 0.3 us -- the release / acquire cache maintenance between the two is what goes.  Without it a consumer on another XCD may read stale lines, so results
// under this key are NOT valid; it prices what boundaries without cache maintenance would return.
#include <hip/hip_ext.h>
extern int g_launch_any_order;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)                                                      \
  do {                                                                                                                                         \
    if (g_launch_any_order)                                                                                                                    \
      hipExtLaunchKernelGGL((kernelName), dim3(numBlocks), dim3(numThreads), (memPerBlock), (streamId), nullptr, nullptr, hipExtAnyOrderLaunch, \
                            __VA_ARGS__);                                                                                                      \
    else                                                                                                                                       \
      hipLaunchKernelGGLInternal((kernelName), numBlocks, numThreads, memPerBlock, streamId, __VA_ARGS__);                                     \
  } while (0)
#endif

// ------------------------------------------------------------------------------------------------ GEMM
// C[M,N] = epilogue(A[M,K] @ W[N,K]^T), fp32 accumulate on MFMA.  K % 64 == 0, lda/ldw % 8 == 0.
enum {
  EPI_NONE = 0,      // C = T(acc + bias?)
  EPI_GELU = 1,      // C = T(gelu_erf(T(acc + bias?)))                       (InternMLP fc1, projector linear_1)
  EPI_LS_RESID = 2,  // C = T(resid + T(T(acc + bias?) * ls))                 (ViT: x + branch * ls)
  EPI_RESID = 3,     // C = T(resid + T(acc + bias?))                         (decoder o_proj / down_proj)
  EPI_SWIGLU = 4,    // W rows interleaved [16 gate | 16 up]: C[M,N/2] = T(T(silu(T(g))) * T(u))
  EPI_PARTIAL = 5,   // skinny GEMM only: raw fp32 K-slice sums Y[ksplit][b][ldy] (split-K across workgroups)
  EPI_F32OUT = 6,    // MFMA GEMM only: C is float [M, ldc]: the raw fp32 accumulators (tensor parallelism: row-parallel partial sums that are
                     // all-reduced in fp32 and finished by launch_tp_finish; ldc % 4 == 0, C 16-byte aligned)
  // round 6 (the ViT's norms folded into its GEMMs): the same epilogues that ALSO leave, per row and per wave-column block ("slot"), the sum of
  // squares of the 16-bit values they store -- GemmArgs.stats, SLOT-MAJOR fp32 [slots][stats_ld >= M], slot = first column of the wave tile / its width.  The
  // consumer (the next GEMM's row scale, the ViT q / k norm) sums a row's slots in slot order: a fixed order, so the statistics are deterministic
  EPI_LS_RESID_STATS = 7,
  EPI_NONE_STATS = 8,
  // teacher-forced scoring: NOTHING is stored to C.  Every wave tile reduces each of its rows over its valid columns to an
  // online pair (m = max, s = sum exp(x - m)) of the raw fp32 accumulators and leaves it in GemmArgs.stats, slot-major as the statistics above with
  // two planes per slot: stats[(2 * slot) * stats_ld + row] = m, stats[(2 * slot + 1) * stats_ld + row] = s, slot = first column of the wave tile / 64
  // (cdiv(N, 64) slots: both kernels this mode runs on have 64-column wave tiles).  The one lane that owns column lse_labels[row] also writes that
  // accumulator to lse_tgt[row] (labels outside [0, N) write nothing).  Finished by launch_score_finish (score.hip)
  EPI_LSE = 9,
};
struct GemmArgs {
  const void* A; int lda;
  const void* W; int ldw;
  void* C; int ldc;
  int M, N, K;
  const void* bias;   // [N] or null
  const void* ls;     // [N] layer-scale (EPI_LS_RESID)
  const void* resid;  // [M, ldr] (EPI_LS_RESID / EPI_RESID); may alias C
  int ldr;
  int epi;
  int force_tile;     // 0 auto, 1 = 128x128, 2 = 256x256 (staggered 4-phase), 3 = 256x192, 4 = 224x256, 5 = 192x256, 6 = 256x256 (one barrier)
  void* sk_ws; size_t sk_ws_bytes;   // stream-K workspace (gemm_sk_ws_bytes()), null = data-parallel only
  int stream_k;       // 0 auto (when a workspace is given), -1 never, 1 required
  // fp8 x fp8 MFMA (BASELINE configs[4], "fp8 MFMA weights"): A [M, K] and W [N, K] are OCP e4m3 bytes (lda / ldw in bytes) with one fp32
  // scale per row each; C = epi(a_scale[m] * w_scale[n] * sum_k A8 W8) in the 16-bit type.  K % 128 == 0.  256x256 tile, 128-deep K
  // steps: the same LDS bytes per step as the 16-bit kernel feed twice the MFMAs.
  int f8;
  const float* a_scale; const float* w_scale;
  // round 6: C = epi(row_scale[m] * (A W^T) + bias ...): the RMSNorm in front of a ViT projection as a per-row factor on the fp32 accumulators
  // (x * rsqrt(mean x^2 + eps) commutes with the product; the norm WEIGHT is folded into W's columns at load time: model.hip fold_norm_weights)
  const float* row_scale = nullptr;
  // ... or finished inside the launch from the producing GEMM's statistics slots: row_scale[m] = rsqrt(sum_{s < rs_nslots} rs_stats[s * rs_ld + m] / rs_dim + rs_eps)
  // (once per tile, into LDS, after the K loop: no launch between the producer and this GEMM)
  const float* rs_stats = nullptr; int rs_ld = 0, rs_nslots = 0, rs_dim = 0; float rs_eps = 0.f;
  // EPI_*_STATS: per-row partial sums of squares of the stored outputs (slot-major); *stats_nslots receives the number of slots the launch(es) wrote
  float* stats = nullptr; int stats_ld = 0; int* stats_nslots = nullptr;
  // EPI_LSE: device int32 [M] labels and the fp32 [M] target logits
  const int* lse_labels = nullptr; float* lse_tgt = nullptr;
};
int launch_gemm(int dtype, const GemmArgs& a, hipStream_t stream);
// finishes the per-slot partials of an EPI_*_STATS GEMM (or of launch_row_sumsq); statistics are SLOT-MAJOR, stats[slot * ld + m], ld >= rows:
// for group g < ngroups, t_g = sum_{s < nslots} stats[(slot0 + g * nslots + s) * ld + m] in slot order;  dim > 0: out[m * ngroups + g] = rsqrt(t_g / dim + eps) (a GEMM row scale),
// dim == 0: out[m * ngroups + g] = t_g (the [rows, 2] sums launch_vit_qknorm and the attention's q norm take)
int launch_stats_finish(const float* stats, int ld, int slot0, int nslots, int ngroups, int rows, int dim, float eps, float* out, hipStream_t s);
// stats[m] = sum_c x[m][c]^2 (slot 0 of slot-major statistics): the statistics of a residual stream that no GEMM epilogue produced (the ViT's embeddings)
int launch_row_sumsq(int dtype, const void* x, int ldx, int rows, int H, float* stats, hipStream_t s);
size_t gemm_sk_ws_bytes();
void gemm_set_skew(int v);
void gemm_set_persist(int v);
void gemm_set_wide_store(int v);      // tuning key 37
void gemm_set_skip_dead(int v);       // tuning key 43

// ------------------------------------------------------------------------------------------------ skinny GEMM (decode)
// Y[b,N] = epilogue(X[b,K] @ W[N,K]^T) for b <= 16: weight-streaming, HBM-bound.  K % 64 == 0.
struct GemvArgs {
  const void* X; int ldx;
  const void* W; int ldw;
  void* Y; int ldy;         // T, or float when out_f32
  int b, N, K;
  const void* bias;
  const void* resid; int ldr;
  int epi;                  // EPI_NONE | EPI_RESID | EPI_SWIGLU | EPI_PARTIAL
  int out_f32;
  int ksplit;               // K slices across workgroups (EPI_PARTIAL), <= 1 = none
  int force_mfma;           // 1 = always the MFMA form (tests / A-B); default: b == 1 uses the whole-row streaming form
  const float* w_scale;     // non-null: W is OCP e4m3 bytes [N][ldw] with one fp32 scale per row (weight-only fp8, b == 1 only)
  // batched decode (b <= 32) with operands in MFMA fragment order (common.h: packed_x_index / packed_w_index): every wave load is 1 KiB
  // contiguous instead of 16 rows x 64 B (measured, tools/experiments/tune_gemv32.hip: gate|up at b = 32 84 -> 53 us, down 50 -> 28 us)
  int x_packed;             // X is packed with NB = b > 16 ? 2 : 1 (ldx ignored)
  int w_packed;             // W is the packed replica (ldw ignored); needs x_packed
  int y_packed;             // EPI_SWIGLU only: write Y in the packed x layout of the consumer (same NB; ldy ignored)
  // b == 1, ksplit <= 1, whole-row form: X is the RAW hidden row and y = epi(W RMSNorm(X; norm_w, norm_eps)) -- the norm runs in registers
  const void* norm_w; float norm_eps;
  // optional: 65 x 64 unsigned (65 lines of 256 bytes) of ZEROED device memory owned by the caller and used by no other launch at the same time (the kernel leaves them
  // zero): the loop form of a norm GEMV then takes its outputs from atomic work counters (gemv_rows_norm_dyn_kernel) instead of equal shares
  void* dyn_ctr = nullptr;
  // batched x-stationary form, EPI_RESID (round 5): the result rows are ALSO written in the packed x layout here (same NB), un-normalised --
  // the consuming gate|up GEMV normalises them in registers (norm_w with x_packed)
  void* y_pack = nullptr;
  // experiments build, measurement only: 8 x 64-bit clock stamps of this launch's layer (see model.hip dbg_stamps)
  unsigned long long* dbg = nullptr;
  // non-null: W is MXFP4 -- [N][ldw] bytes (ldw >= K / 2) of two OCP e2m1 codes each, the even k in the low nibble -- and mx_scale [N][K / 32]
  // holds one e8m0 byte per 32 consecutive k (weight-only, b == 1 only, K % 32 == 0); not together with w_scale.
  // With x_packed && w_packed (1 <= b <= 32, K % 64 == 0, N % 16 == 0): W / mx_scale are the PACKED MXFP4 replica that launch_pack_w4 writes
  // (common.h: packed_w4_index / packed_s4_index; ldw ignored) and the packed batched forms run on it; epilogues NONE / SWIGLU / PARTIAL
  const unsigned char* mx_scale = nullptr;
  // non-null: W is the bf16x12 coding of a bf16 [N][K] matrix (launch_encode_bf16x12: rows of ldw = K * 3 / 2 bytes) with x12_top [N],
  // x12_cnt [N] (every count <= 32) and x12_patch [N][32]; the launch gives the bits of the same launch on the 16-bit matrix.  bf16, b == 1,
  // K % 512 == 0, and one of the three long batch-1 forms: norm_w with EPI_SWIGLU / EPI_NONE (K <= 4096), or EPI_RESID without split-K
  // on 4096 < K <= 32768
  const unsigned char* x12_top = nullptr;
  const unsigned char* x12_cnt = nullptr;
  const unsigned* x12_patch = nullptr;
};
// bf16x12 (tests/bf16x12_ref.py is the definition): W bf16 [N][ldw] -> coded [N][K * 3 / 2] bytes, top [N], cnt [N] (min(misses, 33)),
// patch [N][32] (k << 16 | bits, sorted by k); *over (device, zeroed by the caller) is set to 1 when a row needs more than 32 patches.  K % 512 == 0
int launch_encode_bf16x12(const void* W, int ldw, int N, int K, void* coded, unsigned char* top, unsigned char* cnt, unsigned* patch, int* over,
                          hipStream_t stream);
// row-major [rows <= 32][K] -> packed x (tests, tools); row-major W [N][ldw] -> packed replica (N % 16 == 0)
int launch_pack_x(int dtype, const void* X, int ldx, int b, int K, void* out, hipStream_t s);
int launch_pack_w(int dtype, const void* W, int ldw, int N, int K, void* out, hipStream_t s);
// row-major MXFP4 (W4 [N][K / 2] bytes, S [N][K / 32] e8m0 bytes: what launch_quant_mxfp4_rows writes) -> packed replica W4P (N K / 2 bytes),
// SP (N K / 32 bytes); a byte shuffle.  N % 16 == 0, K % 64 == 0
int launch_pack_w4(const void* W4, const unsigned char* S, int N, int K, void* W4P, unsigned char* SP, hipStream_t s);
int launch_gemv(int dtype, const GemvArgs& a, hipStream_t stream);
// What the tuning keys set for the GEMVs (process-global: one instance in gemv.hip behind gemv_set_* / gemv_get_*; gemv.hip has each key's meaning)
struct GemvTuning {
  int force_mfma = 0, no_xs = 0, shard = 15, norm_loop = 0, gu_rr = 1, gu_rr8 = 1, dyn = 0, longk_direct = 0, rows_balance = 1;
  unsigned skew = 0;
};
const GemvTuning& gemv_tuning();
// kernel families of launch_gemv (omchat_op_gemv_plan reports them by these numbers); the last two exist in -DOMCHAT_EXPERIMENTS=1 builds only
enum GemvFamily { GF_MFMA = 0, GF_PK, GF_XS, GF_XS_SPLIT, GF_ROWS, GF_ROWS_NORM, GF_ROWS_NORM_LOOP, GF_ROWS_LONGK, GF_ROWS_NORM_DYN, GF_ROWS_LONGK_DIRECT };
constexpr int WF_16 = 0, WF_E4M3 = 1, WF_MX4 = 2, WF_X12 = 3;      // weight forms (gemv.hip)
// The whole launch decision of one launch_gemv call: either `refusal` (launch_gemv's error text) or the kernel -- family, weight form, epilogue
// and the integer template arguments that the family has (the others stay 0) -- with its grid, block, dynamic LDS and scalar arguments.
struct GemvPlan {
  const char* refusal;
  int family, wf, wpack, epi, ntile, waves, unroll, nb, rr, nch, norm;      // norm: gemv_xs_kernel's NORM (experiments build)
  int gx, gy, block, lds;
  int per_wg; unsigned skew;      // gemv_rows_norm_loop_kernel
  int rows_per_wg;                // gemv_rows_longk_kernel
  int n5;                         // gemv_xs_split_kernel
  int xskew;                      // GemvP::xskew of the non-loop gate|up form (experiments build, tuning key 28 < 256)
};
// pure: reads its arguments only (of a's pointers only whether they are null); n_cu = the device's compute units
GemvPlan gemv_plan(int dtype, const GemvArgs& a, const GemvTuning& t, int n_cu);
constexpr int DEC_KS_MAX = 8;
// K slices (ksplit of the EPI_PARTIAL launch) of a decode step's o_proj (down = false, K = q width) or down_proj (down = true, K = mlp width)
// at batch b and hidden size H; packed: the step streams a packed replica (16-bit or MXFP4)
int gemv_split_k(int b, int K, int H, bool packed, bool down, const GemvTuning& t);
// experiments build (tuning key 42): the batch-1 o_proj GEMV launched out of order behind the split-KV merge, waiting on its per-head completion flags
int launch_gemv_wait(int dtype, const GemvArgs& a, const unsigned* flags, unsigned epoch, int nflags, unsigned* err, int mode, hipStream_t s);
// per-row (output channel) symmetric quantisation of W [N][ldw] (T) to OCP e4m3: scale[n] = absmax_n / 448 (1 if the row is 0),
// W8[n][k] = e4m3_rne(W[n][k] / scale[n])
int launch_quant_fp8_rows(int dtype, const void* W, int ldw, int N, int K, void* W8, int ld8, float* scale, hipStream_t stream);
// MXFP4 (OCP Microscaling v1.0) of W [N][ldw] (T), K % 32 == 0: per row and block of 32 k, e = floor(log2(absmax)) - 2 clamped to [-127, 127],
// S[n][k / 32] = e + 127 (127 for a zero block), codes = e2m1 round-to-nearest (ties to the even code, saturating at 6) of w / 2^e, sign in
// bit 3 (never on a zero code); W4 [N][ld4] bytes, the even k in the low nibble
int launch_quant_mxfp4_rows(int dtype, const void* W, int ldw, int N, int K, void* W4, int ld4, unsigned char* S, hipStream_t stream);
void gemv_set_force_mfma(int v);
int gemv_get_force_mfma();
void gemm_set_autotune(int v);
int gemm_tune_load(const char* path);
int gemm_tune_dump(const char* path);
long gemm_tune_runs();
void model_set_ar_min_rows(int v);
void model_set_tp_f32(int v);
void model_set_pack_replica(int v);
void model_set_norm_in_gemv(int v);
void model_set_vit_fused(int v);        // tuning key 44
void model_set_tp_sp(int v);            // tuning key 45
// out[r][c] = T(W[r][c] * n[c]): a norm weight folded into the columns of the linear map that follows it (model.hip ensure_vit_folded)
int launch_fold_cols(int dtype, const void* W, const void* n, void* out, int rows, int cols, hipStream_t s);

// ------------------------------------------------------------------------------------------------ norms
// y = T(w * T(x * rsqrt(mean(x^2) + eps)))  (InternRMSNorm / Qwen2RMSNorm), rows of width H (H % 8 == 0, H <= 16384)
int launch_layernorm(int dtype, const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int rows, int H, float eps, hipStream_t stream);
// pack_nb != 0: y is written in the packed x layout (common.h) with NB = pack_nb instead of row-major (rows <= 16 * pack_nb)
int launch_rmsnorm(int dtype, const void* x, int ldx, const void* w, void* y, int ldy, int rows, int H, float eps, hipStream_t s, int pack_nb = 0);
// RMSNorm whose output goes to an fp8 x fp8 GEMM: y8[row] = e4m3(T(w * T(x * rsqrt(..))) / s_row), s_row = absmax / 448 (per token)
int launch_rmsnorm_q8(int dtype, const void* x, int ldx, const void* w, void* y8, int ldy, float* scale, int rows, int H, float eps, hipStream_t s);
// per-row e4m3 quantisation of an activation matrix [rows, H] (16-bit) -> bytes + one fp32 scale per row
int launch_quant_rows_q8(int dtype, const void* x, int ldx, void* y8, int ldy, float* scale, int rows, int H, hipStream_t s);
// decode: x = T(x + T(sum_s part[s])) in place, then xn = rmsnorm(x) * w (w == null: skip the norm).  part fp32 [ks][rows][H]
int launch_resid_rmsnorm(int dtype, void* x, int ldx, const float* part, int ks, const void* w, void* xn, int ldn, int rows, int H, float eps,
                         hipStream_t s, int pack_nb = 0);
// sequence-parallel tensor parallelism (round 6): x = T(x + y) in place on `rows` rows (y: the 16-bit sum of a row-parallel projection's partials),
// then xn = RMSNorm(x) * w (b == null), LayerNorm(x) * w + b, or nothing (w == null)
int launch_resid16_norm(int dtype, void* x, int ldx, const void* y, int ldy, const void* w, const void* b, void* xn, int ldn, int rows, int H, float eps,
                        hipStream_t s);
// ViT joint-head q/k RMSNorm in place on the fused qkv buffer [rows, 3C] (q = cols [0,C), k = [C,2C)); q is also
// multiplied by q_scale with the reference's rounding (modeling_intern_vit.py:143-148).
// sumsq_in: optional [rows,2] fp32 externally reduced sum of squares (tensor parallel); C_total = divisor.
int launch_vit_qknorm(int dtype, void* qkv, int ld, const void* wq, const void* wk, int rows, int C, int C_total,
                      float eps, float q_scale, const float* sumsq_in, hipStream_t s, int only_k = 0);      // only_k: the K half alone (round 6: Q is normed where the attention loads it)
int launch_vit_qk_sumsq(int dtype, const void* qkv, int ld, int rows, int C, float* sumsq_out, hipStream_t s);
// round 6: the K half of that norm straight from the qkv GEMM's statistics slots (slot-major stats [2 * nslots][stats_ld >= rows]: q slots [0, nslots),
// k slots [nslots, 2 nslots), nslots <= 64): k (the K columns of the fused buffer, row stride ld) = T(w_k * T(k * rsqrt(sum of the k slots / C_total + eps))) in place, and
// sumsq_q[row] = sum of the q slots for the attention kernel's q norm on load (AttnArgs.qn_sumsq)
int launch_vit_knorm_slots(int dtype, void* k, int ld, const void* wk, int rows, int C, int C_total, float eps, const float* stats, int stats_ld, int nslots,
                           float* sumsq_q, hipStream_t s);
// ------------------------------------------------------------------------------------------------ attention
struct AttnArgs {
  const void* Q; int64_t q_sb, q_sh, q_sr;     // strides in elements: batch, head, row(token)
  const void* K; int64_t k_sb, k_sh, k_sr;
  const void* V; int64_t v_sb, v_sh, v_sr;
  void* O; int64_t o_sb, o_sh, o_sr;
  int batch, q_heads, kv_heads;
  int Sq, Skv;              // common lengths; per-batch overrides below
  const int* kv_len;        // optional device [batch] (valid keys per sequence), null -> Skv
  const int* kv_start;      // optional device [batch]: keys < kv_start[b] are masked (left-padded batches), null -> 0
  int causal;               // key j visible to query i iff kv_start <= j < kv_len and (!causal or j <= i + q_pos0)
  int q_pos0;               // absolute position of query row 0 (0 for a fresh prefill)
  float scale;              // applied to scores in fp32
  int head_dim;             // 128 (0 = 128) or 64 (InternViT-300M)
  // round 6, MHA only (q_heads == kv_heads, head_dim 128): the Q half of the ViT's joint-head q / k norm applied on load -- see attn_common.h AttnP
  const float* qn_sumsq = nullptr; int qn_stride = 0, qn_dim = 0; const void* qn_w = nullptr; float qn_eps = 0.f, qn_scale = 1.f;
};
int launch_attn_prefill(int dtype, const AttnArgs& a, hipStream_t s);
// query rows i < kv_start[b] of a left-padded batch (no visible key): O = sum_j T(1 / Skv) * V[j] over ALL Skv keys, the reference's eager
// attention on a fully masked row (modeling_qwen2.py:150-172 with every score at finfo.min); needs a.kv_start
int launch_attn_uniform_rows(int dtype, const AttnArgs& a, hipStream_t s);
void attn_set_v2(int v);
void model_set_fuse_peer_norm(int v);
void attn_set_tpw(int v);
void attn_set_klds(int v);
void attn_set_dma(int v);
void attn_set_dma_slots(int v);
void attn_set_dma_rot(int v);
void attn_set_hsplit(int v);
void attn_set_mha_xcd(int v);
void attn_set_kg(int v);      // tuning key 36
void attn_set_peel(int v);    // tuning key 46
void attn_set_kv8_tpw(int v); // tuning key 47
void attn_set_kv8_fuse(int v); // tuning key 48
void attn_set_4w(int v);       // tuning key 52
void model_set_extend_attn(int v); // tuning key 49
void model_set_x12_roles(int v);   // tuning key 50
void model_set_suffix_attn(int v); // tuning key 51
int gemv_x12_default_forms();      // bit per bf16x12 role (1 gate|up, 2 down_proj, 4 lm_head) whose 16-bit launch is in its default form (no tuning key moved it)
bool attn_decode_kv8_fuses_rope(int batch, int kv_heads, int L, bool masked);
void attn_set_merge_mid_min(int v);
void attn_set_merge_dg(int v);
void gemv_set_norm_loop(int v);
void gemv_set_dyn(int v);
void gemv_set_skew(int v);
void gemv_set_rows_balance(int v);
void gemv_set_no_xs(int v);
void gemv_set_shard_shapes(int v);      // tuning key 34
void gemv_set_gu_rr(int v);             // tuning key 38
void gemv_set_longk_direct(int v);      // tuning key 39
void norm_set_wave(int v);              // tuning key 40
void model_set_ao_oproj(int v);         // tuning key 42
int gemv_get_shard_shapes();

// what every split-KV attention launch shares (launch_attn_decode, launch_attn_block): the operands with their strides in elements, the heads,
// the workspace of the partials and the optional fused-append view.  Which strides a launch reads, and what a row of Q / O is, is the
// launch's own contract (below).
struct AttnOperands {
  const void* Q; int64_t q_sb, q_sh;            // [rows, q_heads, 128] (row stride q_sb)
  const void* K; int64_t k_sb, k_sh, k_sr;      // cache [rows, kv_heads, cap, 128]; written through (cast) by the fused appends
  const void* V; int64_t v_sb, v_sh, v_sr;
  void* O; int64_t o_sb, o_sh;                  // [rows, q_heads, 128]
  int q_heads, kv_heads;
  float scale;
  float* ws; size_t ws_bytes;                   // workspace for partials
  const float* rope; int rope_max;              // cos/sin table [max_pos][64][2] or null (= q, K, V already rotated/appended)
  const void* k_new; const void* v_new; int64_t new_sb;   // raw k / v of the new tokens: [rows][kv_heads*128] views, row stride new_sb
  int o_pack_nb;                                // != 0: O is written as packed x ([rows][q_heads*128] rows, common.h) for the o_proj GEMV
};

// decode: one query token per sequence, q heads grouped per kv head; split-KV partials + merge.
// Operands: Q / O [b, q_heads, 128], K / V cache [b, kv_heads, L, 128].
// rope != null: optional fused RoPE + KV append of the token being decoded (replaces rope_kv for S = 1): q is rotated in registers,
// the split that owns position pos[b] rotates k, appends k/v to the cache and uses them from LDS
struct AttnDecodeArgs : AttnOperands {
  int batch;
  int L;                                        // kv length used when kv_len == null
  const int* kv_len;                            // optional device [batch]; null = every sequence holds exactly L keys (one dependent load less)
  const int* pos;                               // device [batch]; kv_len[b] must be pos[b] + 1
  // fp8 KV cache (BASELINE configs[4]): K / V point at OCP e4m3 bytes in the SAME [b, kv_heads, L, 128] layout (strides in elements),
  // with one fp32 scale per (sequence, kv head, key): k_scale / v_scale [b][kv_heads][scale_cap]; rope must be null (the new token is
  // rotated, appended and quantised before the call)
  const float* k_scale; const float* v_scale; int64_t scale_sb, scale_sh;
  // ... unless attn_decode_kv8_fuses_rope(batch, kv_heads, L, masked) (round 6): then `rope`, `k_new`, `v_new` are given as for the 16-bit cache
  // and the launch rotates q / k itself, appends the new rows to the e4m3 cache + scales (written through K / V / k_scale / v_scale) and to the
  // 16-bit cache k16_w / v16_w (same [b, kv_heads, L, 128] strides) -- rope_kv_kernel's bytes, no launch in front
  void* k16_w = nullptr; void* v16_w = nullptr;
  // padded batch as the reference decodes it (omchat_decode_step_masked): key j of sequence b is visible iff key_mask[b * mask_sb + j] != 0
  // (device bytes, rows zero-padded to mask_sb % 64 == 0); `pos` then holds the RoPE positions (not kv_len - 1); kv_len must be null
  const unsigned char* key_mask; int64_t mask_sb;
  // experiments build (tuning key 42): the merge launch publishes done_flags[head] = done_epoch after an agent-scope release (batch 1, <= 64 splits only)
  unsigned* done_flags = nullptr; unsigned done_epoch = 0; int done_mode = 0;
  unsigned long long* done_dbg = nullptr;      // experiments build, measurement only: clock stamp of the merge's end
};
// quantise rows [pos0, pos1) of every (sequence < b, kv head) of a 16-bit cache [b_cap, kv_heads, cap, 128] into the fp8 cache + scales
// (pos1 = null-terminated per sequence: rows >= len[b] are skipped when len != null)
int launch_kv_quant(int dtype, const void* kc, const void* vc, void* k8, void* v8, float* ks, float* vs, int b, int kv_heads, int64_t c_sb, int64_t c_sh,
                    int64_t s_sb, int64_t s_sh, const int* pos_lo, int pos0, const int* len, int max_rows, hipStream_t s);
size_t attn_decode_ws_bytes(int batch, int q_heads, int max_len);
int launch_attn_decode(int dtype, const AttnDecodeArgs& a, hipStream_t s);
// the split-KV merge alone over given partials ws [rows][q_heads][nsplit][132] (O 0..127, m at 128, l at 129), as launch_attn_decode ends: row r
// holds kv_len[r] keys (null: L) in splits of split_keys; out [rows][q_heads][128], unpacked (test hook omchat_op_attn_merge)
int launch_attn_merge(int dtype, const float* ws, int nsplit, int q_heads, int rows, const int* kv_len, int L, float scale, void* O, int split_keys,
                      hipStream_t s);

// Multi-query decode attention (prompt-lookup verify): T consecutive new tokens of ONE sequence on top of its L cached
// keys.  Query row t sits at position L + t and sees keys 0 .. L + t.  Every K / V tile is read once for all T x n_rep query rows.
// rope != null: q and the new k rows are rotated at positions L .. L + T - 1 and k / v are appended to the cache (rope_kv_kernel's bytes);
// the raw new rows are read from k_new / v_new, never from the cache slots being written.  rope == null: Q is rotated and the cache already
// holds L + T keys.  Partials go to ws as a batch of T rows (attn_decode_ws_bytes(T, q_heads, L + T)), merged by the decode merge.
// ATTN_VERIFY: S = T <= 16 with T n_rep <= 128, L; Q / O [T, q_heads, 128], K / V the cache of the sequence [kv_heads, cap, 128] (k_sb / v_sb unread).
//
// Split-KV block attention of omchat_prefill_extend: Sq new query rows of ONE sequence at positions L .. L + Sq - 1 (Q already
// rotated) over the L + Sq keys its cache already holds; row t sees keys 0 .. L + t.  The keys are split over workgroups for any Sq (16-token
// query chunks x key splits), partials in ws (attn_extend_ws_bytes), folded by the decode merge.  q_heads / kv_heads <= 8.
// ATTN_EXTEND: S = Sq, L; Q / O [Sq, q_heads, 128], K / V as for ATTN_VERIFY; rope must be null and o_pack_nb 0.
//
// Shared-prompt decode attention (omchat_group_begin with share = 1): G groups of N consecutive rows, one query token per
// row.  The rows of a group share the keys [0, P), which only its first row (the leader, row g N) holds; every row holds its own keys
// [P, len) in its own cache row.  The prefix is read once per group for the N x n_rep query rows, never beyond P; the suffix per row.
// L = keys per row counting the new one; with kv_len (device [G N]: the true lengths, all <= L) L only sizes the grid and the workspace.
// rope != null: q is rotated at len - 1, the new key (k_new / v_new row of the sequence) is rotated and appended at slot len - 1 of the row's
// own cache; rope == null: Q is rotated and the caches are complete.  N <= 16, N n_rep <= 128.
// ATTN_SHARED: G, N, P, L, kv_len (optional); Q / O [G N, q_heads, 128], K / V caches [G N rows, kv_heads, cap, 128]; ws of attn_shared_ws_bytes.
//
// Suffix-pass attention of omchat_prefill_suffixes: N rows of S query tokens each (Q already rotated, b-major), row j valid
// below kv_len[j] - P.  Query (j, t) sees the keys [0, P) of row 0 (the leader) and the keys [P, P + t] of row j's own cache; no slot >= P of
// the leader is read through the prefix, no slot < P of a sibling j > 0, no slot >= kv_len[j] of any row.  One attention launch and one
// merge whatever N is.  Rows t >= kv_len[j] - P are padding: computed from the row's valid keys, finite when the padding q is.
// q_heads / kv_heads <= 8, N S <= 65535.
// ATTN_SUFFIX: N, S, P, kv_len (device [N]: keys row j holds counting its suffix, in [P + 1, P + S]); Q / O [N S, q_heads, 128], K / V caches
// [N rows, kv_heads, cap, 128]; ws of attn_suffix_ws_bytes; rope must be null and o_pack_nb 0.
enum AttnBlockMode { ATTN_VERIFY = 0, ATTN_EXTEND, ATTN_SHARED, ATTN_SUFFIX };
struct AttnBlockArgs : AttnOperands {
  int mode;                                     // AttnBlockMode: which of the four contracts above holds; the integers it does not name are ignored
  int G, N, S, P, L;
  const int* kv_len;
};
constexpr int VERIFY_MAX_T = 16;
size_t attn_block_ws_bytes(const AttnBlockArgs& a);      // bytes of partials the launch needs: reads the mode, its integers and the heads only
int launch_attn_block(int dtype, const AttnBlockArgs& a, hipStream_t s);
int attn_verify_tpw(int keys, int kv_heads);      // 64-key tiles per split of an ATTN_VERIFY launch over `keys` keys
// the plan launch_attn_block takes for a mode and its integers on this device: out = {tpw, nsp, nss, tps} (test hook omchat_op_attn_block_plan)
int attn_block_plan_query(int mode, int G, int N, int S, int q_heads, int kv_heads, int P, int L, int out[4]);
size_t attn_extend_ws_bytes(int Sq, int q_heads, int kv_heads, int L);
size_t attn_shared_ws_bytes(int G, int N, int q_heads, int kv_heads, int P, int L);
size_t attn_suffix_ws_bytes(int N, int S, int q_heads, int kv_heads, int P);

// batch-1 decode on one GPU (fused_decode.hip, round 4): launch_attn_decode + the o_proj GEMV with EPI_RESID as ONE launch, same bits.
// x [H] is the residual stream (read, x + o_proj(attn) written in place), Wo [H][qd] row-major; ws = fused_decode_ws_bytes(q_heads) bytes
// of zero-initialised device memory owned by the caller and used by no other launch at the same time; epoch: a value that no earlier launch
// on the same ws has used (monotonic counter, never 0); err: device word that collects time-out bits (0 = every hand-off completed).
struct FusedDecodeArgs {
  const void* Wo; int ldw;
  void* x; int H, qd;
  void* ws; unsigned epoch;
  unsigned* err; int timeout_ms;
  void* dbg = nullptr;      // diagnostic build of tools/experiments/tune_fused.hip only: phase stamps [CUs][16]; the library never sets it
};
size_t fused_decode_ws_bytes(int q_heads);
bool attn_oproj_fused_ok(const AttnDecodeArgs& a, int H, int qd);
int launch_attn_oproj_fused(int dtype, const AttnDecodeArgs& a, const FusedDecodeArgs& f, hipStream_t s);
void model_set_fuse_attn_oproj(int v);
void model_set_decode_layer(int v);
void model_set_shard_as_tp1(int v);      // tuning key 35

// batch-1 decode on one GPU (decode_layer.hip, round 4): ONE decoder layer -- the six launches qkv GEMV (+ input RMSNorm), split-KV
// attention (+ RoPE, cache append), merge, o_proj (+ residual), gate|up GEMV (+ post-attention RMSNorm, SwiGLU), down_proj (+ residual) -- as
// ONE launch with in-launch hand-offs; the same bits.  Weights row-major as the context holds them (wgu: gate / up interleaved in 16-row
// blocks); x [H] is the residual stream, read and overwritten with the layer's output; kc / vc this layer's cache [kv_heads][cap][128] with
// head stride k_sh elements; kv_len = keys after this step (the new token at kv_len - 1).  ws = decode_layer_ws_bytes(...) bytes of
// zero-initialised device memory used by no other launch at the same time; epoch: a value no earlier launch on the same ws has used (never 0).
struct DecodeLayerArgs {
  const void *ln1, *ln2, *wqkv, *bqkv, *wo, *wgu, *wd;
  void *kc, *vc; int64_t k_sh;
  void* x;
  int H, qd, kvd, It, q_heads, kv_heads, kv_len;
  const float* rope; int rope_max;
  float eps, scale;
  void* ws; unsigned epoch;
  unsigned* err; int timeout_ms;
  void* dbg = nullptr;      // diagnostic build only
};
size_t decode_layer_ws_bytes(int q_heads, int H, int qd, int kvd, int It);
bool decode_layer_ok(const DecodeLayerArgs& a);
int launch_decode_layer(int dtype, const DecodeLayerArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------ RoPE + KV append
// qkv [rows, (nq + 2 nkv) * 128] post-bias; rotate q in place, write rotated k and raw v into the caches at
// position pos[row] of sequence seq[row] (rows are b-major: row = b_idx * S + s).
struct RopeArgs {
  void* qkv; int ld;
  int rows, S;                 // rows = b * S
  int nq, nkv;
  const int* pos;              // device [rows] absolute positions, or null -> pos0 + (row % S)
  int pos0;
  const float* cos_sin;        // table [max_pos][64][2] fp32 (cos, sin)
  int max_pos;
  void* kcache; void* vcache;  // [b, nkv, cap, 128]
  int64_t c_sb, c_sh;          // cache strides (elements); row stride 128
  // optional (fp8 KV cache, decode): the appended k / v rows are ALSO quantised here (what launch_kv_quant would do to them in a launch
  // of its own): e4m3 bytes into k8 / v8 (same [b, nkv, cap, 128] layout, strides in elements = bytes), one fp32 scale per row into
  // ks / vs [b][nkv][s_sh]
  void* k8 = nullptr; void* v8 = nullptr; float* ks = nullptr; float* vs = nullptr; int64_t s_sb = 0, s_sh = 0;
  // cache slot of row r when it differs from the RoPE position (masked decode of a padded batch: every row appends at the COMMON slot and
  // rotates to its own position, omchat_arch.py:61-70): slot0 + (r % S); -1 = the position itself
  int slot0 = -1;
  // suffix pass (omchat_prefill_suffixes): device [b] end of each sequence's valid slots; a k / v row whose slot is >= kv_end[row / S] is a
  // padding row and is not stored (q is still rotated).  null = every row is stored
  const int* kv_end = nullptr;
};
int launch_rope_kv(int dtype, const RopeArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------ data movement
// im2col for Conv2d(3->C, k=p, s=p): pixels [B,3,HW,HW] -> cols [B*g*g, Kpad] (zero padded K)
int launch_im2col(int dtype, const void* pixels, void* cols, int B, int HW, int patch, int Kpad, hipStream_t s);
// x[b, 0] = cls + pos[0];  x[b, 1+p] = pe[b*np + p] + pos[1+p]
int launch_vit_assemble(int dtype, const void* pe, const void* cls, const void* pos, void* x, int B, int np, int C, hipStream_t s);
// out[r] = table[idx[r]] (idx >= 0) | feats[-1 - idx[r]] (idx <= -1, > PAD) | 0 (idx == INT_MIN)
// out[M, N] = epi(sum[M, N] (fp32), bias, ls, resid) with the rounding points of the GEMM epilogues (EPI_NONE / EPI_RESID / EPI_LS_RESID)
int launch_tp_finish(int dtype, const float* sum, const void* bias, const void* ls, const void* resid, void* out, int M, int N, int epi, hipStream_t s);
int launch_gather_rows(int dtype, const int* idx, const void* table, const void* feats, void* out, int rows, int H, hipStream_t s);
// strided row copy (drop CLS etc.): dst[r] = src[map(r)]
int launch_copy_rows(int dtype, const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int rows, int H,
                     int group, int skip, hipStream_t s);   // src row = (r / group) * (group + skip) + skip + r % group
// argmax over fp32 logits [b, V] -> int32 [b] (first index wins ties)
size_t argmax_scratch_bytes(int b);
// adv_pos / adv_len (optional, device [b]): incremented by one in the second stage -- the decode step's position bookkeeping without a launch of its own
int launch_argmax(const float* logits, int ld, int b, int V, int* out, void* scratch, hipStream_t s, int* adv_pos = nullptr, int* adv_len = nullptr);   // scratch: argmax_scratch_bytes(b)
// on-device sampling (sample.hip): repetition penalty, temperature, top-k, top-p, Gumbel-max draw keyed by (seed, row, step[row], global
// index); tests/sampling_ref.py restates it.  Rank-local logits [b, ld]; under tensor parallelism (tp > 1) the integer histograms and the final
// (value, index) pairs go through xchg (the context's fp32 all-reduce) and `table` ([tp][b][2] fp32, the greedy exchange's).
// HF's four warpers behind top-p, in HF's order: MinP, Typical, Epsilon, Eta (min_tokens_to_keep = 1).  Off: min_p < 0, the others >= 1.
// With any of them the kept set is a key interval [lo, hi] of the processed logits (typical_p can cut the top): DESIGN.md section 9.
struct SampleFilters {
  double min_p = -1.0, typical_p = 1.0, epsilon = 1.0, eta = 1.0;
  bool min_p_on() const { return min_p >= 0.0; }
  bool typical_on() const { return typical_p < 1.0; }
  bool epsilon_on() const { return epsilon < 1.0; }
  bool eta_on() const { return eta < 1.0; }
  bool any() const { return min_p_on() || typical_on() || epsilon_on() || eta_on(); }
  bool operator==(const SampleFilters& o) const { return min_p == o.min_p && typical_p == o.typical_p && epsilon == o.epsilon && eta == o.eta; }
};
struct SampleArgs {
  const float* logits = nullptr; int ld = 0, b = 0, V = 0, V_total = 0;   // V: this rank's vocabulary slice
  int rank = 0, tp = 1;
  uint64_t seed = 0; float temperature = 1.f; int top_k = 0; double top_p = 1.0; float penalty = 1.f;
  SampleFilters f;
  uint32_t* bitmap = nullptr; int bm_words = 0;     // [b][bm_words] seen tokens of this rank's slice (read when penalty != 1, picked id set)
  int* last_set = nullptr;                          // [b] local index whose bit the last pick set, -1 = none (omchat_kv_rewind)
  int* step = nullptr;                              // [b] device step counters, advanced by one
  int* adv_pos = nullptr; int* adv_len = nullptr;   // optional: decode positions advanced with the pick
  int* out = nullptr; uint32_t* thr_out = nullptr;  // picked ids [b]; optional threshold keys [b] (test hook)
  uint32_t* hi_out = nullptr;                       // optional upper keys [b] (test hook): 0xFFFFFFFF when the top is kept
  void* ws = nullptr;                               // sample_ws_bytes(b)
  float* table = nullptr;
  // verify form (omchat_decode_verify with OMCHAT_VERIFY_SAMPLE): vtokens (device int32 [b], 2 <= b <= 16) = the last
  // emitted id and the drafts of sequence 0.  Row j draws with the key of row 0 at step[0] + j and, under the penalty, sees bitmap row 0 plus
  // vtokens[1..j] (built into vseen, scratch [SMP_VERIFY_ROWS][bm_words]).  Every other per-row state stays indexed by j.  Nothing is
  // committed: out[j] only; bitmap, last_set, step and the decode positions are left to the acceptance.
  const int32_t* vtokens = nullptr;
  uint32_t* vseen = nullptr;
  int (*xchg)(void* user, float* buf, size_t count, hipStream_t s) = nullptr;
  void* xchg_user = nullptr;
};
constexpr int SMP_VERIFY_ROWS = VERIFY_MAX_T;
size_t sample_ws_bytes(int b);
int launch_sample(const SampleArgs& a, hipStream_t s);
// take back n picks: clears the bit the last pick set (n == 1), step -= n
int launch_sample_rewind(uint32_t* bitmap, int bm_words, int* last_set, int* step, int b, int n, hipStream_t s);
// take back the last r of the cnt picks a sampled verify step committed to sequence 0: clears the bits vlast[cnt - r .. cnt) recorded as
// newly set (bitmap: row 0, or nullptr without the penalty), step[0] -= r
int launch_sample_rewind_verify(uint32_t* bitmap, int* vlast, int* step, int cnt, int r, hipStream_t s);
// where the last launch_sample on (ws, b) left row r's kept-set threshold key: words[r * *stride]; nullptr when the parameters keep every token.
// *hi: the upper key of the kept interval, same stride; nullptr when the parameters keep the top (typical_p off)
const uint32_t* sample_thr_words(const void* ws, int b, int V_total, int top_k, double top_p, const SampleFilters& f, int* stride,
                                 const uint32_t** hi);
// per-token log-probabilities of picked ids (logprob.hip; tests/logprob_ref.py restates it).  Rank-local fp32 logits
// [b, V]; raw = log_softmax(raw)[id], processed = log_softmax(scores)[id] with scores evaluated on the fly from `proc` (the banned copy of
// the constraints, or raw): ban bitmap, repetition penalty over `seen` (the bit the pick itself set, last_set, not counted), / temperature,
// kept iff thr[row * thr_stride] <= smp_key(value) <= thr_hi[row * thr_stride] (thr == nullptr: no lower bound, thr_hi == nullptr: no upper
// bound; top1: only the maxima are kept, the sampler's top_k == 1).
// An id that is not among the maxima records -inf under top1, as any cut id does.
// Both land in rec = float [2][max_new][rec_ld] at column `row`, line cnt[row], and cnt[row] advances.  tp > 1: one xchg of `table`.
struct LogprobArgs {
  const float* raw = nullptr; int raw_ld = 0;
  const float* proc = nullptr; int proc_ld = 0;     // nullptr: raw
  int b = 0, V = 0, rank = 0, tp = 1;
  const int* ids = nullptr;                          // [b] picked ids, global index, device
  const uint32_t* ban = nullptr;                     // optional [b][bm_words]
  const uint32_t* seen = nullptr; int bm_words = 0; const int* last_set = nullptr;
  float temperature = 1.f, penalty = 1.f;
  const uint32_t* thr = nullptr; const uint32_t* thr_hi = nullptr; int thr_stride = 1; int top1 = 0;
  void* ws = nullptr;                                // logprob_ws_bytes(b)
  float* table = nullptr;                            // logprob_table_bytes(b, tp), tp > 1
  int (*xchg)(void* user, float* buf, size_t count, hipStream_t s) = nullptr;
  void* xchg_user = nullptr;
  float* rec = nullptr; int* cnt = nullptr; int max_new = 0, rec_ld = 0;
  // extras (both 0: the launches above and nothing else): the top_n <= 20 best (log_softmax(raw) value, global id) pairs of every row, by
  // value descending (-0 == +0) then id ascending, into top_vals / top_ids [max_new][rec_ld][top_n], and the raw log-probability of the
  // n_score <= 32 global ids score_ids (device) into scored [max_new][rec_ld][n_score] -- line cnt[row], before it advances; the values are
  // lp_value(x, m0, s0) with the (m0, s0) of the picked id's raw value.  top_ws: logprob_top_ws_bytes(b, top_n); tp > 1: table is
  // logprob_table_bytes_ex(b, tp, top_n, n_score), still one xchg, and V * tp < 2^24 (ids cross as fp32)
  int top_n = 0, n_score = 0;                       // <= LP_MAX_TOP, <= LP_MAX_SCORED
  const int* score_ids = nullptr;
  void* top_ws = nullptr;
  float* top_vals = nullptr; int* top_ids = nullptr; float* scored = nullptr;
};
constexpr int LP_MAX_TOP = 20, LP_MAX_SCORED = 32;      // the public header's OMCHAT_LP_MAX_* (capi.hip asserts they agree)
size_t logprob_ws_bytes(int b);
size_t logprob_table_bytes(int b, int tp);
size_t logprob_top_ws_bytes(int b, int top_n);
size_t logprob_table_bytes_ex(int b, int tp, int top_n, int n_score);
int launch_logprob(const LogprobArgs& a, hipStream_t s);
int launch_logprob_rewind(int* cnt, int b, int n, hipStream_t s);      // cnt[i] -= n for rows < b

// ------------------------------------------------------------------------------------------------ teacher-forced scoring (score.hip)
// logprob[row] = log_softmax(A[row] W^T)[labels[row]] without the logits: launch_gemm with EPI_LSE leaves the (max, sum) pairs of every 64-column
// slot and the label's logit in the workspace, launch_score_finish folds a row's slots in a fixed order (one wave per row).  A row whose label
// is -100 gets 0; a label outside {-100} u [0, N) is the caller's to refuse before the launch (the kernels stay in bounds and write NaN).
// ws: score_ws_bytes(M, N) bytes, 16-byte aligned.  lse [M] may be null.
size_t score_ws_bytes(int M, int N);
int launch_score(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int* labels, float* logprob, float* lse,
                 void* ws, size_t ws_bytes, hipStream_t s);
// out[0] = -sum logprob over the rows with label >= 0, out[1] = their number, out[2 + i] = sum logprob of sequence i (rows [i * S, (i + 1) * S)),
// out[2 + b + i] = its number of scored rows.  One workgroup, fixed trees: the same bits every run
int launch_score_reduce(const float* logprob, const int* labels, int b, int S, float* out, hipStream_t s);
// HF logits constraints (constrain.hip; tests/constraints_ref.py restates the ban set).  The caps are the public
// header's OMCHAT_CON_* (capi.hip asserts they agree).
constexpr int CON_NGRAM_MAX = 64, CON_EOS_MAX = 16, CON_SUPPRESS_MAX = 1024, CON_BAD_WORDS_MAX = 1024, CON_BAD_WORD_IDS_MAX = 8192;
constexpr int CON_LIST_WORDS = CON_EOS_MAX + 2 * CON_SUPPRESS_MAX + CON_BAD_WORDS_MAX + 1 + CON_BAD_WORD_IDS_MAX;      // int32 words of the device lists
struct ConstrainArgs {
  int32_t* hist = nullptr; int hist_ld = 0;         // [b][hist_ld] token history as HF's processors see it (prompt row + fed ids)
  int* len = nullptr; const int* plen = nullptr;    // [b] ids held / ids of the prompt row
  const int32_t* tok = nullptr;                     // [b] the token this decode step is fed (appended at hist[len]), NULL at the first pick
  int b = 0, V = 0, V_total = 0, gbase = 0;         // V: this rank's vocabulary slice, gbase = rank * V
  int ngram = 0, min_new = 0, min_len = 0;
  const int32_t *eos = nullptr, *sup = nullptr, *bsup = nullptr, *bw_ids = nullptr, *bw_off = nullptr;
  int n_eos = 0, n_sup = 0, n_bsup = 0, n_bw = 0;
  uint32_t* ban = nullptr; int bmw = 0;             // [b][bmw] ban bitmap, all-zero on entry; bits of this pick's ban set are set
  uint32_t* seen = nullptr;                         // [b][bmw] or NULL: the ids of the row's history (beam search's repetition penalty, beam.hip)
};
int launch_constrain_ban(const ConstrainArgs& a, hipStream_t s);
// out [b][V] = logits with the banned ids at -inf; clears the bitmap; len (optional) += 1: the fed token the ban pass stored is now counted
int launch_constrain_apply(const float* logits, int ld, int b, int V, uint32_t* ban, int bmw, float* out, int* len, int hist_ld, hipStream_t s);
int launch_constrain_append(int32_t* hist, int hist_ld, int* len, const int32_t* tok, int b, hipStream_t s);
int launch_constrain_rewind(int* len, const int* plen, int b, int n, hipStream_t s);
int constrain_pack_lists(const int32_t* eos, int n_eos, const int32_t* sup, int n_sup, const int32_t* bsup, int n_bsup, const int32_t* bw_ids,
                         const int32_t* bw_off, int n_bw, int32_t* out, ConstrainArgs& a);      // out: [CON_LIST_WORDS], host
void constrain_bind_lists(const int32_t* d_lists, ConstrainArgs& a);
// finite-state token constraints (fsm.hip; tests/fsm_ref.py restates them).  The caps are the public header's
// OMCHAT_FSM_* (capi.hip asserts they agree): every index of the table stays in int32.
constexpr int FSM_MAX_STATES = 1 << 20, FSM_MAX_EDGES = 1 << 26, FSM_DEAD = -1;
struct FsmTable {      // CSR in device memory; tok 16-byte aligned and allocated up to a multiple of four ids behind the last edge
  const int32_t* off = nullptr; const int32_t* tok = nullptr; const int32_t* nxt = nullptr; int n_states = 0;
};
struct FsmArgs {
  int32_t* trail = nullptr; int cap = 0;          // [b][cap] the row's state after k fed tokens at trail[row][k]
  int* cnt = nullptr;                             // [b] fed tokens so far
  int32_t* cur = nullptr;                         // [b] the state this pick masks with (written by the mark pass, read by the apply pass)
  const int32_t* fed = nullptr;                   // [b] the token the decode step is fed, or NULL (first pick after the prefill: no advance)
  int b = 0, V = 0, gbase = 0;                    // rank-local slice [gbase, gbase + V)
  uint32_t* bm = nullptr; int bmw = 0;            // [b][bmw] allowed bitmap, all-zero on entry and again behind the apply pass
};
int launch_fsm_mark(const FsmTable& T, const FsmArgs& a, hipStream_t s);
// out [b][V] = logits with the ids whose bit is clear at -inf (DEAD rows pass through; logits == out allowed); clears the bitmap; advance: cnt += 1
int launch_fsm_apply(const float* logits, int ld, const FsmArgs& a, float* out, bool advance, hipStream_t s);
int launch_fsm_advance(const FsmTable& T, const FsmArgs& a, hipStream_t s);      // a step that picks nothing: trail and cnt move, no mask
int launch_fsm_rewind(int* cnt, int b, int n, hipStream_t s);                    // cnt = max(cnt - n, 0)
int fsm_validate(int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, int V_total);      // host arrays; sets the error
// classifier-free guidance (guidance.hip; tests/guidance_ref.py restates it): logits fp32 [2b][ld], rows [0, b)
// conditional, rows [b, 2b) their twins; out [b][ld_out] = scale * (lc - lu) + lu over the V ids of a row (ld, ld_out >= V), lc / lu the two
// log-softmaxes; -inf wherever either logit is -inf.  ws: guidance_ws_bytes(b, V) bytes, written and read by the two launches of one call.
// Deterministic (fixed reduction orders, no atomics).
size_t guidance_ws_bytes(int b, int V);
int launch_guidance(const float* logits, int ld, int b, int V, float scale, void* ws, float* out, int ld_out, hipStream_t s);
// behind the pick: next_tokens[b + r] = next_tokens[r]; with pos / len (both or neither) pos += 1, len += 1 for all 2b rows
int launch_guidance_twin(int32_t* next_tokens, int b, int* pos, int* len, hipStream_t s);
// layer-contrastive decoding (dola.hip; tests/dola_ref.py restates it): logits fp32 [(k + 1) * b][ld], rows [0, b) the
// final layer's, row (1 + j) * b + r candidate j of sequence r; out [b][ld_out] = the relative-top-filtered contrast of each sequence's final
// row with the candidate of the largest Jensen-Shannon divergence from it (the lowest j on ties; k == 1: no divergence is computed).
// picked (or NULL): that candidate's position per sequence.  rec (or NULL): layers[position] is appended to line cnt[r] of the int32 record
// [cap][rec_ld] and cnt[r] += 1.  ws: dola_ws_bytes(b, k, V) bytes, written and read by the launches of one call.  Deterministic.
constexpr int DOLA_MAX_LAYERS = 16;
struct DolaArgs {
  const float* logits = nullptr; int ld = 0, V = 0, b = 0, k = 0;
  float relative_top = 0.1f;
  float* out = nullptr; int ld_out = 0;
  int32_t* picked = nullptr;
  void* ws = nullptr; size_t ws_bytes = 0;
  const int32_t* layers = nullptr; int32_t* rec = nullptr; int* cnt = nullptr; int cap = 0, rec_ld = 0;
};
size_t dola_ws_bytes(int b, int k, int V);
int launch_dola(const DolaArgs& a, hipStream_t s);
// contrastive search (contrastive.hip; tests/contrastive_ref.py restates it).  Deterministic: fixed orders, no atomics.
constexpr int CS_KMAX = 16;              // candidates per step
constexpr int CS_EOS_MAX = 8;
constexpr int CS_REC_WORDS = 52;         // a step's record: ids [16], probabilities [16], penalties [16], the pick, the emitted id, chunks, history rows
// the penalty launch's cut of L history rows into chunks of rows_per_chunk rows (a multiple of 16; one wave per chunk, up to 4 per CU)
void cs_plan(int L, int cus, int* chunks, int* rows_per_chunk);
// inv[r] = 1 / ||rows[r]||_2 in fp32 for n 16-bit rows [n][H] (H % 8 == 0)
int launch_cs_norms(int dtype, const void* rows, int n, int H, float* inv, hipStream_t s);
// part[c * 16 + i] = max over the history rows j of chunk c of dot(cand_i, hist_j) * inv[j] * inv_c[i]; cand: k 16-bit rows, row-major [k][H]
// (cand_nb = 0) or in the packed x layout of common.h with cand_nb blocks of 16 rows; cand_inv [k] receives inv_c.  H % 32 == 0, L >= 1.
int launch_cs_penalty(int dtype, const void* hist, const float* inv, int L, int H, const void* cand, int cand_nb, int k, float* part,
                      float* cand_inv, hipStream_t s);
// ids / probs [k]: the k largest of row (row_sel ? *row_sel : 0) of fp32 logits [rows][ld] by (value descending, id ascending) and their
// softmax probabilities under the fp32 (max, sum exp) of the row's V ids; columns at or beyond V are never read.  ws: cs_topk_ws_bytes(V)
size_t cs_topk_ws_bytes(int V);
int launch_cs_topk(const float* logits, int ld, const int* row_sel, int V, int k, int32_t* ids, float* probs, void* ws, hipStream_t s);
// the fold of the partial maxima, the scores (1 - alpha) p_i - alpha pen_i, the pick (the first maximum), the emitted id and the done word
// (an EOS id, or `last`), the append of the picked row and its inverse norm to the history at row n_hist, the step's record, parents[r] = pick
struct CsSelectArgs {
  const float* part = nullptr; int chunks = 0, k = 0;
  float alpha = 0.f, one_minus_alpha = 1.f;
  const int32_t* ids = nullptr; const float* probs = nullptr; const float* cand_inv = nullptr;
  const void* cand = nullptr; int cand_nb = 0, H = 0;
  void* hist = nullptr; float* inv = nullptr; int n_hist = 0;
  int eos[CS_EOS_MAX] = {0}; int n_eos = 0; int last = 0;
  int32_t* rec = nullptr;                  // the step's CS_REC_WORDS words (or NULL)
  int* parents = nullptr; int* sel = nullptr; int32_t* token = nullptr; int32_t* done_word = nullptr;      // (each may be NULL)
};
int launch_cs_select(int dtype, const CsSelectArgs& a, hipStream_t s);
// beam search (beam.hip; tests/beam_ref.py restates it).  The vocabulary is cut into beam_slices(V, tp) equal slices
// of at most BEAM_SLICE_CAP ids, the same at every TP degree; a rank owns ns / tp whole slices.  Exchange table: [rows][ns][4 + 2K] fp32.
constexpr int BEAM_KMAX = 32;            // candidates kept per step and prompt: max(2, 1 + n_eos) * N
constexpr int BEAM_NMAX = 16;
constexpr int BEAM_EOS_MAX = 8;
constexpr int BEAM_NS_MAX = 16;
constexpr int BEAM_SLICE_CAP = 20480;
int beam_slices(int V_total, int tp);    // -1: no slicing for this vocabulary and TP degree
// state words (int32 / fp32 bits) of b prompts x N beams: running score, finished score / flag / step / parent beam / token ([6][b * N]),
// early-stop flag [b], done flag [b], backpointers [max_new][b * N][2] (parent beam, token), two counters
enum { BST_RUN = 0, BST_FSC = 1, BST_FFL = 2, BST_FSTEP = 3, BST_FPAR = 4, BST_FTOK = 5 };
__host__ __device__ inline size_t beam_state_words(int b, int N, int max_new) {
  return (size_t)6 * b * N + 2 * (size_t)b + (size_t)2 * max_new * b * N + 2;
}
struct BeamFinishArgs {
  const float* table = nullptr; int ns = 1, K = 0, KB = 0, V_total = 0;
  int b = 0, N = 0, t = 0, max_new = 0;
  int es = 0; bool lp_pos = false;         // early_stopping: 0 False, 1 True, 2 "never"; length_penalty > 0
  const float* dn = nullptr;               // [max_new + 1]: dn[g] = fp32(pow(g, length_penalty))
  int eos[BEAM_EOS_MAX] = {0}; int n_eos = 0;
  int* state = nullptr;                    // beam_state_words(b, N, max_new)
  int* tokens = nullptr; int* parents = nullptr; int* done_word = nullptr;      // [b * N], [b * N] (cache rows), 1 word
  bool proc = false;                       // the table's values are processed log-probabilities (launch_beam_select_processed), not raw logits
};
int launch_beam_select(const float* logits, int ld, int rows, int V_local, int rank, int tp, int ns, int K, float* table, hipStream_t s);
int launch_beam_finish(const BeamFinishArgs& a, hipStream_t s);
// beam search on processed scores (omchat_beam_processors; tests/beam_proc_ref.py restates it; TP = 1 only).  Two launches in place of
// launch_beam_select: the statistics pass leaves every (row, slice) max and fixed-point sum in the table; the selection pass recomputes the
// row's (max, lse) from them, forms lp = fl(fl(x - max) - lse) in registers, scales the ids of `seen` (NULL: no penalty) by the repetition
// penalty (lp < 0 ? lp * penalty : lp / penalty), sets the ids of `ban` to -inf and keeps each slice's top K (lp, id) pairs.  The bitmaps
// [rows][bmw] are only read: launch_beam_hist_move clears them behind the finish.
int launch_beam_stats(const float* logits, int ld, int rows, int V, int ns, int K, float* table, hipStream_t s);
int launch_beam_select_processed(const float* logits, int ld, int rows, int V, int ns, int K, float* table, const uint32_t* ban,
                                 const uint32_t* seen, int bmw, float penalty, hipStream_t s);
// per-path token histories [rows][ld]: dst[r][P, P + g) = src[parents[r]][P, P + g), dst[r][P + g] = tokens[r], len[r] = P + g + 1 for
// rows r < rows (rows = 0: nothing moves); a parent outside row r's own prompt (N rows each) counts as r itself.  The prompt parts [0, P)
// are not touched.  Also zeroes bm_words words at bm (the ban and seen bitmaps of the step just finished).
int launch_beam_hist_move(const int32_t* src, int32_t* dst, int rows, int N, int ld, int P, int g, const int* parents, const int* tokens, int* len,
                          uint32_t* bm, size_t bm_words, hipStream_t s);
// KV rows between sequences: cache layout [layers][rows_cap][kvh][max_seq][128] (16-bit; e4m3 bytes in the same layout, scales
// [layers][rows_cap][kvh][max_seq]); the stash holds [layers][st_rows][kvh][st_slots] slots of the same kinds
struct KvGatherArgs {
  char *k = nullptr, *v = nullptr, *k8 = nullptr, *v8 = nullptr; float *ks = nullptr, *vs = nullptr;
  int layers = 0, kvh = 0, max_seq = 0, rows_cap = 0;
  char *sk = nullptr, *sv = nullptr, *sk8 = nullptr, *sv8 = nullptr; float *sks = nullptr, *svs = nullptr;
  int st_rows = 0, st_slots = 0;
};
// row r in [row0, row0 + nrows) becomes a copy of its parent over slots [lo, hi): parents (device, values in [row0, row0 + nrows)) through
// the stash, free of hazards for any parent map; parents == nullptr: every row <- fork_src, straight (the caller orders forks)
int launch_kv_gather(const KvGatherArgs& a, const int* parents, int row0, int nrows, int fork_src, int lo, int hi, hipStream_t s);
// deterministic synthetic fill (bit-identical to omchat_amd/synth.py::uniform)
int launch_fill_uniform(int dtype, void* dst, int64_t n, uint64_t key, float scale, float offset, hipStream_t s);
int launch_cast_f32(int dtype, const void* src, float* dst, int64_t n, hipStream_t s);
