// Weight-streaming skinny GEMM for decode:  Y[b,N] = epi(X[b,K] @ W[N,K]^T), b <= 32 (one or two 16-row batch tiles).  HBM-bound: every weight byte
// is read exactly once, straight from global memory into MFMA A-operand registers (no LDS round trip:
// cdna_hip_programming.md §5 "GEMV / M <= 16 decode weights").
//
// Replaces the decode-step `nn.Linear`s of transformers' Qwen2 (q/k/v/o/gate/up/down/lm_head with M = batch).
//
// One workgroup = 8 waves = NTILE*16 weight rows.  Wave w walks 64-wide K chunks w, w+8, w+16, ... : per chunk a
// lane loads 2 x 16 B of its weight row (A operand, row = lane&15, k = 8*(lane>>4)+j) and 2 x 16 B of x (B operand,
// column = batch row = lane&15; lanes >= b feed zeros), then 2 MFMA 16x16x32.  UNROLL chunks are in flight per wave
// (8 waves x UNROLL x 2 KiB per workgroup).  The 8 partial 16x16 fp32 tiles are summed through LDS in a fixed order
// (deterministic, no atomics), and wave 0 applies the epilogue.
#include "kernels.h"
#include "rowdot.h"
#include <type_traits>

namespace {

struct GemvP {
  const void* X; const void* W; void* Y; const void* bias; const void* resid;
  int ldx, ldw, ldy, ldr, b, N, K, out_f32, ksplit;
  const float* w_scale;
  int y_packed;
  const void* norm_w; float norm_eps;      // whole-row batch-1 form: X is the RAW hidden row, normalised in registers (gemv_rows_norm_kernel)
  unsigned* dyn;                           // gemv_rows_norm_dyn_kernel: 8 pool counters + 1 completion counter (one 256-byte line each), zero before the first launch
  void* y_pack;                            // gemv_xs_kernel<EPI_RESID>: packed copy of the result rows
  unsigned long long* dbg;                 // experiments build: clock stamps (measurement of the out-of-order prototype), else null
  const unsigned char* mx_s;               // non-null: W is MXFP4 (two e2m1 codes per byte, ldw in bytes) and mx_s [N][K / 32] holds the e8m0 block scales
  const unsigned char* x12_top;            // non-null: W is bf16x12 (coded rows of ldw = K * 3 / 2 bytes) with x12_top [N], x12_cnt [N], x12_patch [N][32]
  const unsigned char* x12_cnt;
  const unsigned* x12_patch;
#if OMCHAT_EXPERIMENTS
  int xskew;                               // tuning key 28 < 256 (experiment): workgroups moved from every odd XCD's share to every even XCD's (gate|up non-loop form)
#endif
};
// weight format of the whole-row batch-1 forms (template switch): 16-bit, OCP e4m3 bytes + one fp32 scale per row, MXFP4 (OCP Microscaling
// v1.0: e2m1 codes, two per byte, + one e8m0 scale per 32 consecutive k)
// ... and bf16x12, the lossless 12-bit coding of bf16 rows (below: "bf16x12"): the same weights bit for bit, three quarters of the bytes
// (WF_16 / WF_E4M3 / WF_MX4 / WF_X12: kernels.h)
// stamps: [0] merge end, [1] o_proj first start (stored inverted: max of ~t), [2] o_proj flags seen, [3] o_proj end, [4] gate|up first start (inverted), [5] gate|up end,
// [6] down_proj first start (inverted), [7] down_proj end, [8] qkv first start (inverted), [9] qkv end, [10] attention first start (inverted), [11] attention end, [12] merge first start (inverted), [16 + x] gate|up end on XCD x
#if OMCHAT_EXPERIMENTS
#define OM_DBG_MIN(slot, cond) do { if (p.dbg && (cond) && threadIdx.x == 0) atomicMax(p.dbg + (slot), ~wall_clock64()); } while (0)
#define OM_DBG_MAX(slot, cond) do { if (p.dbg && (cond) && threadIdx.x == 0) atomicMax(p.dbg + (slot), wall_clock64()); } while (0)
#else
#define OM_DBG_MIN(slot, cond) do { } while (0)
#define OM_DBG_MAX(slot, cond) do { } while (0)
#endif

template <typename T, int NTILE, int N, int WAVES, bool NTL, int NB>
__device__ __forceinline__ void gemv_group(f32x4 (&acc)[NTILE][NB], const T* const (&wrow)[NTILE], const T* const (&xrow)[NB], int k0,
                                           const bool (&xvalid)[NB]) {
  typedef typename V8<T>::type frag_t;
  frag_t wf[N][NTILE][2], xf[N][NB][2];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int k = k0 + u * WAVES * 64;
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
      if constexpr (NTL) {
        wf[u][t][0] = __builtin_nontemporal_load(reinterpret_cast<const frag_t*>(wrow[t] + k));
        wf[u][t][1] = __builtin_nontemporal_load(reinterpret_cast<const frag_t*>(wrow[t] + k + 32));
      } else {
        wf[u][t][0] = ld8<T>(wrow[t] + k);
        wf[u][t][1] = ld8<T>(wrow[t] + k + 32);
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      xf[u][nb][0] = ld8<T>(xrow[nb] + k);
      xf[u][nb][1] = ld8<T>(xrow[nb] + k + 32);
    }
  }
  frag_t zero;
#pragma unroll
  for (int j = 0; j < 8; ++j) zero[j] = (T)0.f;
#pragma unroll
  for (int u = 0; u < N; ++u) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (!xvalid[nb]) { xf[u][nb][0] = zero; xf[u][nb][1] = zero; }
#pragma unroll
      for (int t = 0; t < NTILE; ++t) {
        acc[t][nb] = mfma16(wf[u][t][0], xf[u][nb][0], acc[t][nb]);
        acc[t][nb] = mfma16(wf[u][t][1], xf[u][nb][1], acc[t][nb]);
      }
    }
  }
}

template <typename T, int NTILE, int N, int WAVES, bool NTL, int NB>
__device__ __forceinline__ void gemv_tail(int rem, f32x4 (&acc)[NTILE][NB], const T* const (&wrow)[NTILE], const T* const (&xrow)[NB], int k0,
                                          const bool (&xvalid)[NB]) {
  if constexpr (N > 0) {
    if (rem == N) gemv_group<T, NTILE, N, WAVES, NTL, NB>(acc, wrow, xrow, k0, xvalid);
    else gemv_tail<T, NTILE, N - 1, WAVES, NTL, NB>(rem, acc, wrow, xrow, k0, xvalid);
  }
}

// NB = batch tiles of 16 rows sharing every weight fragment (b <= 16 * NB): the weights are still read exactly once
template <typename T, int NTILE, int EPI, int GV_WAVES = 8, int GV_UNROLL = 4, bool NTL = false, int NB = 1>
__global__ __launch_bounds__(GV_WAVES * 64) void gemv_kernel(GemvP p) {
  typedef typename V8<T>::type frag_t;
  __shared__ float red[GV_WAVES][NTILE * NB][256];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * (NTILE * 16);

  const T* W = (const T*)p.W;
  const T* X = (const T*)p.X;
  const T* wrow[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    int r = n0 + t * 16 + fr; r = r < p.N ? r : p.N - 1;
    wrow[t] = W + (size_t)r * p.ldw + fg * 8;
  }
  bool xvalid[NB];
  const T* xrow[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    xvalid[nb] = nb * 16 + fr < p.b;
    xrow[nb] = X + (size_t)(xvalid[nb] ? nb * 16 + fr : 0) * p.ldx + fg * 8;
  }

  f32x4 acc[NTILE][NB];
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[t][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // K slice of this workgroup (blockIdx.y of ksplit): chunks [c_lo, c_hi)
  const int nchunk_all = p.K / 64;
  const int c_lo = (int)(((long)nchunk_all * blockIdx.y) / p.ksplit);
  const int nchunk = (int)(((long)nchunk_all * (blockIdx.y + 1)) / p.ksplit);
  // Wave w owns chunks c_lo + w, c_lo + w + WAVES, ...: full groups of GV_UNROLL chunks in flight, then ONE group of
  // exactly the remaining count (compile-time unrolled per count, so the tail is as deep as the body).
  const int first = c_lo + wave;
  const int n_w = first < nchunk ? (nchunk - first + GV_WAVES - 1) / GV_WAVES : 0;
  int g = 0;
  for (; g + GV_UNROLL <= n_w; g += GV_UNROLL)
    gemv_group<T, NTILE, GV_UNROLL, GV_WAVES, NTL, NB>(acc, wrow, xrow, (first + g * GV_WAVES) * 64, xvalid);
  gemv_tail<T, NTILE, GV_UNROLL - 1, GV_WAVES, NTL, NB>(n_w - g, acc, wrow, xrow, (first + g * GV_WAVES) * 64, xvalid);

  // acc[t][nb][r] = Y^T[n = n0 + t*16 + 4*fg + r][batch = 16*nb + fr]
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][t * NB + nb][(fg * 4 + r) * 16 + fr] = acc[t][nb][r];
  __syncthreads();
  if (wave != 0) return;

  // wave 0: lane -> 4 (n, batch) pairs per tile; element e = lane + 64*i : n_local = e >> 4, batch = e & 15
  const T* bias = (const T*)p.bias;
  const T* R = (const T*)p.resid;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float v[NTILE][4];
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < GV_WAVES; ++w) s += red[w][t * NB + nb][lane + 64 * i];
        v[t][i] = s;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i, nl = e >> 4, bi = nb * 16 + (e & 15);
      if (bi >= p.b) continue;
      if constexpr (EPI == EPI_PARTIAL) {
        // raw fp32 K-slice sums, layout [ksplit][b][ldy]; the consumer (resid_rmsnorm) adds the slices in a fixed order
#pragma unroll
        for (int t = 0; t < NTILE; ++t) {
          const int n = n0 + t * 16 + nl;
          if (n < p.N) ((float*)p.Y)[((size_t)blockIdx.y * p.b + bi) * p.ldy + n] = v[t][i];
        }
      } else if constexpr (EPI == EPI_SWIGLU) {
        // tile 0 = 16 gate rows, tile 1 = the matching 16 up rows
        const int n = (n0 >> 1) + nl;
        if (n0 + 16 + nl < p.N) {
          const float g = rnd<T>(v[0][i]), u = rnd<T>(v[1][i]);
          ((T*)p.Y)[(size_t)bi * p.ldy + n] = fromf<T>(rnd<T>(silu(g)) * u);
        }
      } else {
#pragma unroll
        for (int t = 0; t < NTILE; ++t) {
          const int n = n0 + t * 16 + nl;
          if (n >= p.N) continue;
          float y = v[t][i] + (bias ? tof(bias[n]) : 0.f);
          if (p.out_f32) {
            ((float*)p.Y)[(size_t)bi * p.ldy + n] = y;
          } else {
            y = rnd<T>(y);
            if constexpr (EPI == EPI_RESID) y = tof(R[(size_t)bi * p.ldr + n]) + y;
            ((T*)p.Y)[(size_t)bi * p.ldy + n] = fromf<T>(y);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// MXFP4 weights in the packed batched forms below (WF_MX4; common.h: packed_w4_index / packed_s4_index).  One (tile, chunk, half) unit = 16
// weight rows x 32 consecutive k = one MX block per row = one A operand of mfma16: a lane's dword holds its 8 codes, four
// v_cvt_scalef32_pk_{f16,bf16}_fp4 at scale 1 widen them (exact), the MFMA runs from a ZERO C operand, and its four results per lane
// (weight rows 4 fg + r) are folded into the running fp32 accumulators by 2^e of those rows -- one fmaf each.  The scale stays out of the
// convert for the reason given at rw_dot8_fp4: folded in, a 2^e near 2^-22 underflows f16.
// ---------------------------------------------------------------------------------------------------------
typedef unsigned int rw_u32x2 __attribute__((ext_vector_type(2)));
// e8m0 byte -> 2^(byte - 127) (byte 0 = 2^-127 is an fp32 subnormal: ldexp, not a shift into the exponent field)
__device__ __forceinline__ float mx_scale_of(unsigned byte) { return ldexpf(1.0f, (int)byte - 127); }
template <typename T> __device__ __forceinline__ typename V8<T>::type mx4_frag(unsigned w);
template <> __device__ __forceinline__ f16x8 mx4_frag<f16>(unsigned w) {
  const rw_u32x4 v = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3))};
  return __builtin_bit_cast(f16x8, v);
}
template <> __device__ __forceinline__ bf16x8 mx4_frag<bf16>(unsigned w) {
  const rw_u32x4 v = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 0)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 1)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 2)),
                      __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 3))};
  return __builtin_bit_cast(bf16x8, v);
}
// the four e8m0 bytes of weight rows 4 fg .. 4 fg + 3 (one aligned dword) -> 2^e
__device__ __forceinline__ void mx4_scales(unsigned s4, float (&sc)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[r] = mx_scale_of((s4 >> (8 * r)) & 0xffu);
}
// acc += 2^e (rows) * (A x): one unit against one batch tile
template <typename F>
__device__ __forceinline__ f32x4 mx4_fold(F a, F x, const float (&sc)[4], f32x4 acc) {
  const f32x4 t = mfma16(a, x, (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = fmaf(t[r], sc[r], acc[r]);
  return acc;
}
// a wave's registers for one MXFP4 weight tile over its NCH chunks (x-stationary forms): the codes per half, the 2 x 4 scale bytes of a chunk
template <int NCH> struct XsMx4 { unsigned c[NCH][2]; rw_u32x2 s[NCH]; };


// ---------------------------------------------------------------------------------------------------------
// Batched decode (2 <= b <= 32) with PACKED operands (common.h: packed_x_index / packed_w_index).  The kernel above loads
// fragment-shaped operands (16 rows x 64 B per wave instruction) for W AND for x; at b = 32 the x loads (L2 hits, as many bytes
// as the weights) make it address-path bound: 3.2 TB/s on gate|up.  Here x arrives packed from its producer (RMSNorm, attention
// merge, SwiGLU epilogue) and W optionally from the packed replica, so every wave load is 1 KiB contiguous; NTILE row tiles share
// each x fragment.  Measured (tools/experiments/tune_gemv32.hip, MI355X, b = 32): gate|up 84 -> 66 us with packed x, -> 53 us with packed W
// too (5.1 TB/s); down_proj 50 -> 28 us; qkv 17.7 -> 12.2; o_proj 13.8 -> 9.0; lm_head 318 -> 207.
// Wave w of a workgroup walks K chunks (64 wide) c_lo + UNROLL * (w + WAVES * i) + u; partial tiles are summed through LDS in a
// fixed order by all waves, which also apply the epilogue.
// ---------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------
// x-stationary form of the packed batched GEMV for the long launches (gate|up, lm_head; K = 64 * 8 * NCH, no split-K).  In gemv_pk_kernel
// every workgroup re-reads the whole packed x (229 KB at K = 3584, NB = 2): as many bytes through the CU's load path as its share of
// the weights (tools/experiments/tune_gemv32.hip: with x served from L1 gate|up takes 47.6 instead of 53.3 us).  Here one persistent workgroup per
// CU keeps x in REGISTERS -- wave w owns K chunks w, w + 8, ... for the whole launch -- and walks 16-row weight tiles with stride
// gridDim.x; the eight partial tiles meet in LDS (parity double buffer: one barrier per tile) and the NEXT tile's weight fragments are
// loaded before the current tile is reduced, so the weight stream never stops.  Measured in the harness: gate|up 53.3 -> 48.6 us,
// lm_head 219 -> 191 us at b = 32.  SwiGLU: the workgroup takes tiles in (gate, up) pairs; the thread that reduces element (row, batch)
// of the gate tile reduces the same element of the up tile and keeps the gate value in a register.
// Same summation order per output as gemv_pk_kernel with WAVES = 8 would give only if its chunk -> wave deal were identical; it is not
// (there: groups of UNROLL consecutive chunks per wave), so results agree to fp32 rounding of the K sum, not bit for bit.
// ---------------------------------------------------------------------------------------------------------
// c_base: first K chunk of this workgroup's slice (the slice is exactly 8 * NCH chunks), slice: its index for the split-K output
// NORM (round 5, the batched twin of the batch-1 norm-in-GEMV forms): X holds the RAW residual rows in the packed layout and the RMSNorm that
// precedes the projection (transformers modeling_qwen2.py:247-252) runs here, on the registers that keep x for the whole launch: per-row sum
// of squares over the wave's chunks, over the four lanes of a row and over the eight waves (LDS), then T(T(x * rstd) * w) with the reference's
// two roundings.  Every workgroup repeats it (x is read by every workgroup anyway); the residual + RMSNorm launch in front of gate|up goes away.
template <typename T, int EPI, int NB, int NCH, bool NORM = false, int WF = WF_16>
__device__ __forceinline__ void gemv_xs_body(const GemvP& p, float (&red)[2][8][NB][256], int c_base, int slice) {
  typedef typename V8<T>::type frag_t;
  static_assert(WF == WF_16 || (WF == WF_MX4 && !NORM && EPI != EPI_RESID), "MXFP4: the plain, SwiGLU and split-K epilogues");
  typedef typename std::conditional<WF == WF_MX4, XsMx4<NCH>, frag_t[NCH][2]>::type wtile_t;
  constexpr int WAVES = 8;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nchunk_all = p.K >> 6, n_tiles = p.N >> 4;
  // The slice is dealt to the waves chunk by chunk: wave w owns chunks c_base + w, c_base + w + 8, ...  No guards inside the load groups on
  // purpose: a ragged variant with per-chunk validity tests kept the compiler from issuing a tile's 2 * NCH weight loads back to back and
  // measured 8 % SLOWER than gemv_pk_kernel.
  const T* W = (const T*)p.W;
  frag_t xf[NCH][NB][2];
  auto load_x = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = c_base + wave + WAVES * i;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          frag_t z;
#pragma unroll
          for (int j = 0; j < 8; ++j) z[j] = fromf<T>(0.f);
          xf[i][nb][h] = nb * 16 + fr < p.b ? ld8<T>((const T*)p.X + ((size_t)(c * 2 + h) * NB + nb) * 512 + lane * 8) : z;
        }
    }
  };
  // (x in FRONT of the first weight tile: the other order -- HBM requests first, x from L2 behind them -- measured slower, configs[2] decode
  // 4.33-4.35 vs 4.27-4.30 ms per step on one box, round 5)
  load_x();
  if constexpr (NORM) {
    float ss[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float v = tof(xf[i][nb][h][j]); a = fmaf(v, v, a); }
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      ss[nb] = a;
      if (fg == 0) red[1][wave][nb][fr] = a;          // parity 1: finish(0) writes parity 0 and every wave has passed its barrier before parity 1 is reused
    }
    __syncthreads();
    const T* nw = (const T*)p.norm_w;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) tot += red[1][w][nb][fr];      // fixed order
      const float rstd = rsqrtf(tot / (float)p.K + p.norm_eps);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = c_base + wave + WAVES * i;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          __builtin_amdgcn_sched_barrier(0);      // one norm-weight fragment live at a time: hoisting all 2 NCH of them spilled 120 VGPRs
          const frag_t wv = ld8<T>(nw + (size_t)c * 64 + h * 32 + fg * 8);
          frag_t o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = fromf<T>(rnd<T>(tof(xf[i][nb][h][j]) * rstd) * tof(wv[j]));
          xf[i][nb][h] = o;
        }
      }
    }
  }
  auto load_w = [&](wtile_t& wf, int tile) {
    if constexpr (WF == WF_MX4) {
      // (tile, chunk): 2 x 64 code dwords, 4 x 8 scale bytes (lane group fg: half 0 rows 4 fg .. 4 fg + 3, then half 1)
      const unsigned* cb = (const unsigned*)p.W + ((size_t)tile * nchunk_all + c_base) * 128 + lane;
      const rw_u32x2* sb = (const rw_u32x2*)p.mx_s + ((size_t)tile * nchunk_all + c_base) * 4 + fg;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int h = 0; h < 2; ++h) wf.c[i][h] = __builtin_nontemporal_load(cb + (size_t)(wave + WAVES * i) * 128 + h * 64);
        wf.s[i] = __builtin_nontemporal_load(sb + (size_t)(wave + WAVES * i) * 4);
      }
    } else {
      const T* base = W + ((size_t)tile * nchunk_all + c_base) * 1024 + lane * 8;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) wf[i][h] = __builtin_nontemporal_load(reinterpret_cast<const frag_t*>(base + (size_t)(wave + WAVES * i) * 1024 + h * 512));
    }
  };
  // j-th tile of this workgroup: SwiGLU walks (gate, up) pairs, the others single tiles
  const int n_units = EPI == EPI_SWIGLU ? n_tiles >> 1 : n_tiles;
  const int my_units = (int)blockIdx.x < n_units ? (n_units - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  const int my_tiles = EPI == EPI_SWIGLU ? 2 * my_units : my_units;
  auto tile_of = [&](int j) { return EPI == EPI_SWIGLU ? 2 * ((int)blockIdx.x + (j >> 1) * (int)gridDim.x) + (j & 1) : (int)blockIdx.x + j * (int)gridDim.x; };
  const T* bias = (const T*)p.bias;
  float gate = 0.f;
  // plain epilogue with a bias (qkv): the bias element of the output this thread will reduce is requested when the tile's weights are -- loaded
  // after the reduction it was a dependent L2 round trip per tile (round 4).  No branch around the load: without a bias it reads x[0].
  const bool has_bias = EPI != EPI_SWIGLU && EPI != EPI_PARTIAL && bias != nullptr;
  const T* bsrc = has_bias ? bias : (const T*)p.X;
  auto bias_of = [&](int j) { const int e = threadIdx.x & 255, n = tile_of(j) * 16 + (e >> 4); return tof(bsrc[has_bias ? (n < p.N ? n : p.N - 1) : 0]); };
  // EPI_RESID (un-split o_proj of a batched step, round 5): the residual element this thread will add is requested with the tile's weights, like
  // the bias; it rides in the same two registers (a launch has a bias or a residual, never both)
  const bool has_res = EPI == EPI_RESID;
  const T* rsrc = has_res ? (const T*)p.resid : (const T*)p.X;
  auto res_of = [&](int j) {
    const int i = threadIdx.x & (NB * 256 - 1), nb = i >> 8, e = i & 255, n = tile_of(j) * 16 + (e >> 4), bi = nb * 16 + (e & 15);
    return tof(rsrc[has_res ? (size_t)(bi < p.b ? bi : 0) * p.ldr + (n < p.N ? n : p.N - 1) : 0]);
  };
  float bias_a = 0.f, bias_b = 0.f;
  auto finish = [&](wtile_t& wf, int j, float bias_v) {
    const int tile = tile_of(j), par = j & 1;
    f32x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (WF == WF_MX4) {
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float sc[4];
          mx4_scales(h ? wf.s[i].y : wf.s[i].x, sc);
          const frag_t a = mx4_frag<T>(wf.c[i][h]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[nb] = mx4_fold(a, xf[i][nb][h], sc, acc[nb]);
        }
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          acc[nb] = mfma16(wf[i][0], xf[i][nb][0], acc[nb]);
          acc[nb] = mfma16(wf[i][1], xf[i][nb][1], acc[nb]);
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[par][wave][nb][(fg * 4 + r) * 16 + fr] = acc[nb][r];
    __syncthreads();
    const int i = threadIdx.x;
    if (i < NB * 256) {
      const int nb = i >> 8, e = i & 255, nl = e >> 4, bi = nb * 16 + (e & 15);
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) v += red[par][w][nb][e];      // fixed order: deterministic
      if constexpr (EPI == EPI_SWIGLU) {
        if ((j & 1) == 0) gate = rnd<T>(v);
        else if (bi < p.b) {
          const int n = (tile >> 1) * 16 + nl;
          const T y = fromf<T>(rnd<T>(silu(gate)) * rnd<T>(v));
          if (p.y_packed) ((T*)p.Y)[packed_x_index(bi, n, NB)] = y;
          else ((T*)p.Y)[(size_t)bi * p.ldy + n] = y;
        }
      } else if constexpr (EPI == EPI_PARTIAL) {
        if (bi < p.b) ((float*)p.Y)[((size_t)slice * p.b + bi) * p.ldy + tile * 16 + nl] = v;      // [ksplit][b][ldy]
      } else if constexpr (EPI == EPI_RESID) {
        if (bi < p.b) {                                   // T(resid + T(acc)) as gemm_epilogue's EPI_RESID; row-major (may alias resid) and packed
          const int n = tile * 16 + nl;
          const T y = fromf<T>(bias_v + rnd<T>(v));
          ((T*)p.Y)[(size_t)bi * p.ldy + n] = y;
          if (p.y_pack) ((T*)p.y_pack)[packed_x_index(bi, n, NB)] = y;
        }
      } else if (bi < p.b) {
        const int n = tile * 16 + nl;
        const float y = v + (has_bias ? bias_v : 0.f);
        if (p.out_f32) ((float*)p.Y)[(size_t)bi * p.ldy + n] = y;
        else ((T*)p.Y)[(size_t)bi * p.ldy + n] = fromf<T>(y);
      }
    }
  };
  wtile_t wa, wb;
  auto pre_of = [&](int j) { if constexpr (EPI == EPI_RESID) return res_of(j); else return bias_of(j); };
  if (my_tiles > 0) { load_w(wa, tile_of(0)); bias_a = pre_of(0); }
  for (int j = 0; j < my_tiles; j += 2) {
    if (j + 1 < my_tiles) { load_w(wb, tile_of(j + 1)); bias_b = pre_of(j + 1); }
    finish(wa, j, bias_a);
    if (j + 1 < my_tiles) {
      if (j + 2 < my_tiles) { load_w(wa, tile_of(j + 2)); bias_a = pre_of(j + 2); }
      finish(wb, j + 1, bias_b);
    }
  }
}

template <typename T, int EPI, int NB, int NCH, bool NORM = false>
__global__ __launch_bounds__(512) void gemv_xs_kernel(GemvP p) {
  __shared__ float red[2][8][NB][256];
  gemv_xs_body<T, EPI, NB, NCH, NORM>(p, red, 0, 0);
}

// split-K form (down_proj): the K = 64 * 8 * q chunks are cut into slices that deal evenly to the 8 waves -- n5 slices of 40 chunks
// (5 per wave) then slices of 16 chunks (2 per wave), blockIdx.y = slice -- each written as one fp32 slice [ksplit][b][ldy] for the
// fused residual + RMSNorm kernel.  (q = 37 for K = 18944: 7 x 40 + 1 x 16 = 8 slices.)
template <typename T, int NB>
__global__ __launch_bounds__(512) void gemv_xs_split_kernel(GemvP p, int n5) {
  __shared__ float red[2][8][NB][256];
  const int y = blockIdx.y;
  if (y < n5) gemv_xs_body<T, EPI_PARTIAL, NB, 5>(p, red, y * 40, y);
  else gemv_xs_body<T, EPI_PARTIAL, NB, 2>(p, red, n5 * 40 + (y - n5) * 16, y);
}

// the same two forms on the packed MXFP4 replica (same launch shapes, same chunk -> wave deal, same reduction order)
template <typename T, int EPI, int NB, int NCH>
__global__ __launch_bounds__(512) void gemv_xs_mx4_kernel(GemvP p) {
  __shared__ float red[2][8][NB][256];
  gemv_xs_body<T, EPI, NB, NCH, false, WF_MX4>(p, red, 0, 0);
}
template <typename T, int NB>
__global__ __launch_bounds__(512) void gemv_xs_split_mx4_kernel(GemvP p, int n5) {
  __shared__ float red[2][8][NB][256];
  const int y = blockIdx.y;
  if (y < n5) gemv_xs_body<T, EPI_PARTIAL, NB, 5, false, WF_MX4>(p, red, y * 40, y);
  else gemv_xs_body<T, EPI_PARTIAL, NB, 2, false, WF_MX4>(p, red, n5 * 40 + (y - n5) * 16, y);
}

template <typename T, int NTILE, int EPI, int WAVES, int UNROLL, int NB, bool WPACK, int WF>
__device__ __forceinline__ void gemv_pk_body(const GemvP p, float (&red)[WAVES][NTILE * NB][256]) {
  typedef typename V8<T>::type frag_t;
  static_assert(WF == WF_16 || (WF == WF_MX4 && WPACK), "MXFP4: the packed replica only");
  typedef typename std::conditional<WF == WF_MX4, unsigned, frag_t>::type wreg_t;      // a lane's 8 weights of one (chunk, half)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int tile0 = blockIdx.x * NTILE;
  const int n_tiles = (p.N + 15) >> 4;
  const int nchunk_all = p.K >> 6;
  const int c_lo = (int)(((long)nchunk_all * blockIdx.y) / p.ksplit), c_hi = (int)(((long)nchunk_all * (blockIdx.y + 1)) / p.ksplit);

  const T* W = (const T*)p.W;
  const T* wbase[NTILE];
  const unsigned* cbase[NTILE];          // MXFP4: (tile, chunk) = 2 x 64 code dwords, 4 x 8 scale bytes (lane group fg: half 0's four rows, then half 1's)
  const rw_u32x2* sbase[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    const int tl = tile0 + t < n_tiles ? tile0 + t : n_tiles - 1;
    if constexpr (WF == WF_MX4) {
      cbase[t] = (const unsigned*)p.W + (size_t)tl * nchunk_all * 128 + lane;
      sbase[t] = (const rw_u32x2*)p.mx_s + (size_t)tl * nchunk_all * 4 + fg;
    } else if constexpr (WPACK) wbase[t] = W + (size_t)tl * nchunk_all * 1024 + lane * 8;
    else { int r = tl * 16 + fr; r = r < p.N ? r : p.N - 1; wbase[t] = W + (size_t)r * p.ldw + fg * 8; }
  }
  const T* xbase = (const T*)p.X + lane * 8;
  // lanes whose batch row (16 nb + fr) does not exist load nothing: the x re-read of every workgroup (half of the CU-side traffic at
  // b = 32, tools/experiments/tune_gemv32.hip) then scales with b instead of with the 16-row padding of the packed layout
  bool xrow[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) xrow[nb] = nb * 16 + fr < p.b;

  f32x4 acc[NTILE][NB];
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[t][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int c0 = c_lo + wave * UNROLL; c0 < c_hi; c0 += WAVES * UNROLL) {
    wreg_t wf[UNROLL][NTILE][2];
    frag_t xf[UNROLL][NB][2];
    rw_u32x2 ws[UNROLL][NTILE];                                 // MXFP4: the 2 x 4 scale bytes of (tile, chunk) for this lane group
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int c = c0 + u < c_hi ? c0 + u : c_hi - 1;          // ragged last group: re-load the last chunk, skip its MFMAs below
#pragma unroll
      for (int t = 0; t < NTILE; ++t) {
        if constexpr (WF == WF_MX4) {
#pragma unroll
          for (int h = 0; h < 2; ++h) wf[u][t][h] = __builtin_nontemporal_load(cbase[t] + (size_t)c * 128 + h * 64);
          ws[u][t] = __builtin_nontemporal_load(sbase[t] + (size_t)c * 4);
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const T* q = WPACK ? wbase[t] + (size_t)c * 1024 + h * 512 : wbase[t] + c * 64 + h * 32;
            wf[u][t][h] = __builtin_nontemporal_load(reinterpret_cast<const frag_t*>(q));
          }
        }
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          frag_t z;
#pragma unroll
          for (int j = 0; j < 8; ++j) z[j] = fromf<T>(0.f);
          xf[u][nb][h] = xrow[nb] ? ld8<T>(xbase + ((size_t)(c * 2 + h) * NB + nb) * 512) : z;
        }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (c0 + u < c_hi) {                                      // wave-uniform
        if constexpr (WF == WF_MX4) {
#pragma unroll
          for (int t = 0; t < NTILE; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              float sc[4];
              mx4_scales(h ? ws[u][t].y : ws[u][t].x, sc);
              const frag_t a = mx4_frag<T>(wf[u][t][h]);
#pragma unroll
              for (int nb = 0; nb < NB; ++nb) acc[t][nb] = mx4_fold(a, xf[u][nb][h], sc, acc[t][nb]);
            }
        } else {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int t = 0; t < NTILE; ++t) {
              acc[t][nb] = mfma16(wf[u][t][0], xf[u][nb][0], acc[t][nb]);
              acc[t][nb] = mfma16(wf[u][t][1], xf[u][nb][1], acc[t][nb]);
            }
        }
      }
    }
  }
  // acc[t][nb][r] = Y^T[n = (tile0 + t)*16 + 4*fg + r][batch = 16*nb + fr]
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][t * NB + nb][(fg * 4 + r) * 16 + fr] = acc[t][nb][r];
  __syncthreads();

  const T* bias = (const T*)p.bias;
  for (int i = threadIdx.x; i < NB * 256; i += WAVES * 64) {
    const int nb = i >> 8, e = i & 255, nl = e >> 4, bi = nb * 16 + (e & 15);
    float v[NTILE];
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += red[w][t * NB + nb][e];      // fixed order: deterministic
      v[t] = s;
    }
    if (bi >= p.b) continue;
    if constexpr (EPI == EPI_PARTIAL) {
#pragma unroll
      for (int t = 0; t < NTILE; ++t) {
        const int n = (tile0 + t) * 16 + nl;
        if (n < p.N) ((float*)p.Y)[((size_t)blockIdx.y * p.b + bi) * p.ldy + n] = v[t];
      }
    } else if constexpr (EPI == EPI_SWIGLU) {
      // tiles (2q, 2q + 1) = 16 gate rows and the matching 16 up rows of the fused, interleaved weight
#pragma unroll
      for (int t = 0; t < NTILE; t += 2) {
        const int row = (tile0 + t) * 16 + nl;                  // gate row in the fused layout
        if (row + 16 < p.N) {
          const int n = ((tile0 + t) >> 1) * 16 + nl;
          const float g = rnd<T>(v[t]), u = rnd<T>(v[t + 1]);
          const T y = fromf<T>(rnd<T>(silu(g)) * u);
          if (p.y_packed) ((T*)p.Y)[packed_x_index(bi, n, NB)] = y;
          else ((T*)p.Y)[(size_t)bi * p.ldy + n] = y;
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < NTILE; ++t) {
        const int n = (tile0 + t) * 16 + nl;
        if (n >= p.N) continue;
        const float y = v[t] + (bias ? tof(bias[n]) : 0.f);
        if (p.out_f32) ((float*)p.Y)[(size_t)bi * p.ldy + n] = y;
        else ((T*)p.Y)[(size_t)bi * p.ldy + n] = fromf<T>(y);
      }
    }
  }
}

template <typename T, int NTILE, int EPI, int WAVES, int UNROLL, int NB, bool WPACK>
__global__ __launch_bounds__(WAVES * 64) void gemv_pk_kernel(GemvP p) {
  __shared__ float red[WAVES][NTILE * NB][256];
  gemv_pk_body<T, NTILE, EPI, WAVES, UNROLL, NB, WPACK, WF_16>(p, red);
}
template <typename T, int NTILE, int EPI, int WAVES, int UNROLL, int NB>
__global__ __launch_bounds__(WAVES * 64) void gemv_pk_mx4_kernel(GemvP p) {
  __shared__ float red[WAVES][NTILE * NB][256];
  gemv_pk_body<T, NTILE, EPI, WAVES, UNROLL, NB, true, WF_MX4>(p, red);
}

// row-major -> packed (model load time / tests)
template <typename T>
__global__ void pack_x_kernel(const T* X, int ldx, int b, int K, T* out, int NB) {
  const int n8 = NB * 16 * (K >> 3);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += gridDim.x * blockDim.x) {
    const int row = i / (K >> 3), k = (i % (K >> 3)) * 8;
    typename V8<T>::type v;
    if (row < b) v = ld8<T>(X + (size_t)row * ldx + k);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    }
    st8<T>(out + packed_x_index(row, k, NB), v);
  }
}
template <typename T>
__global__ void pack_w_kernel(const T* W, int ldw, int N, int K, T* out) {
  const long n8 = (long)N * (K >> 3);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    // destination-linear: consecutive threads write consecutive 16-byte pieces of the packed image
    const long piece = i;
    const int lane = (int)(piece & 63), half = (int)((piece >> 6) & 1);
    const long tc = piece >> 7;
    const int chunk = (int)(tc % (K >> 6)), tile = (int)(tc / (K >> 6));
    const int row = tile * 16 + (lane & 15), k = chunk * 64 + half * 32 + (lane >> 4) * 8;
    st8<T>(out + piece * 8, ld8<T>(W + (size_t)row * ldw + k));
  }
}
// row-major MXFP4 replica (W4 [N][K / 2] bytes, S [N][K / 32] e8m0 bytes) -> the packed one (common.h: packed_w4_index / packed_s4_index): a
// byte shuffle, the quantiser stays the single source of the codes.  Thread i writes code dword i of the packed image and moves scale byte i.
__global__ void pack_w4_kernel(const unsigned char* W4, const unsigned char* S, int N, int K, unsigned* W4P, unsigned char* SP) {
  const long n8 = (long)N * (K >> 3), ns = (long)N * (K >> 5);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63), half = (int)((i >> 6) & 1);
    const long tc = i >> 7;
    const int chunk = (int)(tc % (K >> 6)), tile = (int)(tc / (K >> 6));
    const int row = tile * 16 + (lane & 15), k = chunk * 64 + half * 32 + (lane >> 4) * 8;
    W4P[i] = *reinterpret_cast<const unsigned*>(W4 + (size_t)row * (K >> 1) + (k >> 1));
    if (i < ns) {
      const int srow = (int)(i / (K >> 5)), blk = (int)(i % (K >> 5));
      SP[packed_s4_index(srow, blk, K)] = S[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// b = 1: whole-row streaming + packed dot products.  Measured on MI355X (tools/experiments/tune_rowdot.hip): 6.5-6.8 TB/s on the
// gate|up shape against 5.5 TB/s for the MFMA form above, whose 16-row x 64-B fragment reads reach ~6.0 TB/s at best; here
// every wave instruction reads 1 KiB of ONE row (non-temporal).  x (this workgroup's K slice) sits in registers; a wave
// takes R rows at a time (all R x NCH loads in flight), v_dot2 per 32 bits, butterfly over the wave, lane 0 applies the
// epilogue.  Split-K slices are chunk ranges of 512 elements, <= RW_MAXC chunks each.
// ---------------------------------------------------------------------------------------------------------
// The tuning state (GemvTuning, kernels.h), by omchat_op_set_tuning key:
// force_mfma (key 1): A/B the two forms
// no_xs (key 11): 1 = batched decode never takes the x-stationary persistent kernel (A/B)
// shard (key 34): launch shapes for the SHARD widths of a tensor-parallel rank (round 5; N or K an eighth of the model's):
// bit 0 = x-stationary form for short EPI_NONE outputs (qkv shard: one tile per workgroup), bit 1 = one-tile / one-chunk-per-wave form for
// short-K split-K slices (o_proj / down_proj shards), bit 2 = one (gate, up) pair per wave for the short batch-1 gate|up,
// bit 3 = x-stationary form, one (gate, up) tile pair per workgroup, for a batched gate|up shard of at most one pair per CU
// longk_direct (key 39, experiments build): waves per workgroup (1, 2, 4) of the no-LDS long-K form; 0 = x through LDS (gemv_rows_longk_kernel)
// rows_balance (key 17): 1 = one-row-per-wave launches whose rows deal evenly to 2 workgroups per CU take N / (2 CUs) waves per workgroup (o_proj 7, qkv 9)
// skew (key 28, experiment): per-(blockIdx % 8) share deltas of the loop form, eight nibbles (d + 8)
// dyn (key 24): 1 = the loop form takes its outputs from atomic work counters when the caller provides them (gemv_rows_norm_dyn_kernel)
// gu_rr (key 38): (gate, up) pairs per wave of the NON-loop norm form of the batch-1 gate|up GEMV.  Round 5: ONE pair per wave (4736
// workgroups of four waves for Qwen2-7B) beats the loop form's one resident round of 512 workgroups x 37 pairs: decode 2.650 -> 2.597 ms per token on
// one box (3 pairs per wave: 2.671, 2: 2.624).  The XCDs do not deliver the same HBM bandwidth when all stream at once, so a
// static equal split ends on the slowest XCD; thousands of 14 KB-per-wave workgroups are re-balanced by the dispatcher as they retire, the way the
// lm_head launch (9504 workgroups) always was -- it streams at 7.0 TB/s where the loop form reached 6.35.
// gu_rr8: the same for the e4m3 replica (key 38, value x 16): 1.700 -> 1.678 -> 1.658 ms per token at 4 / 2 / 1 pairs per wave
// norm_loop (key 16): loop form (gemv_rows_norm_loop_kernel) of a batch-1 step's bit 0 = gate|up, 1 = qkv, 2 = e4m3 gate|up, 3 = lm_head
GemvTuning g_tune;
constexpr int RW_MAXC = 8;
// weight-only fp8 (OCP e4m3): 8 weights of a lane = 8 bytes.  gfx950's v_cvt_scalef32_pk_{bf16,f16}_fp8 widens two e4m3
// values to a packed 16-bit pair in one instruction (exact: 3 mantissa bits), which then feeds the same v_dot2 as the
// 16-bit kernel with x still packed in registers: 4 converts + 4 dot2 per 8 weights.
template <typename T> __device__ __forceinline__ float rw_dot8_fp8(rw_u32x2 w, rw_u32x4 x, float acc);
template <> __device__ __forceinline__ float rw_dot8_fp8<bf16>(rw_u32x2 w, rw_u32x4 x, float acc) {
  typedef bf16 v2 __attribute__((ext_vector_type(2)));
  const unsigned w0 = w.x, w1 = w.y, x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false), __builtin_bit_cast(v2, x0), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true), __builtin_bit_cast(v2, x1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false), __builtin_bit_cast(v2, x2), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true), __builtin_bit_cast(v2, x3), acc, false);
  return acc;
}
template <> __device__ __forceinline__ float rw_dot8_fp8<f16>(rw_u32x2 w, rw_u32x4 x, float acc) {
  typedef f16 v2 __attribute__((ext_vector_type(2)));
  const unsigned w0 = w.x, w1 = w.y, x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), __builtin_bit_cast(v2, x0), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true), __builtin_bit_cast(v2, x1), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), __builtin_bit_cast(v2, x2), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true), __builtin_bit_cast(v2, x3), acc, false);
  return acc;
}

// weight-only MXFP4: 8 weights of a lane = 4 bytes, all inside one block of 32 (k = 512 c + 8 lane), so one e8m0 byte goes with them.
// gfx950's v_cvt_scalef32_pk_{f16,bf16}_fp4 widens the two codes of a byte (low nibble first = the even k) to a packed 16-bit pair; the
// convert runs at scale 1 (exact: every e2m1 value is representable) and the block scale 2^e multiplies the lane's fp32 partial sum --
// folded into the convert a small 2^e underflows f16 and the result leaves the de-quantised reference.  4 converts + 4 dot2 per 8 weights,
// as for e4m3, + one multiply-add per chunk.
template <typename T> __device__ __forceinline__ float rw_dot8_fp4(unsigned w, rw_u32x4 x);
template <> __device__ __forceinline__ float rw_dot8_fp4<bf16>(unsigned w, rw_u32x4 x) {
  typedef bf16 v2 __attribute__((ext_vector_type(2)));
  const unsigned x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
  float acc = 0.f;
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 0), __builtin_bit_cast(v2, x0), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 1), __builtin_bit_cast(v2, x1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 2), __builtin_bit_cast(v2, x2), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 3), __builtin_bit_cast(v2, x3), acc, false);
  return acc;
}
template <> __device__ __forceinline__ float rw_dot8_fp4<f16>(unsigned w, rw_u32x4 x) {
  typedef f16 v2 __attribute__((ext_vector_type(2)));
  const unsigned x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
  float acc = 0.f;
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0), __builtin_bit_cast(v2, x0), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1), __builtin_bit_cast(v2, x1), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2), __builtin_bit_cast(v2, x2), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3), __builtin_bit_cast(v2, x3), acc, false);
  return acc;
}
// (mx_scale_of, the e8m0 byte -> 2^(byte - 127), is defined with the packed batched forms above)

// registers of a lane's 8 weights per format, their (non-temporal) load at element k of weight row `row`, and their dot product with 8 x
template <int WF> struct RwW { typedef rw_u32x4 type; };
template <> struct RwW<WF_E4M3> { typedef rw_u32x2 type; };
template <> struct RwW<WF_MX4> { typedef rw_u32x2 type; };      // .x = the 8 codes, .y = the e8m0 byte of their block
// ---------------------------------------------------------------------------------------------------------
// bf16x12: bf16 rows coded losslessly in 12 bits per weight (tests/bf16x12_ref.py is the definition).  A record of 512
// weights is 512 low bytes (e[0] + mantissa, untouched) and 256 nibble bytes (sign << 3 | code; code 0: e[7:1] = 0, code c: e[7:1] = top - 7 + c,
// top = the row's largest e[7:1]); lane l of chunk c reads the 8 low bytes and the nibble word of weights k = 512 c + 8 l .. + 7 and rebuilds the
// four registers the 16-bit load delivers -- the dot products behind it are the 16-bit kernel's, in its order: the same bits.  The rare
// elements outside the code (<= 32 per row, k-sorted [N][32] list of k << 16 | bits) are written over the decoded registers by their lane.
// Decode of 8 weights: 3 and/shift for the codes, 2 v_perm against the row's 8-entry table (two registers), 3 for the signs, 4 v_perm to
// interleave high and low bytes.
// ---------------------------------------------------------------------------------------------------------
struct X12W { rw_u32x2 lo; unsigned nib; };
template <> struct RwW<WF_X12> { typedef X12W type; };
struct X12Row {
  unsigned top_raw, cnt_raw;      // as loaded (uniform over the wave)
  unsigned pv;                    // lane j < 32: patch entry j of the row
  unsigned tlo, thi;              // code -> high byte (without the sign), entries 0..3 and 4..7
  int cnt, pi;                    // wave-uniform: patches of the row, the next one to apply
};
// (row and chunk are the same in every lane of a wave: the record's address is scalar, a lane adds its two 32-bit offsets)
__device__ __forceinline__ X12W x12_ldw(const GemvP& p, size_t row, int chunk, int lane) {
  const unsigned char* rec = (const unsigned char*)p.W + row * (size_t)p.ldw + (size_t)chunk * 768;
  const unsigned lo_off = 8u * (unsigned)lane, nib_off = 512u + 4u * (unsigned)lane;
  X12W w;
  w.lo = __builtin_nontemporal_load(reinterpret_cast<const rw_u32x2*>(rec + lo_off));
  w.nib = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(rec + nib_off));
  return w;
}
// the row's top, patch count and patch entries: requested with the weight loads ...
__device__ __forceinline__ void x12_row_load(X12Row& s, const GemvP& p, size_t row, int lane) {
  s.top_raw = p.x12_top[row];
  s.cnt_raw = p.x12_cnt[row];
  s.pv = p.x12_patch[row * 32 + (lane & 31)];
}
// ... and turned into the table once they are in (scalar work: the values are the same in every lane)
__device__ __forceinline__ void x12_row_finish(X12Row& s) {
  const int t = __builtin_amdgcn_readfirstlane((int)s.top_raw) - 7;
  s.cnt = __builtin_amdgcn_readfirstlane((int)s.cnt_raw);
  s.pi = 0;
  s.tlo = ((unsigned)((t + 1) & 0x7f) << 8) | ((unsigned)((t + 2) & 0x7f) << 16) | ((unsigned)((t + 3) & 0x7f) << 24);
  s.thi = (unsigned)((t + 4) & 0x7f) | ((unsigned)((t + 5) & 0x7f) << 8) | ((unsigned)((t + 6) & 0x7f) << 16) | ((unsigned)((t + 7) & 0x7f) << 24);
}
__device__ __forceinline__ rw_u32x4 x12_decode(const X12W& w, const X12Row& s) {
  const unsigned n = w.nib;
  const unsigned c0 = n & 0x07070707u, c1 = (n >> 4) & 0x07070707u;
  unsigned h0 = __builtin_amdgcn_perm(s.thi, s.tlo, c0), h1 = __builtin_amdgcn_perm(s.thi, s.tlo, c1);
  h0 |= (n & 0x08080808u) << 4;
  h1 |= n & 0x80808080u;
  rw_u32x4 r;
  r.x = __builtin_amdgcn_perm(h0, w.lo.x, 0x05010400u);
  r.y = __builtin_amdgcn_perm(h0, w.lo.x, 0x07030602u);
  r.z = __builtin_amdgcn_perm(h1, w.lo.y, 0x05010400u);
  r.w = __builtin_amdgcn_perm(h1, w.lo.y, 0x07030602u);
  return r;
}
__device__ __forceinline__ void x12_apply(rw_u32x4& w, unsigned e, int lane) {
  const unsigned k = e >> 16, i = k & 7u, sh = (i & 1u) * 16u;
  const unsigned keep = ~(0xffffu << sh), ins = (e & 0xffffu) << sh;
  const bool mine = lane == (int)((k >> 3) & 63u);
  w.x = (mine && (i >> 1) == 0u) ? ((w.x & keep) | ins) : w.x;
  w.y = (mine && (i >> 1) == 1u) ? ((w.y & keep) | ins) : w.y;
  w.z = (mine && (i >> 1) == 2u) ? ((w.z & keep) | ins) : w.z;
  w.w = (mine && (i >> 1) == 3u) ? ((w.w & keep) | ins) : w.w;
}
// A group of G consecutive chunks of one row, chunk0 first, decoded into the 16-bit kernel's registers.  Straight-line but for one
// wave-uniform test: does the row's next patch lie in this group?  Rarely: then the patches of the group go over the decoded registers in k
// order and the cursor moves on (groups come in rising chunk order).  A chunk at or beyond nch reads weights 0..7 of the row in EVERY lane
// against zeros of x, as the 16-bit kernel's clamped address does (long-K form, last pass): every lane takes the patches at k < 8.
template <int G>
__device__ __forceinline__ void x12_group(rw_u32x4 (&wd)[G], const X12W* w, X12Row& s, int chunk0, int nch, int lane) {
#pragma unroll
  for (int i = 0; i < G; ++i) wd[i] = x12_decode(w[i], s);
  while (s.pi < s.cnt) {
    const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)s.pv, s.pi);
    const int ch = (int)(e >> 25) - chunk0;
    if (ch >= G) break;
#pragma unroll
    for (int i = 0; i < G; ++i) if (ch == i) x12_apply(wd[i], e, lane);
    ++s.pi;
  }
  if (chunk0 + G > nch) {
    for (int j = 0; j < s.cnt; ++j) {
      const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)s.pv, j);
      if ((e >> 19) != 0u) break;      // k >= 8
#pragma unroll
      for (int i = 0; i < G; ++i) if (chunk0 + i >= nch) x12_apply(wd[i], e, 0);
    }
  }
}

template <typename T, int WF>
__device__ __forceinline__ typename RwW<WF>::type rw_ldw(const GemvP& p, size_t row, int k) {
  if constexpr (WF == WF_X12) return x12_ldw(p, row, k >> 9, (k >> 3) & 63); else
  if constexpr (WF == WF_E4M3) {
    return __builtin_nontemporal_load(reinterpret_cast<const rw_u32x2*>((const unsigned char*)p.W + row * p.ldw + k));
  } else if constexpr (WF == WF_MX4) {
    rw_u32x2 w;
    w.x = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>((const unsigned char*)p.W + row * p.ldw + (k >> 1)));
    w.y = __builtin_nontemporal_load(p.mx_s + row * (size_t)(p.K >> 5) + (k >> 5));
    return w;
  } else {
    return __builtin_nontemporal_load(reinterpret_cast<const rw_u32x4*>((const T*)p.W + row * p.ldw + k));
  }
}
template <typename T, int WF>
__device__ __forceinline__ float rw_dotw(typename RwW<WF>::type w, rw_u32x4 x, float acc) {
  if constexpr (WF == WF_E4M3) return rw_dot8_fp8<T>(w, x, acc);
  else if constexpr (WF == WF_MX4) return fmaf(rw_dot8_fp4<T>(w.x, x), mx_scale_of(w.y), acc);
  else return rw_dot8<T>(w, x, acc);
}

// epilogue operands of a one-shot row GEMV, requested right BEHIND the weight rows (they return with them instead of costing a dependent L2
// round trip after the reduction; in front of the weights a cold 2-byte load would hold the whole in-order queue): two 16-bit vectors
// (bias, residual; a dummy valid pointer + index 0 when absent -- no branch around the loads)
template <typename T, int R> struct RwTail { const T* p0; const T* p1; int idx[R]; float v0[R], v1[R]; };
template <typename T, int R> __device__ __forceinline__ void rw_tail_load(RwTail<T, R>& t) {
#pragma unroll
  for (int r = 0; r < R; ++r) { t.v0[r] = tof(t.p0[t.idx[r]]); t.v1[r] = tof(t.p1[t.idx[r]]); }
}
// quantised rows (e4m3 / MXFP4) of the one-shot form
template <typename T, int R, int NCH, int WF>
__device__ __forceinline__ void rw_rows_q(const GemvP& p, const int (&rows)[R], int k0, int lane, const rw_u32x4 (&xr)[RW_MAXC], float (&acc)[R],
                                          RwTail<T, R>& tail) {
  typename RwW<WF>::type w[R][NCH];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      int k = k0 + c * 512 + lane * 8;
      k = k < p.K ? k : k0;
      w[r][c] = rw_ldw<T, WF>(p, (size_t)rows[r], k);
    }
  float sc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) sc[r] = WF == WF_E4M3 ? p.w_scale[rows[r]] : 1.f;
  rw_tail_load<T, R>(tail);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) a = rw_dotw<T, WF>(w[r][c], xr[c], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    acc[r] = WF == WF_E4M3 ? a * sc[r] : a;
  }
}

template <typename T, int R, int N, int WF>
__device__ __forceinline__ void rw_dispatch_q(int nch, const GemvP& p, const int (&rows)[R], int k0, int lane, const rw_u32x4 (&xr)[RW_MAXC],
                                              float (&acc)[R], RwTail<T, R>& tail) {
  if constexpr (N > 0) {
    if (nch == N) rw_rows_q<T, R, N, WF>(p, rows, k0, lane, xr, acc, tail);
    else rw_dispatch_q<T, R, N - 1, WF>(nch, p, rows, k0, lane, xr, acc, tail);
  }
}

// rows r0 .. r0+R-1 (already mapped to weight-row indices by the caller) over NCH chunks starting at element k0
template <typename T, int R, int NCH>
__device__ __forceinline__ void rw_rows(const T* W, int ldw, const int (&rows)[R], int k0, int K, int lane, const rw_u32x4 (&xr)[RW_MAXC],
                                        float (&acc)[R], RwTail<T, R>& tail) {
  rw_u32x4 w[R][NCH];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      int k = k0 + c * 512 + lane * 8;
      k = k < K ? k : k0;                       // ragged last chunk: clamp (x is zero there)
      w[r][c] = __builtin_nontemporal_load(reinterpret_cast<const rw_u32x4*>(W + (size_t)rows[r] * ldw + k));
    }
  rw_tail_load<T, R>(tail);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) a = rw_dot8<T>(w[r][c], xr[c], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    acc[r] = a;
  }
}

template <typename T, int R, int N>
__device__ __forceinline__ void rw_dispatch(int nch, const T* W, int ldw, const int (&rows)[R], int k0, int K, int lane,
                                            const rw_u32x4 (&xr)[RW_MAXC], float (&acc)[R], RwTail<T, R>& tail) {
  if constexpr (N > 0) {
    if (nch == N) rw_rows<T, R, N>(W, ldw, rows, k0, K, lane, xr, acc, tail);
    else rw_dispatch<T, R, N - 1>(nch, W, ldw, rows, k0, K, lane, xr, acc, tail);
  }
}

template <typename T, int EPI, int RR, int WAVES, int F8>
__device__ __forceinline__ void gemv_rows_body(const GemvP& p) {
  constexpr int R = EPI == EPI_SWIGLU ? 2 * RR : RR;      // SwiGLU: RR (gate, up) row pairs per group
  constexpr int OUT = RR;                                 // outputs per group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* W = (const T*)p.W;
  if constexpr (EPI == EPI_RESID && WAVES == 7) OM_DBG_MIN(1, blockIdx.x < 8);
  // K slice of this workgroup row (blockIdx.y): chunk range [c_lo, c_hi)
  const int nch_all = (p.K + 511) / 512;
  const int c_lo = (int)(((long)nch_all * blockIdx.y) / p.ksplit), c_hi = (int)(((long)nch_all * (blockIdx.y + 1)) / p.ksplit);
  const int nch = c_hi - c_lo, k0 = c_lo * 512;
  rw_u32x4 xr[RW_MAXC];
#pragma unroll
  for (int c = 0; c < RW_MAXC; ++c) {
    const int k = k0 + c * 512 + lane * 8;
    rw_u32x4 z = {0u, 0u, 0u, 0u};
    xr[c] = (c < nch && k < p.K) ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
  }
  const int n_out = EPI == EPI_SWIGLU ? p.N / 2 : p.N;
  const int ngroups = (n_out + OUT - 1) / OUT;
  for (int g = blockIdx.x * WAVES + wave; g < ngroups; g += gridDim.x * WAVES) {
    int rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (EPI == EPI_SWIGLU) {
        int n = g * RR + (r % RR); n = n < n_out ? n : n_out - 1;
        rows[r] = 32 * (n >> 4) + (n & 15) + (r / RR) * 16;       // gate rows, then the matching up rows
      } else {
        const int n = g * R + r;
        rows[r] = n < p.N ? n : p.N - 1;
      }
    }
    float acc[R];
    RwTail<T, R> tail;
    {
      constexpr bool plain = EPI != EPI_SWIGLU && EPI != EPI_PARTIAL;
      const bool hb = plain && p.bias, hr = EPI == EPI_RESID && !p.out_f32;
      tail.p0 = hb ? (const T*)p.bias : (const T*)p.X;
      tail.p1 = hr ? (const T*)p.resid : (const T*)p.X;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = g * OUT + r;
        tail.idx[r] = (hb || hr) ? (n < n_out ? n : n_out - 1) : 0;
      }
      if (!hb) tail.p0 = tail.p1;      // (one of the two may be absent: read the other's element twice rather than element idx of x)
      if (!hr) tail.p1 = tail.p0;
    }
    if constexpr (F8 != WF_16) rw_dispatch_q<T, R, RW_MAXC, F8>(nch, p, rows, k0, lane, xr, acc, tail);
    else rw_dispatch<T, R, RW_MAXC>(nch, W, p.ldw, rows, k0, p.K, lane, xr, acc, tail);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < OUT; ++r) {
        const int n = g * OUT + r;
        if (n >= n_out) continue;
        if constexpr (EPI == EPI_SWIGLU) {
          const float gt = rnd<T>(acc[r]), up = rnd<T>(acc[r + RR]);
          ((T*)p.Y)[n] = fromf<T>(rnd<T>(silu(gt)) * up);
        } else if constexpr (EPI == EPI_PARTIAL) {
          ((float*)p.Y)[(size_t)blockIdx.y * p.ldy + n] = acc[r];        // [ksplit][1][ldy]
        } else {
          float y = acc[r] + (p.bias ? tail.v0[r] : 0.f);
          if (p.out_f32) ((float*)p.Y)[n] = y;
          else {
            y = rnd<T>(y);
            if constexpr (EPI == EPI_RESID) y = tail.v1[r] + y;
            ((T*)p.Y)[n] = fromf<T>(y);
          }
        }
      }
    }
  }
  if constexpr (EPI == EPI_RESID && WAVES == 7) OM_DBG_MAX(3, (blockIdx.x & 7) == 0);
}

// the kernels of the form: 16-bit / e4m3 weights under the template switch they always had (profiles and tools/kernel_roles.py name these symbols),
// MXFP4 as a kernel of its own over the same body
template <typename T, int EPI, int RR = 4, int WAVES = 4, bool F8 = false>
__global__ __launch_bounds__(WAVES * 64) void gemv_rows_kernel(GemvP p) { gemv_rows_body<T, EPI, RR, WAVES, F8 ? WF_E4M3 : WF_16>(p); }
template <typename T, int EPI, int RR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gemv_rows_mx4_kernel(GemvP p) { gemv_rows_body<T, EPI, RR, WAVES, WF_MX4>(p); }

// ---------------------------------------------------------------------------------------------------------
// Whole-row GEMV with the RMSNorm that precedes the projection computed in registers (round 3; batch 1, no split-K, K = 512 NCH <= 4096):
//   y = epi(W xn),  xn = T(w * T(x * rsqrt(mean(x^2) + eps)))      (Qwen2RMSNorm's rounding points, modeling_qwen2.py:247-252)
// X is the RAW hidden row.  One group of rows per wave; ALL of the group's weight loads are issued first, then the workgroup's four
// waves normalise the row together through LDS (x and the norm weights are read once per WORKGROUP) while those loads are in flight,
// the dot products last.  Measured forms that did not pay: the chain in front of the weight loads, every wave for itself (gate|up
// 41.6 -> 45.8 us: exactly the launch it removes); every wave for itself with half the rows per wave to make room (48.3 us: x and the norm
// weights were then half as many bytes through the CU as the weights).  All waves use the same sum (fixed order): the same bits.
// It removes the residual + RMSNorm launch in front of the gate|up GEMV of a batch-1 decode step (o_proj then writes x + attn itself).
// ---------------------------------------------------------------------------------------------------------
template <typename T, int EPI, int RR, int NCH, int F8, int WAVES>
__device__ __forceinline__ void gemv_rows_norm_body(const GemvP& p) {
  typedef typename V8<T>::type v8;
  constexpr int R = EPI == EPI_SWIGLU ? 2 * RR : RR;
  __shared__ __attribute__((aligned(16))) T xs[NCH * 512];
  __shared__ float red[WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_out = EPI == EPI_SWIGLU ? p.N / 2 : p.N;
  int g = blockIdx.x * WAVES + wave;
#if OMCHAT_EXPERIMENTS
  if constexpr (EPI == EPI_SWIGLU && RR == 1 && WAVES == 4) {
    // experiment (tuning key 28): the odd XCDs end this launch 2-3 us after the even ones (clock stamps), and workgroup ids go
    // round the XCDs -- so XCD x gets a contiguous range of pairs, p.xskew workgroups longer on even x and as much shorter on odd x
    if (p.xskew) {
      const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
      const int base = ((n_out + 3) / 4) / 8;
      const int n_x = base + ((x & 1) ? -p.xskew : p.xskew);
      if (j >= n_x) return;
      g = (x * base + ((x & 1) ? p.xskew : 0) + j) * 4 + wave;
    }
  }
#endif
  if constexpr (EPI == EPI_SWIGLU) OM_DBG_MIN(4, blockIdx.x < 8);
  if constexpr (EPI == EPI_NONE) OM_DBG_MIN(8, blockIdx.x < 8);
  // ---- 0. x and the norm weights are requested IN FRONT of the weight rows (round 4).  Vector memory returns in order: behind the weight
  // loads the 2 x 7 KB of x / norm weights (L2 hits) could not be used before the wave's whole first batch of weights had come in from HBM, and
  // the norm -- two barriers and two LDS round trips -- then ran with nothing left in flight behind it.  In front, the norm is done while the
  // weights are still on their way and the dot products start when they land: qkv 7.95-8.33 -> 7.13 us, e4m3 decode 1.83 -> 1.73 ms per token.
  // (Not in the loop form and not in the long-K kernel: there the same order measured SLOWER, gate|up 42.27 -> 43.00 us, down_proj 23.13 ->
  // 23.49 us -- every wave of the chip asks for the same 14 KB first, and the weight requests of a CU queue behind that hot spot; with
  // three buffers in flight the late norm was hidden already; x BETWEEN the first buffer and the other two measured 42.8 us as well.
  // tools/bench_gemv_b1.py, profiles/r04_al.)
  static_assert(WAVES >= 4 && NCH <= 8, "sum-of-squares order: four owner waves, up to two chunks each");
  constexpr int MC = (NCH + WAVES - 1) / WAVES;
  constexpr int SC = (NCH + 3) / 4;
  rw_u32x4 xq[MC], nq[MC], sq[SC];
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + WAVES * i, k = c * 512 + lane * 8;
    const rw_u32x4 z = {0u, 0u, 0u, 0u};
    const bool ok = c < NCH && k < p.K;
    xq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
    nq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.norm_w + k) : z;
  }
#pragma unroll
  for (int i = 0; i < SC; ++i) {
    if constexpr (WAVES == 4) {
      sq[i] = xq[i];
    } else {
      const int c = wave + 4 * i, k = c * 512 + lane * 8;
      const rw_u32x4 z = {0u, 0u, 0u, 0u};
      sq[i] = (wave < 4 && c < NCH && k < p.K) ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
    }
  }
  // ---- 1. this wave's weight rows: every load issued now
  int rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if constexpr (EPI == EPI_SWIGLU) {
      int n = g * RR + (r % RR); n = n < n_out ? n : n_out - 1;
      rows[r] = 32 * (n >> 4) + (n & 15) + (r / RR) * 16;       // gate rows, then the matching up rows
    } else {
      const int n = g * R + r;
      rows[r] = n < p.N ? n : p.N - 1;
    }
  }
  typedef typename RwW<F8>::type wreg_t;
  wreg_t w[R][NCH];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      int k = c * 512 + lane * 8;
      k = k < p.K ? k : 0;                      // ragged last chunk: clamp (x is zero there)
      if constexpr (F8 == WF_X12) w[r][c] = x12_ldw(p, (size_t)rows[r], c, lane);      // (K = 512 NCH: no ragged chunk)
      else w[r][c] = rw_ldw<T, F8>(p, (size_t)rows[r], k);
    }
  // the epilogue's operands (bias, e4m3 row scales) are requested right BEHIND the weight rows: they come back with them instead of costing a
  // dependent L2 round trip after the reduction.  (In FRONT of the weights they measured slower: a cold 2-byte load at the head of the
  // in-order queue holds every weight row behind it -- profiles/r04_al.)  No branch around the loads: a null bias reads the norm weights.
  float e_bias[RR], e_scale[R];
  {
    const T* bp = (EPI != EPI_SWIGLU && p.bias) ? (const T*)p.bias : (const T*)p.norm_w;
    const int nmax = (EPI != EPI_SWIGLU && p.bias) ? n_out - 1 : 0;
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const int n = g * RR + r;
      e_bias[r] = tof(bp[n < nmax ? n : nmax]);
    }
    if (!(EPI != EPI_SWIGLU && p.bias)) {
#pragma unroll
      for (int r = 0; r < RR; ++r) e_bias[r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) e_scale[r] = 1.f;
    if constexpr (F8 == WF_E4M3) {
#pragma unroll
      for (int r = 0; r < R; ++r) e_scale[r] = p.w_scale[rows[r]];
    }
  }
  X12Row xst[F8 == WF_X12 ? R : 1];      // bf16x12: each row's top, patch count and patches, behind its weights like the operands above
  if constexpr (F8 == WF_X12) {
#pragma unroll
    for (int r = 0; r < R; ++r) x12_row_load(xst[r], p, (size_t)rows[r], lane);
  }
  // ---- 2. the norm, shared by the workgroup: wave w normalises chunks w, w + WAVES, ... (x and the norm weights are read ONCE per
  // workgroup: 2 x 7 KB instead of 7 KB of xn per wave), the normalised row goes to LDS, every wave reads it back.  The plain loads above
  // stay in flight across the two barriers.
  // The sum of squares is ALWAYS taken in the four-wave order -- waves 0..3 own chunks w and w + 4, per-lane accumulation over the two
  // chunks, butterfly, ((r0 + r1) + r2) + r3 -- whatever WAVES is, so that every launch form of a projection (4, 7 or 9 waves, the loop
  // form) gives the same bits on every device (the nine-wave form used to sum its nine per-chunk partials: ADVICE r03).
  __builtin_amdgcn_sched_barrier(0);            // keep every load above the first wait
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < SC; ++i) {
    const v8 xv = __builtin_bit_cast(v8, sq[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float v = tof(xv[j]); ss += v * v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0 && wave < 4) red[wave] = ss;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  float tot = red[0];                           // fixed order: the same bits in every wave and in every launch form
#pragma unroll
  for (int w = 1; w < 4; ++w) tot += red[w];
  const float inv = rsqrtf(tot / (float)p.K + p.norm_eps);
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + WAVES * i;
    if (c < NCH) {
      const v8 xv = __builtin_bit_cast(v8, xq[i]), wv = __builtin_bit_cast(v8, nq[i]);
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fromf<T>(tof(wv[j]) * rnd<T>(tof(xv[j]) * inv));
      *reinterpret_cast<v8*>(xs + c * 512 + lane * 8) = o;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  rw_u32x4 xr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) xr[c] = *reinterpret_cast<const rw_u32x4*>(xs + c * 512 + lane * 8);
  __builtin_amdgcn_sched_barrier(0);
  // ---- 3. dot products
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float a = 0.f;
    if constexpr (F8 == WF_X12) x12_row_finish(xst[r]);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if constexpr (F8 != WF_X12) a = rw_dotw<T, F8>(w[r][c], xr[c], a);
    }
    if constexpr (F8 == WF_X12) {      // the same dot products in the same order on the decoded registers, in groups of up to four chunks
      constexpr int G0 = NCH < 4 ? NCH : 4, G1 = NCH - G0;
      {
        rw_u32x4 wd[G0];
        x12_group<G0>(wd, &w[r][0], xst[r], 0, NCH, lane);
#pragma unroll
        for (int c = 0; c < G0; ++c) a = rw_dot8<T>(wd[c], xr[c], a);
      }
      if constexpr (G1 > 0) {
        rw_u32x4 wd[G1];
        x12_group<G1>(wd, &w[r][G0], xst[r], G0, NCH, lane);
#pragma unroll
        for (int c = 0; c < G1; ++c) a = rw_dot8<T>(wd[c], xr[G0 + c], a);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if constexpr (F8 == WF_E4M3) a *= e_scale[r];
    acc[r] = a;
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const int n = g * RR + r;
      if (n >= n_out) continue;
      if constexpr (EPI == EPI_SWIGLU) {
        const float gt = rnd<T>(acc[r]), up = rnd<T>(acc[r + RR]);
        ((T*)p.Y)[n] = fromf<T>(rnd<T>(silu(gt)) * up);
      } else {
        const float y = acc[r] + e_bias[r];
        if (p.out_f32) ((float*)p.Y)[n] = y;
        else ((T*)p.Y)[n] = fromf<T>(y);
      }
    }
  }
  if constexpr (EPI == EPI_SWIGLU) { OM_DBG_MAX(5, blockIdx.x + 64 >= gridDim.x); OM_DBG_MAX(16 + (blockIdx.x & 7), blockIdx.x + 512 >= gridDim.x); }      // + the end per XCD
  if constexpr (EPI == EPI_NONE) OM_DBG_MAX(9, (blockIdx.x & 7) == 0);
}

template <typename T, int EPI, int RR, int NCH, bool F8, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64) void gemv_rows_norm_kernel(GemvP p) { gemv_rows_norm_body<T, EPI, RR, NCH, F8 ? WF_E4M3 : WF_16, WAVES>(p); }
template <typename T, int EPI, int RR, int NCH, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64) void gemv_rows_norm_mx4_kernel(GemvP p) { gemv_rows_norm_body<T, EPI, RR, NCH, WF_MX4, WAVES>(p); }
// bf16x12 rows: the batch-1 step's gate|up (EPI_SWIGLU, one pair per wave) and lm_head (EPI_NONE, four rows per wave) launches
template <typename T, int EPI, int RR, int NCH>
__global__ __launch_bounds__(256) void gemv_rows_norm_x12_kernel(GemvP p) { gemv_rows_norm_body<T, EPI, RR, NCH, WF_X12, 4>(p); }

// ---------------------------------------------------------------------------------------------------------
// Loop form of gemv_rows_norm_kernel (round 3): ONE resident round of workgroups (2 per CU), each owning a contiguous range of outputs
// and every wave walking its share one output at a time (a row, or a (gate, up) pair) through a ring of three register buffers -- two
// outputs' weights in flight under the dot products of the third.  Why: the one-shot form deals 12 outputs per workgroup, and gate|up has
// 18944 = 37 x 512 of them: 1579 workgroups on 512 slots leave a fourth, 8 %-full round whose 43 workgroups finish alone on 43 CUs; here
// every workgroup gets 37 outputs (waves 10 / 9 / 9 / 9) and the launch ends everywhere at once.  The norm prologue is the same and runs
// once per workgroup.  Per output the arithmetic and its order are those of the one-shot form: the same bits.
// ---------------------------------------------------------------------------------------------------------
template <typename T, int EPI, int NCH, int F8>
__device__ __forceinline__ void gemv_rows_norm_loop_body(const GemvP& p, int per_wg, unsigned skew) {
  typedef typename V8<T>::type v8;
  constexpr int R = EPI == EPI_SWIGLU ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T xs[NCH * 512];
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_out = EPI == EPI_SWIGLU ? p.N / 2 : p.N;
  int o0 = blockIdx.x * per_wg, o1 = o0 + per_wg < n_out ? o0 + per_wg : n_out;
  if constexpr (EPI == EPI_SWIGLU) OM_DBG_MIN(4, blockIdx.x < 8);
  if (skew) {      // experiment (tuning key 28): shares by blockIdx % 8, per_wg + d_l with d_l = nibble l of skew - 8 (the deltas sum to 0)
    const int l = blockIdx.x & 7;
    int pre = 0;
    for (int i = 0; i < l; ++i) pre += per_wg + (int)((skew >> (4 * i)) & 15u) - 8;
    o0 = (blockIdx.x >> 3) * 8 * per_wg + pre;
    o1 = o0 + per_wg + (int)((skew >> (4 * l)) & 15u) - 8;
    o1 = o1 < n_out ? o1 : n_out;
  }
  typedef typename RwW<F8>::type wreg_t;
  auto row_of = [&](int n, int r) { return EPI == EPI_SWIGLU ? 32 * (n >> 4) + (n & 15) + r * 16 : n; };
  auto load_w = [&](wreg_t (&w)[R][NCH], int n) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t row = (size_t)row_of(n, r);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int k = c * 512 + lane * 8;
        k = k < p.K ? k : 0;                    // ragged last chunk: clamp (x is zero there)
        w[r][c] = rw_ldw<T, F8>(p, row, k);
      }
    }
  };
  // ---- 1. the first three outputs of this wave: every load issued now
  wreg_t wa[R][NCH], wb[R][NCH], wc[R][NCH];
  const int u0 = o0 + wave;
  if (u0 < o1) load_w(wa, u0);
  if (u0 + 4 < o1) load_w(wb, u0 + 4);
  if (u0 + 8 < o1) load_w(wc, u0 + 8);
  // ---- 2. the norm, shared by the workgroup (gemv_rows_norm_kernel step 2)
  constexpr int MC = (NCH + 3) / 4;
  rw_u32x4 xq[MC], nq[MC];
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + 4 * i, k = c * 512 + lane * 8;
    const rw_u32x4 z = {0u, 0u, 0u, 0u};
    const bool ok = c < NCH && k < p.K;
    xq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
    nq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.norm_w + k) : z;
  }
  __builtin_amdgcn_sched_barrier(0);            // keep every load above the first wait
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const v8 xv = __builtin_bit_cast(v8, xq[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float v = tof(xv[j]); ss += v * v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wave] = ss;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  const float inv = rsqrtf((((red[0] + red[1]) + red[2]) + red[3]) / (float)p.K + p.norm_eps);
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + 4 * i;
    if (c < NCH) {
      const v8 xv = __builtin_bit_cast(v8, xq[i]), wv = __builtin_bit_cast(v8, nq[i]);
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fromf<T>(tof(wv[j]) * rnd<T>(tof(xv[j]) * inv));
      *reinterpret_cast<v8*>(xs + c * 512 + lane * 8) = o;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  rw_u32x4 xr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) xr[c] = *reinterpret_cast<const rw_u32x4*>(xs + c * 512 + lane * 8);
  __builtin_amdgcn_sched_barrier(0);
  // ---- 3. dot products, one output at a time; the buffer just consumed is refilled with the output three steps ahead
  auto finish = [&](wreg_t (&w)[R][NCH], int n) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        a = rw_dotw<T, F8>(w[r][c], xr[c], a);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if constexpr (F8 == WF_E4M3) a *= p.w_scale[row_of(n, r)];
      acc[r] = a;
    }
    if (lane == 0) {
      if constexpr (EPI == EPI_SWIGLU) {
        const float gt = rnd<T>(acc[0]), up = rnd<T>(acc[R - 1]);
        ((T*)p.Y)[n] = fromf<T>(rnd<T>(silu(gt)) * up);
      } else {
        const float y = acc[0] + (p.bias ? tof(((const T*)p.bias)[n]) : 0.f);
        if (p.out_f32) ((float*)p.Y)[n] = y;
        else ((T*)p.Y)[n] = fromf<T>(y);
      }
    }
  };
  for (int u = u0; u < o1; u += 12) {
    finish(wa, u);
    if (u + 12 < o1) load_w(wa, u + 12);
    if (u + 4 < o1) {
      finish(wb, u + 4);
      if (u + 16 < o1) load_w(wb, u + 16);
    }
    if (u + 8 < o1) {
      finish(wc, u + 8);
      if (u + 20 < o1) load_w(wc, u + 20);
    }
  }
  if constexpr (EPI == EPI_SWIGLU) {      // measurement (experiments build): start / end of the launch and the end per XCD (workgroup ids go round the 8 XCDs)
    OM_DBG_MAX(5, (blockIdx.x & 7) == 0);
    OM_DBG_MAX(16 + (blockIdx.x & 7), true);
  }
}

template <typename T, int EPI, int NCH, bool F8>
__global__ __launch_bounds__(256) void gemv_rows_norm_loop_kernel(GemvP p, int per_wg, unsigned skew) {
  gemv_rows_norm_loop_body<T, EPI, NCH, F8 ? WF_E4M3 : WF_16>(p, per_wg, skew);
}
template <typename T, int EPI, int NCH>
__global__ __launch_bounds__(256) void gemv_rows_norm_loop_mx4_kernel(GemvP p, int per_wg, unsigned skew) {
  gemv_rows_norm_loop_body<T, EPI, NCH, WF_MX4>(p, per_wg, skew);
}

// ---------------------------------------------------------------------------------------------------------
// Dynamic form of the loop kernel (round 4).  The loop form deals every workgroup the same number of outputs and ends when the SLOWEST
// workgroup ends -- and the eight XCDs of this chip do not stream at the same rate: with equal shares the gate|up phase of a CU took
// 32.8 / 39.9 / 34.7 / 37.8 / 33.0 / 38.2 / 35.1 / 38.1 us by blockIdx % 8 (= the XCD group under round-robin dispatch; phase stamps of
// tools/experiments/tune_layer.hip), i.e. the launch waits ~10 % for three of the XCDs.  Here the outputs are cut into chunks of DYN_CH and dealt by
// atomic counters: DYN_POOLS pools (workgroup b starts at pool b % DYN_POOLS, so pool p is drained by one XCD group, p % 8), a wave takes
// chunks from its pool and, when that is empty, from the following pools -- the fast XCDs end up with more chunks.  (Eight pools measured
// 80 us per launch: a counter under streaming load answers ~15 tickets per us, not the 88 of an idle chip.)
// Which wave computes an output changes nothing in its arithmetic: the same bits as the loop form.  Placement independent: the pool index
// is only a shard label.  A chunk id is requested BEFORE the loads of the previous chunk are issued and used when that chunk is half
// done, so the returning atomic never waits behind weight loads that are younger than the ones the wave needs next.
// Counters: one 256-byte line each (nine counters in ONE line took 331 us per launch: the memory-side atomic unit serialises a line):
// p.dyn[64 g] pool g, p.dyn[64 DYN_POOLS] finished waves; the last wave to finish zeroes them for the next launch on the same slot.
// ---------------------------------------------------------------------------------------------------------
constexpr int DYN_CH = 2;
constexpr int DYN_POOLS = 64;      // work counters per launch, one 256-byte line each (a counter then sees ~4 grabs per us)
template <typename T, int EPI, int NCH, int F8>
__device__ __forceinline__ void gemv_rows_norm_dyn_body(const GemvP& p) {
  typedef typename V8<T>::type v8;
  constexpr int R = EPI == EPI_SWIGLU ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T xs[NCH * 512];
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_out = EPI == EPI_SWIGLU ? p.N / 2 : p.N;
  const int n_chunks = (n_out + DYN_CH - 1) / DYN_CH, pool_sz = (n_chunks + DYN_POOLS - 1) / DYN_POOLS;
  typedef typename RwW<F8>::type wreg_t;
  auto row_of = [&](int n, int r) { return EPI == EPI_SWIGLU ? 32 * (n >> 4) + (n & 15) + r * 16 : n; };
  auto load_w = [&](wreg_t (&w)[R][NCH], int n) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t row = (size_t)row_of(n, r);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int k = c * 512 + lane * 8;
        k = k < p.K ? k : 0;
        w[r][c] = rw_ldw<T, F8>(p, row, k);
      }
    }
  };
  // ---- chunk queue of this wave.  `pool` walks the eight pools starting at the workgroup's own; a raw ticket >= the pool's size means
  // that pool is empty: move on (blocking grabs from then on: the tail of the launch).
  int pool = 0;                                   // pools tried so far (DYN_POOLS = nothing left anywhere)
  const int g0 = blockIdx.x % DYN_POOLS;
  auto pool_count = [&](int g) { const int lo = g * pool_sz; return lo >= n_chunks ? 0 : (lo + pool_sz <= n_chunks ? pool_sz : n_chunks - lo); };
  auto ticket = [&]() -> unsigned {               // one ticket from the current pool (returning atomic; wave-uniform through lane 0)
    unsigned t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(p.dyn + 64 * ((g0 + pool) % DYN_POOLS), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return t;
  };
  auto resolve = [&](unsigned t) -> int {         // ticket -> chunk id, or -1 when every pool is empty
    int tk = (int)__builtin_amdgcn_readfirstlane(t);
    for (;;) {
      const int g = (g0 + pool) % DYN_POOLS;
      if (tk < pool_count(g)) return g * pool_sz + tk;
      if (++pool >= DYN_POOLS) return -1;
      tk = (int)__builtin_amdgcn_readfirstlane(ticket());
    }
  };
  // ---- 1. the first two chunks: tickets first, then the first chunk's loads as soon as its id is known
  int cur = resolve(ticket());
  unsigned nxt_t = cur >= 0 ? ticket() : 0u;
  wreg_t wa[R][NCH], wb[R][NCH], wc[R][NCH];
  auto out_ok = [&](int chunk, int i) { return chunk >= 0 && chunk * DYN_CH + i < n_out; };
  if (out_ok(cur, 0)) load_w(wa, cur * DYN_CH);
  if (out_ok(cur, 1)) load_w(wb, cur * DYN_CH + 1);
  // ---- 2. the norm, shared by the workgroup (gemv_rows_norm_kernel step 2; four-wave order)
  constexpr int MC = (NCH + 3) / 4;
  rw_u32x4 xq[MC], nq[MC];
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + 4 * i, k = c * 512 + lane * 8;
    const rw_u32x4 z = {0u, 0u, 0u, 0u};
    const bool ok = c < NCH && k < p.K;
    xq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
    nq[i] = ok ? *reinterpret_cast<const rw_u32x4*>((const T*)p.norm_w + k) : z;
  }
  __builtin_amdgcn_sched_barrier(0);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const v8 xv = __builtin_bit_cast(v8, xq[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float v = tof(xv[j]); ss += v * v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wave] = ss;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  const float inv = rsqrtf((((red[0] + red[1]) + red[2]) + red[3]) / (float)p.K + p.norm_eps);
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int c = wave + 4 * i;
    if (c < NCH) {
      const v8 xv = __builtin_bit_cast(v8, xq[i]), wv = __builtin_bit_cast(v8, nq[i]);
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fromf<T>(tof(wv[j]) * rnd<T>(tof(xv[j]) * inv));
      *reinterpret_cast<v8*>(xs + c * 512 + lane * 8) = o;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  rw_u32x4 xr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) xr[c] = *reinterpret_cast<const rw_u32x4*>(xs + c * 512 + lane * 8);
  __builtin_amdgcn_sched_barrier(0);
  auto finish = [&](wreg_t (&w)[R][NCH], int n) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        a = rw_dotw<T, F8>(w[r][c], xr[c], a);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if constexpr (F8 == WF_E4M3) a *= p.w_scale[row_of(n, r)];
      acc[r] = a;
    }
    if (lane == 0) {
      if constexpr (EPI == EPI_SWIGLU) {
        const float gt = rnd<T>(acc[0]), up = rnd<T>(acc[R - 1]);
        ((T*)p.Y)[n] = fromf<T>(rnd<T>(silu(gt)) * up);
      } else {
        const float y = acc[0] + (p.bias ? tof(((const T*)p.bias)[n]) : 0.f);
        if (p.out_f32) ((float*)p.Y)[n] = y;
        else ((T*)p.Y)[n] = fromf<T>(y);
      }
    }
  };
  // ---- 3. chunks of two outputs through three register buffers: while chunk j is computed, the first output of chunk j + 1 is in flight
  // (its id was requested before chunk j's loads were issued), and the ticket of chunk j + 2 goes out before chunk j + 1's loads
  while (cur >= 0) {
    const int nxt = resolve(nxt_t);               // usually long answered; blocking only when a pool ran dry
    if (nxt >= 0) nxt_t = ticket();
    if (out_ok(nxt, 0)) load_w(wc, nxt * DYN_CH);
    finish(wa, cur * DYN_CH);
    if (out_ok(nxt, 1)) load_w(wa, nxt * DYN_CH + 1);
    if (out_ok(cur, 1)) finish(wb, cur * DYN_CH + 1);
    cur = nxt;
    if (cur < 0) break;
    // the roles of the buffers rotate: (wa, wb, wc) held (cur.0, cur.1, nxt.0); now cur.0 sits in wc and cur.1 in wa
    const int nx2 = resolve(nxt_t);
    if (nx2 >= 0) nxt_t = ticket();
    if (out_ok(nx2, 0)) load_w(wb, nx2 * DYN_CH);
    finish(wc, cur * DYN_CH);
    if (out_ok(nx2, 1)) load_w(wc, nx2 * DYN_CH + 1);
    if (out_ok(cur, 1)) finish(wa, cur * DYN_CH + 1);
    cur = nx2;
    if (cur < 0) break;
    // now cur.0 sits in wb and cur.1 in wc
    const int nx3 = resolve(nxt_t);
    if (nx3 >= 0) nxt_t = ticket();
    if (out_ok(nx3, 0)) load_w(wa, nx3 * DYN_CH);
    finish(wb, cur * DYN_CH);
    if (out_ok(nx3, 1)) load_w(wb, nx3 * DYN_CH + 1);
    if (out_ok(cur, 1)) finish(wc, cur * DYN_CH + 1);
    cur = nx3;                                    // cur.0 in wa, cur.1 in wb again
  }
  // ---- 4. the last wave of the launch zeroes the counters for the next launch on this slot
  if (lane == 0) {
    const unsigned done = __hip_atomic_fetch_add(p.dyn + 64 * DYN_POOLS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (done == gridDim.x * 4u - 1u) {
      for (int i = 0; i <= DYN_POOLS; ++i) __hip_atomic_store(p.dyn + 64 * i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, int EPI, int NCH, bool F8>
__global__ __launch_bounds__(256) void gemv_rows_norm_dyn_kernel(GemvP p) { gemv_rows_norm_dyn_body<T, EPI, NCH, F8 ? WF_E4M3 : WF_16>(p); }
template <typename T, int EPI, int NCH>
__global__ __launch_bounds__(256) void gemv_rows_norm_dyn_mx4_kernel(GemvP p) { gemv_rows_norm_dyn_body<T, EPI, NCH, WF_MX4>(p); }

// ---------------------------------------------------------------------------------------------------------
// Whole-row GEMV for LONG K without split-K (round 3; batch 1: down_proj, K = 18944): y[n] = resid[n] + T(sum_k W[n][k] x[k]), in place.
// The split-K form leaves fp32 slices that a residual + RMSNorm launch must sum; here a workgroup stages x (37 KB) in LDS once, every
// wave streams whole rows in passes of 8 chunks of 512 (weights of pass p + 1 in flight under the dot products of pass p) and lane 0
// adds the residual: x + mlp is complete when the launch ends, and the NEXT projection normalises it in its own registers
// (gemv_rows_norm_kernel).  Rows are dealt to 2 workgroups per CU, row r of a workgroup to wave r % 4.
// ---------------------------------------------------------------------------------------------------------
// CP chunks per pass and, for the bf16x12 rows, G chunks per decode group are compile-time: a lane adds chunk after chunk into one accumulator,
// so how the chunks are grouped into passes changes no bit.  CP divides 8, so the passes cover exactly the 16-bit form's ceil8(nch)
// chunks: those in [nch, ceil8(nch)) read weights 0..7 against zeros of x (the clamped address) and there is none beyond -- with
// K % 4096 == 0 no w * 0 term exists, and a row with an infinite weight among its first eight stays infinite at every CP.
// 16-bit, e4m3 and MXFP4 rows: 8 chunks.  bf16x12: 4 chunks, where 8 leave one workgroup per CU.
// NB = 0 is the three-buffer loop of rounds 3-4, whose rotation is in the source only: its loads stand under conditions, the compiler's wait in
// front of a pass's dot products is the smallest count over the paths that meet there, and the tail path has none behind the buffer in use --
// the 16-bit instance waits vmcnt(7) .. vmcnt(0) behind the loads it has just issued and computes with nothing in flight; x is staged as a
// chain of load, vmcnt(0), LDS write per vector, whose first wait drains the three buffers.  NB > 0 is the counted pipeline over NB buffers
// (below): the coded instance runs NB = 3 and waits vmcnt(22) / (20) / (18) / (16) in front of its four chunks -- two whole passes stay in
// flight -- at 93 VGPRs, no scratch, 5 waves per SIMD by registers, both workgroups of a CU resident.  The 16-bit instance did not gain from
// it in the role bench (8 x 2, 4 x 3, 4 x 4: LOG.md 2026-10-20) and keeps NB = 0 with the e4m3 and MXFP4 ones, which were not timed.
template <typename T, int F8, int CP = 8, int G = 2, int NB = 0, int XB = 6>
__device__ __forceinline__ void gemv_rows_longk_body(const GemvP& p, int rows_per_wg) {
  static_assert(8 % CP == 0 && CP % G == 0, "whole passes cover ceil8(nch) chunks, whole decode groups a pass");
  extern __shared__ __attribute__((aligned(16))) char xs_raw[];
  T* xs = (T*)xs_raw;
  // one row per wave, rows_per_wg (<= 8) waves per workgroup: every wave of a workgroup streams the same number of bytes (7 rows per
  // workgroup at N = 3584 on 2 x 256 workgroups; two rows per wave on 4 waves left the fourth wave idle half the time: 26.0 us)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nch = (p.K + 511) >> 9, npass8 = (nch + 7) >> 3, npass = npass8 * (8 / CP);
  const int n = blockIdx.x * rows_per_wg + wave;
  const bool valid = n < p.N;
  const int row = valid ? n : p.N - 1;
  OM_DBG_MIN(6, blockIdx.x < 8);
  typedef typename RwW<F8>::type wreg_t;
  auto load_w = [&](wreg_t (&w)[CP], int pass) {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int k = (pass * CP + c) * 512 + lane * 8;
      k = k < p.K ? k : 0;                      // beyond K: any valid address (x is zero there)
      if constexpr (F8 == WF_X12) w[c] = x12_ldw(p, (size_t)row, pass * CP + c < nch ? pass * CP + c : 0, pass * CP + c < nch ? lane : 0);
      else w[c] = rw_ldw<T, F8>(p, (size_t)row, k);
    }
  };
  float acc = 0.f;
  X12Row xst;
  auto dots = [&](wreg_t (&w)[CP], int pass) {
    if constexpr (F8 == WF_X12) {      // the 16-bit kernel's dot products in its order, on registers decoded G chunks at a time
#pragma unroll
      for (int h = 0; h < CP / G; ++h) {
        rw_u32x4 wd[G];
        x12_group<G>(wd, &w[G * h], xst, pass * CP + G * h, nch, lane);
#pragma unroll
        for (int c = 0; c < G; ++c) {
          const rw_u32x4 xr = *reinterpret_cast<const rw_u32x4*>(xs + (pass * CP + G * h + c) * 512 + lane * 8);
          acc = rw_dot8<T>(wd[c], xr, acc);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const rw_u32x4 xr = *reinterpret_cast<const rw_u32x4*>(xs + (pass * CP + c) * 512 + lane * 8);
        acc = rw_dotw<T, F8>(w[c], xr, acc);
      }
    }
    // the counted form: the pass's sum is complete HERE (the compiler otherwise sinks the dot products of all passes of an iteration to its
    // end and keeps their decoded weights and x rows live: 199 VGPRs)
    if constexpr (NB > 0) asm volatile("" : "+v"(acc));
  };
  if constexpr (NB > 0) {
    // ---- the counted pipeline.  The vector-memory counter is in order and the compiler's wait in front of a use is the SMALLEST number of
    // younger loads over all paths that reach it: one path without loads behind the use's operand and the wait is vmcnt(0) for every path.
    // So (a) x goes out FIRST, all of a thread's vectors (XB per batch, the condition in the address), and is written to LDS behind one wait that
    // leaves the weight passes in flight; (b) every load_w of the repeated part is unconditional; (c) the passes that finish a row are
    // straight-line cases per number of remaining passes that meet only at the reduction, with nothing in flight.
    const int nx = npass8 * 8 * 64, bd = (int)blockDim.x;
    const rw_u32x4 z = {0u, 0u, 0u, 0u};
    // vector j of a batch; one beyond the staged x repeats the thread's own first vector (nx >= 1024 > threadIdx.x: the same value to the same
    // address again), so that neither a load nor a write stands under a branch
    auto xi = [&](int base, int j) { const int i = base + (int)threadIdx.x + j * bd; return i < nx ? i : (int)threadIdx.x; };
    rw_u32x4 xv[XB];
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      xv[j] = *reinterpret_cast<const rw_u32x4*>((const T*)p.X + (xi(0, j) * 8 < p.K ? xi(0, j) * 8 : 0));
    }
    __builtin_amdgcn_sched_barrier(0);
    wreg_t w[NB][CP];
    load_w(w[0], 0);
    if constexpr (F8 == WF_X12) x12_row_load(xst, p, (size_t)row, lane);
    __builtin_amdgcn_sched_barrier(0);          // (the row's top and patch count stay right behind the first pass: scheduled last, their wait drains every buffer)
#pragma unroll
    for (int b = 1; b < NB; ++b) {            // K > 4096: at least 16 / CP passes, loaded without a condition
      if (b < 16 / CP || b < npass) load_w(w[b], b);
    }
    const float e_bias_raw = tof(((const T*)(p.bias ? p.bias : p.X))[p.bias ? row : 0]);
    const float e_res_raw = tof(((const T*)(p.resid ? p.resid : p.X))[p.resid ? row : 0]);
    const float e_bias = p.bias ? e_bias_raw : 0.f, e_res = p.resid ? e_res_raw : 0.f;
    float e_scale = 1.f;
    if constexpr (F8 == WF_E4M3) e_scale = p.w_scale[row];
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      *reinterpret_cast<rw_u32x4*>(xs + xi(0, j) * 8) = xi(0, j) * 8 < p.K ? xv[j] : z;
    }
    // (a workgroup of fewer than nx / XB threads -- few rows per workgroup, or K beyond XB * 512 * rows_per_wg: the rest in further batches)
    for (int base = XB * bd; base < nx; base += XB * bd) {
#pragma unroll
      for (int j = 0; j < XB; ++j) {
        xv[j] = *reinterpret_cast<const rw_u32x4*>((const T*)p.X + (xi(base, j) * 8 < p.K ? xi(base, j) * 8 : 0));
      }
#pragma unroll
      for (int j = 0; j < XB; ++j) {
        *reinterpret_cast<rw_u32x4*>(xs + xi(base, j) * 8) = xi(base, j) * 8 < p.K ? xv[j] : z;
      }
    }
    __syncthreads();
    if constexpr (F8 == WF_X12) x12_row_finish(xst);
    // w[b] holds pass ps + b; NB - 1 whole passes stay in flight under every dots() of the repeated part
    auto last = [&](int ps, auto rem) {         // the last rem passes of the row (1 .. 2 NB - 1), the first min(rem, NB) of them loaded or on their way
#pragma unroll
      for (int b = 0; b < decltype(rem)::value; ++b) {
        dots(w[b % NB], ps + b);
        if (b + NB < decltype(rem)::value) load_w(w[b % NB], ps + b + NB);
      }
    };
    int ps = 0;
#pragma unroll 1
    for (; ps + 2 * NB <= npass; ps += NB) {
#pragma unroll
      for (int b = 0; b < NB; ++b) { dots(w[b], ps + b); load_w(w[b], ps + b + NB); }
    }
    switch (npass - ps) {
      case 1: last(ps, std::integral_constant<int, 1>()); break;
      case 2: last(ps, std::integral_constant<int, 2>()); break;
      case 3: last(ps, std::integral_constant<int, 3 < 2 * NB ? 3 : 1>()); break;
      case 4: last(ps, std::integral_constant<int, 4 < 2 * NB ? 4 : 1>()); break;
      case 5: last(ps, std::integral_constant<int, 5 < 2 * NB ? 5 : 1>()); break;
      case 6: last(ps, std::integral_constant<int, 6 < 2 * NB ? 6 : 1>()); break;
      default: last(ps, std::integral_constant<int, 7 < 2 * NB ? 7 : 1>()); break;
    }
    float a = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if constexpr (F8 == WF_E4M3) a *= e_scale;
    if (lane == 0 && valid) {
      const float y = rnd<T>(a + e_bias);
      ((T*)p.Y)[n] = fromf<T>(e_res + y);
    }
    OM_DBG_MAX(7, (blockIdx.x & 7) == 0);
    return;
  }
  wreg_t wa[CP], wb[CP], wc[CP];
  load_w(wa, 0);
  if constexpr (F8 == WF_X12) x12_row_load(xst, p, (size_t)row, lane);      // bf16x12: the row's top and patches right behind the first pass, which needs them
  if (npass > 1) load_w(wb, 1);
  if (npass > 2) load_w(wc, 2);      // all three buffers are on their way before x is staged (round 4: the third used to wait for the barrier below)
  // the epilogue's operands (bias, residual -- which may alias Y: only this wave writes element n --, the e4m3 row scale) right behind the first
  // weight passes: they come back with them instead of costing a dependent L2 round trip after the reduction (no branch around the loads)
  const float e_bias_raw = tof(((const T*)(p.bias ? p.bias : p.X))[p.bias ? row : 0]);
  const float e_res_raw = tof(((const T*)(p.resid ? p.resid : p.X))[p.resid ? row : 0]);
  const float e_bias = p.bias ? e_bias_raw : 0.f, e_res = p.resid ? e_res_raw : 0.f;
  float e_scale = 1.f;
  if constexpr (F8 == WF_E4M3) e_scale = p.w_scale[row];
  // x -> LDS (zero beyond K up to the last whole pass of 8), once per workgroup, under the first passes' weight loads
  for (int i = threadIdx.x; i < npass8 * 8 * 64; i += blockDim.x) {
    const rw_u32x4 z = {0u, 0u, 0u, 0u};
    const rw_u32x4 v = i * 8 < p.K ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + i * 8) : z;
    *reinterpret_cast<rw_u32x4*>(xs + i * 8) = v;
  }
  __syncthreads();
  if constexpr (F8 == WF_X12) x12_row_finish(xst);
  // three register buffers.  In this source the weights of passes ps + 1 and ps + 2 are in flight under the dot products of pass ps; in the
  // machine code the conditions around the loads make every wait a vmcnt(0) behind the newest load (see the head of this body)
  for (int ps = 0; ps < npass; ps += 3) {
    if (ps > 0 && ps + 2 < npass) load_w(wc, ps + 2);
    dots(wa, ps);
    if (ps + 1 < npass) {
      if (ps + 3 < npass) load_w(wa, ps + 3);
      dots(wb, ps + 1);
    }
    if (ps + 2 < npass) {
      if (ps + 4 < npass) load_w(wb, ps + 4);
      dots(wc, ps + 2);
    }
  }
  float a = acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if constexpr (F8 == WF_E4M3) a *= e_scale;
  if (lane == 0 && valid) {
    const float y = rnd<T>(a + e_bias);
    ((T*)p.Y)[n] = fromf<T>(e_res + y);
  }
  OM_DBG_MAX(7, (blockIdx.x & 7) == 0);
}

template <typename T, bool F8>
__global__ __launch_bounds__(512) void gemv_rows_longk_kernel(GemvP p, int rows_per_wg) { gemv_rows_longk_body<T, F8 ? WF_E4M3 : WF_16>(p, rows_per_wg); }
template <typename T>
__global__ __launch_bounds__(512) void gemv_rows_longk_mx4_kernel(GemvP p, int rows_per_wg) { gemv_rows_longk_body<T, WF_MX4>(p, rows_per_wg); }
template <typename T>
__global__ __launch_bounds__(512) void gemv_rows_longk_x12_kernel(GemvP p, int rows_per_wg) { gemv_rows_longk_body<T, WF_X12, 4, 2, 3>(p, rows_per_wg); }

#if OMCHAT_EXPERIMENTS
// The same rows WITHOUT the LDS stage (round 5, tuning key 39): a wave streams one row and uses every x element once, so the LDS copy only saves L2
// reads of x (37 KB, resident in every XCD's L2).  Here a wave loads its x passes from L2 next to its weight passes, two passes in flight:
// no barrier and no shared state, so the workgroups can be as small as one wave and the dispatcher re-deals them over the XCDs as they retire (what
// made the one-pair-per-wave gate|up launch faster).  Same chunk order and the same dot products as the LDS form: bit-identical.
// MEASURED SLOWER (same box, configs[1] decode ms per token): LDS form 2.605; this form as 1 / 2 / 4 waves per workgroup 2.700 / 2.707 / 2.712 -- the
// x registers halve the waves per SIMD (204 VGPRs) and 3584 rows no longer fit one resident round.  Experiments build only.
template <typename T, int F8>
__device__ __forceinline__ void gemv_rows_longk_direct_body(const GemvP& p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nch = (p.K + 511) >> 9, npass = (nch + 7) >> 3;
  const int n = blockIdx.x * (int)(blockDim.x >> 6) + wave;
  if (n >= p.N) return;
  const int row = n;
  typedef typename RwW<F8>::type wreg_t;
  auto load_w = [&](wreg_t (&w)[8], int pass) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int k = (pass * 8 + c) * 512 + lane * 8;
      k = k < p.K ? k : 0;
      w[c] = rw_ldw<T, F8>(p, (size_t)row, k);
    }
  };
  auto load_x = [&](rw_u32x4 (&x)[8], int pass) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int k = (pass * 8 + c) * 512 + lane * 8;
      const rw_u32x4 z = {0u, 0u, 0u, 0u};
      x[c] = k < p.K ? *reinterpret_cast<const rw_u32x4*>((const T*)p.X + k) : z;
    }
  };
  float acc = 0.f;
  auto dots = [&](wreg_t (&w)[8], rw_u32x4 (&x)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      acc = rw_dotw<T, F8>(w[c], x[c], acc);
    }
  };
  wreg_t wa[8], wb[8];
  rw_u32x4 xa[8], xb[8];
  load_w(wa, 0);
  load_x(xa, 0);
  if (npass > 1) { load_w(wb, 1); load_x(xb, 1); }
  const float e_bias_raw = tof(((const T*)(p.bias ? p.bias : p.X))[p.bias ? row : 0]);
  const float e_res_raw = tof(((const T*)(p.resid ? p.resid : p.X))[p.resid ? row : 0]);
  const float e_bias = p.bias ? e_bias_raw : 0.f, e_res = p.resid ? e_res_raw : 0.f;
  float e_scale = 1.f;
  if constexpr (F8 == WF_E4M3) e_scale = p.w_scale[row];
  // two passes of weights and x in flight per wave (128 registers: three to four waves per SIMD); a buffer pair is refilled right after its dot products
  for (int ps = 0; ps < npass; ps += 2) {
    dots(wa, xa);
    if (ps + 2 < npass) { load_w(wa, ps + 2); load_x(xa, ps + 2); }
    if (ps + 1 < npass) {
      dots(wb, xb);
      if (ps + 3 < npass) { load_w(wb, ps + 3); load_x(xb, ps + 3); }
    }
  }
  float a = acc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if constexpr (F8 == WF_E4M3) a *= e_scale;
  if (lane == 0) {
    const float y = rnd<T>(a + e_bias);
    ((T*)p.Y)[n] = fromf<T>(e_res + y);
  }
}

template <typename T, bool F8>
__global__ __launch_bounds__(256) void gemv_rows_longk_direct_kernel(GemvP p) { gemv_rows_longk_direct_body<T, F8 ? WF_E4M3 : WF_16>(p); }
template <typename T>
__global__ __launch_bounds__(256) void gemv_rows_longk_direct_mx4_kernel(GemvP p) { gemv_rows_longk_direct_body<T, WF_MX4>(p); }

#endif

// ---------------------------------------------------------------------------------------------------------
// Host side.  gemv_plan decides which kernel a call takes and with which grid (pure: every shape rule and every refusal, once);
// gemv_launch is the table from such a plan to the kernel instantiation.
// ---------------------------------------------------------------------------------------------------------
// rows (SwiGLU: pairs) per wave of the whole-row batch-1 forms, by weight form.
// rows per wave-group from tools/experiments/tune_rows.hip (MI355X, r01): short outputs (fused qkv) are latency-bound and want the most
// waves (R = 1: 7.8 vs 8.8 us), everything else is flat in R; 4 waves per workgroup beat 8.  fp8 rows are half as many
// bytes: the wide lm_head takes 8 rows per group, the split-K shapes measured flat (o_proj slightly worse) and keep 4.
// quantised weights (e4m3 rows are half as many bytes as 16-bit ones, MXFP4 a quarter): the same launch shapes for both
int rows_per_wave(const GemvArgs& a, int wf, const GemvTuning& t, int n_cu) {
  if (a.norm_w) {          // the norm shared through LDS; 3 (gate, up) pairs per wave: 6 x 7 chunks of weights + the row fit 256 VGPRs
    // bf16x12 rows on the 16-bit launch's default grid: gate|up one pair per wave, everything else four rows per wave
    if (wf == WF_X12) return a.epi == EPI_SWIGLU ? 1 : 4;
    if (a.epi == EPI_NONE) return a.N < 32768 ? 2 : 4;      // qkv: 8 rows (56 KB) per workgroup against 14 KB of x + norm weights
    if (wf == WF_16) return t.gu_rr == 2 || t.gu_rr == 3 ? t.gu_rr : 1;
    return t.gu_rr8 == 2 || t.gu_rr8 == 1 ? t.gu_rr8 : 4;
  }
  if ((a.epi == EPI_NONE || a.epi == EPI_RESID) && a.N < 32768) return 1;      // short outputs: one row per wave (latency-bound)
  if (wf != WF_16) return a.epi == EPI_NONE ? 8 : 4;      // lm_head: 80.7 vs 82.3 us
  // a tensor-parallel rank's gate|up shard (2368 pairs at TP = 8): 4 pairs per wave are 148 workgroups on 256 CUs; one pair per wave
  // gives every CU ~9 waves (round 5)
  return a.epi == EPI_SWIGLU && (t.shard & 4) && a.N / 2 < 16 * n_cu ? 1 : 4;
}
// one row per wave, `waves` per workgroup, when the rows then deal evenly to 2 workgroups per CU (tuning key 17)
bool plan_balanced(GemvPlan& g, int n_out, int waves, const GemvTuning& t, int n_cu) {
  if (!t.rows_balance || n_out != waves * 2 * n_cu) return false;
  g.rr = 1; g.waves = waves; g.gx = 2 * n_cu; g.gy = 1; g.block = 64 * waves;
  return true;
}
void plan_rows(GemvPlan& g, const GemvArgs& a, int ks, const GemvTuning& t, int n_cu) {
  const int n_out = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
  g.family = GF_ROWS; g.waves = 4; g.block = 256; g.gy = ks;
  // o_proj of a batch-1 step: 3584 rows as 896 four-wave workgroups are 3.5 per CU (one CU in two streams a fourth workgroup); as
  // 512 seven-wave workgroups every CU streams the same 14 rows (profiles/r03_r)
  if (g.rr == 1 && a.epi == EPI_RESID && ks == 1 && plan_balanced(g, n_out, 7, t, n_cu)) return;
  g.gx = std::min(2048, cdiv(cdiv(n_out, g.rr), 4));
}
void plan_rows_norm(GemvPlan& g, const GemvArgs& a, const GemvTuning& t, int n_cu) {
  const int n_out = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
  const int chunks = cdiv(a.K, 512);
  g.family = GF_ROWS_NORM; g.waves = 4; g.block = 256; g.nch = chunks >= 1 && chunks <= 7 ? chunks : 8;      // (K = 0 passes the checks: 0 chunks take 8)
  if (g.wf != WF_X12 && g.nch >= 4) {        // the decoder's hidden sizes only (K > 1536): keeps the instantiation count down
    // measured (profiles/r03_p): gate|up 44.3 -> 42.8 us (2.778 -> 2.738 ms per token); qkv 9.2 us either way; e4m3 gate|up 0.6 % slower
    const bool want = a.epi == EPI_SWIGLU ? (t.norm_loop & (g.wf != WF_16 ? 4 : 1)) : (a.N < 32768 ? (t.norm_loop & 2) : (t.norm_loop & 8));
    if (want && n_out >= 8 * n_cu) {
      g.rr = g.waves = 0;
      // dynamic form: the outputs dealt by atomic counters instead of equal shares (the XCDs do not stream at the same rate); tuning key 24
      if (OMCHAT_EXPERIMENTS && a.dyn_ctr && t.dyn) { g.family = GF_ROWS_NORM_DYN; g.gx = 2 * n_cu; return; }
      g.family = GF_ROWS_NORM_LOOP;
      g.per_wg = cdiv(n_out, 2 * n_cu);
      g.skew = (t.skew >= 256u && n_out == g.per_wg * 2 * n_cu && (2 * n_cu) % 8 == 0) ? t.skew : 0u;
      g.gx = cdiv(n_out, g.per_wg);
      return;
    }
    // qkv of a batch-1 step: 4608 rows = 9 x 512: one row per wave, nine waves per workgroup, 2 workgroups per CU (every CU streams 18 rows)
    // instead of 576 workgroups of 8 rows on 4 waves (2.25 per CU)
    if (a.epi == EPI_NONE && g.rr <= 2 && plan_balanced(g, n_out, 9, t, n_cu)) return;
  }
  // (four waves per workgroup: 8 / 16 waves -- fewer repeats of the norm -- measured 2.633 / 2.646 against 2.599 ms per token; down_proj's long-K form
  // with fewer rows per workgroup 2.615-2.765: each workgroup stages the 37 KB x for itself; lm_head with 2 / 1 rows per wave 2.591 against 2.597: noise)
  g.gx = cdiv(cdiv(n_out, g.rr), 4);
  if (OMCHAT_EXPERIMENTS && g.wf != WF_X12 && a.epi == EPI_SWIGLU && g.rr == 1) {
    const int nwg = cdiv(n_out, 4), xs = (int)(t.skew < 256u ? t.skew : 0u);
    if (xs > 0 && nwg % 8 == 0 && n_out % 4 == 0 && xs < nwg / 8) { g.xskew = xs; g.gx = 8 * (nwg / 8 + xs); }
  }
}
// long K in one piece: x through LDS, the result complete when the launch ends
void plan_longk(GemvPlan& g, const GemvArgs& a, const GemvTuning& t, int n_cu) {
  if (OMCHAT_EXPERIMENTS && t.longk_direct > 0) {      // (no bf16x12 instantiation: such rows would go to the 16-bit kernel; gemv_x12_default_forms keeps model.hip from it)
    g.family = GF_ROWS_LONGK_DIRECT; g.waves = std::min(4, t.longk_direct);
    if (g.wf == WF_X12) g.wf = WF_16;
    g.gx = cdiv(a.N, g.waves); g.block = 64 * g.waves;
    return;
  }
  g.family = GF_ROWS_LONGK;
  g.rows_per_wg = std::max(1, std::min(8, cdiv(a.N, 2 * n_cu)));                // two workgroups per CU
  g.gx = cdiv(a.N, g.rows_per_wg); g.block = 64 * g.rows_per_wg;
  g.lds = (cdiv(a.K, 512) + 7) / 8 * 8 * 512 * 2;
}
// packed x, one of the x-stationary persistent forms; false = none fits
bool plan_xs(GemvPlan& g, const GemvArgs& a, int ks, const GemvTuning& t, int n_cu) {
  if (!a.w_packed || t.no_xs) return false;
  g.block = 512; g.nch = 7;
  // long launches with K = 64 * 8 * 7 (= 3584: gate|up, lm_head): x-stationary persistent form, one workgroup per CU, >= 4 units each
  // (units = what one workgroup walks: (gate, up) tile pairs or single tiles; fewer than 4 per workgroup leaves the last round too empty)
  const int tiles = a.N / 16, units = a.epi == EPI_SWIGLU ? a.N / 32 : tiles;
  if (OMCHAT_EXPERIMENTS && ks == 1 && (a.K >> 6) == 56 && a.epi == EPI_RESID) {      // un-split o_proj (+ residual): one tile per workgroup
    g.family = GF_XS; g.gx = tiles;
    return true;
  }
  if (ks == 1 && (a.K >> 6) == 56 && a.N % 32 == 0 && (a.epi == EPI_SWIGLU || a.epi == EPI_NONE) &&
      (units >= 4 * n_cu || (a.epi == EPI_NONE && tiles >= n_cu && tiles <= 2 * n_cu) ||
       ((t.shard & 1) && a.epi == EPI_NONE && tiles < n_cu) || ((t.shard & 8) && a.epi == EPI_SWIGLU && units <= n_cu))) {
    // the fused qkv projection (288 tiles on 256 CUs) cannot give every CU 4 units: it takes HALF as many workgroups as tiles, two tiles
    // each -- x is read 144 times instead of 288 and the second tile's loads run under the first's reduction (13.3 -> 11.7 us at b = 32)
    // a tensor-parallel rank's qkv shard (768 rows = 48 tiles at TP = 8) is shorter than one tile per CU: one tile per workgroup, 48
    // workgroups that each read x once, instead of gemv_pk_kernel's 24 workgroups of two tiles (round 5: 11.4 us -> see DESIGN.md section 6)
    g.family = GF_XS; g.norm = OMCHAT_EXPERIMENTS && a.epi == EPI_SWIGLU && a.norm_w;
    g.gx = units >= 4 * n_cu ? n_cu : (a.epi == EPI_SWIGLU || tiles < n_cu ? units : a.N / 32);
    return true;
  }
  // split-K launch whose chunks cut into ks slices of 40 and 16 (down_proj at TP = 1: 296 = 7 x 40 + 16, ks = 8): same form, one slice per blockIdx.y
  if (a.epi == EPI_PARTIAL && ks > 1 && (a.K >> 6) % 8 == 0 && a.N % 16 == 0) {
    const int q = (a.K >> 6) / 8;                 // chunks per wave over the whole K
    // q = 5 * a5 + 2 * a2 with a5 + a2 == ks
    int a5 = -1;
    for (int i = 0; i <= ks; ++i) if (5 * i + 2 * (ks - i) == q) a5 = i;
    int gx = std::max(1, n_cu / ks);
    // short launches (o_proj: 224 tiles x 2 slices): two tiles per workgroup instead of >= 4 units on every CU (as for qkv)
    if (tiles < 4 * gx && tiles % 2 == 0 && (long)tiles * ks >= n_cu && (long)tiles * ks <= 2L * n_cu) gx = tiles / 2;
    if (a5 >= 0 && (tiles >= 4 * gx || gx == tiles / 2)) {
      g.family = GF_XS_SPLIT; g.nch = 0; g.gx = gx; g.gy = ks; g.n5 = a5;
      return true;
    }
  }
  g.block = g.nch = 0;
  return false;
}
}  // namespace

// Every tuple of template integers that a rule here or in the plan_* helpers can answer must also be listed in gemv_launch below: a tuple
// that is missing there is found at run time only ("the plan names no kernel instantiation"), not by the compiler.
#define OM_NEED(cond, text) do { if (!(cond)) { g.refusal = text; return g; } } while (0)
GemvPlan gemv_plan(int dtype, const GemvArgs& a, const GemvTuning& t, int n_cu) {
  GemvPlan g{};
  OM_NEED(a.b >= 1 && a.b <= 32, "launch_gemv: batch must be 1..32 per call");
  OM_NEED(!a.x_packed || !a.w_scale, "launch_gemv: packed x: 16-bit or MXFP4 weights");
  OM_NEED(!(a.x_packed && a.mx_scale) || (a.w_packed && a.K % 64 == 0), "launch_gemv: packed x with MXFP4 weights: the packed MXFP4 replica (w_packed), K % 64 == 0");
  OM_NEED(!(a.w_scale && a.mx_scale), "launch_gemv: one weight format per launch: e4m3 (w_scale) or MXFP4 (mx_scale)");      // (EPI_RESID: x-stationary form only, checked below)
  OM_NEED(!a.w_packed || (a.x_packed && a.N % 16 == 0), "launch_gemv: packed W needs packed x and N % 16 == 0");
  OM_NEED(!a.y_packed || (a.x_packed && a.epi == EPI_SWIGLU), "launch_gemv: packed y: SwiGLU epilogue of the packed kernel only");
  if (a.mx_scale) OM_NEED(a.K % 32 == 0 && a.ldw % 4 == 0 && a.ldx % 8 == 0, "launch_gemv: MXFP4 weights: K % 32 == 0 (one e8m0 scale per 32 k), ldw (bytes) % 4, ldx % 8");
  else OM_NEED(a.K % 64 == 0 && a.ldw % 8 == 0 && a.ldx % 8 == 0, "launch_gemv: K % 64, ldw % 8, ldx % 8");
  OM_NEED((!a.w_scale && !(a.mx_scale && !a.x_packed)) || a.b == 1, "launch_gemv: fp8 / MXFP4 weights: batch 1 only (MXFP4 at b > 1: packed x and the packed MXFP4 replica)");
  OM_NEED(a.epi == EPI_NONE || a.epi == EPI_RESID || a.epi == EPI_SWIGLU || a.epi == EPI_PARTIAL, "launch_gemv: bad epilogue");
  OM_NEED(a.ksplit <= 1 || a.epi == EPI_PARTIAL, "launch_gemv: ksplit > 1 only with EPI_PARTIAL (fp32 slices)");
  OM_NEED(a.ksplit <= (a.K + 63) / 64, "launch_gemv: ksplit exceeds the number of 64-wide K chunks");
  OM_NEED(a.epi != EPI_RESID || a.resid, "launch_gemv: resid missing");
  OM_NEED(a.epi != EPI_SWIGLU || a.N % 32 == 0, "launch_gemv: SwiGLU needs N % 32 == 0");
  OM_NEED(!(a.out_f32 && a.epi != EPI_NONE), "launch_gemv: fp32 output only with EPI_NONE");
  OM_NEED(dtype == OMCHAT_F16 || dtype == OMCHAT_BF16, "launch_gemv: bad dtype");
  const int ks = a.ksplit > 1 ? a.ksplit : 1;
  const bool mfma = a.force_mfma || t.force_mfma;
  g.epi = a.epi; g.gy = 1;
  g.wf = a.x12_top ? WF_X12 : a.mx_scale ? WF_MX4 : a.w_scale ? WF_E4M3 : WF_16;
  OM_NEED(!(a.norm_w && a.x_packed) || (a.w_packed && ks == 1 && (a.K >> 6) == 56 && a.epi == EPI_SWIGLU && a.N % 32 == 0 && !t.no_xs),
          "launch_gemv: the in-register RMSNorm on packed x exists for the x-stationary gate|up form only (packed W, K = 3584, no split-K)");
  OM_NEED(!(a.epi == EPI_RESID && a.x_packed) || (a.w_packed && ks == 1 && (a.K >> 6) == 56 && a.N % 16 == 0 && a.N / 16 <= n_cu && !t.no_xs),
          "launch_gemv: the batched residual epilogue exists for the x-stationary form only (packed W, K = 3584, N / 16 <= CUs, no split-K)");
  if (a.x_packed) {
    g.nb = a.b > 16 ? 2 : 1;
    if (g.wf == WF_X12) g.wf = WF_16;      // (packed operands carry no bf16x12 form: x12_top is not read)
    OM_NEED(!(a.mx_scale && (a.norm_w || a.epi == EPI_RESID)), "launch_gemv: the batched norm-in-GEMV / residual forms read 16-bit weights only (no MXFP4 instantiation)");
    // the seven-launch batched layer (un-split o_proj + residual, RMSNorm in the gate|up GEMV's registers; round 5) measured SLOWER than the eight
    // launches (configs[2] decode 4.57-4.87 vs 4.28 ms per step: the norm delays the weight stream by ~3 us in every workgroup and the NB = 2
    // form spills 35-120 VGPRs next to the 168 registers that hold x and two weight tiles): compiled with -DOMCHAT_EXPERIMENTS=1 only
    OM_NEED(OMCHAT_EXPERIMENTS || !(a.norm_w || a.epi == EPI_RESID), "launch_gemv: the batched norm-in-GEMV / residual forms need a -DOMCHAT_EXPERIMENTS=1 build");
    if (plan_xs(g, a, ks, t, n_cu)) return g;
    OM_NEED(!a.norm_w, "launch_gemv: packed-x RMSNorm form: gate|up shape outside the x-stationary launch (N / 32 >= 4 CUs)");
    // launch shapes from tools/experiments/tune_gemv32.hip (MI355X): <NTILE, WAVES, UNROLL> per shape class
    g.family = GF_PK; g.wpack = a.w_packed != 0; g.ntile = 2; g.waves = 8; g.unroll = 4;
    if (a.epi == EPI_PARTIAL) {
      // short K slices (a tensor-parallel rank's o_proj: K = 512 = 8 chunks; down_proj: 37 chunks in two slices): one chunk per wave per
      // step so that all eight waves of a workgroup load, and one tile per workgroup so that the grid covers the CUs (round 5)
      const int cps = cdiv(a.K >> 6, ks);
      if ((t.shard & 2) && cps <= 32) { g.ntile = 1; g.unroll = cps <= 8 ? 1 : 2; }
      else if (a.K / ks >= 1536) { g.ntile = 4; g.waves = 4; g.unroll = 2; }
    } else if (a.epi == EPI_NONE && a.N >= 32768) { g.ntile = 4; g.waves = 4; }
    g.gx = cdiv(cdiv(a.N, 16), g.ntile); g.gy = ks; g.block = 64 * g.waves;
    return g;
  }
  if (a.x12_top) {      // bf16x12 rows: the three long launches of the batch-1 step, nothing else
    const bool ok = dtype == OMCHAT_BF16 && a.b == 1 && !a.w_packed && ks == 1 && a.K >= 512 && a.K % 512 == 0 &&
                    a.ldw == a.K / 2 * 3 && a.x12_cnt && a.x12_patch && !a.w_scale && !a.mx_scale && !mfma;
    const bool norm = ok && a.norm_w && (a.epi == EPI_SWIGLU || a.epi == EPI_NONE) && a.K <= RW_MAXC * 512;
    const bool longk = ok && !a.norm_w && a.epi == EPI_RESID && !a.out_f32 && a.K > RW_MAXC * 512 && a.K <= 32768;
    OM_NEED(norm || longk, "launch_gemv: bf16x12 weights: bf16, b == 1, K % 512 == 0, and norm_w with EPI_SWIGLU / EPI_NONE (K <= 4096) or EPI_RESID on 4096 < K <= 32768");
    if (longk) plan_longk(g, a, t, n_cu);
    else { g.rr = rows_per_wave(a, WF_X12, t, n_cu); plan_rows_norm(g, a, t, n_cu); }
    return g;
  }
  if (a.b == 1 && a.epi == EPI_RESID && ks == 1 && !a.out_f32 && a.K > RW_MAXC * 512 && a.K % 8 == 0 && a.K <= 32768 && (!mfma || a.mx_scale)) {
    plan_longk(g, a, t, n_cu);
    return g;
  }
  const bool rows_ok = a.b == 1 && cdiv(cdiv(a.K, 512), ks) <= RW_MAXC;
  OM_NEED(!a.norm_w || (rows_ok && ks == 1 && !mfma && (a.epi == EPI_NONE || a.epi == EPI_SWIGLU)),
          "launch_gemv: the in-register RMSNorm needs the whole-row batch-1 form without split-K (K <= 4096), epilogue NONE / SWIGLU");
  OM_NEED(!(a.w_scale || a.mx_scale) || rows_ok, "launch_gemv: fp8 / MXFP4 weights need b == 1 and <= 8 chunks of 512 per K slice");
  if (rows_ok && (a.w_scale || a.mx_scale || !mfma)) {       // whole-row streaming form
    g.rr = rows_per_wave(a, g.wf, t, n_cu);
    if (a.norm_w) plan_rows_norm(g, a, t, n_cu);
    else plan_rows(g, a, ks, t, n_cu);
    return g;
  }
  // the MFMA form.  Launch shapes measured with tools/experiments/tune_gemv.hip on MI355X (r01): plain loads beat non-temporal ones for this access
  // shape (gate|up 54.9 -> 49.4 us), split-K slices prefer 4 waves x 8 chunks in flight when a slice is short.
  // b > 16: two batch tiles per weight fragment: weights still stream once for b <= 32
  g.family = GF_MFMA; g.nb = a.b > 16 ? 2 : 1; g.waves = 8; g.unroll = 4;
  // wide outputs (lm_head): 2 tiles per workgroup halves the x re-reads
  g.ntile = a.epi == EPI_SWIGLU || (a.epi == EPI_NONE && (g.nb == 2 || a.N >= 16384)) ? 2 : 1;
  if (g.nb == 1 && a.epi == EPI_PARTIAL && a.K / 64 / ks <= 32) { g.waves = 4; g.unroll = 8; }
  if (g.nb == 1 && a.epi == EPI_NONE) g.unroll = 8;
  g.gx = cdiv(a.N, 16 * g.ntile); g.gy = ks; g.block = 64 * g.waves;
  return g;
}
#undef OM_NEED

int gemv_split_k(int b, int K, int H, bool packed, bool down, const GemvTuning& t) {
  // K slices: batch 1 (whole-row streaming form) wants <= 8 chunks of 512 per slice and >= ~2500 waves in the grid;
  // the MFMA form (b > 1) wants ~2-3 workgroups per CU
  // (tools/experiments/tune_rows.hip: down_proj 18944 -> 8 slices 23.3 us vs 5 slices 27.6 us; o_proj is latency-bound, 1-3 slices alike)
  if (b == 1) { const int nch = cdiv(K, 512); return nch >= 16 ? std::min(DEC_KS_MAX, nch) : std::max(1, std::min(3, nch)); }
  // batched o_proj: K = 3584 cuts into two exact slices for the x-stationary form (40 + 16 chunks, gemv_xs_split_kernel) when the packed
  // replica is in use; otherwise ~2 workgroups per CU for the MFMA form
  if (!down && packed && K == 3584) return 2;
  // shard widths of a tensor-parallel rank (round 5): a K of <= 64 chunks is cut into slices of >= 16 chunks only (o_proj K = 512: one
  // slice, down_proj K = 2368: two) -- eight slices of 4-5 chunks left seven of a workgroup's eight waves without a chunk, and every slice
  // is 4 b H bytes that the residual + RMSNorm launch (under TP: the peer exchange) has to read
  if ((t.shard & 2) && K / 64 <= 64) return std::max(1, std::min(DEC_KS_MAX, (K / 64) / 16));
  return std::max(1, std::min(DEC_KS_MAX, std::min(K / 64, (down ? 3 : 1) * cdiv(512, cdiv(H, 16)))));
}

namespace {
template <auto KERNEL, typename... A>
int launch_k(const GemvPlan& g, hipStream_t s, const A&... args) {
  hipLaunchKernelGGL(KERNEL, dim3(g.gx, g.gy), dim3(g.block), (size_t)g.lds, s, args...);
  return 0;
}
// ... after raising the kernel's dynamic-LDS limit to 64 KB, once per device
template <auto KERNEL, typename... A>
int launch_k_lds64(const GemvPlan& g, hipStream_t s, const A&... args) {
  static PerDeviceOnce set;
  if (set.first()) OM_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
  return launch_k<KERNEL>(g, s, args...);
}
// runtime integer -> template argument: f(std::integral_constant<int, V>) for the listed V that equals v; -1 when none does
template <int... V, typename F>
int with_int(int v, F&& f) {
  int rc = -1;
  (void)((v == V ? (rc = f(std::integral_constant<int, V>{}), true) : false) || ...);
  return rc;
}
#define IV(c) decltype(c)::value
// the (epilogue, rows per wave) pairs that rows_per_wave answers without / with norm_w, for 16-bit (q = false) and quantised rows (the norm
// form's one row per wave on EPI_NONE exists as the nine-wave workgroup only).  gemv_launch asks them in a plain `if`, not `if constexpr`, on
// purpose: the library's device code has always held the kernels of the other pairs too (no launch reaches them, and the host compiler drops
// their stubs as dead code), and a discarded branch would take them out of it.
constexpr bool rows_rr(int epi, int rr, bool q) {
  return epi == EPI_NONE ? rr == 1 || rr == (q ? 8 : 4) : epi == EPI_RESID ? rr == 1 || rr == 4 : epi == EPI_SWIGLU ? rr == 4 || (rr == 1 && !q) : rr == 4;
}
constexpr bool norm_rr(int epi, int rr, bool q) { return epi == EPI_NONE ? rr == 2 || rr == 4 : q ? rr == 1 || rr == 2 || rr == 4 : rr <= 3; }

// The only place that names kernel instantiations: the library holds exactly the ones listed here.  -1 = the plan names none.
template <typename T>
int gemv_launch(const GemvPlan& g, const GemvP& p, hipStream_t s) {
  switch (g.family) {
    case GF_MFMA:
#define OM_MFMA(NT_, EPI_, WV_, UN_, NB_)                                                                  \
  if (g.ntile == NT_ && g.epi == EPI_ && g.waves == WV_ && g.unroll == UN_ && g.nb == NB_)                 \
    return launch_k<gemv_kernel<T, NT_, EPI_, WV_, UN_, false, NB_>>(g, s, p)
      OM_MFMA(1, EPI_PARTIAL, 8, 4, 2); OM_MFMA(2, EPI_SWIGLU, 8, 4, 2); OM_MFMA(1, EPI_RESID, 8, 4, 2); OM_MFMA(2, EPI_NONE, 8, 4, 2);
      OM_MFMA(1, EPI_PARTIAL, 4, 8, 1); OM_MFMA(1, EPI_PARTIAL, 8, 4, 1); OM_MFMA(2, EPI_SWIGLU, 8, 4, 1); OM_MFMA(1, EPI_RESID, 8, 4, 1);
      OM_MFMA(2, EPI_NONE, 8, 8, 1); OM_MFMA(1, EPI_NONE, 8, 8, 1);
#undef OM_MFMA
      return -1;
    case GF_PK:
#define OM_PK(NT_, EPI_, WV_, UN_)                                                                         \
  if (g.ntile == NT_ && g.epi == EPI_ && g.waves == WV_ && g.unroll == UN_)                                \
    return with_int<1, 2>(g.nb, [&](auto NB) {                                                             \
      if (g.wf == WF_MX4) return launch_k<gemv_pk_mx4_kernel<T, NT_, EPI_, WV_, UN_, IV(NB)>>(g, s, p);      \
      if (g.wpack) return launch_k<gemv_pk_kernel<T, NT_, EPI_, WV_, UN_, IV(NB), true>>(g, s, p);           \
      return launch_k<gemv_pk_kernel<T, NT_, EPI_, WV_, UN_, IV(NB), false>>(g, s, p);                       \
    })
      OM_PK(2, EPI_SWIGLU, 8, 4); OM_PK(1, EPI_PARTIAL, 8, 1); OM_PK(1, EPI_PARTIAL, 8, 2); OM_PK(4, EPI_PARTIAL, 4, 2); OM_PK(2, EPI_PARTIAL, 8, 4);
      OM_PK(4, EPI_NONE, 4, 4); OM_PK(2, EPI_NONE, 8, 4);
#undef OM_PK
      return -1;
    case GF_XS:
      return with_int<1, 2>(g.nb, [&](auto NB) {
#if OMCHAT_EXPERIMENTS
        if (g.epi == EPI_RESID) return launch_k<gemv_xs_kernel<T, EPI_RESID, IV(NB), 7>>(g, s, p);
        if (g.norm) return launch_k<gemv_xs_kernel<T, EPI_SWIGLU, IV(NB), 7, true>>(g, s, p);
#endif
        return with_int<EPI_SWIGLU, EPI_NONE>(g.epi, [&](auto EPI) {
          if (g.wf == WF_MX4) return launch_k<gemv_xs_mx4_kernel<T, IV(EPI), IV(NB), 7>>(g, s, p);
          return launch_k<gemv_xs_kernel<T, IV(EPI), IV(NB), 7>>(g, s, p);
        });
      });
    case GF_XS_SPLIT:
      return with_int<1, 2>(g.nb, [&](auto NB) {
        if (g.wf == WF_MX4) return launch_k<gemv_xs_split_mx4_kernel<T, IV(NB)>>(g, s, p, g.n5);
        return launch_k<gemv_xs_split_kernel<T, IV(NB)>>(g, s, p, g.n5);
      });
    case GF_ROWS:      // four waves, the rows per wave that rows_per_wave can answer; seven waves for the balanced o_proj
      return with_int<EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_PARTIAL>(g.epi, [&](auto EPI) {
        return with_int<1, 4, 8>(g.rr, [&](auto RR) {
          auto wf = [&](auto WAVES) {
            if (rows_rr(IV(EPI), IV(RR), true)) {
              if (g.wf == WF_MX4) return launch_k<gemv_rows_mx4_kernel<T, IV(EPI), IV(RR), IV(WAVES)>>(g, s, p);
              if (g.wf == WF_E4M3) return launch_k<gemv_rows_kernel<T, IV(EPI), IV(RR), IV(WAVES), true>>(g, s, p);
            }
            if constexpr (IV(RR) != 8) if (rows_rr(IV(EPI), IV(RR), false) && g.wf == WF_16) return launch_k<gemv_rows_kernel<T, IV(EPI), IV(RR), IV(WAVES), false>>(g, s, p);
            return -1;
          };
          if constexpr (IV(EPI) == EPI_RESID && IV(RR) == 1) if (g.waves == 7) return wf(std::integral_constant<int, 7>{});
          return wf(std::integral_constant<int, 4>{});
        });
      });
    case GF_ROWS_NORM:      // four waves; RR = 3 for 16-bit rows only; nine waves for the balanced qkv; bf16x12: one pair or four rows per wave
      return with_int<EPI_SWIGLU, EPI_NONE>(g.epi, [&](auto EPI) {
        return with_int<1, 2, 3, 4, 5, 6, 7, 8>(g.nch, [&](auto NCH) {
          if (g.wf == WF_X12) {
            constexpr int RR = IV(EPI) == EPI_SWIGLU ? 1 : 4;
            if constexpr (std::is_same<T, bf16>::value) if (g.rr == RR) return launch_k<gemv_rows_norm_x12_kernel<bf16, IV(EPI), RR, IV(NCH)>>(g, s, p);
            return -1;
          }
          if constexpr (IV(EPI) == EPI_NONE && IV(NCH) >= 4) if (g.waves == 9 && g.rr == 1) {
            if (g.wf == WF_MX4) return launch_k<gemv_rows_norm_mx4_kernel<T, IV(EPI), 1, IV(NCH), 9>>(g, s, p);
            return g.wf == WF_E4M3 ? launch_k<gemv_rows_norm_kernel<T, IV(EPI), 1, IV(NCH), true, 9>>(g, s, p) : launch_k<gemv_rows_norm_kernel<T, IV(EPI), 1, IV(NCH), false, 9>>(g, s, p);
          }
          return with_int<1, 2, 3, 4>(g.rr, [&](auto RR) {
            if constexpr (IV(RR) != 3) if (norm_rr(IV(EPI), IV(RR), true)) {
              if (g.wf == WF_MX4) return launch_k<gemv_rows_norm_mx4_kernel<T, IV(EPI), IV(RR), IV(NCH)>>(g, s, p);
              if (g.wf == WF_E4M3) return launch_k<gemv_rows_norm_kernel<T, IV(EPI), IV(RR), IV(NCH), true>>(g, s, p);
            }
            if (norm_rr(IV(EPI), IV(RR), false) && g.wf == WF_16) return launch_k<gemv_rows_norm_kernel<T, IV(EPI), IV(RR), IV(NCH), false>>(g, s, p);
            return -1;
          });
        });
      });
    case GF_ROWS_NORM_LOOP:
      return with_int<EPI_SWIGLU, EPI_NONE>(g.epi, [&](auto EPI) {
        return with_int<4, 5, 6, 7, 8>(g.nch, [&](auto NCH) {
          if (g.wf == WF_MX4) return launch_k<gemv_rows_norm_loop_mx4_kernel<T, IV(EPI), IV(NCH)>>(g, s, p, g.per_wg, g.skew);
          return g.wf == WF_E4M3 ? launch_k<gemv_rows_norm_loop_kernel<T, IV(EPI), IV(NCH), true>>(g, s, p, g.per_wg, g.skew) : launch_k<gemv_rows_norm_loop_kernel<T, IV(EPI), IV(NCH), false>>(g, s, p, g.per_wg, g.skew);
        });
      });
    case GF_ROWS_LONGK:
      if (g.wf == WF_X12) {
        if constexpr (std::is_same<T, bf16>::value) return launch_k_lds64<gemv_rows_longk_x12_kernel<T>>(g, s, p, g.rows_per_wg);
        return -1;
      }
      if (g.wf == WF_MX4) return launch_k_lds64<gemv_rows_longk_mx4_kernel<T>>(g, s, p, g.rows_per_wg);
      return g.wf == WF_E4M3 ? launch_k_lds64<gemv_rows_longk_kernel<T, true>>(g, s, p, g.rows_per_wg) : launch_k_lds64<gemv_rows_longk_kernel<T, false>>(g, s, p, g.rows_per_wg);
#if OMCHAT_EXPERIMENTS
    case GF_ROWS_NORM_DYN:
      return with_int<EPI_SWIGLU, EPI_NONE>(g.epi, [&](auto EPI) {
        return with_int<4, 5, 6, 7, 8>(g.nch, [&](auto NCH) {
          if (g.wf == WF_MX4) return launch_k<gemv_rows_norm_dyn_mx4_kernel<T, IV(EPI), IV(NCH)>>(g, s, p);
          return g.wf == WF_E4M3 ? launch_k<gemv_rows_norm_dyn_kernel<T, IV(EPI), IV(NCH), true>>(g, s, p) : launch_k<gemv_rows_norm_dyn_kernel<T, IV(EPI), IV(NCH), false>>(g, s, p);
        });
      });
    case GF_ROWS_LONGK_DIRECT:
      if (g.wf == WF_MX4) return launch_k<gemv_rows_longk_direct_mx4_kernel<T>>(g, s, p);
      return g.wf == WF_E4M3 ? launch_k<gemv_rows_longk_direct_kernel<T, true>>(g, s, p) : launch_k<gemv_rows_longk_direct_kernel<T, false>>(g, s, p);
#endif
  }
  return -1;
}
}  // namespace

const GemvTuning& gemv_tuning() { return g_tune; }
void gemv_set_force_mfma(int v) { g_tune.force_mfma = v; }
int gemv_get_force_mfma() { return g_tune.force_mfma; }
void gemv_set_no_xs(int v) { g_tune.no_xs = v; }
void gemv_set_shard_shapes(int v) { g_tune.shard = v; }
int gemv_get_shard_shapes() { return g_tune.shard; }
void gemv_set_norm_loop(int v) { g_tune.norm_loop = v; }
void gemv_set_gu_rr(int v) { if (v >= 16) g_tune.gu_rr8 = v / 16; else g_tune.gu_rr = v; }
void gemv_set_dyn(int v) { g_tune.dyn = v; }
void gemv_set_longk_direct(int v) { g_tune.longk_direct = v; }
void gemv_set_skew(int v) { g_tune.skew = (unsigned)v; }
void gemv_set_rows_balance(int v) { g_tune.rows_balance = v; }
int gemv_x12_default_forms() {
  return ((g_tune.norm_loop & 1) == 0 && g_tune.gu_rr == 1 && g_tune.skew == 0u ? 1 : 0) | (g_tune.longk_direct == 0 ? 2 : 0) | ((g_tune.norm_loop & 8) == 0 ? 4 : 0);
}

namespace {
// one wave per row: absmax, then e4m3 (round to nearest even) of w / scale, 8 weights per lane per step
template <typename T>
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const T* __restrict__ W, int ldw, int N, int K, unsigned char* __restrict__ W8, int ldq,
                                                             float* __restrict__ scale) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const T* w = W + (size_t)n * ldw;
  float m = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const typename V8<T>::type v = ld8<T>(w + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(tof(v[j])));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const float sc = m > 0.f ? m / 448.0f : 1.0f;
  if (lane == 0) scale[n] = sc;
  for (int k = lane * 8; k < K; k += 512) {
    const typename V8<T>::type v = ld8<T>(w + k);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = tof(v[j]) / sc;
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    rw_u32x2 o2 = {(unsigned)lo, (unsigned)hi};
    *reinterpret_cast<rw_u32x2*>(W8 + (size_t)n * ldq + k) = o2;
  }
}
}  // namespace

int launch_quant_fp8_rows(int dtype, const void* W, int ldw, int N, int K, void* W8, int ld8, float* scale, hipStream_t s) {
  OM_CHECK(K % 8 == 0 && ldw % 8 == 0 && ld8 % 8 == 0, "K, ldw, ld8 must be multiples of 8");
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(quant_fp8_rows_kernel<f16>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const f16*)W, ldw, N, K, (unsigned char*)W8, ld8, scale);
  else if (dtype == OMCHAT_BF16) hipLaunchKernelGGL(quant_fp8_rows_kernel<bf16>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const bf16*)W, ldw, N, K, (unsigned char*)W8, ld8, scale);
  else { omchat_set_error("launch_quant_fp8_rows: bad dtype"); return 1; }
  OM_LAUNCH_CHECK();
  return 0;
}

namespace {
// MXFP4 quantiser (kernels.h: launch_quant_mxfp4_rows).  One wave per row, 8 weights per lane per step: the four lanes of a block of 32 share
// the absmax.  The exponent comes from the bits of the fp32 absmax (no log2f): floor(log2(m)) = exponent field - 127 for a normal m; a
// subnormal m lies below 2^-126, where e clamps to -127 anyway.  w / 2^e is exact (a power of two), and the code is the count of rounding
// thresholds below |w| / 2^e -- the midpoints of {0, .5, 1, 1.5, 2, 3, 4, 6}, each tie going to the even code -- so 7 and above saturate at 6.
template <typename T>
__global__ __launch_bounds__(256) void quant_mxfp4_rows_kernel(const T* __restrict__ W, int ldw, int N, int K, unsigned char* __restrict__ W4, int ld4,
                                                               unsigned char* __restrict__ S) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const T* w = W + (size_t)n * ldw;
  for (int k = lane * 8; k < K; k += 512) {      // K % 32 == 0: the four lanes of a block are in the loop together
    const typename V8<T>::type v = ld8<T>(w + k);
    float f[8], m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = tof(v[j]); m = fmaxf(m, fabsf(f[j])); }
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    m = fmaxf(m, __shfl_xor(m, 2, 64));
    const int field = (int)((__float_as_uint(m) >> 23) & 0xffu);
    int e = field - 127 - 2;
    e = e < -127 ? -127 : e;
    if (m == 0.f) e = 0;
    const float inv = ldexpf(1.0f, -e);           // 2^-e, e in [-127, 125]: a normal fp32
    unsigned codes = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = fabsf(f[j]) * inv;
      const unsigned c = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) + (unsigned)(a > 2.5f) +
                         (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
      const unsigned sgn = (c != 0u && f[j] < 0.f) ? 8u : 0u;
      codes |= (c | sgn) << (4 * j);
    }
    *reinterpret_cast<unsigned*>(W4 + (size_t)n * ld4 + (k >> 1)) = codes;
    if ((lane & 3) == 0) S[(size_t)n * (K >> 5) + (k >> 5)] = (unsigned char)(e + 127);
  }
}
}  // namespace

int launch_quant_mxfp4_rows(int dtype, const void* W, int ldw, int N, int K, void* W4, int ld4, unsigned char* S, hipStream_t s) {
  OM_CHECK(W && W4 && S, "null argument");
  OM_CHECK(N >= 1 && K >= 32 && K % 32 == 0, "MXFP4: K must be a multiple of 32 (one e8m0 scale per 32 consecutive k)");
  OM_CHECK(ldw % 8 == 0 && ld4 % 4 == 0 && ld4 >= K / 2, "ldw % 8, ld4 (bytes) % 4 and >= K / 2");
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(quant_mxfp4_rows_kernel<f16>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const f16*)W, ldw, N, K, (unsigned char*)W4, ld4, S);
  else if (dtype == OMCHAT_BF16) hipLaunchKernelGGL(quant_mxfp4_rows_kernel<bf16>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const bf16*)W, ldw, N, K, (unsigned char*)W4, ld4, S);
  else { omchat_set_error("launch_quant_mxfp4_rows: bad dtype"); return 1; }
  OM_LAUNCH_CHECK();
  return 0;
}

namespace {
// bf16x12 encoder (kernels.h: launch_encode_bf16x12; tests/bf16x12_ref.py is the definition).  One workgroup of one wave per row: the
// row's top, then per chunk of 512 the lane's 8 low bytes and its nibble word; the misses of a chunk (rare) take their slots of the patch
// list in k order through a scan over the lanes.
__global__ __launch_bounds__(64) void encode_bf16x12_kernel(const unsigned short* __restrict__ W, int ldw, int N, int K, unsigned char* __restrict__ coded,
                                                            unsigned char* __restrict__ top, unsigned char* __restrict__ cnt, unsigned* __restrict__ patch,
                                                            int* __restrict__ over) {
  const int lane = threadIdx.x, n = blockIdx.x;
  const unsigned short* w = W + (size_t)n * ldw;
  int t = 0;
  for (int k = lane * 8; k < K; k += 512) {
    const rw_u32x4 v = *reinterpret_cast<const rw_u32x4*>(w + k);
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = (int)((u[i >> 1] >> (16 * (i & 1) + 7)) & 0xffu);
      if (e != 0xff) t = max(t, e >> 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t = max(t, __shfl_xor(t, o, 64));
  unsigned char* row = coded + (size_t)n * (size_t)(K / 512) * 768;
  int total = 0;
  for (int c = 0; c < K / 512; ++c) {
    const int k0 = c * 512 + lane * 8;
    const rw_u32x4 v = *reinterpret_cast<const rw_u32x4*>(w + k0);
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
    unsigned lo0 = 0, lo1 = 0, nib = 0, mm = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned h = (u[i >> 1] >> (16 * (i & 1))) & 0xffffu;
      const int e = (int)((h >> 7) & 0xffu), e71 = e >> 1, cc = e71 - (t - 7);
      const bool hit = e != 0xff && (e71 == 0 || cc >= 1);
      const unsigned code = e71 == 0 ? 0u : (unsigned)cc;
      if (hit) {
        if (i < 4) lo0 |= (h & 0xffu) << (8 * i); else lo1 |= (h & 0xffu) << (8 * (i - 4));
        nib |= (((h >> 15) << 3) | code) << (8 * (i & 3) + 4 * (i >> 2));
      } else {
        mm |= 1u << i;
      }
    }
    const rw_u32x2 lo = {lo0, lo1};
    *reinterpret_cast<rw_u32x2*>(row + (size_t)c * 768 + lane * 8) = lo;
    *reinterpret_cast<unsigned*>(row + (size_t)c * 768 + 512 + lane * 4) = nib;
    if (__ballot(mm != 0u)) {
      const int pc = __popc(mm);
      int inc = pc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
      int off = total + inc - pc;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if ((mm >> i) & 1u) {
          const unsigned h = (u[i >> 1] >> (16 * (i & 1))) & 0xffffu;
          if (off < 32) patch[(size_t)n * 32 + off] = ((unsigned)(k0 + i) << 16) | h;
          ++off;
        }
      }
      total += __shfl(inc, 63, 64);
    }
  }
  if (lane < 32 && lane >= total) patch[(size_t)n * 32 + lane] = 0u;      // the unused slots read zero
  if (lane == 0) {
    top[n] = (unsigned char)t;
    cnt[n] = (unsigned char)(total > 32 ? 33 : total);
    if (total > 32) *over = 1;
  }
}
}  // namespace

int launch_encode_bf16x12(const void* W, int ldw, int N, int K, void* coded, unsigned char* top, unsigned char* cnt, unsigned* patch, int* over, hipStream_t s) {
  OM_CHECK(W && coded && top && cnt && patch && over, "null argument");
  OM_CHECK(N >= 1 && K >= 512 && K % 512 == 0 && K < 65536 && ldw % 8 == 0 && ldw >= K, "bf16x12: K a multiple of 512 below 65536, ldw % 8 == 0");
  hipLaunchKernelGGL(encode_bf16x12_kernel, dim3(N), dim3(64), 0, s, (const unsigned short*)W, ldw, N, K, (unsigned char*)coded, top, cnt, patch, over);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_pack_x(int dtype, const void* X, int ldx, int b, int K, void* out, hipStream_t s) {
  OM_CHECK(b >= 1 && b <= 32 && K % 64 == 0 && ldx % 8 == 0, "pack_x: 1 <= b <= 32, K % 64, ldx % 8");
  const int NB = b > 16 ? 2 : 1;
  const int grid = cdiv(NB * 16 * (K / 8), 256);
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(pack_x_kernel<f16>, dim3(grid), dim3(256), 0, s, (const f16*)X, ldx, b, K, (f16*)out, NB);
  else if (dtype == OMCHAT_BF16) hipLaunchKernelGGL(pack_x_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)X, ldx, b, K, (bf16*)out, NB);
  else { omchat_set_error("launch_pack_x: bad dtype"); return 1; }
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_pack_w4(const void* W4, const unsigned char* S, int N, int K, void* W4P, unsigned char* SP, hipStream_t s) {
  OM_CHECK(W4 && S && W4P && SP, "null argument");
  OM_CHECK(N >= 16 && N % 16 == 0, "pack_w4: N % 16 == 0 (16-row weight tiles)");
  OM_CHECK(K >= 64 && K % 64 == 0, "pack_w4: K % 64 == 0 (64-wide K chunks)");
  const long n8 = (long)N * (K / 8);
  const int grid = (int)(cdiv64(n8, 256) > 8192 ? 8192 : cdiv64(n8, 256));
  hipLaunchKernelGGL(pack_w4_kernel, dim3(grid), dim3(256), 0, s, (const unsigned char*)W4, S, N, K, (unsigned*)W4P, SP);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_pack_w(int dtype, const void* W, int ldw, int N, int K, void* out, hipStream_t s) {
  OM_CHECK(N % 16 == 0 && K % 64 == 0 && ldw % 8 == 0, "pack_w: N % 16, K % 64, ldw % 8");
  const long n8 = (long)N * (K / 8);
  const int grid = (int)(cdiv64(n8, 256) > 8192 ? 8192 : cdiv64(n8, 256));
  if (dtype == OMCHAT_F16) hipLaunchKernelGGL(pack_w_kernel<f16>, dim3(grid), dim3(256), 0, s, (const f16*)W, ldw, N, K, (f16*)out);
  else if (dtype == OMCHAT_BF16) hipLaunchKernelGGL(pack_w_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)W, ldw, N, K, (bf16*)out);
  else { omchat_set_error("launch_pack_w: bad dtype"); return 1; }
  OM_LAUNCH_CHECK();
  return 0;
}

#if OMCHAT_EXPERIMENTS
// PROTOTYPE (round 5, tuning key 42): the batch-1 o_proj GEMV launched OUT OF ORDER behind the split-KV merge (hipExtAnyOrderLaunch: its workgroups are
// placed as soon as the merge's are) -- every wave issues its weight row first, wave 0 then polls the merge's per-head completion flags (epoch values,
// written after an agent-scope release by each merge workgroup), the workgroup acquires and only then loads the attention row.  One row per wave, K = NCH x 512
// in one piece, residual in the epilogue: the same chunk order and dot products as gemv_rows_kernel<EPI_RESID> -- the same bits.
template <typename T, int NCH>
__global__ __launch_bounds__(448) void gemv_rows_wait_kernel(GemvP p, const unsigned* flags, unsigned epoch, int nflags, unsigned* err, int mode) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x * (int)(blockDim.x >> 6) + wave;
  const bool valid = n < p.N;
  const int row = valid ? n : p.N - 1;
  OM_DBG_MIN(1, blockIdx.x < 8);
  rw_u32x4 w[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) w[c] = __builtin_nontemporal_load(reinterpret_cast<const rw_u32x4*>((const T*)p.W + (size_t)row * p.ldw + c * 512 + lane * 8));
  const float e_res = tof(((const T*)p.resid)[row]);
  __builtin_amdgcn_sched_barrier(0);
  if (wave == 0) {
    const unsigned long long t0 = wall_clock64();
    unsigned spins = 0;
    for (;;) {
      const unsigned f = lane < nflags ? __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
      if (__all(f == epoch)) break;
      if (mode & 8) __builtin_amdgcn_s_sleep(32); else __builtin_amdgcn_s_sleep(1);      // mode bit 3: ~1 us between polls instead of ~30 ns
      if ((++spins & 255u) == 0u && wall_clock64() - t0 > 200000000ull) { if (lane == 0) atomicOr(err, 4u); break; }      // 2 s of the 100 MHz clock
    }
  }
  OM_DBG_MAX(2, blockIdx.x < 8);
  __syncthreads();
  rw_u32x4 xr[NCH];
  if (mode & 2) {
    // mode bit 1: the attention row by cache-bypassing loads (sc0 sc1) instead of an agent-scope acquire (buffer_inv sc1 in 3584 waves) in front of plain loads
    const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.X), 0, NCH * 1024, 0x00020000);
#pragma unroll
    for (int c = 0; c < NCH; ++c) xr[c] = __builtin_bit_cast(rw_u32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, c * 1024 + lane * 16, 0, 17));
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int c = 0; c < NCH; ++c) xr[c] = *reinterpret_cast<const rw_u32x4*>((const T*)p.X + c * 512 + lane * 8);
  }
  float a = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) a = rw_dot8<T>(w[c], xr[c], a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0 && valid) ((T*)p.Y)[n] = fromf<T>(e_res + rnd<T>(a));
  OM_DBG_MAX(3, (blockIdx.x & 7) == 0);
}

template <typename T>
static int launch_gemv_wait_t(const GemvArgs& a, const unsigned* flags, unsigned epoch, int nflags, unsigned* err, int mode, hipStream_t s) {
  GemvP p{a.X, a.W, a.Y, a.bias, a.resid, a.ldx, a.ldw, a.ldy, a.ldr, a.b, a.N, a.K, 0, 1, nullptr, 0, nullptr, 0.f, nullptr, nullptr, a.dbg};
  int wpw = cdiv(a.N, 2 * device_cus());
  wpw = wpw < 1 ? 1 : (wpw > 7 ? 7 : wpw);
  hipExtLaunchKernelGGL((gemv_rows_wait_kernel<T, 7>), dim3(cdiv(a.N, wpw)), dim3(64 * wpw), 0, s, nullptr, nullptr, hipExtAnyOrderLaunch, p, flags, epoch, nflags, err, mode);
  OM_LAUNCH_CHECK();
  return 0;
}
#endif

// experiments build: see gemv_rows_wait_kernel.  Requirements: b = 1, K = 3584, 16-bit weights, EPI_RESID without bias, nflags <= 64.
int launch_gemv_wait(int dtype, const GemvArgs& a, const unsigned* flags, unsigned epoch, int nflags, unsigned* err, int mode, hipStream_t s) {
#if OMCHAT_EXPERIMENTS
  OM_CHECK(a.b == 1 && a.K == 3584 && !a.w_scale && a.epi == EPI_RESID && !a.bias && a.resid && !a.x_packed && nflags >= 1 && nflags <= 64 && flags && err,
           "launch_gemv_wait: batch 1, K = 3584, 16-bit weights, residual epilogue without bias");
  if (dtype == OMCHAT_F16) return launch_gemv_wait_t<f16>(a, flags, epoch, nflags, err, mode, s);
  if (dtype == OMCHAT_BF16) return launch_gemv_wait_t<bf16>(a, flags, epoch, nflags, err, mode, s);
  omchat_set_error("bad dtype");
  return 1;
#else
  (void)dtype; (void)a; (void)flags; (void)epoch; (void)nflags; (void)err; (void)mode; (void)s;
  omchat_set_error("launch_gemv_wait: -DOMCHAT_EXPERIMENTS=1 builds only");
  return 1;
#endif
}

int launch_gemv(int dtype, const GemvArgs& a, hipStream_t s) {
  const GemvPlan g = gemv_plan(dtype, a, g_tune, device_cus());
  if (g.refusal) { omchat_set_error(g.refusal); return 1; }
  GemvP p{a.X, a.W, a.Y, a.bias, a.resid, a.ldx, a.ldw, a.ldy, a.ldr, a.b, a.N, a.K, a.out_f32, a.ksplit > 1 ? a.ksplit : 1, a.w_scale, a.y_packed, a.norm_w, a.norm_eps,
          (unsigned*)a.dyn_ctr, a.y_pack, a.dbg, a.mx_scale, a.x12_top, a.x12_cnt, a.x12_patch};
#if OMCHAT_EXPERIMENTS
  p.xskew = g.xskew;
#endif
  const int rc = dtype == OMCHAT_F16 ? gemv_launch<f16>(g, p, s) : gemv_launch<bf16>(g, p, s);
  if (rc < 0) { omchat_set_error("launch_gemv: the plan names no kernel instantiation"); return 1; }
  if (rc) return rc;
  OM_LAUNCH_CHECK();
  return 0;
}

