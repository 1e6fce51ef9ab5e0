// Teacher-forced scoring: log p(label | row) for given labels without the [rows, V] logits.  launch_gemm with EPI_LSE
// leaves, per row and 64-column slot of the vocabulary, the online pair (max, sum exp(x - max)) of the raw fp32 logits, and the label's own
// logit; here one wave per row folds the slots and a single workgroup reduces the rows to the loss sums.  No float atomics and no
// arrival-order folds anywhere: two runs give the same bits.  tests/score_ref.py is the fp64 restatement.
#include "kernels.h"
#include <math.h>

namespace {

constexpr int SC_IGNORE = -100;      // IGNORE_INDEX of the reference (omchat/constants.py)

// One wave per row (four rows a workgroup).  Lane l folds the slots l, l + 64, ... in ascending order, the 64 lanes meet by the fixed xor tree.
// part: slot-major planes, part[(2 * slot) * ld + row] = max, part[(2 * slot + 1) * ld + row] = sum
__global__ __launch_bounds__(256) void score_finish_kernel(const float* part, int ld, int nslots, const int* labels, const float* tgt, int M, int N,
                                                          float* logprob, float* lse) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                                          // wave-uniform
  float m = -INFINITY, s = 0.f;
  for (int sl = lane; sl < nslots; sl += 64) lse_merge(m, s, part[(size_t)(2 * sl) * ld + row], part[(size_t)(2 * sl + 1) * ld + row]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane != 0) return;
  const float l = __fadd_rn(m, logf(s));
  if (lse) lse[row] = l;
  const int lab = labels[row];
  // (a label outside {-100} u [0, N) is refused on the host; should one arrive, it is scored NaN rather than silently ignored)
  logprob[row] = lab == SC_IGNORE ? 0.f : (lab >= 0 && lab < N ? __fsub_rn(tgt[row], l) : NAN);
}

// 256-thread fixed tree over LDS: every thread ends with the same two sums
__device__ __forceinline__ void block_sum2(float& a, float& c, float* sh) {
  const int t = threadIdx.x;
  __syncthreads();                                                               // the previous use of sh is over
  sh[t] = a; sh[256 + t] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { sh[t] = __fadd_rn(sh[t], sh[t + o]); sh[256 + t] = __fadd_rn(sh[256 + t], sh[256 + t + o]); }
    __syncthreads();
  }
  a = sh[0]; c = sh[256];
}

// one workgroup: sequence by sequence, thread t takes the rows t, t + 256, ... in ascending order, then the tree; the sequences' sums are added
// in sequence order.  Counts are exact in fp32 (rows <= max_prefill_rows < 2^24)
__global__ __launch_bounds__(256) void score_reduce_kernel(const float* logprob, const int* labels, int b, int S, float* out) {
  __shared__ float sh[512];
  float total = 0.f, count = 0.f;
  for (int i = 0; i < b; ++i) {
    float a = 0.f, c = 0.f;
    for (int t = threadIdx.x; t < S; t += 256) {
      const size_t r = (size_t)i * S + t;
      if (labels[r] != SC_IGNORE) { a = __fadd_rn(a, logprob[r]); c += 1.f; }
    }
    block_sum2(a, c, sh);
    if (threadIdx.x == 0) { out[2 + i] = a; out[2 + b + i] = c; }
    total = __fadd_rn(total, a); count += c;
  }
  if (threadIdx.x == 0) { out[0] = -total; out[1] = count; }
}

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace

// [2 * cdiv(N, 64)][ld = M rounded up to 16 rows] (max, sum) planes, then the [M] target logits
size_t score_ws_bytes(int M, int N) {
  const size_t ld = align16((size_t)M);
  return (size_t)2 * cdiv(N, 64) * ld * 4 + align16((size_t)M * 4);
}

int launch_score(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int* labels, float* logprob, float* lse,
                 void* ws, size_t ws_bytes, hipStream_t s) {
  OM_CHECK(A && W && labels && logprob && ws, "null argument");
  OM_CHECK(M >= 1 && N >= 1 && K >= 1, "empty problem");
  OM_CHECK(ws_bytes >= score_ws_bytes(M, N) && ((uintptr_t)ws & 15) == 0, "workspace: score_ws_bytes(M, N) bytes, 16-byte aligned");
  const int ld = (int)align16((size_t)M), nslots = cdiv(N, 64);
  float* part = (float*)ws;
  float* tgt = part + (size_t)2 * nslots * ld;
  GemmArgs g{A, lda, W, ldw, nullptr, 0, M, N, K, nullptr, nullptr, nullptr, 0, EPI_LSE, 0, nullptr, 0, -1};
  g.stats = part; g.stats_ld = ld; g.lse_labels = labels; g.lse_tgt = tgt;
  if (int rc = launch_gemm(dtype, g, s)) return rc;
  hipLaunchKernelGGL(score_finish_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, part, ld, nslots, labels, tgt, M, N, logprob, lse);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_score_reduce(const float* logprob, const int* labels, int b, int S, float* out, hipStream_t s) {
  OM_CHECK(logprob && labels && out && b >= 1 && S >= 1, "bad argument");
  hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(256), 0, s, logprob, labels, b, S, out);
  OM_LAUNCH_CHECK();
  return 0;
}
