// On-device HF logits constraints for generate(): no_repeat_ngram_size, bad_words_ids, min_new_tokens / min_length, suppress_tokens and
// begin_suppress_tokens.  All of them set logits to -inf, so one ban stage in front of the pick is exact for the argmax
// and for the sampler.  Two launches per pick: the ban pass computes, per row, the bitmap of rank-local ids HF's processors would exclude
// given the row's token history; the apply pass writes a copy of the logits with those ids at -inf -- the existing picks then run on the
// copy unchanged, the caller's logits are never written -- and clears the words it read, so the bitmap is all-zero between picks without a
// memset.  tests/constraints_ref.py is the CPU restatement, pinned to HF's own processors.
#include "kernels.h"
#include <math.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int CON_CH = 8;          // workgroups per row of the ban pass (they stride the history)
constexpr int CON_TILE = 2048;     // logits per workgroup of the apply pass = 64 bitmap words, owned by that workgroup alone

// ids outside the vocabulary (the -200 image sentinel) are never banned; other ranks' ids are theirs to ban
__device__ __forceinline__ void con_ban(uint32_t* bm, int id, int gbase, int V, int V_total) {
  if (id < 0 || id >= V_total) return;
  const int li = id - gbase;
  if (li < 0 || li >= V) return;
  atomicOr(&bm[li >> 5], 1u << (li & 31));
}

// The history HF's processors see at this pick is hist[0, len) plus, on a decode step, the token the step is fed (tok != NULL): every
// workgroup reads that id from `tok`, workgroup 0 also stores it at hist[len]; the apply pass advances len behind this launch.
__global__ __launch_bounds__(256) void con_ban_kernel(ConstrainArgs a) {
  const int row = blockIdx.y, t = threadIdx.x;
  int32_t* h = a.hist + (size_t)row * a.hist_ld;
  const int Lm = a.len[row];
  const bool fed = a.tok != nullptr && Lm < a.hist_ld;
  const int tk = fed ? a.tok[row] : 0;
  const int L = Lm + (fed ? 1 : 0);
  uint32_t* bm = a.ban + (size_t)row * a.bmw;
  auto H = [&](int i) { return i < Lm ? h[i] : tk; };
  const int n = a.ngram;
  // NoRepeatNGramLogitsProcessor: every start i in [0, L - n] whose n - 1 ids equal the last n - 1 ids bans the id behind them
  if (n >= 1 && L + 1 >= n) {
    __shared__ int tail[CON_NGRAM_MAX];
    for (int j = t; j < n - 1; j += 256) tail[j] = H(L - (n - 1) + j);
    __syncthreads();
    const int last = L - n;
    for (int i0 = (blockIdx.x * 256 + t) * 4; i0 <= last; i0 += CON_CH * 256 * 4) {
      int v[4];
      if (i0 + 3 < Lm) {      // rows start 16-byte aligned and hist_ld % 4 == 0
        const int4 q = *(const int4*)(h + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i0 + e < L ? H(i0 + e) : 0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e;
        if (i > last) break;
        if (n == 1) { con_ban(bm, v[e], a.gbase, a.V, a.V_total); continue; }
        if (v[e] != tail[0]) continue;
        bool same = true;
        for (int j = 1; j < n - 1 && same; ++j) same = H(i + j) == tail[j];
        if (same) con_ban(bm, H(i + n - 1), a.gbase, a.V, a.V_total);
      }
    }
  }
  // the row's seen set (the repetition penalty of a beam search on processed scores, beam.hip): every id of the history, in a bitmap of its own
  if (a.seen) {
    uint32_t* sb = a.seen + (size_t)row * a.bmw;
    for (int i = blockIdx.x * 256 + t; i < L; i += CON_CH * 256) con_ban(sb, H(i), a.gbase, a.V, a.V_total);
  }
  if (blockIdx.x != 0) return;
  // NoBadWordsLogitsProcessor: a word of m ids bans its last id when the m - 1 ids in front equal the history's tail; m = 1 always bans,
  // words longer than the history are skipped
  for (int w = t; w < a.n_bw; w += 256) {
    const int o = a.bw_off[w], m = a.bw_off[w + 1] - o;
    if (m < 1 || (m > 1 && m > L)) continue;
    bool same = true;
    for (int j = 0; j < m - 1 && same; ++j) same = H(L - (m - 1) + j) == a.bw_ids[o + j];
    if (same) con_ban(bm, a.bw_ids[o + m - 1], a.gbase, a.V, a.V_total);
  }
  const int P = a.plen[row];
  // MinNewTokensLength / MinLength: the EOS ids; SuppressTokens; SuppressTokensAtBegin at the first generated position
  if (L - P < a.min_new || L < a.min_len)
    for (int j = t; j < a.n_eos; j += 256) con_ban(bm, a.eos[j], a.gbase, a.V, a.V_total);
  for (int j = t; j < a.n_sup; j += 256) con_ban(bm, a.sup[j], a.gbase, a.V, a.V_total);
  if (L == P)
    for (int j = t; j < a.n_bsup; j += 256) con_ban(bm, a.bsup[j], a.gbase, a.V, a.V_total);
  if (fed && t == 0) h[Lm] = tk;
}

// out = logits with the banned ids at -inf; the bitmap words of the tile are read once into LDS and cleared by the thread that read them
template <bool VEC>
__global__ __launch_bounds__(256) void con_apply_kernel(const float* logits, int ld, int V, uint32_t* ban, int bmw, float* out, int* len,
                                                        int hist_ld) {
  __shared__ uint32_t w[CON_TILE / 32];
  const int row = blockIdx.y, t = threadIdx.x, t0 = blockIdx.x * CON_TILE;
  uint32_t* bm = ban + (size_t)row * bmw;
  if (t < CON_TILE / 32) {
    const int wi = t0 / 32 + t;
    const uint32_t x = wi < bmw ? bm[wi] : 0u;
    w[t] = x;
    if (x) bm[wi] = 0u;
  }
  __syncthreads();
  const float* lg = logits + (size_t)row * ld;
  float* o = out + (size_t)row * V;
  auto banned = [&](int i) { return (w[(i - t0) >> 5] >> (i & 31)) & 1u; };
  if (VEC) {
#pragma unroll
    for (int e = 0; e < CON_TILE / 1024; ++e) {
      const int i = t0 + (e * 256 + t) * 4;
      if (i >= V) break;      // V % 4 == 0
      float4 x = *(const float4*)(lg + i);
      if (banned(i)) x.x = -INFINITY;
      if (banned(i + 1)) x.y = -INFINITY;
      if (banned(i + 2)) x.z = -INFINITY;
      if (banned(i + 3)) x.w = -INFINITY;
      *(float4*)(o + i) = x;
    }
  } else {
#pragma unroll
    for (int e = 0; e < CON_TILE / 256; ++e) {
      const int i = t0 + e * 256 + t;
      if (i < V) o[i] = banned(i) ? -INFINITY : lg[i];
    }
  }
  if (len && blockIdx.x == 0 && t == 0 && len[row] < hist_ld) len[row] += 1;
}

// a decode step that picks nothing still appends the token it is fed
__global__ void con_append_kernel(int32_t* hist, int hist_ld, int* len, const int32_t* tok, int b) {
  const int i = threadIdx.x;
  if (i >= b) return;
  const int L = len[i];
  if (L < hist_ld) { hist[(size_t)i * hist_ld + L] = tok[i]; len[i] = L + 1; }
}

__global__ void con_rewind_kernel(int* len, const int* plen, int b, int n) {
  const int i = threadIdx.x;
  if (i >= b) return;
  len[i] = max(len[i] - n, plen[i]);
}

}  // namespace

int launch_constrain_ban(const ConstrainArgs& a, hipStream_t s) {
  OM_CHECK(a.b >= 1 && a.V >= 1 && a.hist && a.len && a.plen && a.ban, "launch_constrain_ban: bad argument");
  OM_CHECK(a.hist_ld % 4 == 0 && ((uintptr_t)a.hist & 15) == 0, "constraints: history rows must be 16-byte aligned");
  OM_CHECK(a.ngram >= 0 && a.ngram <= CON_NGRAM_MAX, "constraints: no_repeat_ngram_size above the limit");
  OM_CHECK(a.bmw * 32 >= a.V, "constraints: bitmap narrower than the vocabulary slice");
  hipLaunchKernelGGL(con_ban_kernel, dim3(CON_CH, a.b), dim3(256), 0, s, a);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_constrain_apply(const float* logits, int ld, int b, int V, uint32_t* ban, int bmw, float* out, int* len, int hist_ld, hipStream_t s) {
  OM_CHECK(logits && ban && out && b >= 1 && V >= 1 && bmw * 32 >= V, "launch_constrain_apply: bad argument");
  const bool vec = V % 4 == 0 && ld % 4 == 0 && (((uintptr_t)logits | (uintptr_t)out) & 15) == 0;
  const dim3 g(cdiv(V, CON_TILE), b);
  if (vec) hipLaunchKernelGGL(con_apply_kernel<true>, g, dim3(256), 0, s, logits, ld, V, ban, bmw, out, len, hist_ld);
  else hipLaunchKernelGGL(con_apply_kernel<false>, g, dim3(256), 0, s, logits, ld, V, ban, bmw, out, len, hist_ld);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_constrain_append(int32_t* hist, int hist_ld, int* len, const int32_t* tok, int b, hipStream_t s) {
  hipLaunchKernelGGL(con_append_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, hist, hist_ld, len, tok, b);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_constrain_rewind(int* len, const int* plen, int b, int n, hipStream_t s) {
  hipLaunchKernelGGL(con_rewind_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, len, plen, b, n);
  OM_LAUNCH_CHECK();
  return 0;
}

// host side of omchat_set_constraints / omchat_op_constrain: validate the lists against the caps and lay them out in out[CON_LIST_WORDS] as the ban pass
// reads them // ([eos | suppress | begin_suppress | bad-word offsets (n + 1) | bad-word ids]); bad words equal to a single EOS id are dropped
int constrain_pack_lists(const int32_t* eos, int n_eos, const int32_t* sup, int n_sup, const int32_t* bsup, int n_bsup, const int32_t* bw_ids,
                         const int32_t* bw_off, int n_bw, int32_t* out, ConstrainArgs& a) {
  OM_CHECK(n_eos >= 0 && n_eos <= CON_EOS_MAX && (n_eos == 0 || eos), "constraints: at most 16 eos ids");
  OM_CHECK(n_sup >= 0 && n_sup <= CON_SUPPRESS_MAX && (n_sup == 0 || sup), "constraints: at most 1024 suppress_tokens");
  OM_CHECK(n_bsup >= 0 && n_bsup <= CON_SUPPRESS_MAX && (n_bsup == 0 || bsup), "constraints: at most 1024 begin_suppress_tokens");
  OM_CHECK(n_bw >= 0 && n_bw <= CON_BAD_WORDS_MAX && (n_bw == 0 || (bw_ids && bw_off)), "constraints: at most 1024 bad words");
  std::vector<int32_t> off(1, 0), ids;
  for (int w = 0; w < n_bw; ++w) {
    const int o = bw_off[w], m = bw_off[w + 1] - o;
    OM_CHECK(o >= 0 && m >= 1, "constraints: bad-word offsets must ascend, every word at least one id");
    bool is_eos = false;
    for (int q = 0; q < n_eos && m == 1; ++q) is_eos = is_eos || bw_ids[o] == eos[q];
    if (is_eos) continue;
    ids.insert(ids.end(), bw_ids + o, bw_ids + o + m);
    off.push_back((int32_t)ids.size());
  }
  OM_CHECK(ids.size() <= (size_t)CON_BAD_WORD_IDS_MAX, "constraints: at most 8192 bad-word ids in total");
  std::fill(out, out + CON_LIST_WORDS, 0);
  int32_t* p = out;
  if (n_eos) std::copy(eos, eos + n_eos, p);
  if (n_sup) std::copy(sup, sup + n_sup, p + CON_EOS_MAX);
  if (n_bsup) std::copy(bsup, bsup + n_bsup, p + CON_EOS_MAX + CON_SUPPRESS_MAX);
  std::copy(off.begin(), off.end(), p + CON_EOS_MAX + 2 * CON_SUPPRESS_MAX);
  std::copy(ids.begin(), ids.end(), p + CON_EOS_MAX + 2 * CON_SUPPRESS_MAX + CON_BAD_WORDS_MAX + 1);
  a.n_eos = n_eos; a.n_sup = n_sup; a.n_bsup = n_bsup; a.n_bw = (int)off.size() - 1;
  return 0;
}

void constrain_bind_lists(const int32_t* d_lists, ConstrainArgs& a) {
  a.eos = d_lists;
  a.sup = d_lists + CON_EOS_MAX;
  a.bsup = d_lists + CON_EOS_MAX + CON_SUPPRESS_MAX;
  a.bw_off = d_lists + CON_EOS_MAX + 2 * CON_SUPPRESS_MAX;
  a.bw_ids = d_lists + CON_EOS_MAX + 2 * CON_SUPPRESS_MAX + CON_BAD_WORDS_MAX + 1;
}
