// Finite-state token constraints for generate(token_fsm=): a deterministic automaton over token ids, CSR in device
// memory (off [n_states + 1], tok [E] ascending within a state, nxt [E]), one state per row.  Two launches per pick while it is on: the mark
// pass advances the row's state over the token the step is fed (a cooperative search of the state's edge list), stores it in the row's trail
// and sets the ALLOWED bits of the new state's edges in a bitmap of this rank's vocabulary slice; the apply pass writes the context's copy of
// the logits with every id whose bit is clear at -inf -- or passes a DEAD row through -- and clears the words it read.  The picks then run on
// the copy unchanged.  tests/fsm_ref.py is the CPU restatement, pinned to HF's PrefixConstrainedLogitsProcessor.
#include "kernels.h"
#include <math.h>
#include <string>
#include <vector>

namespace {

constexpr int FSM_CH = 32;         // workgroups per row of the mark pass (they stride the state's edge list: 5 rounds for 152 064 edges)
constexpr int FSM_TILE = 2048;     // logits per workgroup of the apply pass = 64 bitmap words, owned by that workgroup alone

// delta(s, tk) by all 256 threads of a workgroup: each round probes 256 evenly spaced edges of the range left and keeps the one piece that
// can hold tk, so a 152 064-edge list takes three dependent rounds of loads (594-edge pieces, 3-edge pieces, the edges themselves).
// Every thread returns the same value.  `sh` is one LDS word of the caller.
__device__ int fsm_delta(const FsmTable& T, int s, int tk, int* sh) {
  if (s < 0) return FSM_DEAD;
  const int t = threadIdx.x;
  int lo = T.off[s], hi = T.off[s + 1];
  while (hi - lo > 256) {
    const int step = (hi - lo + 255) / 256;
    if (t == 0) *sh = -1;
    __syncthreads();
    const int p = lo + t * step;
    // the one probe whose piece [p, p + step) can hold tk: tok[p] <= tk < tok[p + step]
    if (p < hi && T.tok[p] <= tk && (p + step >= hi || T.tok[p + step] > tk)) *sh = p;
    __syncthreads();
    const int q = *sh;
    __syncthreads();
    if (q < 0) return FSM_DEAD;      // tk lies below the first edge left
    lo = q;
    hi = min(q + step, hi);
  }
  if (t == 0) *sh = -1;
  __syncthreads();
  if (lo + t < hi && T.tok[lo + t] == tk) *sh = lo + t;
  __syncthreads();
  const int e = *sh;
  __syncthreads();
  return e < 0 ? FSM_DEAD : T.nxt[e];
}

// The state at this pick is trail[cnt] or, on a decode step (fed != NULL), delta(trail[cnt], fed): every workgroup of the row computes it
// from slots no workgroup of this launch writes; workgroup 0 stores it at trail[cnt + 1] and in cur[row], which the apply pass reads.  cnt
// is advanced behind this launch (fsm_apply_kernel).
__global__ __launch_bounds__(256) void fsm_mark_kernel(FsmTable T, FsmArgs a) {
  __shared__ int sh;
  const int row = blockIdx.y, t = threadIdx.x;
  const int k = a.cnt[row];
  int s = a.trail[(size_t)row * a.cap + k];
  const bool fed = a.fed != nullptr && k + 1 < a.cap;
  if (fed) s = fsm_delta(T, s, a.fed[row], &sh);
  if (blockIdx.x == 0 && t == 0) {
    if (fed) a.trail[(size_t)row * a.cap + k + 1] = s;
    a.cur[row] = s;
  }
  if (s < 0) return;      // DEAD: no bit is set, the apply pass passes the row through
  uint32_t* bm = a.bm + (size_t)row * a.bmw;
  const int e0 = T.off[s], e1 = T.off[s + 1];
  // whole 16-byte pieces of tok from the aligned index at or below e0 (tok is 16-byte aligned and padded to a multiple of four)
  // (the trip count is the wave's, not the lane's: the shuffles below need every lane)
  for (int i0 = (e0 & ~3) + (blockIdx.x * 256 + (t & ~63)) * 4; i0 < e1; i0 += FSM_CH * 256 * 4) {
    const int i = i0 + (t & 63) * 4;
    int word = -1; uint32_t bits = 0u;      // ascending ids: neighbours mostly share a word, one atomic for them
    if (i < e1) {
      const int4 q = *(const int4*)(T.tok + i);
      const int v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i + e < e0 || i + e >= e1) continue;
        const int li = v[e] - a.gbase;      // other ranks' ids are theirs to allow
        if (li < 0 || li >= a.V) continue;
        if ((li >> 5) != word) {
          if (bits) atomicOr(&bm[word], bits);
          word = li >> 5; bits = 0u;
        }
        bits |= 1u << (li & 31);
      }
    }
    // a dense state: the eight lanes that hold 32 consecutive ids end on one word -- one atomic for the eight
    int same = 1; uint32_t acc = bits;
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      const int w2 = __shfl_xor(word, m);
      const uint32_t b2 = __shfl_xor(acc, m);
      const int s2 = __shfl_xor(same, m);
      same = same && s2 && w2 == word;
      acc |= b2;
    }
    if (same && word >= 0) { if ((t & 7) == 0) atomicOr(&bm[word], acc); }
    else if (bits) atomicOr(&bm[word], bits);
  }
}

// out = logits with every id whose bit is clear at -inf (a DEAD row: the logits as they are); the bitmap words of the tile are read once into
// LDS and cleared by the thread that read them.  logits == out is allowed: each element is read and written by the same thread.
template <bool VEC>
__global__ __launch_bounds__(256) void fsm_apply_kernel(const float* logits, int ld, int V, uint32_t* bmap, int bmw, float* out, const int* cur,
                                                        int* cnt, int cap) {
  __shared__ uint32_t w[FSM_TILE / 32];
  const int row = blockIdx.y, t = threadIdx.x, t0 = blockIdx.x * FSM_TILE;
  uint32_t* bm = bmap + (size_t)row * bmw;
  if (t < FSM_TILE / 32) {
    const int wi = t0 / 32 + t;
    const uint32_t x = wi < bmw ? bm[wi] : 0u;
    w[t] = x;
    if (x) bm[wi] = 0u;
  }
  __syncthreads();
  const bool dead = cur[row] < 0;
  const float* lg = logits + (size_t)row * ld;
  float* o = out + (size_t)row * V;
  auto ok = [&](int i) { return dead || ((w[(i - t0) >> 5] >> (i & 31)) & 1u); };
  if (VEC) {
#pragma unroll
    for (int e = 0; e < FSM_TILE / 1024; ++e) {
      const int i = t0 + (e * 256 + t) * 4;
      if (i >= V) break;      // V % 4 == 0
      float4 x = *(const float4*)(lg + i);
      if (!ok(i)) x.x = -INFINITY;
      if (!ok(i + 1)) x.y = -INFINITY;
      if (!ok(i + 2)) x.z = -INFINITY;
      if (!ok(i + 3)) x.w = -INFINITY;
      *(float4*)(o + i) = x;
    }
  } else {
#pragma unroll
    for (int e = 0; e < FSM_TILE / 256; ++e) {
      const int i = t0 + e * 256 + t;
      if (i < V) o[i] = ok(i) ? lg[i] : -INFINITY;
    }
  }
  // (no workgroup of this launch reads cnt)
  if (cnt && blockIdx.x == 0 && t == 0 && cnt[row] + 1 < cap) cnt[row] += 1;
}

// a decode step that picks nothing still advances: one workgroup per row, so the thread that moves cnt is behind every read of it
__global__ __launch_bounds__(256) void fsm_advance_kernel(FsmTable T, FsmArgs a) {
  __shared__ int sh;
  const int row = blockIdx.x;
  const int k = a.cnt[row];
  if (k + 1 >= a.cap) return;
  const int s = fsm_delta(T, a.trail[(size_t)row * a.cap + k], a.fed[row], &sh);
  if (threadIdx.x == 0) { a.trail[(size_t)row * a.cap + k + 1] = s; a.cnt[row] = k + 1; }
}

__global__ void fsm_rewind_kernel(int* cnt, int b, int n) {
  const int i = threadIdx.x;
  if (i < b) cnt[i] = max(cnt[i] - n, 0);
}

}  // namespace

int launch_fsm_mark(const FsmTable& T, const FsmArgs& a, hipStream_t s) {
  OM_CHECK(T.off && T.tok && T.nxt && T.n_states >= 1, "launch_fsm_mark: no table");
  OM_CHECK(a.b >= 1 && a.V >= 1 && a.trail && a.cnt && a.cur && a.bm && a.cap >= 1, "launch_fsm_mark: bad argument");
  OM_CHECK(((uintptr_t)T.tok & 15) == 0, "fsm: the edge tokens must be 16-byte aligned");
  OM_CHECK(a.bmw * 32 >= a.V, "fsm: bitmap narrower than the vocabulary slice");
  hipLaunchKernelGGL(fsm_mark_kernel, dim3(FSM_CH, a.b), dim3(256), 0, s, T, a);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_fsm_apply(const float* logits, int ld, const FsmArgs& a, float* out, bool advance, hipStream_t s) {
  OM_CHECK(logits && out && a.b >= 1 && a.V >= 1 && a.bm && a.cur && a.bmw * 32 >= a.V, "launch_fsm_apply: bad argument");
  const bool vec = a.V % 4 == 0 && ld % 4 == 0 && (((uintptr_t)logits | (uintptr_t)out) & 15) == 0;
  const dim3 g(cdiv(a.V, FSM_TILE), a.b);
  int* cnt = advance ? a.cnt : nullptr;
  if (vec) hipLaunchKernelGGL(fsm_apply_kernel<true>, g, dim3(256), 0, s, logits, ld, a.V, a.bm, a.bmw, out, a.cur, cnt, a.cap);
  else hipLaunchKernelGGL(fsm_apply_kernel<false>, g, dim3(256), 0, s, logits, ld, a.V, a.bm, a.bmw, out, a.cur, cnt, a.cap);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_fsm_advance(const FsmTable& T, const FsmArgs& a, hipStream_t s) {
  OM_CHECK(T.off && T.tok && T.nxt && a.b >= 1 && a.trail && a.cnt && a.fed && a.cap >= 1, "launch_fsm_advance: bad argument");
  hipLaunchKernelGGL(fsm_advance_kernel, dim3(a.b), dim3(256), 0, s, T, a);
  OM_LAUNCH_CHECK();
  return 0;
}

int launch_fsm_rewind(int* cnt, int b, int n, hipStream_t s) {
  hipLaunchKernelGGL(fsm_rewind_kernel, dim3(1), dim3(64 > b ? 64 : b), 0, s, cnt, b, n);
  OM_LAUNCH_CHECK();
  return 0;
}

// host side of omchat_fsm_load / omchat_op_fsm: the caps, then the contract of a table.  off is read before tok and nxt, so a table above the
// edge cap is refused from its offsets alone.
int fsm_validate(int n_states, const int32_t* off, const int32_t* tok, const int32_t* nxt, int V_total) {
  OM_CHECK(n_states >= 1 && n_states <= FSM_MAX_STATES, "fsm: 1 <= n_states <= 1048576 (OMCHAT_FSM_MAX_STATES)");
  OM_CHECK(off && off[0] == 0, "fsm: off[0] must be 0");
  for (int s = 0; s < n_states; ++s) OM_CHECK(off[s + 1] >= off[s] && off[s + 1] <= FSM_MAX_EDGES, "fsm: offsets must ascend, at most 67108864 edges (OMCHAT_FSM_MAX_EDGES)");
  const int E = off[n_states];
  OM_CHECK(E == 0 || (tok && nxt), "fsm: null edge arrays");
  std::vector<char> target(n_states, 0);
  for (int s = 0; s < n_states; ++s)
    for (int e = off[s]; e < off[s + 1]; ++e) {
      OM_CHECK(tok[e] >= 0 && tok[e] < V_total, "fsm: state " + std::to_string(s) + " has an edge token outside the vocabulary");
      OM_CHECK(e == off[s] || tok[e] > tok[e - 1], "fsm: the edges of state " + std::to_string(s) + " must be sorted by token, without duplicates");
      OM_CHECK(nxt[e] >= 0 && nxt[e] < n_states, "fsm: state " + std::to_string(s) + " has an edge to a state outside the table");
      target[nxt[e]] = 1;
    }
  // any state may be handed over as a start state, so every edge's source counts as reachable, and with it the edge's target
  for (int s = 0; s < n_states; ++s)
    OM_CHECK(!target[s] || off[s + 1] > off[s], "fsm: state " + std::to_string(s) + " can be reached and has no edge: every row there would be -inf; add an EOS edge");
  return 0;
}
