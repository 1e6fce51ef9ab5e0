"""Engine: owns one `omchat_ctx` (one GPU / one tensor-parallel rank) and exposes the hot path on torch CUDA tensors.

torch is plumbing here (device memory for inputs/outputs, the current HIP stream); all arithmetic happens inside
libomchat_hip.so.  There is no CPU fallback: constructing an Engine without a GPU raises."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import OmchatConfig, check, ptr, cur_stream
from .config import OmChatConfig


def _torch():
    import torch
    return torch


# generate(num_return_sequences=N, share_prompt=None): the shared-prompt decode step is taken from this prompt length on (cache slots), where
# tools/bench_group.py measured it faster than the forked rows at every N by more than the pass-to-pass spread (slower
# at 64 slots, inside the spread at 1 024 for N = 4); None would mean that no such length exists: forked by default, shared opt-in
GROUP_SHARE_P_MIN = 2048


def group_share_refusal(fp8_kv, tp_size, q_heads, kv_heads, N):
    """why omchat_group_begin(share = 1) is not available for N rows per prompt (the library's own conditions, restated on the host so that
    generate() can refuse before any work), or None"""
    if fp8_kv:
        return "the e4m3 KV cache"
    if tp_size != 1:
        return "tensor parallelism"
    if not 2 <= N <= 16 or N * (q_heads // max(1, kv_heads)) > 128:
        return "N outside 2 <= N <= 16 and N * (q heads per kv head) <= 128"
    return None


class Engine:
    def __init__(self, cfg: OmChatConfig, dtype="bf16", max_seq=4096, max_batch=1, max_tiles=4, max_prefill_rows=None,
                 tp_rank=0, tp_size=1, comm=None, device=None, vision=True, text=True):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.OmchatError("omchat_amd.Engine needs a HIP device: the HIP path has no CPU fallback")
        self.lib = _lib.lib()
        self.cfg = cfg
        self.dtype_code = {"f16": _lib.F16, "fp16": _lib.F16, "bf16": _lib.BF16}[dtype] if isinstance(dtype, str) else _lib.dtype_code(dtype)
        self.torch_dtype = _lib.torch_dtype(self.dtype_code)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.tp_rank, self.tp_size = tp_rank, tp_size
        v, t = cfg.vision, cfg.text
        from .tp import local_dims
        ld = local_dims(cfg, tp_rank, tp_size)
        self.local = ld
        c = OmchatConfig()
        c.v_hidden = v["hidden_size"]; c.v_heads = ld["v_heads"]; c.v_qk_channels = v["hidden_size"]; c.v_mlp = ld["v_mlp"]
        c.v_layers = v["num_hidden_layers"] if vision else 0
        c.v_patch = v["patch_size"]; c.v_image = v["image_size"]; c.v_eps = v["layer_norm_eps"]
        c.t_hidden = t["hidden_size"]; c.t_layers = t["num_hidden_layers"] if text else 0
        c.t_heads = ld["t_heads"]; c.t_kv_heads = ld["t_kv_heads"]; c.t_mlp = ld["t_mlp"]; c.t_vocab = ld["t_vocab"]
        c.t_vocab_total = t["vocab_size"]; c.t_eps = t["rms_norm_eps"]; c.rope_theta = t["rope_theta"]
        c.max_seq = max_seq; c.max_batch = max_batch; c.max_tiles = max_tiles
        c.max_prefill_rows = max_prefill_rows if max_prefill_rows is not None else max_seq * max_batch
        c.dtype = self.dtype_code
        c.v_head_dim = v.get("head_dim", 128)
        c.v_norm_type = 1 if v.get("norm_type", "rms_norm") == "layer_norm" else 0
        c.v_no_qk_norm = 0 if v.get("qk_normalization", True) else 1
        self.c = c
        self.ntok = cfg.num_image_tokens
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.omchat_ctx_create(C.byref(c), tp_rank, tp_size, comm, C.byref(h)))
        self.h = h
        self._keep = []
        self._lookup_st = dict(verify_steps=0, drafted=0, accepted=0)
        # generate(reuse_cache=True): what sequence 0's cache holds (omchat_amd/prefix.py) with last call's tiles and feature rows
        self._prefix = None
        self._tile_key_next = 0
        self._ext_st = dict(kept_slots=0, prefilled_rows=0, tiles_encoded=0, tiles_reused=0)
        self._lp_max_new, self._logprobs_on, self._lp_extras = 0, False, (0, 0)      # set_logprobs
        self._enc_st = dict(calls=0, tiles=0)               # encode_images
        self._sfx_st = dict(tiles_encoded=0, prompt_rows=0, suffix_rows=0, shared=False)      # generate(suffixes=...)

    def close(self):
        if getattr(self, "h", None):
            self.lib.omchat_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_tensor(self, name, t):
        """t: torch tensor (CPU or CUDA; fp32 or the engine dtype) or numpy fp32 array, already rank-local."""
        torch = _torch()
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if t.dtype not in (torch.float32, self.torch_dtype):
            t = t.to(torch.float32)
        t = t.contiguous()
        shape = (C.c_int64 * max(t.dim(), 1))(*(list(t.shape) or [1]))
        check(self.lib.omchat_load_tensor(self.h, name.encode(), ptr(t), shape, max(t.dim(), 1), _lib.dtype_code(t.dtype)))
        self._prefix = None      # the cache rows came from other weights

    def load_state_dict(self, sd, strict=True):
        """sd: omchat-native keys -> full (unsharded) tensors; sharded here for tp_size > 1."""
        from .tp import shard_tensor
        from .weights import prepare_state_dict
        sd = prepare_state_dict(sd, self.cfg, self.c.v_layers > 0, self.c.t_layers > 0)
        for k, v in sd.items():
            self.load_tensor(k, shard_tensor(k, v, self.cfg, self.tp_rank, self.tp_size))
        if strict:
            n = self.lib.omchat_weights_missing(self.h)
            if n:
                raise KeyError(self.lib.omchat_last_error().decode())

    def fill_synthetic(self, seed=0, local=False):
        """local=True (shard profiling, bench.py --shard-of): every tensor of THIS rank's shapes is filled directly -- right geometry,
        not a sharding of the TP = 1 values.
        Deterministic synthetic weights (omchat_amd/synth.py's generator, evaluated on the device).  Under tensor parallelism
        every rank generates each FULL tensor on its GPU and keeps its shard (tp.shard_tensor semantics: zero-padded heads,
        replicated kv heads), so a TP = N group computes the same function as the TP = 1 context filled with the same seed."""
        if self.tp_size == 1 or local:
            check(self.lib.omchat_fill_synthetic(self.h, seed))
            return
        import math
        torch = _torch()
        from . import synth
        from .tp import shard_tensor
        with torch.cuda.device(self.device):
            for key, shape, std, off in synth.tensor_specs(self.cfg):
                vis = key.startswith(synth.TOWER) or key.startswith("model.mm_projector")
                if (vis and self.c.v_layers == 0) or (not vis and self.c.t_layers == 0):
                    continue
                n = int(np.prod(shape))
                full = torch.empty(n, dtype=self.torch_dtype, device=self.device)
                scale = float(np.float32(std)) * math.sqrt(3.0)      # same arithmetic as omchat_fill_synthetic (model.hip)
                check(self.lib.omchat_op_fill_uniform(self.dtype_code, ptr(full), n, (synth.fnv1a64(key) ^ seed) & 0xFFFFFFFFFFFFFFFF,
                                                      scale, off, cur_stream()))
                torch.cuda.current_stream().synchronize()
                self.load_tensor(key, shard_tensor(key, full.view(*shape), self.cfg, self.tp_rank, self.tp_size))
                del full

    def set_noop_allreduce(self):
        """Measurement only (bench.py --shard-of N): the tensor-parallel sums of this context become no-ops, so one rank's share of the
        work runs alone on one GPU.  The outputs are then NOT the model's outputs."""
        fn = C.cast(self.lib.omchat_allreduce_noop, C.c_void_p)
        check(self.lib.omchat_set_allreduce_hook(self.h, fn, None))

    def set_peer(self, peer, max_bytes=0, all_sizes=False):
        """attach a peer all-reduce group member (tp.init_peer) for the tensor-parallel sums of this context"""
        check(self.lib.omchat_ctx_set_peer(self.h, peer, max_bytes, int(all_sizes)))

    def allreduce(self, t):
        """in-place sum of a contiguous CUDA tensor (engine dtype or fp32, byte count a multiple of 16) over the tensor-parallel group"""
        if self.tp_size > 1:
            check(self.lib.omchat_ctx_allreduce(self.h, ptr(t), t.numel(), _lib.dtype_code(t.dtype), cur_stream()))
        return t

    def encode_images_dp(self, tower, pixels, select_layer=-1):
        """Data-parallel vision tower (optional throughput mode): `tower` is a REPLICATED vision-only Engine (tp_size 1)
        on this rank; the tiles are dealt to the ranks in contiguous shares, every rank encodes its share into a zero-filled feature
        buffer and one all-reduce over this (tensor-parallel) engine's transports gathers them: x + 0 is exact, so every rank ends with
        the bits a single tower would have produced.  Replaces ~90 ViT-sized all-reduces per sample by one."""
        torch = _torch()
        n = pixels.shape[0]
        out = torch.zeros(n, self.ntok, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device)
        lo, hi = self.tp_rank * n // self.tp_size, (self.tp_rank + 1) * n // self.tp_size
        if hi > lo:
            out[lo:hi] = tower.encode_images(pixels[lo:hi], select_layer)
        return self.allreduce(out)

    def comm_stats(self):
        a, b = C.c_long(0), C.c_long(0)
        check(self.lib.omchat_ctx_comm_stats(self.h, C.byref(a), C.byref(b)))
        rs, ag = C.c_long(0), C.c_long(0)
        check(self.lib.omchat_ctx_sp_stats(self.h, C.byref(rs), C.byref(ag)))
        return dict(peer_allreduces=a.value, rccl_allreduces=b.value, sp_reduce_scatters=rs.value, sp_all_gathers=ag.value)

    def enable_fp8_decode(self, on=True):
        """Weight-only OCP e4m3 replica of the decode-streamed decoder weights (quantised on first call); batch-1 decode only."""
        check(self.lib.omchat_enable_fp8_decode(self.h, int(on)))
        self._fp8_decode = bool(on)

    def enable_mxfp4_decode(self, on=True, batched=False):
        """Weight-only MXFP4 replica (OCP Microscaling: e2m1 codes + one e8m0 scale per 32 k, 4.25 bits per weight) of the decode-streamed
        decoder weights, quantised on the first call and again after a weight reload.  batched=False: batch-1 decode steps only; batched
        steps, the prompt-lookup verify step and beam search keep the 16-bit weights, as under enable_fp8_decode.  batched=True: every
        step of 2 <= b <= 32 rows (batched, padded-batch, beam and verify steps) streams a packed copy of the same codes as well, so one
        generation reads one weight format; a step of more than 32 rows is then refused.  Refused before the weights are loaded, together
        with enable_fp8_decode, under tensor parallelism, and (batched) for a geometry outside the packed GEMV path or when the packed
        copy does not fit; a refusal leaves the mode as it was."""
        check(self.lib.omchat_enable_mxfp4_decode(self.h, (2 if batched else 1) if on else 0))
        self._mxfp4_decode = bool(on)
        self._mxfp4_batched = bool(on) and bool(batched)

    def enable_fp8_kv(self, on=True):
        """fp8 (e4m3 + per-position scale) KV cache for the decode steps that follow the NEXT prefill (BASELINE configs[4])"""
        check(self.lib.omchat_enable_fp8_kv(self.h, int(on)))
        self._fp8_kv = bool(on)
        self._prefix = None

    def masked_decode_supported(self):
        """omchat_decode_step_masked (padded-batch decode as omchat_arch.py:61-70 computes it) runs on one GPU; see include/omchat_hip.h"""
        return self.tp_size == 1

    def enable_fp8_prefill(self, on=True):
        """fp8 x fp8 MFMA for the qkv and gate|up GEMMs of the prefill (activations quantised per token, weights per output row)"""
        check(self.lib.omchat_enable_fp8_prefill(self.h, int(on)))
        self._fp8_prefill = bool(on)
        self._prefix = None

    def enable_decode_graph(self, on=True):
        """Replay each decode step as one hipGraph launch (TP = 1, b <= 32); same kernels and results as the eager step."""
        check(self.lib.omchat_enable_decode_graph(self.h, int(on)))

    def decode_graph_stats(self):
        st, rp, cp = C.c_long(0), C.c_long(0), C.c_long(0)
        check(self.lib.omchat_decode_graph_stats(self.h, C.byref(st), C.byref(rp), C.byref(cp)))
        return dict(steps=st.value, replays=rp.value, captures=cp.value)

    def bf16x12_stats(self):
        """bf16x12 rows of the batch-1 step: the roles in use (tuning key 50), and per role (gate|up, down_proj, lm_head)
        the coded launches enqueued so far and the tensors that are coded"""
        roles, launches, coded = C.c_int(0), (C.c_long * 3)(), (C.c_int * 3)()
        check(self.lib.omchat_bf16x12_stats(self.h, C.byref(roles), launches, coded))
        return dict(roles=roles.value, launches=list(launches), coded=list(coded))

    def prof_enable(self, on=True):
        check(self.lib.omchat_prof_enable(self.h, int(on)))

    def prof_read(self, cat, reset=True):
        ms, n = C.c_double(0), C.c_long(0)
        check(self.lib.omchat_prof_read(self.h, cat, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def device_bytes(self):
        return int(self.lib.omchat_device_bytes(self.h))

    # ------------------------------------------------------------------ vision
    def _px(self, pixels):
        torch = _torch()
        if pixels.dim() != 4 or pixels.shape[1] != 3:
            raise ValueError(f"wrong pixel_values size: {tuple(pixels.shape)}")      # modeling_intern_vit.py:337-338
        s = self.cfg.vision["image_size"]
        if pixels.shape[2] != s or pixels.shape[3] != s:
            raise ValueError(f"expected {s}x{s} tiles, got {tuple(pixels.shape[2:])}")
        return pixels.to(device=self.device, dtype=self.torch_dtype).contiguous()

    def vit_forward(self, pixels, select_layer=-1, select_feature="patch"):
        torch = _torch()
        if select_feature not in ("patch", "cls_patch"):
            raise ValueError(f"Unexpected select feature: {select_feature}")           # internVIT_encoder.py:42
        px = self._px(pixels)
        n = px.shape[0]
        keep = select_feature == "cls_patch"
        out = torch.empty(n, self.ntok + (1 if keep else 0), self.cfg.vision["hidden_size"], dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_vit_forward(self.h, ptr(px), n, select_layer, int(keep), ptr(out), cur_stream()))
        return out

    def projector_forward(self, x):
        torch = _torch()
        x = x.to(device=self.device, dtype=self.torch_dtype).contiguous()
        rows = x.numel() // x.shape[-1]
        out = torch.empty(*x.shape[:-1], self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_projector_forward(self.h, ptr(x), rows, ptr(out), cur_stream()))
        return out

    def encode_images(self, pixels, select_layer=-1):
        torch = _torch()
        px = self._px(pixels)
        n = px.shape[0]
        out = torch.empty(n, self.ntok, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_encode_images(self.h, ptr(px), n, select_layer, ptr(out), cur_stream()))
        self._enc_st["calls"] += 1; self._enc_st["tiles"] += n
        return out

    def encode_stats(self, reset=False):
        """counters of encode_images since the engine was made (or the last reset): calls and tiles run through the tower + projector"""
        out = dict(self._enc_st)
        if reset:
            self._enc_st = dict(calls=0, tiles=0)
        return out

    # ------------------------------------------------------------------ splice
    def splice(self, input_ids, attention_mask, feats, padding_side="right", max_length=None, return_plan=False):
        """input_ids int64 [b,T] (CPU or CUDA), attention_mask [b,T] or None, feats [n_tiles, ntok, H] CUDA or None.
        Returns (inputs_embeds [b,S,H] CUDA, lengths list, valid-mask bool [b,S] CPU); with return_plan also the host plan src_index
        int32 [b,S] (>= 0: a token slot; what omchat_amd/scoring.py splices labels with)."""
        torch = _torch()
        ids = input_ids.detach().to("cpu", torch.int64).contiguous()
        b, T = ids.shape
        m = None if attention_mask is None else attention_mask.detach().to("cpu").ne(0).to(torch.uint8).contiguous()
        n_tiles = 0 if feats is None else feats.shape[0]
        ntok = self.ntok if feats is None else feats.shape[1]
        side = 1 if padding_side == "left" else 0
        ml = -1 if max_length is None else int(max_length)
        S = C.c_int(0)
        lens = torch.zeros(b, dtype=torch.int32)
        check(self.lib.omchat_splice_plan(ptr(ids), ptr(m), b, T, ntok, n_tiles, side, ml, None, ptr(lens), C.byref(S), self.c.t_vocab_total))
        idx = torch.empty(b, S.value, dtype=torch.int32)
        check(self.lib.omchat_splice_plan(ptr(ids), ptr(m), b, T, ntok, n_tiles, side, ml, ptr(idx), ptr(lens), C.byref(S), 0))
        idx_d = idx.to(self.device)
        f = None if feats is None else feats.to(device=self.device, dtype=self.torch_dtype).contiguous()
        out = torch.empty(b, S.value, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_splice_gather(self.h, ptr(idx_d), ptr(f), ptr(out), b * S.value, cur_stream()))
        res = (out, [int(x) for x in lens], idx.ne(_lib.PAD_ROW))
        return res + (idx,) if return_plan else res

    # ------------------------------------------------------------------ decoder
    def prefill(self, embeds, lengths=None, want_hidden=False, want_logits=True, padding_side="right"):
        """padding_side='left': rows hold their tokens at the END (omchat_arch.py:176-184); logits are those of position S - 1 and
        decode steps are refused afterwards (see include/omchat_hip.h: omchat_prefill_left)."""
        torch = _torch()
        e = embeds.to(device=self.device, dtype=self.torch_dtype).contiguous()
        b, S, _ = e.shape
        lens = torch.tensor(lengths if lengths is not None else [S] * b, dtype=torch.int32)
        logits = torch.empty(b, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        hidden = torch.empty(b, S, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device) if want_hidden else None
        fn = self.lib.omchat_prefill_left if padding_side == "left" else self.lib.omchat_prefill
        self._prefix = None      # every prefill overwrites sequence 0: generate(reuse_cache=True) records again after its own
        check(fn(self.h, ptr(e), b, S, ptr(lens), ptr(logits), ptr(hidden), cur_stream()))
        return logits, hidden

    def prefill_extend(self, embeds, keep, want_hidden=False, want_logits=True):
        """Continue sequence 0's cache (include/omchat_hip.h: omchat_prefill_extend): embeds [S_new, H] (or [1, S_new, H]) are the rows at
        positions keep .. keep + S_new - 1; slots >= keep are forgotten, slots < keep stay.  -> (logits fp32 [1, V] of the last row,
        hidden [1, S_new, H] or None)"""
        torch = _torch()
        e = embeds.to(device=self.device, dtype=self.torch_dtype).contiguous()
        if e.dim() == 3:
            if e.shape[0] != 1:
                raise ValueError("prefill_extend continues ONE sequence: embeds [S_new, H] or [1, S_new, H]")
            e = e[0]
        S = e.shape[0]
        logits = torch.empty(1, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        hidden = torch.empty(1, S, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device) if want_hidden else None
        check(self.lib.omchat_prefill_extend(self.h, ptr(e), S, int(keep), ptr(logits), ptr(hidden), cur_stream()))
        return logits, hidden

    def extend_attn_form(self, S_new, keep):
        """0 = prefill_extend(S_new rows, keep) takes the prefill attention kernel with q_pos0, 1 = the split-KV block attention"""
        return int(self.lib.omchat_extend_attn_form(int(S_new), int(keep), self.c.t_kv_heads))

    def kv_read(self, layer, which, pos0, n):
        """test hook: rows [pos0, pos0 + n) of sequence 0's K (which = 0) / V (1) cache of one layer -> [kv_heads, n, 128]"""
        torch = _torch()
        out = torch.empty(self.c.t_kv_heads, n, 128, dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_kv_read(self.h, int(layer), int(which), int(pos0), int(n), ptr(out), cur_stream()))
        return out

    def prefill_suffixes(self, embeds, lengths, keep, want_hidden=False, want_logits=True):
        """N suffixes over one prefilled prompt (include/omchat_hip.h: omchat_prefill_suffixes): rows 0 .. N - 1 each
        hold `keep` slots of the prompt (group_begin(1, N, keep, share) first; N == 1: the b = 1 state itself).  embeds [N, S_max, H], row j
        valid in [0, lengths[j]).  -> (logits fp32 [N, V] of every row's last valid position, hidden [N, S_max, H] or None)"""
        torch = _torch()
        e = embeds.to(device=self.device, dtype=self.torch_dtype).contiguous()
        if e.dim() != 3 or len(lengths) != e.shape[0]:
            raise ValueError("prefill_suffixes: embeds [N, S_max, H] and N lengths")
        N, S, _ = e.shape
        lens = torch.tensor([int(x) for x in lengths], dtype=torch.int32)
        logits = torch.empty(N, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        hidden = torch.empty(N, S, self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device) if want_hidden else None
        check(self.lib.omchat_prefill_suffixes(self.h, ptr(e), N, S, ptr(lens), int(keep), ptr(logits), ptr(hidden), cur_stream()))
        self._prefix = None      # the rows are siblings now, not one conversation
        return logits, hidden

    def suffix_attn_form(self, shared):
        """1 = prefill_suffixes takes the suffix attention kernel, 0 = the batched prefill kernel with q_pos0 = keep (forked rows only)"""
        return int(self.lib.omchat_suffix_attn_form(int(bool(shared)), self.c.t_heads // max(1, self.c.t_kv_heads)))

    def kv_read_row(self, row, layer, which, pos0, n):
        """test hook: kv_read for cache row `row` (the sibling rows of a group)"""
        torch = _torch()
        out = torch.empty(self.c.t_kv_heads, n, 128, dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_kv_read_row(self.h, int(row), int(layer), int(which), int(pos0), int(n), ptr(out), cur_stream()))
        return out

    def suffix_stats(self, reset=False):
        """the last generate(suffixes=...) / score(suffixes=...) call: tiles run through the tower, prompt rows prefilled (once), suffix rows
        prefilled (the sum of the suffix lengths) and whether the rows share the prompt's slots"""
        out = dict(self._sfx_st)
        if reset:
            self._sfx_st = dict(tiles_encoded=0, prompt_rows=0, suffix_rows=0, shared=False)
        return out

    def extend_stats(self, reset=False):
        """the last generate(reuse_cache=True) call: cache slots kept, rows prefilled, tiles run through the tower / taken from last call"""
        out = dict(self._ext_st)
        if reset:
            for key in self._ext_st:
                self._ext_st[key] = 0
        return out

    def drop_prefix(self):
        """forget what sequence 0's cache holds, with the kept tiles and feature rows (model.reset_cache())"""
        self._prefix = None

    def tile_keys(self, px):
        """content keys of the tiles px [n, 3, s, s] (engine dtype, on the device): a tile bit-equal to one kept from the last
        reuse_cache call gets that tile's key, any other a fresh one.  One device-to-host copy.  -> (keys, index of the equal kept tile or -1)"""
        torch = _torch()
        n = 0 if px is None else px.shape[0]
        kept = self._prefix
        src = [-1] * n
        if n and kept is not None and kept.get("px") is not None and kept["px"].shape[1:] == px.shape[1:]:
            eq = torch.stack([(kept["px"] == px[j]).flatten(1).all(dim=1) for j in range(n)]).cpu()
            for j in range(n):
                hit = torch.nonzero(eq[j])
                if hit.numel():
                    src[j] = int(hit[0])
        keys = []
        for j in range(n):
            if src[j] >= 0:
                keys.append(kept["keys"][src[j]])
            else:
                keys.append(self._tile_key_next)
                self._tile_key_next += 1
        return keys, src

    def splice_plan(self, input_ids, n_tiles, max_length=None):
        """omchat_splice_plan of ONE unpadded row: -> src_index int32 [S] (CPU)"""
        torch = _torch()
        ids = input_ids.detach().to("cpu", torch.int64).contiguous().view(1, -1)
        T = ids.shape[1]
        ml = -1 if max_length is None else int(max_length)
        S = C.c_int(0)
        lens = torch.zeros(1, dtype=torch.int32)
        check(self.lib.omchat_splice_plan(ptr(ids), None, 1, T, self.ntok, n_tiles, 0, ml, None, ptr(lens), C.byref(S), self.c.t_vocab_total))
        idx = torch.empty(1, S.value, dtype=torch.int32)
        check(self.lib.omchat_splice_plan(ptr(ids), None, 1, T, self.ntok, n_tiles, 0, ml, ptr(idx), ptr(lens), C.byref(S), 0))
        return idx[0]

    def gather_rows(self, src_index, feats):
        """embedding rows of a (slice of a) splice plan: src_index int32 [rows], feats [n_tiles, ntok, H] or None -> [rows, H]"""
        torch = _torch()
        idx_d = src_index.to(torch.int32).contiguous().to(self.device)
        f = None if feats is None else feats.to(device=self.device, dtype=self.torch_dtype).contiguous()
        out = torch.empty(idx_d.shape[0], self.cfg.text["hidden_size"], dtype=self.torch_dtype, device=self.device)
        check(self.lib.omchat_splice_gather(self.h, ptr(idx_d), ptr(f), ptr(out), idx_d.shape[0], cur_stream()))
        return out

    def decode_step(self, tokens, want_logits=False):
        torch = _torch()
        tk = tokens.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        b = tk.shape[0]
        logits = torch.empty(b, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        nxt = torch.empty(b, dtype=torch.int32, device=self.device)
        check(self.lib.omchat_decode_step(self.h, ptr(tk), b, ptr(logits), ptr(nxt), cur_stream()))
        return nxt, logits

    def decode_verify(self, tokens, keep_all=False, want_logits=False, sample=False):
        """Prompt-lookup verify step (include/omchat_hip.h: omchat_decode_verify): tokens = [last emitted token, draft...] (2..16 ids) of
        sequence 0 through the decoder at once.  -> (picks int32 [T] on the device, n accepted drafts); the cache keeps L + 1 + n slots
        (all T with keep_all).  want_logits: -> (picks, n, rank-local logits fp32 [T, V / tp]).  sample=True (set_sampling on): the picks
        are the ids plain sampled steps of sequence 0 would draw at those positions, and the n + 1 emitted ones are committed to its
        step counter and seen set; kv_rewind(1, r) straight afterwards takes the last r <= n + 1 of them back."""
        torch = _torch()
        tk = torch.as_tensor(tokens).to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        T = tk.shape[0]
        logits = torch.empty(T, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        picks = torch.empty(T, dtype=torch.int32, device=self.device)
        n = C.c_int(0)
        check(self.lib.omchat_decode_verify(self.h, ptr(tk), T, ptr(logits), ptr(picks), C.byref(n), (1 if keep_all else 0) | (2 if sample else 0),
                                            cur_stream()))
        st = self._lookup_st
        st["verify_steps"] += 1; st["drafted"] += T - 1; st["accepted"] += n.value
        return (picks, n.value, logits) if want_logits else (picks, n.value)

    def lookup_stats(self, reset=False):
        """counters of decode_verify since the engine was made (or the last reset): verify steps, drafted and accepted draft tokens"""
        out = dict(self._lookup_st)
        if reset:
            for key in self._lookup_st:
                self._lookup_st[key] = 0
        return out

    def verify_max_tokens(self):
        """the most tokens one decode_verify takes on this context: 16, fewer when T * (q heads per kv head) would exceed 128"""
        return min(16, 128 // max(1, self.c.t_heads // max(1, self.c.t_kv_heads)))

    def decode_step_masked(self, tokens, position_ids, attention_mask, want_logits=False):
        """Decode step of a padded batch as the reference computes it (omchat_arch.py:61-70): `position_ids` [b] or [b, 1] and
        `attention_mask` [b, slots + 1] are what the decode branch of prepare_inputs_labels_for_multimodal returns (the token-level
        mask padded with ones, sum(mask) - 1).  The new token of every row goes to the common cache slot; see include/omchat_hip.h."""
        torch = _torch()
        tk = tokens.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        b = tk.shape[0]
        pos = position_ids.detach().to("cpu", torch.int32).contiguous().view(-1)
        m = attention_mask.detach().to("cpu").ne(0).to(torch.uint8).contiguous()
        if pos.shape[0] != b or m.dim() != 2 or m.shape[0] != b:
            raise ValueError("decode_step_masked: position_ids [b], attention_mask [b, slots + 1]")
        logits = torch.empty(b, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        nxt = torch.empty(b, dtype=torch.int32, device=self.device)
        check(self.lib.omchat_decode_step_masked(self.h, ptr(tk), b, ptr(pos), ptr(m), m.shape[1], ptr(logits), ptr(nxt), cur_stream()))
        return nxt, logits

    def masked_decode_begin(self, position_ids, attention_mask):
        """Once after the prefill of a padded batch that HF-style generate will decode: `attention_mask` [b, cols] is the key mask of the
        FIRST decode step as the reference builds it (token-level mask, any ones padding may be left off: slots behind `cols` count as
        visible), `position_ids` [b] its sum(mask) - 1.  decode_step_masked_next then needs no host data (include/omchat_hip.h)."""
        torch = _torch()
        pos = position_ids.detach().to("cpu", torch.int32).contiguous().view(-1)
        m = attention_mask.detach().to("cpu").ne(0).to(torch.uint8).contiguous()
        if m.dim() != 2 or pos.shape[0] != m.shape[0]:
            raise ValueError("masked_decode_begin: position_ids [b], attention_mask [b, cols]")
        cols = min(m.shape[1], self.c.max_seq)
        check(self.lib.omchat_masked_decode_begin(self.h, m.shape[0], ptr(pos), ptr(m), m.shape[1], cols, cur_stream()))

    def decode_step_masked_next(self, tokens, want_logits=False):
        torch = _torch()
        tk = tokens.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        b = tk.shape[0]
        logits = torch.empty(b, self.c.t_vocab, dtype=torch.float32, device=self.device) if want_logits else None
        nxt = torch.empty(b, dtype=torch.int32, device=self.device)
        check(self.lib.omchat_decode_step_masked_next(self.h, ptr(tk), b, ptr(logits), ptr(nxt), cur_stream()))
        return nxt, logits

    def fused_status(self):
        """(launches, timeout_bits) of the fused attention + o_proj decode launches; timeout_bits != 0 means a hand-off gave up."""
        n, bits = C.c_long(0), C.c_uint(0)
        check(self.lib.omchat_fused_status(self.h, C.byref(n), C.byref(bits)))
        return n.value, bits.value

    def lm_head(self, hidden):
        torch = _torch()
        h = hidden.to(device=self.device, dtype=self.torch_dtype).contiguous()
        n = h.numel() // h.shape[-1]
        out = torch.empty(*h.shape[:-1], self.c.t_vocab, dtype=torch.float32, device=self.device)
        check(self.lib.omchat_lm_head(self.h, ptr(h), n, ptr(out), cur_stream()))
        return out

    def score_hidden(self, hidden, shifted_labels):
        """Teacher-forced scoring (include/omchat_hip.h: omchat_score_hidden).  hidden [b, S, H]: the final-normed rows
        of prefill(want_hidden=True); shifted_labels int [b, S] (CPU or CUDA): the token that follows each slot, -100 = not scored.
        -> (logprob fp32 [b, S] with 0 where the label is -100, loss 0-dim fp32 = mean of -logprob over the scored slots (NaN if none),
        seq_sum fp32 [b] = every sequence's sum of logprob, seq_count fp32 [b]), all on the device, no synchronisation.  The [b, S, V]
        logits are never materialised.  Refused under tensor parallelism.  Labels on the CPU (what the model's splice hands over) are
        range-checked here, before the launch: anything but -100 or an id in [0, V) is a ValueError.  Labels already on the device are
        NOT read back (that would synchronise): the kernels stay in bounds and a label outside the range scores NaN, in its row and in
        the loss -- check such labels before uploading them."""
        torch = _torch()
        from .scoring import check_labels
        if self.tp_size > 1:
            raise NotImplementedError("scoring under tensor parallelism: the lm_head is vocabulary-parallel and no exchange of the partials is built")
        h = hidden.to(device=self.device, dtype=self.torch_dtype).contiguous()
        if h.dim() != 3 or tuple(shifted_labels.shape) != tuple(h.shape[:2]):
            raise ValueError("score_hidden: hidden [b, S, H] and shifted_labels [b, S]")
        b, S, _ = h.shape
        if shifted_labels.device.type == "cpu":
            check_labels(shifted_labels, self.c.t_vocab)      # host labels (the model's splice): no synchronisation
        lab = shifted_labels.to(device=self.device, dtype=torch.int32).contiguous()
        logprob = torch.empty(b, S, dtype=torch.float32, device=self.device)
        out = torch.empty(2 + 2 * b, dtype=torch.float32, device=self.device)
        check(self.lib.omchat_score_hidden(self.h, ptr(h), b * S, ptr(lab), b, S, ptr(logprob), ptr(out), cur_stream()))
        return logprob, out[0] / out[1], out[2:2 + b], out[2 + b:]

    def full_logits(self, logits):
        """[b, V / tp] rank-local vocabulary shard -> [b, V] on every rank (HF-style consumers of `out.logits` must not see a
        shard).  Uses the initialised torch.distributed group (the bootstrap channel of tp.init_comm); identity at TP = 1."""
        if self.tp_size == 1 or logits is None:
            return logits
        torch = _torch()
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise _lib.OmchatError("tensor-parallel logits are vocabulary shards: initialise torch.distributed to gather them, or use Engine.argmax")
        cpu = dist.get_backend() == "gloo"
        mine = logits.float().cpu().contiguous() if cpu else logits.float().contiguous()
        parts = [torch.empty_like(mine) for _ in range(self.tp_size)]
        dist.all_gather(parts, mine)
        return torch.cat(parts, dim=-1).to(self.device)

    def kv_lengths(self, b):
        torch = _torch()
        out = torch.zeros(b, dtype=torch.int32)
        check(self.lib.omchat_kv_lengths(self.h, ptr(out), b))
        return [int(x) for x in out]

    def kv_rewind(self, b, n=1):
        """forget the last n decode steps of sequences 0..b-1 (see include/omchat_hip.h: omchat_kv_rewind).  While set_logprobs is on, b
        must cover all the rows it was switched on for: the rows' records go back together"""
        check(self.lib.omchat_kv_rewind(self.h, b, n, cur_stream()))

    def argmax(self, logits):
        torch = _torch()
        out = torch.empty(logits.shape[0], dtype=torch.int32, device=self.device)
        check(self.lib.omchat_greedy(self.h, ptr(logits), logits.shape[0], ptr(out), cur_stream()))
        return out

    # ------------------------------------------------------------------ sampling (include/omchat_hip.h: omchat_set_sampling)
    def set_sampling(self, b, seed=0, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seen=None, min_p=None, typical_p=None,
                     epsilon_cutoff=None, eta_cutoff=None):
        """every following token pick of rows 0..b-1 samples (HF order: repetition penalty, temperature, top-k, top-p, min_p, typical_p,
        epsilon_cutoff, eta_cutoff; Gumbel-max keyed by (seed, row, step, global id)); seen: per-row lists of already-seen ids for the
        penalty (ids outside the vocabulary are ignored).  The last four are on under HF's rules: min_p when not None, typical_p when < 1,
        the cutoffs when in (0, 1).  Resets the rows' step counters.  b = 0: greedy again."""
        torch = _torch()
        seen = seen if seen is not None else [[] for _ in range(max(b, 0))]
        n = torch.tensor([len(r) for r in seen] or [0], dtype=torch.int32)
        flat = torch.tensor([int(i) for r in seen for i in r] or [0], dtype=torch.int32)
        check(self.lib.omchat_set_sampling(self.h, int(b), int(seed) & 0xFFFFFFFFFFFFFFFF, float(temperature), int(top_k or 0),
                                           float(1.0 if top_p is None else top_p), float(repetition_penalty), ptr(flat), ptr(n), cur_stream()))
        if int(b) > 0:
            cut = lambda v: float(v) if v is not None and 0.0 < float(v) < 1.0 else 1.0
            check(self.lib.omchat_set_sampling_filters(self.h, -1.0 if min_p is None else float(min_p),
                                                       1.0 if typical_p is None or float(typical_p) >= 1.0 else float(typical_p),
                                                       cut(epsilon_cutoff), cut(eta_cutoff), cur_stream()))

    def sampling_off(self):
        check(self.lib.omchat_set_sampling(self.h, 0, 0, 1.0, 0, 1.0, 1.0, None, None, cur_stream()))

    def sampling_state(self, row=0):
        """(step counter, sorted seen ids) of a row while set_sampling is on; the ids are this rank's slice of the seen set, as global
        ids (test accessor; synchronises)"""
        torch = _torch()
        step = C.c_int(0)
        words = torch.zeros((self.c.t_vocab + 31) // 32, dtype=torch.int32)
        check(self.lib.omchat_read_sampling_state(self.h, int(row), C.byref(step), ptr(words)))
        base = self.tp_rank * self.c.t_vocab
        seen = [base + 32 * w + i for w, v in enumerate(words.tolist()) if v for i in range(32) if (v >> i) & 1]
        return step.value, seen

    def sample(self, logits):
        """the sampled counterpart of argmax (first token after the prefill): rank-local logits [b, V / tp] -> int32 [b]"""
        torch = _torch()
        out = torch.empty(logits.shape[0], dtype=torch.int32, device=self.device)
        check(self.lib.omchat_sample(self.h, ptr(logits), logits.shape[0], ptr(out), cur_stream()))
        return out

    # ------------------------------------------------------------------ per-token log-probabilities (include/omchat_hip.h: omchat_set_logprobs)
    def set_logprobs(self, b, max_new, top_n=0, score_token_ids=None):
        """every following token pick of rows 0..b-1 (argmax or sampler, eager or in the decode graph) records the raw and the processed
        log-probability of its id on the device; at most max_new picks.  Resets the rows' counters.  Sticky until
        logprobs_off() (or b = 0).  top_n (1..20) / score_token_ids (1..32 distinct ids): the extras of omchat_set_logprobs_ex -- the top_n
        alternatives and the listed ids' log-probabilities under the raw distribution, at every pick (read_logprob_extras)."""
        ids = [int(i) for i in (score_token_ids if score_token_ids is not None else [])]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        check(self.lib.omchat_set_logprobs_ex(self.h, int(b), int(max_new), int(top_n), arr if ids else None, len(ids), cur_stream()))
        self._lp_max_new = int(max_new)
        self._logprobs_on = int(b) > 0
        self._lp_extras = (int(top_n), len(ids)) if int(b) > 0 else (0, 0)

    def logprobs_off(self):
        check(self.lib.omchat_set_logprobs(self.h, 0, 0, cur_stream()))
        self._logprobs_on = False
        self._lp_extras = (0, 0)

    def read_logprob_extras(self, b):
        """one synchronising copy of the extras' record -> (top_vals fp32 [b, m, top_n], top_ids int64 [b, m, top_n], scored fp32
        [b, m, n_score], counts list); m = the longest row's count, entries behind a row's own count are 0 / -1 / 0.  Refused by the
        library when the extras are off."""
        torch = _torch()
        n, (tn, ns) = max(self._lp_max_new, 1), self._lp_extras
        vals = torch.zeros(b, n, tn, dtype=torch.float32)
        ids = torch.full((b, n, tn), -1, dtype=torch.int32)
        sc = torch.zeros(b, n, ns, dtype=torch.float32)
        cnt = torch.zeros(b, dtype=torch.int32)
        check(self.lib.omchat_read_logprob_extras(self.h, int(b), ptr(vals) if tn else None, ptr(ids) if tn else None, ptr(sc) if ns else None,
                                                  ptr(cnt), n))
        m = int(cnt.max()) if b else 0
        return vals[:, :m].contiguous(), ids[:, :m].to(torch.int64).contiguous(), sc[:, :m].contiguous(), [int(x) for x in cnt]

    def read_logprobs(self, b):
        """one synchronising copy of the record (the whole device record, every row and line, whatever b: a few KB) -> (raw fp32 [b, n],
        processed fp32 [b, n], counts list); n = the longest row's count, entries behind a row's own count are 0.  Refused by the library
        when logprobs are off."""
        torch = _torch()
        n = max(self._lp_max_new, 1)
        raw = torch.zeros(b, n, dtype=torch.float32)
        proc = torch.zeros(b, n, dtype=torch.float32)
        cnt = torch.zeros(b, dtype=torch.int32)
        check(self.lib.omchat_read_logprobs(self.h, int(b), ptr(raw), ptr(proc), ptr(cnt), n))
        m = int(cnt.max()) if b else 0
        return raw[:, :m].contiguous(), proc[:, :m].contiguous(), [int(x) for x in cnt]

    # ------------------------------------------------------------------ HF logits constraints (include/omchat_hip.h: omchat_set_constraints)
    def set_constraints(self, b, prompt, max_new, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, min_length=0, eos=(),
                        suppress_tokens=(), begin_suppress_tokens=()):
        """every following token pick of rows 0..b-1 (argmax or sampler) excludes what HF's NoRepeatNGram, NoBadWords, MinLength,
        MinNewTokensLength, SuppressTokens and SuppressTokensAtBegin processors would set to -inf.  prompt: the b prompt rows as HF's
        processors see them (lists of ids, -200 sentinels and pads included); every decode step appends the token it is fed on the device.
        max_new: the most decode steps that follow.  Sticky until constraints_off() (or b = 0)."""
        torch = _torch()
        i32 = lambda xs: torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)
        words = [list(w) for w in (bad_words_ids or [])]
        off = [0]
        for w in words:
            off.append(off[-1] + len(w))
        eos, sup, bsup = list(eos or ()), list(suppress_tokens or ()), list(begin_suppress_tokens or ())
        rows = [list(r) for r in prompt]
        t_eos, t_sup, t_bsup, t_bw, t_off = i32(eos), i32(sup), i32(bsup), i32([i for w in words for i in w]), i32(off)
        t_ids, t_len = i32([i for r in rows for i in r]), i32([len(r) for r in rows])
        check(self.lib.omchat_set_constraints(self.h, int(b), int(no_repeat_ngram_size or 0), int(min_new_tokens or 0), int(min_length or 0),
                                              ptr(t_eos), len(eos), ptr(t_sup), len(sup), ptr(t_bsup), len(bsup), ptr(t_bw), ptr(t_off),
                                              len(words), ptr(t_ids), ptr(t_len), int(max_new), cur_stream()))

    def constraints_off(self):
        check(self.lib.omchat_set_constraints(self.h, 0, 0, 0, 0, None, 0, None, 0, None, 0, None, None, 0, None, None, 0, cur_stream()))

    # ------------------------------------------------------------------ finite-state token constraints (include/omchat_hip.h: omchat_fsm_load)
    def load_token_fsm(self, fsm):
        """uploads the table of an omchat_amd.fsm.TokenFSM (None: unloads).  The object loaded last is remembered: handing it over again keeps
        the table and the captured decode graphs."""
        torch = _torch()
        if fsm is vars(self).get("_fsm"):
            return
        if fsm is None:
            check(self.lib.omchat_fsm_load(self.h, 0, None, None, None, cur_stream()))
        else:
            i32 = lambda xs: torch.tensor(xs or [0], dtype=torch.int32)
            off, tok, nxt = (i32(a) for a in fsm.arrays())
            check(self.lib.omchat_fsm_load(self.h, int(fsm.n_states), ptr(off), ptr(tok), ptr(nxt), cur_stream()))
        self._fsm = fsm
        self._fsm_on = False

    def token_fsm_begin(self, b, start, max_new):
        """every following token pick of rows 0..b-1 (argmax or sampler, eager or in the decode graph) allows only the ids that are edges of
        the row's state in the loaded table; every decode step first advances the states over the tokens it is fed.  start: one state or
        one per row; max_new: the most decode steps that follow.  Sticky until token_fsm_off()."""
        torch = _torch()
        st = torch.tensor([int(start)] * int(b) if isinstance(start, int) else [int(s) for s in start], dtype=torch.int32)
        if st.numel() != int(b):
            raise ValueError(f"token_fsm_begin: {st.numel()} start states for {b} rows")
        check(self.lib.omchat_fsm_begin(self.h, int(b), ptr(st), int(max_new), cur_stream()))
        self._fsm_on = True

    def token_fsm_off(self):
        if vars(self).get("_fsm_on", False):
            check(self.lib.omchat_fsm_begin(self.h, 0, None, 0, cur_stream()))
        self._fsm_on = False

    def token_fsm_states(self, b):
        """the current states of rows 0..b-1 (omchat_amd.fsm.DEAD included); synchronises"""
        torch = _torch()
        out = torch.zeros(int(b), dtype=torch.int32)
        check(self.lib.omchat_fsm_states(self.h, int(b), ptr(out), cur_stream()))
        return [int(x) for x in out]

    # ------------------------------------------------------------------ classifier-free guidance (include/omchat_hip.h: omchat_set_guidance)
    def set_guidance(self, b, scale):
        """rows 0..b-1 are conditional rows and rows b..2b-1 their twins over the negative prompt: argmax, sample, decode_step and kv_rewind
        then take exactly 2b rows and pick b ids from scale * (lc - lu) + lu; the returned ids have 2b entries, the
        twins' equal to their rows'.  Sampling, constraints, the token FSM and the log-prob record keep taking b.  Sticky until
        guidance_off() (or b = 0); the same b and scale keep the captured decode graphs."""
        check(self.lib.omchat_set_guidance(self.h, int(b), float(scale), cur_stream()))
        self._guidance_on = int(b) > 0

    def guidance_off(self):
        if vars(self).get("_guidance_on", False):
            check(self.lib.omchat_set_guidance(self.h, 0, 1.0, cur_stream()))
        self._guidance_on = False

    def guidance(self, logits, b, scale, out=None):
        """the stage alone (omchat_op_guidance): logits fp32 [2b, ld] (any row stride >= V = logits.shape[1]) -> guided scores fp32 [b, V]"""
        torch = _torch()
        V = logits.shape[1]
        ws = torch.empty(max(int(self.lib.omchat_op_guidance_ws(int(b), int(V))), 16), dtype=torch.uint8, device=self.device)
        out = out if out is not None else torch.empty(b, V, dtype=torch.float32, device=self.device)
        check(self.lib.omchat_op_guidance(ptr(logits), int(logits.stride(0)), int(b), int(V), float(scale), ptr(ws), ptr(out), int(out.stride(0)),
                                          cur_stream()))
        torch.cuda.current_stream().synchronize()      # (ws is released when this returns)
        return out

    # ------------------------------------------------------------------ layer-contrastive decoding (include/omchat_hip.h: omchat_set_dola)
    def set_dola(self, b, layers, relative_top=0.1, norm=False):
        """every following prefill and decode step of rows 0..b-1 also keeps the rows' last-position hidden state at `layers` (indices into
        HF's hidden_states: 0 = the embeddings, i = behind decoder layer i) and pushes them through the head with the final row; every pick
        then runs on the relative-top-filtered contrast of the final row with the candidate of the largest Jensen-Shannon divergence from
        it.  Call it BEFORE the prefill whose logits pick the first token.  Begins a new record (dola_record).
        Sticky until dola_off() (or b = 0); the same arguments keep the captured decode graphs."""
        torch = _torch()
        ls = torch.tensor([int(i) for i in layers] or [0], dtype=torch.int32)
        check(self.lib.omchat_set_dola(self.h, int(b), ptr(ls), len(layers), float(relative_top), int(bool(norm)), cur_stream()))
        self._dola = (int(b), len(layers)) if int(b) > 0 else None

    def dola_off(self):
        if vars(self).get("_dola", None) is not None:
            check(self.lib.omchat_set_dola(self.h, 0, None, 0, 0.1, 0, cur_stream()))
        self._dola = None

    def dola_rows(self):
        """test hook: the raw logits [(k + 1) * b, V] of the last prefill or step on the host -- rows [0, b) the final rows, row
        (1 + j) * b + r candidate j of sequence r (synchronises)"""
        torch = _torch()
        b, k = self._dola
        out = torch.empty((k + 1) * b, self.c.t_vocab, dtype=torch.float32)
        check(self.lib.omchat_dola_rows(self.h, ptr(out)))
        return out

    def dola_record(self, rows, steps):
        """int64 [rows, steps] on the host: the HF index of the layer every pick since set_dola contrasted with, -1 where a row has no such
        pick (synchronises)"""
        torch = _torch()
        out = torch.full((int(rows), max(int(steps), 1)), -1, dtype=torch.int32)
        check(self.lib.omchat_dola_read(self.h, ptr(out), int(rows), max(int(steps), 1)))
        return out[:, :int(steps)].to(torch.int64)

    def dola(self, logits, b, k, relative_top=0.1, out=None):
        """the stage alone (omchat_op_dola): logits fp32 [(k + 1) * b, ld] (any row stride >= V = logits.shape[1]) -> (scores fp32 [b, V],
        the picked candidate positions int32 [b])"""
        torch = _torch()
        V = logits.shape[1]
        n = max(int(self.lib.omchat_op_dola_ws(int(b), int(k), int(V))), 16)
        ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        out = out if out is not None else torch.empty(b, V, dtype=torch.float32, device=self.device)
        picked = torch.empty(b, dtype=torch.int32, device=self.device)
        check(self.lib.omchat_op_dola(ptr(logits), int(logits.stride(0)), int(V), int(b), int(k), float(relative_top), ptr(out), int(out.stride(0)),
                                      ptr(picked), ptr(ws), n, cur_stream()))
        torch.cuda.current_stream().synchronize()      # (ws is released when this returns)
        return out, picked

    # ------------------------------------------------------------------ contrastive search (include/omchat_hip.h: omchat_set_contrastive)
    def set_contrastive(self, k, alpha, max_new, share=False, eos=()):
        """contrastive search for ONE sequence.  Call it BEFORE the b = 1 prefill, which then keeps its post-final-norm
        hidden rows as the history; then contrastive_step(prefill logits), and per emitted id decode_step(candidates) +
        contrastive_step(its logits).  Sticky until contrastive_off()."""
        torch = _torch()
        ev = torch.tensor([int(i) for i in eos] or [0], dtype=torch.int32)
        check(self.lib.omchat_set_contrastive(self.h, int(k), float(alpha), int(max_new), int(bool(share)), ptr(ev), len(eos), cur_stream()))
        self._cs = (int(k), int(max_new))
        self.contrastive_done = torch.zeros(1, dtype=torch.int32, device=self.device)

    def contrastive_off(self):
        if vars(self).get("_cs", None) is not None:
            check(self.lib.omchat_set_contrastive(self.h, 0, 0.0, 0, 0, None, 0, cur_stream()))
        self._cs = None

    def contrastive_step(self, logits):
        """logits fp32 [1, V] of the prefill (the first call: top-k and the fork of the prompt row) or [k, V] of the k-row decode step over
        the candidates (pick, commit, next top-k) -> int32 [k + 1] on the device: the k candidates of the next step, then the emitted id
        (-1 from the first call); self.contrastive_done turns 1 on an EOS id or the last of max_new ids.  Nothing synchronises."""
        torch = _torch()
        k, _ = self._cs
        if not hasattr(self, "_cs_out") or self._cs_out.shape[0] != k + 1:
            self._cs_out = torch.empty(k + 1, dtype=torch.int32, device=self.device)
        lg = logits if logits.is_contiguous() else logits.contiguous()
        check(self.lib.omchat_contrastive_step(self.h, ptr(lg), lg.shape[0], ptr(self._cs_out), ptr(self.contrastive_done), cur_stream()))
        self._prefix = None      # the rows changed hands
        return self._cs_out

    def contrastive_record(self, steps):
        """the record of the first `steps` picks since the prefill (synchronises): dict of numpy arrays -- ids / probs / penalties
        [steps, k], pick, token, chunks, rows [steps] (omchat_amd/contrastive.py: unpack_record)"""
        torch = _torch()
        from .contrastive import REC_WORDS, unpack_record
        out = torch.zeros(max(int(steps), 1), REC_WORDS, dtype=torch.int32)
        check(self.lib.omchat_contrastive_read(self.h, ptr(out), int(steps)))
        return unpack_record(out[:int(steps)].numpy(), self._cs[0])

    def contrastive_rows(self, row0, n, want_cand=True):
        """test hook: (history rows [n, H], their inverse norms fp32 [n], the last k-row step's final-normed rows [k, H]) on the host"""
        torch = _torch()
        H = self.c.t_hidden
        hist = torch.zeros(max(n, 1), H, dtype=self.torch_dtype)
        inv = torch.zeros(max(n, 1), dtype=torch.float32)
        cand = torch.zeros(self._cs[0], H, dtype=self.torch_dtype) if want_cand else None
        check(self.lib.omchat_contrastive_rows(self.h, int(row0), int(n), ptr(hist), ptr(inv), ptr(cand)))
        return hist[:n], inv[:n], cand

    def contrastive_plan(self, L):
        """(chunks, rows_per_chunk) of the penalty launch over L history rows on this device"""
        ch, rpc = C.c_int(0), C.c_int(0)
        check(self.lib.omchat_op_contrastive_plan(int(L), C.byref(ch), C.byref(rpc)))
        return ch.value, rpc.value

    def contrastive_penalty(self, hist, cand, cand_nb=0, k=None, inv=None):
        """the penalty launch alone (omchat_op_contrastive_penalty): hist 16-bit [L, H], cand 16-bit [k, H] row-major (or the packed buffer
        with cand_nb blocks and k given), inv fp32 [L] or None (then computed by the norms launch) -> (partial maxima fp32 [chunks, 16],
        the candidates' inverse norms fp32 [16], inv fp32 [L]), all on the device"""
        torch = _torch()
        L, H = hist.shape
        k = int(k if k is not None else cand.shape[0])
        chunks, _ = self.contrastive_plan(L)
        part = torch.full((chunks, 16), float("nan"), dtype=torch.float32, device=self.device)
        cinv = torch.zeros(16, dtype=torch.float32, device=self.device)
        comp = inv is None
        inv = inv if inv is not None else torch.empty(L, dtype=torch.float32, device=self.device)
        check(self.lib.omchat_op_contrastive_penalty(_lib.dtype_code(hist.dtype), ptr(hist), ptr(inv), int(comp), L, H, ptr(cand), int(cand_nb), k,
                                                     ptr(part), ptr(cinv), cur_stream()))
        return part, cinv, inv

    def contrastive_topk(self, logits, V, k, row_sel=None):
        """the top-k launch alone (omchat_op_contrastive_topk): logits fp32 [rows, ld], the first V ids of row *row_sel (device int32 [1];
        None = row 0) -> (ids int32 [k], probs fp32 [k]) on the device"""
        torch = _torch()
        n = max(int(self.lib.omchat_op_contrastive_topk_ws(int(V))), 16)
        ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        ids = torch.empty(k, dtype=torch.int32, device=self.device)
        probs = torch.empty(k, dtype=torch.float32, device=self.device)
        check(self.lib.omchat_op_contrastive_topk(ptr(logits), int(logits.stride(0)), ptr(row_sel), int(V), int(k), ptr(ids), ptr(probs), ptr(ws),
                                                  cur_stream()))
        torch.cuda.current_stream().synchronize()      # (ws is released when this returns)
        return ids, probs

    def contrastive_select(self, part, k, alpha, ids, probs, cand_inv, cand=None, cand_nb=0, hist=None, inv=None, n_hist=0, eos=(), last=False):
        """the select-and-commit launch alone (omchat_op_contrastive_select) -> dict(rec int32 [REC_WORDS], parents int32 [k], sel, token,
        done int32 [1]) on the device; with hist / inv / cand the picked row is appended at row n_hist"""
        torch = _torch()
        from .contrastive import REC_WORDS
        dev = self.device
        out = dict(rec=torch.zeros(REC_WORDS, dtype=torch.int32, device=dev), parents=torch.full((k,), -1, dtype=torch.int32, device=dev),
                   sel=torch.full((1,), -1, dtype=torch.int32, device=dev), token=torch.full((1,), -1, dtype=torch.int32, device=dev),
                   done=torch.full((1,), -1, dtype=torch.int32, device=dev))
        ev = torch.tensor([int(i) for i in eos] or [0], dtype=torch.int32)
        H = int(cand.shape[-1]) if (cand is not None and cand_nb == 0) else (int(hist.shape[1]) if hist is not None else 0)
        check(self.lib.omchat_op_contrastive_select(self.dtype_code, ptr(part), int(part.shape[0]), int(k), float(alpha), ptr(ids), ptr(probs),
                                                    ptr(cand_inv), ptr(cand), int(cand_nb), H, ptr(hist), ptr(inv), int(n_hist), ptr(ev), len(eos),
                                                    int(bool(last)), ptr(out["rec"]), ptr(out["parents"]), ptr(out["sel"]), ptr(out["token"]),
                                                    ptr(out["done"]), cur_stream()))
        return out

    # ------------------------------------------------------------------ sampled groups (include/omchat_hip.h: omchat_group_begin)
    def group_share_refusal(self, N):
        """why the shared-prompt form is not available for N rows per prompt on this engine, or None (host data only)"""
        return group_share_refusal(getattr(self, "_fp8_kv", False), self.tp_size, self.c.t_heads, self.c.t_kv_heads, int(N))

    def group_share_default(self, N, prompt_len):
        """the engine's rule for share_prompt=None: available and prompt_len >= GROUP_SHARE_P_MIN (None: never)"""
        return self.group_share_refusal(N) is None and GROUP_SHARE_P_MIN is not None and int(prompt_len) >= GROUP_SHARE_P_MIN

    def group_begin(self, b, N, prompt_len=None, share=False):
        """after the prefill of b equal-length prompts: b * N rows, prompt-major, every row prompt_len keys long.  share=False: the prompt's
        slots are forked into every row and decode_step(b * N) runs as on any batch; share=True: only each group's first row holds the
        prompt and decode_step reads it once per group until the next prefill (or group_end)."""
        P = prompt_len if prompt_len is not None else self.kv_lengths(b)[0]
        check(self.lib.omchat_group_begin(self.h, int(b), int(N), int(P), int(bool(share)), cur_stream()))
        self._prefix = None      # the rows changed hands

    def group_end(self):
        check(self.lib.omchat_group_begin(self.h, 0, 0, 0, 0, cur_stream()))

    # ------------------------------------------------------------------ beam search (include/omchat_hip.h: omchat_beam_begin)
    def beam_begin(self, b, num_beams, length_penalty=1.0, early_stopping=False, eos=(), max_new=20, prompt_len=None):
        """after the prefill of b equal-length prompts: HF's _beam_search state on the device.  early_stopping: False, True or "never"."""
        torch = _torch()
        es = 2 if early_stopping == "never" else int(bool(early_stopping))
        ev = torch.tensor(list(eos) or [0], dtype=torch.int32)
        P = prompt_len if prompt_len is not None else self.kv_lengths(b)[0]
        check(self.lib.omchat_beam_begin(self.h, int(b), int(num_beams), float(length_penalty), es, ptr(ev), len(eos), int(max_new), int(P),
                                         cur_stream()))
        self._beam = (int(b), int(num_beams), int(max_new))
        self._prefix = None      # the fork overwrites sequence 0's row
        self.beam_done = torch.zeros(1, dtype=torch.int32, device=self.device)

    def beam_processors(self, prompt, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, min_length=0,
                        suppress_tokens=(), begin_suppress_tokens=()):
        """between beam_begin and the first beam_step: the search ranks processed scores, as HF's _beam_search does -- the repetition
        penalty on the log-probabilities of the ids of each beam's own history, then HF's token bans (the lists of set_constraints; the
        EOS ids are the search's own).  prompt: the b equal-length prompt rows as HF's processors see them (-200 sentinels included).
        A penalty of 1 with nothing to ban leaves the search plain."""
        torch = _torch()
        i32 = lambda xs: torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)
        words = [list(w) for w in (bad_words_ids or [])]
        off = [0]
        for w in words:
            off.append(off[-1] + len(w))
        sup, bsup = list(suppress_tokens or ()), list(begin_suppress_tokens or ())
        rows = [list(r) for r in prompt]
        bm = vars(self).get("_beam")      # (None: no beam_begin yet -- the context refuses the call)
        if not rows or len({len(r) for r in rows}) != 1 or not rows[0] or (bm is not None and len(rows) != bm[0]):
            raise ValueError("beam_processors: one prompt row per prompt of the search, all of one length >= 1")
        t_sup, t_bsup, t_bw, t_off = i32(sup), i32(bsup), i32([i for w in words for i in w]), i32(off)
        t_ids = i32([i for r in rows for i in r])
        check(self.lib.omchat_beam_processors(self.h, float(repetition_penalty), int(no_repeat_ngram_size or 0), int(min_new_tokens or 0),
                                              int(min_length or 0), ptr(t_sup), len(sup), ptr(t_bsup), len(bsup), ptr(t_bw), ptr(t_off), len(words),
                                              ptr(t_ids), len(rows[0]), cur_stream()))

    def beam_step(self, logits):
        """one beam step on rank-local logits [rows, V / tp] (the prefill's b rows first, then the b * num_beams beam rows) -> the next
        tokens of the b * num_beams rows (int32, device); self.beam_done turns 1 once every prompt is done"""
        torch = _torch()
        b, N, _ = self._beam
        out = torch.empty(b * N, dtype=torch.int32, device=self.device)
        check(self.lib.omchat_beam_step(self.h, ptr(logits), logits.shape[0], ptr(out), ptr(self.beam_done), cur_stream()))
        return out

    def beam_result(self, num_return=1):
        """-> (list of b * num_return generated id lists, best first per prompt, scores fp32 numpy [b * num_return])"""
        torch = _torch()
        b, N, max_new = self._beam
        toks = torch.zeros(b * num_return, max_new, dtype=torch.int32)
        lens = torch.zeros(b * num_return, dtype=torch.int32)
        scores = torch.zeros(b * num_return, dtype=torch.float32)
        check(self.lib.omchat_beam_result(self.h, int(num_return), ptr(toks), ptr(lens), ptr(scores), max_new))
        return [toks[o, :int(lens[o])].tolist() for o in range(b * num_return)], scores.numpy()
