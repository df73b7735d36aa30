"""Packed-stream execution of the hot path on the HIP library (host orchestration only).

The mirror modules in `acai_omr_amd.models` keep the reference's nn.Module surface and state_dict keys; their
parameters live in stock torch containers (nn.TransformerEncoder/Decoder are used as PARAMETER CONTAINERS only,
their forward is never called).  This file turns those parameters into kernel launches:

  encoder_stack   post-LN ViT blocks on a packed token stream (cu_seqlens, no padding)   [models.py:30-34,76-79]
  DecodeEngine    cross-K/V prefill + hipGraph-replayed greedy decode                      [kv_caching.py:190-302, models.py:562-615]

Precision ("fp32" | "bf16") follows the reference plumbing: fp32 = outside autocast; bf16 = what
torch.autocast(bfloat16) does to linear / SDPA (bf16 operands and outputs, fp32 accumulate, fp32 residual + LayerNorm).
"""
import contextlib
import ctypes
import os

import weakref

import torch

from . import _lib, ops
from .scheduler import SlotScheduler


class WeightCache:
    """bf16 operand copies of fp32 master parameters (autocast's weight cast, done once instead of per call) and
    bf16-rounded fp32 biases.  Entries are refreshed when the parameter's version counter or storage changes."""

    def __init__(self):
        self._c = {}

    # derived data keyed on parameter identity: a copied / pickled module starts with an empty cache
    def __deepcopy__(self, memo):
        return WeightCache()

    def __reduce__(self):
        return (WeightCache, ())

    def invalidate(self):
        """Drop every cached copy.  Needed after writes that do not move a parameter's version counter (`p.data.copy_`, EMA through `.data`,
        weight surgery): the cache keys on (version, storage pointer).  `load_state_dict` and optimizer steps bump versions and need no call."""
        self._c.clear()

    def _get(self, p, kind, make):
        key = (id(p), kind)
        tag = (p._version, p.data_ptr())
        hit = self._c.get(key)
        if hit is not None and hit[0] != tag and kind in self._BATCHED and p.is_cuda and not torch.cuda.is_current_stream_capturing():
            self._refresh_stale(p.device)      # an optimizer step went by: every stale copy on this device in ONE launch
            hit = self._c.get(key)
        if hit is None or hit[0] != tag:
            with torch.no_grad():
                hit = (tag, make(p.detach()), weakref.ref(p))
            self._c[key] = hit
        return hit[1]

    _BATCHED = ("w16", "wtbf16", "b16")

    def _refresh_stale(self, device):
        """Rebuild every cached bf16 / transposed-bf16 / rounded-bias copy whose parameter moved on (version or storage) with one
        `acai_cast_weights` launch (through ATen: one cast or copy launch per tensor and kind, ~300 per training step).  Fresh output tensors:
        a copy still referenced by an autograd graph keeps its old values."""
        groups = {}
        for (pid, kind), (tag, _, ref) in list(self._c.items()):
            p = ref()
            if p is None:
                del self._c[(pid, kind)]
                continue
            if kind not in self._BATCHED or p.device != device or tag == (p._version, p.data_ptr()):
                continue
            if p.dtype != torch.float32 or not p.is_contiguous() or p.dim() != (1 if kind == "b16" else 2):
                continue
            groups.setdefault(pid, (p, set()))[1].add(kind)
        if not groups:
            return
        order = list(groups.values())
        with torch.no_grad():
            outs = ops.cast_weights([(p.detach(), "w16" in ks, "wtbf16" in ks, "b16" in ks) for p, ks in order])
        for (p, ks), (d16, d16t, d32) in zip(order, outs):
            tag = (p._version, p.data_ptr())
            for kind, t in (("w16", d16), ("wtbf16", d16t), ("b16", d32)):
                if kind in ks:
                    self._c[(id(p), kind)] = (tag, t, weakref.ref(p))

    def w(self, p, prec):
        if prec == "fp32":
            return p.detach()
        return self._get(p, "w16", lambda t: t.to(torch.bfloat16).contiguous())

    def wt(self, p, prec):
        """Transposed operand copy [in_features, out_features] in the compute dtype: turns dX = dY . W into the row-major
        (direct-to-LDS) GEMM form; refreshed when the parameter changes (once per optimizer step)."""
        dt = torch.bfloat16 if prec == "bf16" else torch.float32
        def make(t):
            out = torch.empty((t.shape[1], t.shape[0]), dtype=dt, device=t.device)  # fresh row-major strides even for size-1 dims
            out.copy_(t.t())
            return out
        return self._get(p, "wt" + prec, make)

    def b(self, p, prec):
        if p is None:
            return None
        if prec == "fp32":
            return p.detach()
        return self._get(p, "b16", lambda t: t.to(torch.bfloat16).to(torch.float32).contiguous())


_CU_CACHE = {}


def cu_from_lens(lens, device):
    """int32 cu_seqlens of a packed stream on the device.  Cached per (lengths, device) - a training loop asks for the same few every step -
    and uploaded without a host stall (ops.h2d).  The tensors are read-only for every consumer."""
    key = (tuple(int(l) for l in lens), str(device))
    hit = _CU_CACHE.get(key)
    if hit is not None:
        return hit
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(key[0], dtype=torch.int32).cumsum(0)
    out = ops.h2d(cu, device)
    if len(_CU_CACHE) >= 256:
        _CU_CACHE.clear()
    _CU_CACHE[key] = out
    return out


def linear(x32, xb, lin_w, lin_b, prec, wc, residual=None, gelu=False, out_dtype=None):
    """One nn.Linear on a packed stream.  Picks the bf16 copy of the activation in bf16 mode."""
    bf = prec == "bf16"
    a = xb if bf else x32
    if bf and a is None:
        a = ops.cast_bf16(x32)
    if out_dtype is None:
        out_dtype = torch.float32 if residual is not None else (torch.bfloat16 if bf else torch.float32)
    return ops.gemm_nt(a, wc.w(lin_w, prec), wc.b(lin_b, prec), residual=residual, out_dtype=out_dtype, gelu=gelu, round_bf16=bf)


def encoder_stack(stack, x32, xb, cu, max_len, num_heads, prec, wc):
    """nn.TransformerEncoder (post-LN, GELU) on a packed stream.  x32 (M,E) fp32 residual stream, xb its bf16 copy (bf16 mode)."""
    bf = prec == "bf16"
    E = x32.shape[1]
    dh = E // num_heads
    for layer in stack.layers:
        sa = layer.self_attn
        qkv = linear(x32, xb, sa.in_proj_weight, sa.in_proj_bias, prec, wc)
        attn = ops.attn_varlen(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], cu, cu, num_heads, dh, max_len)
        y = linear(None, attn, sa.out_proj.weight, sa.out_proj.bias, prec, wc, residual=x32) if bf else \
            linear(attn, None, sa.out_proj.weight, sa.out_proj.bias, prec, wc, residual=x32)
        x32, xb = ops.layernorm(y, layer.norm1.weight.detach(), layer.norm1.bias.detach(), layer.norm1.eps, want_bf16=bf)
        h = linear(x32, xb, layer.linear1.weight, layer.linear1.bias, prec, wc, gelu=True)
        y = linear(None, h, layer.linear2.weight, layer.linear2.bias, prec, wc, residual=x32) if bf else \
            linear(h, None, layer.linear2.weight, layer.linear2.bias, prec, wc, residual=x32)
        x32, xb = ops.layernorm(y, layer.norm2.weight.detach(), layer.norm2.bias.detach(), layer.norm2.eps, want_bf16=bf)
    if stack.norm is not None:
        x32, xb = ops.layernorm(x32, stack.norm.weight.detach(), stack.norm.bias.detach(), stack.norm.eps, want_bf16=bf)
    return x32, xb


def pad_rows(packed, lens, fill_row=None):
    """packed (M,E) fp32 -> (B, Lmax, E) through one row-gather launch; padded rows take `fill_row` (default zeros)."""
    B, Lm, E = len(lens), max(lens), packed.shape[1]
    M = packed.shape[0]
    ext = torch.empty(M + 1, E, dtype=torch.float32, device=packed.device)
    ext[:M] = packed
    if fill_row is None:
        ext[M].zero_()
    else:
        ext[M] = fill_row
    idx = torch.full((B, Lm), M, dtype=torch.int32)
    mask = torch.ones(B, Lm, dtype=torch.bool)
    o = 0
    for b, l in enumerate(lens):
        idx[b, :l] = torch.arange(o, o + l, dtype=torch.int32)
        mask[b, :l] = False
        o += l
    out = ops.gather_rows(ext, idx.reshape(-1).to(packed.device))
    return out.view(B, Lm, E), mask.to(packed.device)


def unpad_rows(padded, mask):
    """(B, Lmax, E) + mask (True = padding, suffix-shaped as create_attention_mask makes it) -> packed (M,E), lens."""
    B, Lm, E = padded.shape
    if mask is None:
        return padded.reshape(B * Lm, E).float().contiguous(), [Lm] * B
    lens = (~mask).sum(dim=1).tolist()
    m = mask.cpu()
    for b, l in enumerate(lens):
        if bool(m[b, :l].any()):
            raise ValueError("latent_attention_mask must mark a suffix of each row as padding (as Encoder.create_attention_mask does)")
    idx = torch.cat([torch.arange(b * Lm, b * Lm + l, dtype=torch.int32) for b, l in enumerate(lens)]).to(padded.device)
    return ops.gather_rows(padded.reshape(B * Lm, E).float().contiguous(), idx), lens


class DecodeEngine:
    """Owns the KV caches, workspaces and hipGraphs of one CachedTransformerDecoder-equivalent."""

    # keys per cross-attention workgroup (split over the memory, merged in the launch).  1024 (4 splits of S = 4096, 512 workgroups) measured
    # +2.8 % tokens/s over 512 on the same box; 256 and 2048 are slower.  ACAI_CROSS_CHUNK overrides (A/B aid).
    CROSS_CHUNK = int(os.environ.get("ACAI_CROSS_CHUNK", "1024"))
    CROSS_SLOTS = 512   # cross-attention workgroups resident at once (two per CU on 256 CUs)
    # the same for an FP8 memory cache (68-byte key rows instead of 128): ACAI_CROSS_CHUNK_FP8 pins it (A/B aid)
    CROSS_CHUNK_FP8 = 1024

    @classmethod
    def pick_cross_chunk_fp8(cls, lens, H):
        if "ACAI_CROSS_CHUNK_FP8" in os.environ:
            return int(os.environ["ACAI_CROSS_CHUNK_FP8"])
        return cls.CROSS_CHUNK_FP8

    @classmethod
    def pick_cross_chunk(cls, lens, H):
        """Keys per cross-attention workgroup for this batch.  A uniform batch of 8 x 4096 gives 4 x 8 x 16 = 512 workgroups of 1024 keys: one
        full round of the chip.  A RAGGED batch does not: config 4 (1024 ... 9216 patches) makes 624 workgroups of 1024 keys - a second, mostly
        empty round.  The chunk is therefore the multiple of 64 that minimises rounds x keys per workgroup (ties go to CROSS_CHUNK): 1344 keys
        = 512 workgroups for config 4.  ACAI_CROSS_CHUNK pins it (A/B aid)."""
        if "ACAI_CROSS_CHUNK" in os.environ or not lens:
            return cls.CROSS_CHUNK
        best, best_cost = cls.CROSS_CHUNK, None
        for c in [cls.CROSS_CHUNK] + list(range(512, 4096 + 1, 64)):
            n = sum(-(-l // c) for l in lens) * H
            cost = -(-n // cls.CROSS_SLOTS) * (min(c, max(lens)) + 72)   # + ~72 keys' worth of per-workgroup cost (512- against 1024-key chunks on 8 x 4096: -2.8 % tokens/s)
            if best_cost is None or cost < best_cost:
                best, best_cost = c, cost
        return best

    def __init__(self, blocks, omr, max_batch_size, max_len, prec, device, memory_fp8=False):
        self.blocks = blocks        # CachedTransformerDecoder mirror (layers, norm): parameters are read from it
        self.omr = omr              # OMRDecoder mirror (embedding, positions, unembed) or None
        self.prec = prec
        self.bf = prec == "bf16"
        self.cdt = torch.bfloat16 if self.bf else torch.float32
        self.device = device
        self.Bmax, self.Tmax = int(max_batch_size), int(max_len)
        self.L = len(blocks.layers)
        self.E = blocks.layers[0].hidden_dim
        self.H = blocks.layers[0].num_heads
        self.dh = self.E // self.H
        es = 2 if self.bf else 4
        dhp = max(16 // es, 1)
        while dhp < self.dh:
            dhp *= 2
        self.dhp = dhp
        # FP8 memory cache (bf16 engines only): the cross K/V is e4m3fn with one fp32 scale per row, rows of cdhp = max(dhp, 16) elements;
        # every layer's prefill goes through one reused bf16 region (k_stage / v_stage) and is then quantised into the layer's buffers
        self.cross_fp8 = bool(memory_fp8)
        if self.cross_fp8 and not self.bf:
            raise TypeError("an FP8 memory cache needs cache_dtype=torch.bfloat16")
        self.cdhp = max(dhp, 16) if self.cross_fp8 else dhp
        self.k_cross_scale = self.v_cross_scale = None
        self.k_stage = self.v_stage = None
        self.F = blocks.layers[0].linear1.out_features
        self.V = omr.vocab_size if omr is not None else 1
        self.wc = WeightCache()
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        self.k_self = [z(self.Bmax, self.H, self.Tmax, dhp, dt=self.cdt) for _ in range(self.L)]
        self.v_self = [z(self.Bmax, self.H, self.Tmax, dhp, dt=self.cdt) for _ in range(self.L)]
        self.step = z(2, dt=torch.int32)
        self.finished = z(self.Bmax + 1, dt=torch.int32)
        self.seqs = z(self.Bmax, self.Tmax, dt=torch.int64)
        self.logprobs = z(self.Bmax, self.Tmax)
        self.cross_off = z(self.Bmax, dt=torch.int64)
        self.cross_len = z(self.Bmax, dt=torch.int32)
        self.ws = dict(x=z(self.Bmax, self.E), xn=z(self.Bmax, self.E), qkv=z(self.Bmax, 3 * self.E), attn=z(self.Bmax, self.E),
                       proj=z(self.Bmax, self.E), hid=z(self.Bmax, self.F), logits=z(self.Bmax, self.V))
        self.stats = z(6 * self.Bmax)
        self.tickets = z(self.Bmax * self.H, dt=torch.int32)   # self-resetting arrival counters (in-launch split merge)
        # self-attention: one workgroup per (sequence, head) walks the whole cache (t <= 1536 keys) and writes the output
        # itself - no split, no combine launch
        self.SELF_CHUNK = self.Tmax
        self.self_nsplit = 1
        self.partial = None
        self.k_cross = self.v_cross = None
        self.cross_cap = 0
        self.graphs = {}
        self.stream = torch.cuda.Stream(device=device)  # capture / replay stream (the legacy default stream cannot capture)
        self.B = 0
        self.lens = None
        self.group = 1          # decode rows per stored cross K/V (GRPO rollout groups)
        # what a decode step does: ("greedy",), ("sample", top_k, temperature), ("beam", K), ("slot",) (continuous batching),
        # ("slot_sample", top_k, temperature) (continuous batching, sampled), ("spec", D, ngram) (speculative greedy; ngram 0 = drafts from
        # the injected table), ("prompt",) (greedy from given tokens) or ("spec", D, ngram, "prompt") (the two together); a run sets it and
        # restores greedy when it ends.  Grammar-constrained decoding: ("grammar",), ("grammar_sample", top_k, temperature), ("slot_grammar",),
        # ("slot_grammar_sample", top_k, temperature) - the four forms above with the token choice masked by a token automaton.  Loop guard:
        # ("loop", P, R, M) and ("slot_loop", P, R, M) - greedy and slot with the guard's check in the selection launch
        self._mode = ("greedy",)
        self.uniforms = None    # (Bmax, Tmax) uniforms of the sampling step, allocated on first use
        self.beam_anc = None    # beam-search lineage [2][Bmax][Tmax] (anc / tok / lp) and per-row cum / len, allocated on first use
        self._beam_done = 0
        self.slot_t = None      # slot state [Bmax] x 3 (local time, ring start, cap), allocated on first use
        self.slot_steps = 0     # decode steps of the last continuous-batching run (the ring index wrapped slot_steps // Tmax times)
        self.slot_busy = 0      # busy slots summed over those steps (mean occupancy = slot_busy / slot_steps)
        self.slot_polls = 0     # polls of that run (host syncs: one per poll, streamed or not)
        self.slot_urow = None   # sampled slot mode: [Bmax] int32 uniforms row of the sequence in each slot, and the (rows, Tmax) table
        self.slot_uniforms = None
        self.slot_mark = None   # streamed slot mode: [Bmax] int32 first index of each slot not yet sent, the flush buffer and its pinned twin
        self._flush_dev = self._flush_host = None
        self._flush_ld = 0      # entries per slot of that buffer while a streamed run is on (its flush interval), else 0
        self.spec_t = None      # speculative decoding: per-image state (t, cap, steps, key table, next inputs, injected drafts), allocated on first use
        self.prompt_tok = None  # prompted decoding: (Bmax, Tmax) int32 tokens by output index and (Bmax,) int32 lengths, allocated on first use
        self._mem = None        # the packed memories of the last prepare() (mem32, memb): a prompt prefill's pass reads them again
        self.prefilled_tokens = 0   # prompt tokens (rows x depth) that prefilled runs took in their pass instead of in prompt steps, so far
        self.gram_next = None   # grammar-constrained decoding: engine-owned copies of the automaton's tables and the rows' states (_set_grammar)
        self.loop_run = None    # loop guard: (Bmax, 64) int32 run counters and the (3, Bmax) int32 report (stop, period, start), allocated on first use (_set_loop)
        self.cont_loops = None  # the report of the last guarded continuous-batching run, (3, N) int32 per image
        self._per_row_cross = False
        self.cache_len = 0
        self._desc = None
        self._keep = None

    # ---- cross K/V prefill (MemoryCache.cache_memory_keys_and_vals, kv_caching.py:235-253) -----------------------------
    def prepare(self, mem32, memb, lens, group_size=1, per_row_cross=False):
        """mem32 / memb: packed memory (M, E) fp32 / bf16 copy; lens: per-memory lengths.  group_size > 1: every memory serves `group_size`
        consecutive decode rows (the rollouts of one image, models.py:883-891) - its cross K/V is projected and stored ONCE and the rows'
        offsets alias it, instead of the reference's group_size materialised copies.  per_row_cross (speculative decoding): the rows of a
        group go through the per-row cross-attention kernel at the split an ungrouped batch of these memories gets, so that every row's
        arithmetic is the plain greedy step's."""
        G = int(group_size)
        B = len(lens) * G
        self._mode = ("greedy",)
        if B > self.Bmax:
            raise ValueError(f"The current cache has been setup with a max batch size of {self.Bmax}, but found new key tensors with batch size {B}!")
        if G > 1 and self.cross_fp8:
            raise ValueError("an FP8 memory cache does not support grouped cross K/V (group_size > 1: beam search, grouped GRPO rollouts); "
                             "use memory_cache_dtype=None")
        E, H, dhp, dev = self.E, self.H, self.cdhp, self.device
        self._size_cross(sum(lens) * H * dhp, B, lens, 1 if per_row_cross else G)
        self._per_row_cross = bool(per_row_cross)
        offs, o = [], 0
        for l in lens:
            offs.append(o)
            o += l * H * dhp
        self.cross_off[:B] = torch.tensor(offs, dtype=torch.int64).repeat_interleave(G)
        self.cross_len[:B] = torch.tensor(lens, dtype=torch.int32).repeat_interleave(G)
        # the prefill scatters by MEMORY index: its own (ungrouped) offset / length tables
        pre_off, pre_len = torch.tensor(offs, dtype=torch.int64).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
        row_seq = torch.cat([torch.full((l,), b, dtype=torch.int32) for b, l in enumerate(lens)]).to(dev)
        row_pos = torch.cat([torch.arange(l, dtype=torch.int32) for l in lens]).to(dev)
        mem = memb if self.bf else mem32
        if mem is None:
            mem = ops.cast_bf16(mem32)
        for i, layer in enumerate(self.blocks.layers):
            ca = layer.multihead_attn
            w = self.wc.w(ca.in_proj_weight, self.prec)[E:]
            b = self.wc.b(ca.in_proj_bias, self.prec)[E:]
            if self.cross_fp8:
                ops.cross_kv_prefill(mem, w, b, row_seq, row_pos, pre_off, pre_len, self.k_stage, self.v_stage, H, self.dh, dhp, round_bf16=True)
                ops.cross_kv_quantize_fp8(self.k_stage, self.v_stage, self.k_cross[i], self.v_cross[i], self.k_cross_scale[i],
                                          self.v_cross_scale[i], 0, sum(lens) * H, dhp)
            else:
                ops.cross_kv_prefill(mem, w, b, row_seq, row_pos, pre_off, pre_len, self.k_cross[i], self.v_cross[i],
                                     H, self.dh, dhp, round_bf16=self.bf)
        self.B, self.lens, self.group = B, [l for l in lens for _ in range(G)], G
        self._mem = (mem32, memb)
        self.reset_self_cache()
        self._build_desc()

    def _size_cross(self, total, B, lens, group=1):
        """Cross K/V buffers of at least `total` elements per layer, the cross split (keys per workgroup, splits) of memories of lengths
        `lens` shared by `group` rows each, and `partial` for B rows at that split.  A reallocation drops the captured graphs."""
        H, dhp, dev = self.H, self.cdhp, self.device
        if total > self.cross_cap:
            self.cross_cap = total
            if self.cross_fp8:
                self.k_cross = self.v_cross = self.k_cross_scale = self.v_cross_scale = self.k_stage = self.v_stage = None   # (peak memory)
                self.k_cross = [torch.zeros(total, dtype=torch.float8_e4m3fn, device=dev) for _ in range(self.L)]
                self.v_cross = [torch.zeros(total, dtype=torch.float8_e4m3fn, device=dev) for _ in range(self.L)]
                self.k_cross_scale = [torch.zeros(total // dhp, dtype=torch.float32, device=dev) for _ in range(self.L)]
                self.v_cross_scale = [torch.zeros(total // dhp, dtype=torch.float32, device=dev) for _ in range(self.L)]
                self.k_stage = torch.zeros(total, dtype=torch.bfloat16, device=dev)
                self.v_stage = torch.zeros(total, dtype=torch.bfloat16, device=dev)
            else:
                self.k_cross = [torch.zeros(total, dtype=self.cdt, device=dev) for _ in range(self.L)]
                self.v_cross = [torch.zeros(total, dtype=self.cdt, device=dev) for _ in range(self.L)]
            self.graphs.clear()  # pointers changed
        if self.cross_fp8:
            self.cross_chunk = self.pick_cross_chunk_fp8(lens, H)
        else:
            self.cross_chunk = self.pick_cross_chunk(lens, H) if group == 1 else self.CROSS_CHUNK
        self.cross_nsplit = max(1, -(-max(lens) // self.cross_chunk))
        nsplit = max(self.cross_nsplit, self.self_nsplit)
        if self.partial is None or self.partial.numel() < B * H * nsplit * (dhp + 2):
            self.partial = torch.empty(self.Bmax * H * nsplit * (dhp + 2), dtype=torch.float32, device=dev)
            self.graphs.clear()

    def cross_kv_bytes(self):
        """Bytes of the cross K/V allocation over all layers (values and, for an FP8 memory cache, the per-row scales; not the staging)."""
        ts = list(self.k_cross or []) + list(self.v_cross or []) + list(self.k_cross_scale or []) + list(self.v_cross_scale or [])
        return sum(t.numel() * t.element_size() for t in ts)

    def cross_kv_values(self, layer):
        """Layer `layer`'s cross K and V as the decode step reads them, fp32, flat in the stored layout (an FP8 cache: dequantised)."""
        k, v = self.k_cross[layer], self.v_cross[layer]
        if not self.cross_fp8:
            return k.float(), v.float()
        from .fp8 import dequantize_rows
        d = self.cdhp
        return (dequantize_rows(k.view(-1, d), self.k_cross_scale[layer]).view(-1),
                dequantize_rows(v.view(-1, d), self.v_cross_scale[layer]).view(-1))

    def reset_self_cache(self):
        """KVCache.reset (kv_caching.py:47-51): position back to 0 (stale entries are never read: length is step[1]+1)."""
        self.step.zero_()
        self.cache_len = 0

    def _build_desc(self):
        P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        wc, prec, E = self.wc, self.prec, self.E
        layers = (_lib.AcaiDecLayer * self.L)()
        keep = []
        for i, ly in enumerate(self.blocks.layers):
            sa, ca = ly.self_attn, ly.multihead_attn
            t = dict(self_in_w=wc.w(sa.in_proj_weight, prec), self_in_b=wc.b(sa.in_proj_bias, prec),
                     self_out_w=wc.w(sa.out_proj.weight, prec), self_out_b=wc.b(sa.out_proj.bias, prec),
                     cross_q_w=wc.w(ca.in_proj_weight, prec)[:E], cross_q_b=wc.b(ca.in_proj_bias, prec)[:E],
                     cross_out_w=wc.w(ca.out_proj.weight, prec), cross_out_b=wc.b(ca.out_proj.bias, prec),
                     lin1_w=wc.w(ly.linear1.weight, prec), lin1_b=wc.b(ly.linear1.bias, prec),
                     lin2_w=wc.w(ly.linear2.weight, prec), lin2_b=wc.b(ly.linear2.bias, prec),
                     n1_w=ly.norm1.weight.detach(), n1_b=ly.norm1.bias.detach(), n2_w=ly.norm2.weight.detach(), n2_b=ly.norm2.bias.detach(),
                     n3_w=ly.norm3.weight.detach(), n3_b=ly.norm3.bias.detach(),
                     k_self=self.k_self[i], v_self=self.v_self[i], k_cross=self.k_cross[i], v_cross=self.v_cross[i])
            if self.cross_fp8:
                t.update(k_cross_scale=self.k_cross_scale[i], v_cross_scale=self.v_cross_scale[i])
            for k, v in t.items():
                assert v.is_contiguous() or k.startswith("cross_q"), k
                setattr(layers[i], k, P(v))
            keep.append(t)
        own, nrm = self.omr, self.blocks.norm
        d = _lib.AcaiDecoder()
        d.B, d.E, d.H, d.dh, d.dhp, d.F, d.V, d.L, d.Tmax = self.B, E, self.H, self.dh, self.dhp, self.F, self.V, self.L, self.Tmax
        d.dtype = _lib.ACAI_BF16 if self.bf else _lib.ACAI_F32
        d.flags = (_lib.GEMM_ROUND_BF16 if self.bf else 0) | (_lib.DEC_CROSS_FP8 if self.cross_fp8 else 0)
        d.max_len = self.Tmax
        d.cross_group = self.group
        d.self_chunk, d.cross_chunk, d.self_nsplit, d.cross_nsplit = self.SELF_CHUNK, self.cross_chunk, self.self_nsplit, self.cross_nsplit
        d.layers = ctypes.cast(layers, ctypes.POINTER(_lib.AcaiDecLayer))
        top = {}
        if nrm is not None:
            top.update(fn_w=nrm.weight.detach(), fn_b=nrm.bias.detach())
        if own is not None:
            d.bos, d.pad, d.eos = own.bos_idx, own.pad_idx, own.eos_idx
            top.update(emb=own.vocab_embedding.weight.detach(), pos=own.pos_embedding.detach(),
                       unembed_w=wc.w(own.unembed.weight, prec), unembed_b=wc.b(own.unembed.bias, prec))
        for k, v in top.items():
            assert v.is_contiguous(), k
            setattr(d, k, P(v))
        d.cross_off, d.cross_len = P(self.cross_off), P(self.cross_len)
        d.seqs, d.logprobs, d.step, d.finished = P(self.seqs), P(self.logprobs), P(self.step), P(self.finished)
        for k, v in self.ws.items():
            setattr(d, k, P(v))
        d.partial = P(self.partial)
        d.stats = P(self.stats)
        d.tickets = P(self.tickets)
        sig = tuple(getattr(layers[i], f) for i in range(self.L) for f, _ in _lib.AcaiDecLayer._fields_) + \
            tuple(getattr(d, f) for f, t in _lib.AcaiDecoder._fields_ if t is ctypes.c_void_p)
        if getattr(self, "_sig", None) != sig:
            self.graphs.clear()  # a captured graph holds the old pointers
            self._sig = sig
        self._desc, self._keep = d, (layers, keep, top)

    # ---- CachedTransformerDecoder.cached_generate (kv_caching.py:292-302): hidden state for a caller-supplied embedding --
    def hidden_step(self, x):
        if self.cache_len + 1 > self.Tmax:
            raise AssertionError("KV cache overflow: cache_pos + seq_len exceeds max_seq_len")
        x = x.reshape(-1, self.E).to(device=self.device, dtype=torch.float32).contiguous()
        assert x.shape[0] == self.B, f"batch changed from {self.B} to {x.shape[0]} without prepare_caches()"
        _lib.check(_lib.lib().acai_decode_hidden(ctypes.byref(self._desc), x.data_ptr(), ops._st()), "acai_decode_hidden")
        self._x_valid = False   # d->x now holds the caller's embedding, not the chained step's next input
        self.cache_len += 1
        return self.ws["xn"][:self.B]

    # ---- OMRDecoder.cached_generate (models.py:518-528): logits for caller-supplied tokens -----------------------------
    def logits_step(self, tokens, time_step):
        if self.cache_len + 1 > self.Tmax:
            raise AssertionError("KV cache overflow: cache_pos + seq_len exceeds max_seq_len")
        tok = tokens.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        assert tok.numel() == self.B, f"batch changed from {self.B} to {tok.numel()} without prepare_caches()"
        _lib.check(_lib.lib().acai_decode_logits(ctypes.byref(self._desc), tok.data_ptr(), int(time_step), ops._st()), "acai_decode_logits")
        self._x_valid = False
        self.cache_len += 1
        return self.ws["logits"][:self.B]

    @contextlib.contextmanager
    def _run(self, max_len, mode):
        """Frame of a greedy / sampling / beam run of up to max_len-1 steps: the body runs on self.stream in `mode`; the caller's stream
        waits for it.  The mode goes back to greedy however the body ends."""
        if max_len > self.Tmax:
            raise RuntimeError(f"{max_len} decoding steps is too long for max sequence length of {self.Tmax}")
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        self._mode = mode
        try:
            with torch.cuda.stream(self.stream):
                yield
        finally:
            self._mode = ("greedy",)
        cur.wait_stream(self.stream)

    # ---- ViTOMR.cached_greedy_generate (models.py:600-615) ----------------------------------------------------------
    def greedy(self, max_len, poll=16, use_graph=True, on_chunk=None, prompt=None, *, grammar=None, prefill=False, loop_guard=None):
        """Runs up to max_len-1 greedy steps; returns views seqs (B,max_len) int64 and logprobs (B,max_len) fp32.
        Early exit when every row has produced <eos> (checked every `poll` steps; overshoot is masked later).
        prompt (an extension; None = off): one token list / 1-D tensor per row, the row's tokens of indices 1 .. P (_set_prompt); the row
        takes them whatever the model prefers, records the model's log-prob of each, and decodes greedily from index P + 1.
        grammar (an extension; None = off): a grammar.TokenAutomaton - every row takes the best token its automaton state allows and
        logprobs holds the log-softmax over the allowed tokens (_set_grammar); not combinable with prompt.
        prefill (an extension; False = off): with a prompt, the C = min P tokens every row has are computed in one teacher-forced pass
        (_prefill) and the prompt steps start at index C + 1; without a prompt, or with an empty one in the batch, it changes nothing.
        loop_guard (an extension; None = off): a loops.LoopGuard - a row whose tail is periodic by the guard's rule is finished at that index
        inside the replayed graph, like a row that produced <eos> (but no <eos> is written; the caller cuts the row at loop_report()'s
        stop), so a batch of looping rows ends early; mode ("loop", P, R, M).  Not combinable with prompt, grammar or prefill."""
        from .loops import check_guard, refuse_guard
        if check_guard(loop_guard) is not None:
            for arg, what in ((prompt, "prompt (prompted decoding)"), (grammar, "grammar (constrained decoding)"), (prefill or None, "prefill")):
                if arg is not None:
                    refuse_guard(loop_guard, what)
            with self._run(max_len, ("loop",) + loop_guard.params):
                self._set_loop(loop_guard)
                return self._decode_loop(max_len, poll, use_graph, on_chunk)
        if grammar is not None:
            if prompt is not None:
                raise ValueError("grammar (constrained decoding) cannot be combined with prompt (prompted decoding): out of scope here")
            with self._run(max_len, ("grammar",)):
                self._set_grammar(grammar)
                return self._decode_loop(max_len, poll, use_graph, on_chunk)
        if prompt is None:
            with self._run(max_len, ("greedy",)):
                return self._decode_loop(max_len, poll, use_graph, on_chunk)
        plan = self._prefill_plan(prompt, max_len) if prefill else None
        with self._run(max_len, ("prompt",)):
            self._set_prompt(prompt, self.B, max_len)
            return self._decode_loop(max_len, poll, use_graph, on_chunk, prefill=plan)

    # ---- prompted decoding (an extension: the reference starts every sequence from <bos> alone) -------------------------------------------
    def _set_prompt(self, prompt, n, max_len):
        """Fills the engine-owned prompt tables for n sequences: prompt[i] holds sequence i's tokens of output indices 1 .. P_i (0 <= P_i <=
        max_len - 1; validated by the caller - ViTOMR._check_prefix).  The tables keep their address from call to call, so the captured
        prompt-mode graphs stay valid; they are written on the current stream, before arming."""
        if len(prompt) != n:
            raise ValueError(f"prompt holds {len(prompt)} token lists for {n} sequences")
        if self.prompt_tok is None:
            self.prompt_tok = torch.zeros(self.Bmax, self.Tmax, dtype=torch.int32, device=self.device)
            self.prompt_len = torch.zeros(self.Bmax, dtype=torch.int32, device=self.device)
            d = _lib.AcaiPrompt()
            d.tok, d.len, d.pitch, d.rows = self.prompt_tok.data_ptr(), self.prompt_len.data_ptr(), self.Tmax, self.Bmax
            self._prompt_desc = d
        tab = torch.zeros(n, self.Tmax, dtype=torch.int32)
        lens = torch.zeros(n, dtype=torch.int32)
        for i, p in enumerate(prompt):
            p = torch.as_tensor(p).reshape(-1).to(device="cpu", dtype=torch.int32)
            if p.numel() > max_len - 1:
                raise ValueError(f"prompt {i} holds {p.numel()} tokens: more than max_len - 1 = {max_len - 1}")
            tab[i, 1:1 + p.numel()] = p
            lens[i] = p.numel()
        self.prompt_tok[:n].copy_(ops.h2d(tab, self.device))
        self.prompt_len[:n].copy_(ops.h2d(lens, self.device))

    # ---- prompt prefill (an extension): the prompt's common part in one teacher-forced pass instead of one step per token -----------------
    def _prefill_plan(self, prompt, max_len):
        """(C, live) of a prefilled prompt run - the depth C = min_b P_b every row's prompt reaches and whether a row goes on after index C
        (not when every prompt ends there with <eos>: the prompt step's finishing rule at t = C) - checked on the host before anything is
        launched (ValueError for what a prefilled run cannot do); None = nothing to prefill: the run is the plain prompt run.  A wrong
        number of prompts or a too long one is left to _set_prompt."""
        if self.cross_fp8:
            raise ValueError("prefill (prompt prefill) does not support an FP8 memory cache: the pass reads the unquantised memory; use "
                             "memory_cache_dtype=None")
        rows = [torch.as_tensor(p).reshape(-1) for p in prompt]
        if len(rows) != self.B or not rows or max(r.numel() for r in rows) > max_len - 1 or min(r.numel() for r in rows) < 1:
            return None
        if self.group != 1 or self.omr is None or self._mem is None:
            raise ValueError(f"prefill (prompt prefill) needs an OMRDecoder's engine prepared with one memory per row (prepared: group_size="
                             f"{self.group})")
        if self.V > 512:
            raise ValueError(f"prefill (prompt prefill) needs a vocabulary of at most 512 tokens, got {self.V}")
        C = min(r.numel() for r in rows)
        # every id is used as an index where a prompt step would fall back to its arg-max: position j + 1 would then depend on position j
        for i, r in enumerate(rows):
            if r.numel() and (int(r.min()) < 0 or int(r.max()) >= self.V):
                raise ValueError(f"prompt {i} holds a token id outside [0, {self.V}): a prefilled run (prefill) cannot take it")
        eos = self.omr.eos_idx
        return C, any(not (r.numel() == C and int(r[-1]) == eos) for r in rows)

    def _prefill(self, C):
        """The armed engine (arm(), prompt tables set) -> the state after C prompt steps, C = the depth every row's prompt reaches: one
        packed pass over B sequences of C tokens (row b's tokens of indices 0 .. C - 1 at positions 1 .. C, quirk Q1) over the prepared
        memories at the engine's precision - OMRDecoder._layers_packed, eagerly, on the current stream; it projects the cross K/V again -
        whose per-layer qkv goes into the self K/V caches (acai_decode_prefill_self_kv) and whose logits become seqs / logprobs / finished /
        step / x (acai_decode_prefill_arm)."""
        B, own, L, d = self.B, self.omr, _lib.lib(), ctypes.byref(self._desc)
        st = ops._st()
        tok = self.prompt_tok[:B, :C].clone()          # column 0 is not a prompt column: it becomes <bos>
        tok[:, 0] = own.bos_idx
        mem32, memb = self._mem

        def sink(layer, qkv):
            assert qkv.dtype == self.cdt and qkv.shape == (B * C, 3 * self.E) and qkv.stride(1) == 1
            _lib.check(L.acai_decode_prefill_self_kv(d, layer, qkv.data_ptr(), qkv.stride(0), C, st), "acai_decode_prefill_self_kv")

        with torch.no_grad():
            logits = own._layers_packed(own._embed_packed(tok.reshape(-1), [C] * B, True, 1), [C] * B, mem32, memb, self.lens, self.prec,
                                        kv_sink=sink)
        assert logits.dtype == torch.float32 and logits.shape == (B * C, self.V) and logits.is_contiguous()
        _lib.check(L.acai_decode_prefill_arm(d, ctypes.byref(self._prompt_desc), logits.data_ptr(), C, st), "acai_decode_prefill_arm")
        self._x_valid = True
        self.cache_len = C
        self.prefilled_tokens += B * C

    # ---- grammar-constrained decoding (an extension: the reference knows no grammar) -----------------------------------------------------------
    GRAMMAR_MODES = ("grammar", "grammar_sample", "slot_grammar", "slot_grammar_sample")

    def _set_grammar(self, automaton):
        """Copies a grammar.TokenAutomaton's tables into engine-owned device buffers that keep their address from run to run (_set_prompt's
        pattern), so the captured grammar-mode graphs stay valid; written on the current stream, before arming.  A larger automaton
        reallocates the table; that, or another number of states or start state (both are launch arguments), drops the grammar modes'
        graphs.  The copy is skipped when `automaton` is the object of the previous run: an automaton is not edited in place."""
        from .grammar import TokenAutomaton
        if not isinstance(automaton, TokenAutomaton):
            raise TypeError(f"grammar must be a grammar.TokenAutomaton, got {type(automaton).__name__}")
        S, V = automaton.states, automaton.vocab_size
        if V != self.V:
            raise ValueError(f"the grammar is over {V} tokens, the decoder's vocabulary has {self.V}")
        if self.V > 512:
            raise ValueError(f"grammar-constrained decoding needs a vocabulary of at most 512 tokens, got {self.V}")
        stale = False
        if self.gram_next is None:
            self.gram_resync = torch.zeros(V, dtype=torch.int16, device=self.device)
            self.gram_state = torch.zeros(self.Bmax, dtype=torch.int32, device=self.device)
            self._gram_desc = _lib.AcaiGrammar()
            self._gram_src = None
        if self.gram_next is None or self.gram_next.shape[0] < S:
            self.gram_next = torch.zeros(S, V, dtype=torch.int16, device=self.device)
            self._gram_src, stale = None, True
        d = self._gram_desc
        if (d.states, d.start) != (S, automaton.start):
            stale = True
        if stale:
            for key in [k for k in self.graphs if k[4][0] in self.GRAMMAR_MODES]:
                del self.graphs[key]
        d.next, d.resync, d.state = self.gram_next.data_ptr(), self.gram_resync.data_ptr(), self.gram_state.data_ptr()
        d.states, d.start, d.rows = S, automaton.start, self.Bmax
        if self._gram_src is not automaton:
            src_next, src_resync = automaton.next, automaton.resync
            if not src_next.is_cuda:
                src_next, src_resync = ops.h2d(src_next.contiguous(), self.device), ops.h2d(src_resync.contiguous(), self.device)
            self.gram_next[:S].copy_(src_next)
            self.gram_resync.copy_(src_resync)
            self._gram_src = automaton

    # ---- the loop guard (an extension: the reference lets a looping row run to its cap) --------------------------------------------------------
    LOOP_MODES = ("loop", "slot_loop")

    def _set_loop(self, guard):
        """The guard's state in engine-owned device buffers that keep their address from run to run (_set_grammar's pattern), so the
        captured loop-mode graphs stay valid.  P, R and M are launch arguments: they are part of the mode, and with it of the graph key."""
        if self.loop_run is None:
            self.loop_run = torch.zeros(self.Bmax, 64, dtype=torch.int32, device=self.device)
            self.loop_rep = torch.zeros(3, self.Bmax, dtype=torch.int32, device=self.device)
            d = _lib.AcaiLoop()
            d.run, d.rows = self.loop_run.data_ptr(), self.Bmax
            d.stop, d.period, d.start = (self.loop_rep[k].data_ptr() for k in range(3))
            self._loop_desc = d
        self._loop_desc.max_period, self._loop_desc.min_repeats, self._loop_desc.min_tokens = guard.params

    def loop_report(self):
        """(stop, period, start) int32 (B,) views of the last guarded static run's report (period 0: the row did not loop)."""
        return self.loop_rep[0, :self.B], self.loop_rep[1, :self.B], self.loop_rep[2, :self.B]

    # ---- GRPOViTOMR.cached_forward_rollout_policy (models.py:988-1049) ---------------------------------------------------------
    def sample(self, max_actions, top_k, temperature, uniforms=None, poll=16, use_graph=True, *, grammar=None):
        """Up to max_actions-1 sampling steps (top-k, temperature, inverse-CDF draw from `uniforms` (B, max_actions) in [0,1) - drawn from
        torch's generator when None).  Returns views seqs (B, max_actions), logprobs (B, max_actions) and the number of steps run.
        grammar (None = off): a grammar.TokenAutomaton - the top-k, the draw and the recorded log_softmax(kept) run over the tokens the
        row's automaton state allows."""
        mode = ("sample" if grammar is None else "grammar_sample", int(top_k), float(temperature))
        with self._run(max_actions, mode):
            if grammar is not None:
                self._set_grammar(grammar)
            B = self.B
            if self.uniforms is None:
                self.uniforms = torch.zeros(self.Bmax, self.Tmax, dtype=torch.float32, device=self.device)
            if uniforms is None:
                uniforms = torch.rand(B, max_actions, device=self.device)
            assert uniforms.shape == (B, max_actions)
            self.uniforms[:B, :max_actions] = uniforms.to(device=self.device, dtype=torch.float32)
            return self._decode_loop(max_actions, poll, use_graph)

    def greedy_chunks(self, max_len, chunk, prompt=None, *, grammar=None, prefill=False, loop_guard=None):
        """Generator over the greedy loop in chunks of `chunk` tokens (streamed inference): yields (tokens_done, all_finished)
        after each chunk; the decode graph is replayed on the engine's stream, the caller's stream waits for it.
        prompt / grammar: as in greedy(); the mode is ("prompt",) / ("grammar",) while the generator runs and goes back to greedy when it
        ends or is closed.
        prefill: as in greedy().  The C prefilled tokens are there at once: every multiple of `chunk` up to C is yielded without a step in
        between, and the first chunk of steps ends at the next multiple, so tokens_done takes the values it takes without prefill.
        loop_guard: as in greedy(); the mode is ("loop", P, R, M) while the generator runs."""
        from .loops import check_guard, refuse_guard
        if check_guard(loop_guard) is not None:
            for arg, what in ((prompt, "prompt (prompted decoding)"), (grammar, "grammar (constrained decoding)"), (prefill or None, "prefill")):
                if arg is not None:
                    refuse_guard(loop_guard, what)
        if max_len > self.Tmax:
            raise RuntimeError(f"{max_len} decoding steps is too long for max sequence length of {self.Tmax}")
        if grammar is not None and prompt is not None:
            raise ValueError("grammar (constrained decoding) cannot be combined with prompt (prompted decoding): out of scope here")
        plan = self._prefill_plan(prompt, max_len) if prefill and prompt is not None else None
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        if prompt is not None:
            self._mode = ("prompt",)
        if grammar is not None:
            self._mode = ("grammar",)
        if loop_guard is not None:
            self._mode = ("loop",) + loop_guard.params
        try:
            with torch.cuda.stream(self.stream):
                if prompt is not None:
                    self._set_prompt(prompt, self.B, max_len)
                if grammar is not None:
                    self._set_grammar(grammar)
                if loop_guard is not None:
                    self._set_loop(loop_guard)
                self._arm_and_capture(self.B)
                if plan is not None:
                    self._prefill(plan[0])
            done, total = 0, max_len - 1
            if plan is not None:
                C, live = plan
                cur.wait_stream(self.stream)
                for done in range(chunk, C, chunk):
                    yield done, False
                done = C
                if not live or C % chunk == 0:
                    yield done, not live
                if not live:
                    return
            while done < total:
                n = min(chunk - done % chunk, total - done)
                with torch.cuda.stream(self.stream):
                    self.launch_steps(n)
                    fin = int(self.finished[self.B].item()) == 0
                cur.wait_stream(self.stream)
                done += n
                self.cache_len = done
                yield done, fin
                if fin:
                    return
        finally:
            if prompt is not None or grammar is not None or loop_guard is not None:
                self._mode = ("greedy",)

    # ---- beam search (an extension: the reference decodes greedily) ----------------------------------------------------------------------
    def beam(self, max_len, beam_width, length_penalty=1.0, poll=16, use_graph=True):
        """Beam search over the B / K images prepared with group_size = K (rows i*K .. i*K+K-1 are the beam slots of image i): up to
        max_len-1 steps of acai_decode_beam_step, then per image the slot with the highest cum / len^length_penalty (ties: lower slot).
        Returns seqs (B/K, max_len) int64 and log_probs (B/K, max_len) fp32 of the chosen hypotheses and their cumulative log-probs cum (B/K,)."""
        K = int(beam_width)
        with self._run(max_len, ("beam", K)):
            if self.group != K or self.B % K:
                raise ValueError(f"beam width {K} needs the memories prepared with group_size={K} (prepared: {self.group})")
            if self.beam_anc is None:
                z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.device)  # noqa: E731
                self.beam_anc = z(2, self.Bmax, self.Tmax, dt=torch.int32)
                self.beam_tok = z(2, self.Bmax, self.Tmax, dt=torch.int64)
                self.beam_lp = z(2, self.Bmax, self.Tmax, dt=torch.float32)
                self.beam_cum = z(self.Bmax, dt=torch.float32)
                self.beam_len = z(self.Bmax, dt=torch.int32)
                d = _lib.AcaiBeam()
                d.pitch, d.rows = self.Tmax, self.Bmax
                d.anc, d.tok, d.lp = self.beam_anc.data_ptr(), self.beam_tok.data_ptr(), self.beam_lp.data_ptr()
                d.cum, d.len = self.beam_cum.data_ptr(), self.beam_len.data_ptr()
                self._beam_desc = d
            self._beam_desc.K = K
            _, _, self._beam_done = self._decode_loop(max_len, poll, use_graph)
            seqs, lps, cum, _ = self.beam_slots(max_len)
            n = self.B // K
            ln = self.beam_len[:self.B].view(n, K)
            ln = torch.where(ln == 0, torch.full_like(ln, max_len - 1), ln).to(torch.float32)
            c = cum.view(n, K)
            score = torch.where(c == float("-inf"), c, c / ln.pow(float(length_penalty)))
            rows = torch.arange(n, device=self.device) * K + torch.argmax(score, dim=1)   # first maximum: the lower slot on ties
            return seqs.index_select(0, rows), lps.index_select(0, rows), cum.index_select(0, rows)

    # ---- speculative greedy decoding (an extension: the reference emits one token per step) ------------------------------------------------
    def speculative(self, max_len, draft_len, ngram=3, drafts=None, poll=16, use_graph=True, on_chunk=None, prompt=None):
        """Greedy decoding that emits up to draft_len + 1 tokens per step, over the B / R images prepared with group_size = R = draft_len + 1
        and per_row_cross=True (rows i*R .. i*R+R-1 verify consecutive tokens of image i): up to max_len-1 steps of acai_decode_spec_step.
        Drafts come from the sequence's own earlier n-grams (suffixes of up to `ngram` tokens), or from `drafts` (B/R, max_len) int - the
        token proposed for each index, negative = none - when given.  Returns views seqs (B/R, max_len) int64 and logprobs (B/R, max_len)
        fp32, bitwise what greedy() writes up to each image's first <eos> (nothing is written after it), and steps (B/R,) int32, the
        verify steps each image took.  Not combinable with beam search, sampling, slot mode or an FP8 memory cache.
        prompt (None = off): one token list / 1-D tensor per image, as in greedy(): a step consumes up to draft_len + 1 prompt tokens (they
        are their own drafts), so P prompt tokens and the first free token take ceil((P + 1) / (draft_len + 1)) steps; the result is
        bitwise greedy(prompt=...)'s up to each image's first <eos>."""
        D = int(draft_len)
        R = D + 1
        if not 1 <= D <= 7:
            raise ValueError(f"draft_len must be in [1, 7], got {draft_len}")
        if drafts is None and not 1 <= int(ngram) <= 8:
            raise ValueError(f"ngram must be in [1, 8], got {ngram}")
        if self.cross_fp8:
            raise ValueError("speculative decoding does not support an FP8 memory cache; use memory_cache_dtype=None")
        if self.group != R or self.B % R or not self._per_row_cross:
            raise ValueError(f"draft_len {D} needs the memories prepared with group_size={R}, per_row_cross=True (prepared: group_size="
                             f"{self.group}, per_row_cross={self._per_row_cross})")
        n = self.B // R
        if drafts is not None and tuple(drafts.shape) != (n, max_len):
            raise ValueError(f"drafts must be (images, max_len) = ({n}, {max_len}), got {tuple(drafts.shape)}")
        mode = ("spec", D, 0 if drafts is not None else int(ngram))
        with self._run(max_len, mode if prompt is None else mode + ("prompt",)):
            if prompt is not None:
                self._set_prompt(prompt, n, max_len)
            if self.spec_t is None:
                z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.device)  # noqa: E731
                self.spec_t, self.spec_cap, self.spec_steps = z(self.Bmax), z(self.Bmax), z(self.Bmax)
                self.spec_tab, self.spec_next, self.spec_drafts = z(self.Bmax, self.Tmax), z(self.Bmax, 8), z(self.Bmax, self.Tmax)
                d = _lib.AcaiSpec()
                d.pitch, d.rows = self.Tmax, self.Bmax
                d.t, d.cap, d.steps = self.spec_t.data_ptr(), self.spec_cap.data_ptr(), self.spec_steps.data_ptr()
                d.tab, d.next = self.spec_tab.data_ptr(), self.spec_next.data_ptr()
                self._spec_desc = d
            self._spec_desc.D, self._spec_desc.ngram = D, self._mode[2]
            self._spec_desc.drafts = None if drafts is None else self.spec_drafts.data_ptr()
            if drafts is not None:
                self.spec_drafts[:n].fill_(-1)
                self.spec_drafts[:n, :max_len] = drafts.to(device=self.device, dtype=torch.int32)
            self._spec_cap = int(max_len)
            self._decode_loop(max_len, poll, use_graph, on_chunk)
            return self.seqs[:n, :max_len], self.logprobs[:n, :max_len], self.spec_steps[:n]

    def _arm_spec(self, B):
        """Device-side state of a speculative run over B rows = B / R images: image i's tokens in row i of seqs / logprobs, t = 1, the key
        table cleared; acai_decode_spec_arm drafts the first step and writes every row's input."""
        n, own = B // (self._mode[1] + 1), self.omr
        self.seqs[:n].fill_(own.pad_idx)
        self.seqs[:n, 0] = own.bos_idx
        self.logprobs[:n].zero_()
        self.finished.zero_()
        self.reset_self_cache()
        self.step.copy_(torch.tensor([1, 0], dtype=torch.int32))
        self.spec_t.fill_(1)
        self.spec_cap.fill_(self._spec_cap)
        self.spec_steps.zero_()
        self.spec_tab.zero_()
        self.spec_next.fill_(-1)
        if len(self._mode) > 3:
            _lib.check(_lib.lib().acai_decode_spec_prompt_arm(ctypes.byref(self._desc), ctypes.byref(self._spec_desc),
                                                              ctypes.byref(self._prompt_desc), ops._st()), "acai_decode_spec_prompt_arm")
        else:
            _lib.check(_lib.lib().acai_decode_spec_arm(ctypes.byref(self._desc), ctypes.byref(self._spec_desc), ops._st()), "acai_decode_spec_arm")
        self._x_valid = True

    def beam_slots(self, max_len):
        """Every slot of the last beam search as it ended: tokens (B, max_len), per-token log-probs, cum (B,) and len (B,) (0 = unfinished).
        The lineage copy written last is (1 + steps run) & 1."""
        par, B = (1 + self._beam_done) & 1, self.B
        return self.beam_tok[par, :B, :max_len], self.beam_lp[par, :B, :max_len], self.beam_cum[:B], self.beam_len[:B]

    def _arm_beam(self, B):
        K, own = self._mode[1], self.omr
        self.beam_anc[:, :B] = torch.arange(B, dtype=torch.int32, device=self.device).view(1, B, 1)   # every position: the row's own cache row
        self.beam_tok[:, :B].fill_(own.pad_idx)
        self.beam_tok[:, :B, 0] = own.bos_idx
        self.beam_lp[:, :B].zero_()
        c = self.beam_cum[:B].view(B // K, K)
        c.fill_(float("-inf"))
        c[:, 0] = 0.0                 # one live hypothesis per image: step 1 does not produce K copies of it
        self.beam_len[:B].zero_()

    def arm(self, B):
        if self._mode[0] in ("slot", "slot_sample", "slot_grammar", "slot_grammar_sample", "slot_loop"):
            self._slot_reset()
            return
        if self._mode[0] == "spec":
            self._arm_spec(B)
            return
        own = self.omr
        self.seqs[:B].fill_(own.pad_idx)
        self.seqs[:B, 0] = own.bos_idx
        self.logprobs[:B].zero_()
        self.finished.zero_()
        self.reset_self_cache()
        self.step.copy_(torch.tensor([1, 0], dtype=torch.int32))
        if self._mode[0] == "beam":
            self._arm_beam(B)
        if self._mode[0] in ("grammar", "grammar_sample"):
            self.gram_state[:B].fill_(self._gram_desc.start)
        if self._mode[0] == "loop":
            self.loop_run[:B].zero_()
            self.loop_rep[:, :B].zero_()
        # input of the first step (<bos> at position 1, quirk Q1); each step's selection kernel (greedy_select_kernel / sample_select_kernel) writes the next step's input
        _lib.check(_lib.lib().acai_decode_embed(ctypes.byref(self._desc), ops._st()), "acai_decode_embed")
        self._x_valid = True

    STEPS_PER_GRAPH = 8   # a graph replay costs ~10-15 us of launch latency: amortise it over several decode steps

    def _step(self, st):
        """One decode step of the current mode on the current stream."""
        mode, L, d = self._mode, _lib.lib(), ctypes.byref(self._desc)
        if mode[0] == "greedy":
            _lib.check(L.acai_decode_step(d, st), "acai_decode_step")
        elif mode[0] == "sample":
            _lib.check(L.acai_decode_sample_step(d, self.uniforms.data_ptr(), mode[1], mode[2], st), "acai_decode_sample_step")
        elif mode[0] == "beam":
            _lib.check(L.acai_decode_beam_step(d, ctypes.byref(self._beam_desc), st), "acai_decode_beam_step")
        elif mode[0] == "prompt":
            _lib.check(L.acai_decode_prompt_step(d, ctypes.byref(self._prompt_desc), st), "acai_decode_prompt_step")
        elif mode[0] == "spec" and len(mode) > 3:
            _lib.check(L.acai_decode_spec_prompt_step(d, ctypes.byref(self._spec_desc), ctypes.byref(self._prompt_desc), st),
                       "acai_decode_spec_prompt_step")
        elif mode[0] == "spec":
            _lib.check(L.acai_decode_spec_step(d, ctypes.byref(self._spec_desc), st), "acai_decode_spec_step")
        elif mode[0] == "grammar":
            _lib.check(L.acai_decode_grammar_step(d, ctypes.byref(self._gram_desc), st), "acai_decode_grammar_step")
        elif mode[0] == "grammar_sample":
            _lib.check(L.acai_decode_grammar_sample_step(d, ctypes.byref(self._gram_desc), self.uniforms.data_ptr(), mode[1], mode[2], st),
                       "acai_decode_grammar_sample_step")
        elif mode[0] == "slot_grammar":
            _lib.check(L.acai_decode_slot_grammar_step(d, ctypes.byref(self._slot_desc), ctypes.byref(self._gram_desc), st),
                       "acai_decode_slot_grammar_step")
        elif mode[0] == "slot_grammar_sample":
            _lib.check(L.acai_decode_slot_grammar_sample_step(d, ctypes.byref(self._slot_desc), ctypes.byref(self._gram_desc),
                                                              self.slot_uniforms.data_ptr(), self.Tmax, self.slot_urow.data_ptr(), mode[1],
                                                              mode[2], st), "acai_decode_slot_grammar_sample_step")
        elif mode[0] == "loop":
            _lib.check(L.acai_decode_loop_step(d, ctypes.byref(self._loop_desc), st), "acai_decode_loop_step")
        elif mode[0] == "slot_loop":
            _lib.check(L.acai_decode_slot_loop_step(d, ctypes.byref(self._slot_desc), ctypes.byref(self._loop_desc), st), "acai_decode_slot_loop_step")
        elif mode[0] == "slot_sample":
            _lib.check(L.acai_decode_slot_sample_step(d, ctypes.byref(self._slot_desc), self.slot_uniforms.data_ptr(), self.Tmax,
                                                      self.slot_urow.data_ptr(), mode[1], mode[2], st), "acai_decode_slot_sample_step")
        else:
            _lib.check(L.acai_decode_slot_step(d, ctypes.byref(self._slot_desc), st), "acai_decode_slot_step")

    def ensure_graph(self, nsteps=1):
        """hipGraph of `nsteps` consecutive decode steps for the current (B, cross split) configuration.  Must run on self.stream."""
        B = self.B
        key = (B, self.cross_nsplit, self.cross_chunk, nsteps, self._mode, self.group)
        g = self.graphs.get(key)
        if g is None:
            st = ops._st()
            # warm-up launch outside capture (first-use code-object load must not happen inside a capture), then re-arm
            self._step(st)
            torch.cuda.current_stream().synchronize()
            self.arm(B)
            torch.cuda.current_stream().synchronize()
            g = ops.Graph()
            g.begin()
            try:
                for _ in range(nsteps):
                    self._step(st)
            finally:
                g.end()
            self.graphs[key] = g
        return g

    def launch_steps(self, n, use_graph=True):
        """Enqueue n decode steps on the current stream (graphs of STEPS_PER_GRAPH steps + single-step graphs for the rest).
        A chained step takes its input embedding from d->x, which the PREVIOUS step's selection kernel wrote (acai_decode_step no
        longer embeds by itself).  The stepwise entry points (logits_step / hidden_step) overwrite d->x; after one of them the input is
        rebuilt from the device-side sequence state (`acai_decode_embed`: seqs[:, t-1] at position t) before the chain goes on."""
        if n > 0 and not getattr(self, "_x_valid", False):
            _lib.check(_lib.lib().acai_decode_embed(ctypes.byref(self._desc), ops._st()), "acai_decode_embed")
            self._x_valid = True
        if not use_graph:
            st = ops._st()
            for _ in range(n):
                self._step(st)
            return
        big = self.STEPS_PER_GRAPH
        while n >= big:
            self.ensure_graph(big).launch()
            n -= big
        while n > 0:
            self.ensure_graph(1).launch()
            n -= 1

    def _arm_and_capture(self, B, use_graph=True):
        """Arm B rows; with graphs, capture (and warm up) the 1- and STEPS_PER_GRAPH-step graphs first, then re-arm: the warm-up launch
        advances the device state."""
        self.arm(B)
        if use_graph:
            self.ensure_graph(1)
            self.ensure_graph(self.STEPS_PER_GRAPH)
            self.arm(B)

    def _decode_loop(self, max_len, poll, use_graph, on_chunk=None, prefill=None):
        """prefill: _prefill_plan's (C, live) - the loop starts behind the C prefilled indices, and runs no step when no row is live."""
        B = self.B
        self._arm_and_capture(B, use_graph)
        done = 0
        total = max_len - 1
        if prefill is not None:
            done, live = prefill
            self._prefill(done)
            if on_chunk is not None:
                on_chunk(done)
            if not live:
                total = done
        while done < total:
            n = min(poll, total - done)
            self.launch_steps(n, use_graph)
            done += n
            self.cache_len = done
            if on_chunk is not None:
                on_chunk(done)
            if int(self.finished[B].item()) == 0:  # device -> host sync once per `poll` tokens
                break
        return self.seqs[:B, :max_len], self.logprobs[:B, :max_len], done

    # ---- continuous batching (an extension: the reference decodes one static batch) ----------------------------------------------------
    def continuous(self, mem32, memb, lens, caps, slots, poll=16, use_graph=True, sample=None, uniforms=None, group=1, *, grammar=None,
                   flush=None, loop_guard=None):
        """Decode of len(lens) images through `slots` decode rows that are refilled as they finish: greedy, or with sample=(top_k,
        temperature) sampled as DecodeEngine.sample samples.  mem32 / memb: the images' packed memories (M, E) fp32 / bf16 copy, lens
        their lengths, caps[i] image i's cap (its row ends after token index caps[i] - 1, or at <eos>).  Checks the arguments at the call,
        then returns a generator that yields each image's index once its tokens and per-token log-probs are in `cont_seqs` / `cont_lps`
        (N, max(caps)), in completion order.  Every image decodes exactly as it would alone in a greedy (sampled: a sampling) batch; only
        the step schedule is shared.  Slot s owns a cross K/V region of max(lens) rows; an idle slot has cross length 1 and stays finished.
        Sampled runs: sequence i draws token index t from uniforms[i, t] (`uniforms` (N, max(caps)) in [0, 1); from torch's generator on
        the device when None), whichever slot and step it runs in; the mode is ("slot_sample", top_k, temperature), with graphs of its own.
        group = G > 1 (sampled runs only): every memory is queued G times - sequences m*G .. m*G+G-1 decode memory m, caps and uniforms
        are per sequence (N = len(lens) * G), and each admission prefills its own slot region.
        grammar (None = off): a grammar.TokenAutomaton constraining every sequence as DecodeEngine.greedy / sample(grammar=) constrain it;
        a slot's automaton state is set to the start state when the slot is refilled.  Modes ("slot_grammar",) / ("slot_grammar_sample",
        top_k, temperature).
        flush (None = off: the path, the launches and the copies above): F >= 1 streams the run (greedy and grammar modes; with sample= a
        ValueError - rollouts have no consumer for a stream).  The run polls every F steps instead of every `poll`, and each poll's read
        of the finished flags is replaced by one acai_decode_slot_flush launch and one copy of its buffer into pinned memory: per slot the
        tokens and log-probs written since the last poll, and the flag in the header.  The generator then yields, per poll and after the
        next steps are in flight, ("step", image, start, tokens, log_probs) for every busy slot with news, in slot order - tokens int32
        and log_probs fp32, (1, n), on the CPU, the row's indices start .. start + n - 1 - and then ("finish", image) for the slots freed
        at that poll; images with a cap below 2 are ("finish", image) up front.  An image's steps tile its row from index 1 through its
        last token.  The same graphs are replayed: streaming adds no graph key.
        loop_guard (None = off): a loops.LoopGuard - a sequence whose tail is periodic by the guard's rule frees its slot at that index, as a
        cap would; its row holds the tokens through `stop`, and `cont_loops` (3, N) int32 the images' (stop, period, start), copied with
        the row.  Mode ("slot_loop", P, R, M).  Greedy runs only: with sample=, grammar= or flush= a ValueError."""
        from .loops import check_guard, refuse_guard
        if check_guard(loop_guard) is not None:
            for arg, what in ((sample, "sample (sampled rollouts)"), (grammar, "grammar (constrained decoding)"), (flush, "flush (streaming)")):
                if arg is not None:
                    refuse_guard(loop_guard, what)
        S = int(slots)
        caps = [int(c) for c in caps]
        if max(caps) > self.Tmax:
            raise RuntimeError(f"{max(caps)} decoding steps is too long for max sequence length of {self.Tmax}")
        if not 1 <= S <= self.Bmax:
            raise ValueError(f"slots must be in [1, {self.Bmax}] (the cache's max batch size), got {slots}")
        G = int(group)
        if G < 1 or (G > 1 and sample is None):
            raise ValueError(f"group must be >= 1, and above 1 only in a sampled run (got {group})")
        if len(caps) != len(lens) * G:
            raise ValueError(f"{len(caps)} caps for {len(lens) * G} images")
        mode = ("slot",)
        if sample is not None:
            top_k, temperature = int(sample[0]), float(sample[1])
            if not 1 <= top_k <= 64 or not temperature > 0:
                raise ValueError(f"sample=(top_k, temperature) needs 1 <= top_k <= 64 and temperature > 0, got {tuple(sample)}")
            mode = ("slot_sample", top_k, temperature)
            if uniforms is None:
                uniforms = torch.rand(len(caps), max(caps), device=self.device)
            if tuple(uniforms.shape) != (len(caps), max(caps)):
                raise ValueError(f"uniforms must be (N, max(caps)) = ({len(caps)}, {max(caps)}), got {tuple(uniforms.shape)}")
        elif uniforms is not None:
            raise ValueError("uniforms are the draws of a sampled run: pass sample=(top_k, temperature) with them")
        if grammar is not None:
            from .grammar import TokenAutomaton
            if not isinstance(grammar, TokenAutomaton):
                raise TypeError(f"grammar must be a grammar.TokenAutomaton, got {type(grammar).__name__}")
            mode = ("slot_grammar",) if sample is None else ("slot_grammar_sample",) + mode[1:]
        if flush is not None:
            if sample is not None:
                raise ValueError("flush (streaming) cannot be combined with sample: rollouts have no consumer for a stream")
            if isinstance(flush, bool) or not isinstance(flush, int) or not 1 <= flush <= self.Tmax:
                raise ValueError(f"flush must be an int in [1, {self.Tmax}] (the cache's max sequence length), got {flush!r}")
        if loop_guard is not None:
            mode = ("slot_loop",) + loop_guard.params
        return self._continuous(mem32, memb, lens, caps, S, poll, use_graph, mode, uniforms, G, grammar, flush, loop_guard)

    def _continuous(self, mem32, memb, lens, caps, S, poll, use_graph, mode=("slot",), uniforms=None, G=1, grammar=None, flush=None,
                    loop_guard=None):
        N, dev, own = len(caps), self.device, self.omr
        if flush is not None:
            poll = flush
        self._slot_group = G
        mem = memb if self.bf else mem32
        if mem is None:
            mem = ops.cast_bf16(mem32)
        W = max(caps)
        self.cont_seqs = torch.full((N, W), own.pad_idx, dtype=torch.int64, device=dev)
        self.cont_seqs[:, 0] = own.bos_idx
        self.cont_lps = torch.zeros(N, W, dtype=torch.float32, device=dev)
        self.cont_loops = torch.zeros(3, N, dtype=torch.int32, device=dev) if loop_guard is not None else None
        sched = SlotScheduler(caps, S)
        offs = [0]
        for l in lens:
            offs.append(offs[-1] + l)
        cur = torch.cuda.current_stream(dev)
        self.stream.wait_stream(cur)
        self.slot_steps = self.slot_busy = self.slot_polls = 0
        harvested = torch.cuda.Event()
        try:
            with torch.cuda.stream(self.stream):
                self._slot_setup(max(lens), S)
                lens_dev = ops.h2d(torch.tensor(lens, dtype=torch.int32), dev)
                if uniforms is not None:
                    self._slot_uniforms(uniforms)
                if grammar is not None:
                    self._set_grammar(grammar)
                if loop_guard is not None:
                    self._set_loop(loop_guard)
                self._mode = mode
                if flush is not None:
                    self._flush_setup(S, flush)   # before arming: _slot_reset parks the marks with the slots
                self._arm_and_capture(S, use_graph)
            if sched.skipped:
                harvested.record(self.stream)
                cur.wait_event(harvested)
                yield from sched.skipped if flush is None else [("finish", i) for i in sched.skipped]
            with torch.cuda.stream(self.stream):
                self._slot_refill(sched.admit(), mem, offs, lens_dev, caps)
                n = sched.chunk(poll)
                self.launch_steps(n, use_graph)
            while n > 0:
                with torch.cuda.stream(self.stream):
                    if flush is None:
                        fin = self.finished[:S].tolist()   # device -> host sync once per poll
                    else:   # the same one sync: the flags ride in the headers; enqueued before the refill below re-arms a row
                        hdr, busy = self._flush_poll(S), list(sched.image)
                        fin = [h[2] for h in hdr]
                    self.slot_steps += n
                    self.slot_polls += 1
                    self.slot_busy += n * sum(i is not None for i in sched.image)
                    freed = sched.advance(n, fin)
                    for s, i in freed:   # harvest: device-side copies of the finished rows, before the refill re-arms them
                        c = caps[i]
                        self.cont_seqs[i, :c].copy_(self.seqs[s, :c])
                        self.cont_lps[i, :c].copy_(self.logprobs[s, :c])
                        if loop_guard is not None:
                            self.cont_loops[:, i].copy_(self.loop_rep[:, s])
                    harvested.record(self.stream)
                    self._slot_refill(sched.admit(), mem, offs, lens_dev, caps)
                    for s in sched.idle():
                        if s not in self._parked:   # queue drained: the slot goes idle on a 1-key cross length
                            self.cross_len[s:s + 1].fill_(1)
                            self._parked.add(s)
                    n = sched.chunk(poll)
                    self.launch_steps(n, use_graph)   # the next steps run while the caller reads this poll's images
                if flush is not None:   # the pinned buffer is this poll's until the next poll's copy, which follows these yields
                    _, tok, lp = self._flush_host_views
                    for s, (k, start, _, _) in enumerate(hdr):
                        if busy[s] is not None and k > 0:
                            yield ("step", busy[s], start, tok[s:s + 1, :k].clone(), lp[s:s + 1, :k].clone())
                if freed:
                    cur.wait_event(harvested)
                    for _, i in freed:
                        yield i if flush is None else ("finish", i)
        finally:
            self._mode = ("greedy",)
            self._flush_ld = 0
            cur.wait_stream(self.stream)

    def _flush_setup(self, S, F):
        """Streaming state of a slot run of S slots polled every F steps: the marks, and ONE device buffer (S headers, then S x F tokens,
        then S x F log-probs: ops.slot_flush_views) with its pinned twin, both kept and only ever grown.  A slot gains at most one token
        per step, so F entries per slot hold everything a poll can bring."""
        if self.slot_mark is None:
            self.slot_mark = torch.zeros(self.Bmax, dtype=torch.int32, device=self.device)
        need = S * (4 + 2 * F)
        if self._flush_dev is None or self._flush_dev.numel() < need:
            self._flush_dev = torch.zeros(need, dtype=torch.int32, device=self.device)
            self._flush_host = torch.zeros(need, dtype=torch.int32).pin_memory()
        self._flush_ld = F
        self._flush_host_views = ops.slot_flush_views(self._flush_host, S, F)
        hdr, tok, lp = ops.slot_flush_views(self._flush_dev, S, F)
        # (the poll's launch goes straight to the C ABI with these: ops.slot_flush's checks of seven tensors would sit between the sync and
        # the next chunk's launch, where the GPU waits for the host)
        self._flush_args = (self.seqs.data_ptr(), self.logprobs.data_ptr(), self.seqs.stride(0), self.slot_t.data_ptr(), self.finished.data_ptr(),
                            self.slot_mark.data_ptr(), self.Bmax, S, F, tok.data_ptr(), lp.data_ptr(), hdr.data_ptr())

    def _flush_poll(self, S):
        """One flush launch over the S slots, one copy of its buffer into pinned memory, one sync -> the headers [[n, start, finished, 0]]."""
        _lib.check(_lib.lib().acai_decode_slot_flush(*self._flush_args, ops._st()), "acai_decode_slot_flush")
        need = S * (4 + 2 * self._flush_ld)
        self._flush_host[:need].copy_(self._flush_dev[:need], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._flush_host_views[0].tolist()

    def _slot_setup(self, Scap, S):
        """Slot mode for S rows over regions of Scap memory rows: the cross K/V layout, the cross split picked once for [Scap] * S (so that
        the captured graphs stay valid across refills), the slot state and the descriptors."""
        H, dhp, dev = self.H, self.cdhp, self.device
        region = Scap * H * dhp
        self._size_cross(S * region, S, [Scap] * S)
        self.slot_off = torch.arange(S, dtype=torch.int64, device=dev) * region
        self._slot_row0 = [s * (region // dhp) for s in range(S)]
        self.cross_off[:S] = self.slot_off
        self.cross_len[:S].fill_(1)
        self.B, self.lens, self.group = S, [Scap] * S, 1
        if self.slot_t is None:
            self.slot_t, self.slot_first, self.slot_cap = (torch.zeros(self.Bmax, dtype=torch.int32, device=dev) for _ in range(3))
            d = _lib.AcaiSlots()
            d.t, d.first, d.cap, d.rows = self.slot_t.data_ptr(), self.slot_first.data_ptr(), self.slot_cap.data_ptr(), self.Bmax
            self._slot_desc = d
        self._row_seq = torch.zeros(Scap, dtype=torch.int32, device=dev)    # prefill of one image: every row is memory 0 ...
        self._row_pos = torch.arange(Scap, dtype=torch.int32, device=dev)   # ... at its own position
        E, prec = self.E, self.prec
        self._cross_w = [(self.wc.w(ly.multihead_attn.in_proj_weight, prec)[E:], self.wc.b(ly.multihead_attn.in_proj_bias, prec)[E:])
                         for ly in self.blocks.layers]
        self._build_desc()

    def _slot_uniforms(self, uniforms):
        """The run's draws in the (rows, Tmax) table the sampled slot step reads, and the per-slot row index.  The table only grows; a
        reallocation drops the sampled slot graphs (they hold its address; the grammar form's too), never the greedy ones."""
        N, W = uniforms.shape
        if self.slot_uniforms is None or self.slot_uniforms.shape[0] < N:
            self.slot_uniforms = torch.zeros(N, self.Tmax, dtype=torch.float32, device=self.device)
            for key in [k for k in self.graphs if k[4][0] in ("slot_sample", "slot_grammar_sample")]:
                del self.graphs[key]
        if self.slot_urow is None:
            self.slot_urow = torch.zeros(self.Bmax, dtype=torch.int32, device=self.device)
        self.slot_uniforms[:N, :W] = uniforms.to(device=self.device, dtype=torch.float32)

    def _slot_reset(self):
        """Every slot idle: finished, cross length 1, local time 1 at ring start 0; ring write index 0 (step[0] is unused in slot mode)."""
        S = self.B
        self.step.copy_(torch.tensor([1, 0], dtype=torch.int32))
        self.finished.zero_()
        self.finished[:S].fill_(1)
        self.slot_t.fill_(1)
        self.slot_first.zero_()
        self.slot_cap.fill_(2)
        if self._flush_ld:   # a streamed run: a parked slot is finished at t = 1, so its end is 2 - nothing to send
            self.slot_mark.fill_(2)
        self.cross_len[:S].fill_(1)
        if self._mode[0] == "slot_loop":
            self.loop_run[:S].zero_()
            self.loop_rep[:, :S].zero_()
        self._parked = set(range(S))
        self.cache_len = 0
        _lib.check(_lib.lib().acai_decode_slot_arm(ctypes.byref(self._desc), ctypes.byref(self._slot_desc), None, 0, ops._st()),
                   "acai_decode_slot_arm")
        self._x_valid = True

    def _slot_refill(self, admitted, mem, offs, lens_dev, caps):
        """Prefill each admitted image's cross K/V into its slot's region (one prefill per image and layer, so that an image's K/V does not
        depend on which images were admitted with it), set the slot's cross length and arm the slots."""
        if not admitted:
            return
        H, dh, dhp = self.H, self.dh, self.cdhp
        for s, seq in admitted:
            i = seq // self._slot_group   # the memory this sequence decodes
            l = offs[i + 1] - offs[i]
            for li, (w, b) in enumerate(self._cross_w):
                if self.cross_fp8:   # through the staging region at the slot's offset, then quantised into the slot's rows
                    ops.cross_kv_prefill(mem[offs[i]:offs[i + 1]], w, b, self._row_seq[:l], self._row_pos[:l], self.slot_off[s:s + 1],
                                         lens_dev[i:i + 1], self.k_stage, self.v_stage, H, dh, dhp, round_bf16=True)
                    ops.cross_kv_quantize_fp8(self.k_stage, self.v_stage, self.k_cross[li], self.v_cross[li], self.k_cross_scale[li],
                                              self.v_cross_scale[li], self._slot_row0[s], l * H, dhp)
                else:
                    ops.cross_kv_prefill(mem[offs[i]:offs[i + 1]], w, b, self._row_seq[:l], self._row_pos[:l], self.slot_off[s:s + 1],
                                         lens_dev[i:i + 1], self.k_cross[li], self.v_cross[li], H, dh, dhp, round_bf16=self.bf)
            self.cross_len[s:s + 1].copy_(lens_dev[i:i + 1])
            self._parked.discard(s)
            if self._flush_ld:   # a streamed run: the new image is sent from index 1 (<bos> never is); after this poll's flush read the row
                self.slot_mark[s:s + 1].fill_(1)
        table = [[s for s, _ in admitted], [caps[i] for _, i in admitted]]
        sampled = self._mode[0] in ("slot_sample", "slot_grammar_sample")
        if self._mode[0] in ("slot_grammar", "slot_grammar_sample"):   # a refilled row starts in the automaton's start state; rows that stay
            for s, _ in admitted:                                      # idle keep whatever their state holds (it is never read)
                self.gram_state[s:s + 1].fill_(self._gram_desc.start)
        if self._mode[0] == "slot_loop":   # a refilled row starts with no run behind it and no report
            for s, _ in admitted:
                self.loop_run[s].zero_()
                self.loop_rep[:, s].zero_()
        if sampled:
            table.append([i for _, i in admitted])   # the slot's uniforms row: the sequence's own, whichever slot it lands in
        rows = ops.h2d(torch.tensor(table, dtype=torch.int32), self.device)
        if sampled:
            for j, (s, _) in enumerate(admitted):
                self.slot_urow[s:s + 1].copy_(rows[2, j:j + 1])
        _lib.check(_lib.lib().acai_decode_slot_arm(ctypes.byref(self._desc), ctypes.byref(self._slot_desc), rows.data_ptr(), len(admitted),
                                                   ops._st()), "acai_decode_slot_arm")
        self._keep_rows = rows   # (the arm kernel reads it asynchronously)
