"""CPU torch references of the token-to-image alignment (acai_attn_probs_mean, acai_attn_map_locate, the decoder pass around them).  Every
function computes in the dtype of what it is given, so float64 inputs give a float64 reference.  Nothing here shares code with the package:
the softmax is torch's own over full score rows (no log-sum-exp is taken in), the decoder is a plain restatement of
nn.TransformerDecoderLayer (post-LN, GELU) on packed rows."""
import math

import torch
import torch.nn.functional as F


def probs_mean(q, k, lens_q, lens_k, H, dh, head_w):
    """q [sum lens_q, >= H*dh], k [sum lens_k, >= H*dh] packed; head_w [H].  List of (T_b, S_b): sum_h head_w[h] softmax(q_h k_h^T / sqrt(dh))."""
    w = torch.as_tensor(head_w, dtype=q.dtype)
    out, oq, ok = [], 0, 0
    for lq, lk in zip(lens_q, lens_k):
        m = torch.zeros(lq, lk, dtype=q.dtype)
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            s = (q[oq:oq + lq, sl] @ k[ok:ok + lk, sl].t()) * (1.0 / math.sqrt(dh))
            m = m + w[h] * torch.softmax(s, dim=-1)
        out.append(m)
        oq += lq
        ok += lk
    return out


def locate(m, w):
    """One image's map m (T, S) with w patches per image row -> (patch (T,) int64: arg-max, the lower index on ties; loc (T, 6): row sum,
    peak, centroid x, y of the patch centres (x + 1/2, y + 1/2), standard deviations around it).  A row that sums to 0: all zeros."""
    T, S = m.shape
    s = torch.arange(S)
    x, y = (s % w).to(m.dtype) + 0.5, (s // w).to(m.dtype) + 0.5
    tot = m.sum(-1)
    safe = torch.where(tot > 0, tot, torch.ones_like(tot))
    cx, cy = (m * x).sum(-1) / safe, (m * y).sum(-1) / safe
    sx = torch.sqrt((m * (x[None] - cx[:, None]) ** 2).sum(-1) / safe)
    sy = torch.sqrt((m * (y[None] - cy[:, None]) ** 2).sum(-1) / safe)
    peak = m.max(-1).values if S else torch.zeros(T, dtype=m.dtype)
    patch = torch.tensor([int((row == row.max()).nonzero()[0]) for row in m], dtype=torch.int64) if S else torch.zeros(T, dtype=torch.int64)
    loc = torch.stack([tot, peak, cx, cy, sx, sy], -1)
    dead = ~(tot > 0)
    loc[dead, 2:] = 0
    patch[dead] = 0
    return patch, loc


def locate_loop(m, w):
    """locate as a brute-force loop over patches in plain Python floats (the check of `locate` itself)."""
    patches, rows = [], []
    for row in m.tolist():
        tot = sum(row)
        best, arg = -1.0, 0
        for s, p in enumerate(row):
            if p > best:
                best, arg = p, s
        if not tot > 0:
            patches.append(0)
            rows.append([tot, max(best, 0.0), 0.0, 0.0, 0.0, 0.0])
            continue
        cx = sum(p * (s % w + 0.5) for s, p in enumerate(row)) / tot
        cy = sum(p * (s // w + 0.5) for s, p in enumerate(row)) / tot
        vx = sum(p * (s % w + 0.5 - cx) ** 2 for s, p in enumerate(row)) / tot
        vy = sum(p * (s // w + 0.5 - cy) ** 2 for s, p in enumerate(row)) / tot
        patches.append(arg)
        rows.append([tot, best, cx, cy, math.sqrt(vx), math.sqrt(vy)])
    return torch.tensor(patches, dtype=torch.int64), torch.tensor(rows, dtype=m.dtype)


def _rb(x, bf):
    """bf: round to bf16 (nearest even), kept in x's dtype - the rounding points of a bf16 autocast run."""
    return x.to(torch.bfloat16).to(x.dtype) if bf else x


def _linear(x, w, b, bf):
    """F.linear; bf: inputs, weight and bias rounded to bf16, wide accumulation, output rounded."""
    return _rb(_rb(x, bf) @ _rb(w, bf).t() + _rb(b, bf), bf)


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _attention(q, k, v, lens_q, lens_k, H, dh, causal, bf):
    """Per sequence and head softmax(q k^T / sqrt(dh)) v (output rounded under bf) and the list of per-sequence [H, T, S] probabilities."""
    out, probs, oq, ok = torch.empty_like(q), [], 0, 0
    for lq, lk in zip(lens_q, lens_k):
        qs = q[oq:oq + lq].reshape(lq, H, dh).transpose(0, 1)
        ks = k[ok:ok + lk].reshape(lk, H, dh).transpose(0, 1)
        vs = v[ok:ok + lk].reshape(lk, H, dh).transpose(0, 1)
        s = (qs @ ks.transpose(-1, -2)) * (1.0 / math.sqrt(dh))
        if causal:
            s = s.masked_fill(~torch.ones(lq, lk, dtype=torch.bool).tril(), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[oq:oq + lq] = _rb((p @ vs).transpose(0, 1).reshape(lq, H * dh), bf)
        probs.append(p)
        oq += lq
        ok += lk
    return out, probs


def decoder_maps(sd, tokens, mem, lens, num_heads, layers, head_w, position_offset, prec="fp32", prefix="decoder."):
    """Teacher-forced decoder over packed `tokens` (sum T,) and packed memories `mem` (sum S, E); lens = (lens_t, lens_s); the state dict's
    tensors and mem in the dtype to compute in (float64 for a reference).  Token j of a sequence is embedded at position j +
    position_offset.  layers: layer indices (non-negative); head_w: [len(layers), H], summing to 1 over everything.
    Returns (list of (T_b, S_b) maps = sum over the layers and heads of head_w * cross-attention probabilities, packed logits).
    prec "bf16": the rounding points of the bf16 autocast run (linear inputs / outputs, attention outputs, GELU) on top of that dtype."""
    lens_t, lens_s = lens
    bf = prec == "bf16"
    H = num_heads
    E = sd[prefix + "pos_embedding"].shape[1]
    dh = E // H
    pos = torch.cat([torch.arange(t) for t in lens_t]) + position_offset
    x = sd[prefix + "vocab_embedding.weight"][tokens] + sd[prefix + "pos_embedding"][pos]
    head_w = torch.as_tensor(head_w, dtype=x.dtype)
    maps = [torch.zeros(t, s, dtype=x.dtype) for t, s in zip(lens_t, lens_s)]
    i = 0
    while f"{prefix}decoder_blocks.layers.{i}.norm1.weight" in sd:
        p = f"{prefix}decoder_blocks.layers.{i}."
        qkv = _linear(x, sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"], bf)
        a, _ = _attention(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], lens_t, lens_t, H, dh, True, bf)
        a = _linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], bf)
        x = _ln(x + a, sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
        wq, bq = sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"]
        q = _linear(x, wq[:E], bq[:E], bf)
        kv = _linear(mem, wq[E:], bq[E:], bf)
        c, probs = _attention(q, kv[:, :E], kv[:, E:], lens_t, lens_s, H, dh, False, bf)
        if i in layers:
            w = head_w[list(layers).index(i)]
            for b, pr in enumerate(probs):
                maps[b] = maps[b] + (w[:, None, None] * pr).sum(0)
        c = _linear(c, sd[p + "multihead_attn.out_proj.weight"], sd[p + "multihead_attn.out_proj.bias"], bf)
        x = _ln(x + c, sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5)
        h = _rb(F.gelu(_linear(x, sd[p + "linear1.weight"], sd[p + "linear1.bias"], bf)), bf)
        h = _linear(h, sd[p + "linear2.weight"], sd[p + "linear2.bias"], bf)
        x = _ln(x + h, sd[p + "norm3.weight"], sd[p + "norm3.bias"], 1e-5)
        i += 1
    x = _ln(x, sd[prefix + "decoder_blocks.norm.weight"], sd[prefix + "decoder_blocks.norm.bias"], 1e-6)
    return maps, _linear(x, sd[prefix + "unembed.weight"], sd[prefix + "unembed.bias"], bf)
