"""Torch restatement of prompt prefill (acai_decode_prefill_self_kv / acai_decode_prefill_arm, DecodeEngine._prefill): where the pass's self
K/V rows go in the decode's caches, and the sequence state the pass's logits turn into.

Index convention: a prompt is the list p[0 .. P-1] of a row's tokens of output indices 1 .. P (index 0 is <bos>); C = min over the rows of P
is the prefill depth.  The pass runs row b's tokens of indices 0 .. C-1 at positions 1 .. C; its logits row b * C + j scores index j + 1 and
its per-layer in-projection qkv row b * C + p holds the K (columns E:2E) and V (2E:3E) of cache position p."""
import torch


def scatter(k_cache, v_cache, qkv, B, C, E, H, dh):
    """The caches [Bmax][H][Tmax][dhp] after the scatter of qkv (B*C, >= 3E), as new tensors: [b][h][p][d] = qkv[b*C + p][E + h*dh + d]
    (V: 2E + ...) for b < B, p < C, d < dh; everything else as it was."""
    k, v = k_cache.clone(), v_cache.clone()
    k[:B, :, :C, :dh] = qkv[:, E:2 * E].reshape(B, C, H, dh).permute(0, 2, 1, 3)
    v[:B, :, :C, :dh] = qkv[:, 2 * E:3 * E].reshape(B, C, H, dh).permute(0, 2, 1, 3)
    return k, v


def log_probs(logits, toks):
    """float64 log_softmax of logits (N, V) gathered at toks (N,)."""
    return torch.log_softmax(logits.double(), dim=-1).gather(1, toks.reshape(-1, 1).long()).squeeze(1)


def arm_state(logits, prompts, C, bos, pad, eos, max_len, emb, pos, x_before):
    """The state after prefill + arm at depth C from the pass's logits (B*C, V), for rows armed as DecodeEngine.arm arms them (seqs = <bos>
    then <pad>, log-probs 0): dict of seqs (B, max_len) int64, logprobs (B, max_len) float64 (not rounded), finished (B + 1,) int32 - the
    flags and, last, the count of unfinished rows - step [C + 1, C], and x (B, E) fp32 = emb[token of index C] + pos[C + 1], or x_before
    where C + 1 is no position (C + 1 == rows of pos)."""
    B = len(prompts)
    assert all(len(p) >= C for p in prompts) and 1 <= C <= max_len - 1 and logits.shape[0] == B * C
    seqs = torch.full((B, max_len), pad, dtype=torch.int64)
    seqs[:, 0] = bos
    lps = torch.zeros(B, max_len, dtype=torch.float64)
    fin = torch.zeros(B + 1, dtype=torch.int32)
    for b, p in enumerate(prompts):
        toks = torch.as_tensor([int(v) for v in p[:C]], dtype=torch.int64)
        seqs[b, 1:C + 1] = toks
        lps[b, 1:C + 1] = log_probs(logits[b * C:(b + 1) * C].cpu(), toks)
        fin[b] = int(int(toks[-1]) == eos)
        fin[B] += 0 if (fin[b] and C >= len(p)) else 1
    x = x_before.clone()
    if C + 1 < pos.shape[0]:
        x = emb[seqs[:, C]] + pos[C + 1]
    return dict(seqs=seqs, logprobs=lps, finished=fin, step=[C + 1, C], x=x)
