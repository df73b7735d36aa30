"""Restatements of the two confidence kernels (acai_token_confidence, acai_attn_map_weighted_sum) and of the three uncertainty weights in
plain torch, in the precision of their inputs: float64 inputs give the references the GPU tests compare against, float32 inputs the
restatement whose own error sets the tolerance.

The order rule, written out: token i comes BEFORE token j when logit[i] > logit[j], or logit[i] == logit[j] and i < j - raw logits
descending, then index ascending.  It is a total order on rows without NaN; -inf entries are equal to each other and therefore come last,
by index.  rank(c) counts the tokens before c; the top-k are the first k tokens.  Temperature never enters the order (z = logit / tau with
tau > 0 is monotone and the comparisons are on the raw logits)."""
import torch

WEIGHTS = ("entropy", "surprisal", "error")


def order(row):
    """Indices of a 1-D logit row in the order above (a stable sort by descending value keeps equal values in index order)."""
    return torch.sort(row, descending=True, stable=True).indices


def rank_of(row, c):
    """How many tokens come before token c: the definition, not a position in order()."""
    i = torch.arange(row.numel())
    return int(((row > row[c]) | ((row == row[c]) & (i < c))).sum())


def token_confidence(logits, chosen, top_k, temperature=1.0):
    """logits (N, V) float32 or float64, chosen (N,) -> (log_prob (N,), entropy (N,), rank (N,) int64, top_ids (N, K) int64,
    top_log_probs (N, K)) in the dtype of logits.  The order is taken on the logits as given; entries with p = 0 add nothing to the entropy."""
    N, V = logits.shape
    z = logits / temperature
    lsm = torch.log_softmax(z, dim=-1)
    p = torch.exp(lsm)
    ent = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1)
    chosen = chosen.long()
    lp = lsm.gather(-1, chosen[:, None]).squeeze(1)
    ids = torch.stack([order(logits[r])[:top_k] for r in range(N)]) if N else torch.zeros(0, top_k, dtype=torch.int64)
    rank = torch.tensor([rank_of(logits[r], int(chosen[r])) for r in range(N)], dtype=torch.int64)
    return lp, ent, rank, ids, lsm.gather(-1, ids)


def token_confidence_f32(logits, chosen, top_k, temperature=1.0):
    """The float32 torch CPU restatement whose error against float64 is `e32`: log_softmax and -(p * logp).sum in float32."""
    return token_confidence(logits.float(), chosen, top_k, temperature)


def weighted_sum(maps, weights):
    """maps: list of (T_i, S_i), weights: list of (T_i,) -> list of (S_i,): heat_i[s] = sum_j weights_i[j] * map_i[j, s]."""
    return [(w[:, None] * m).sum(0) if m.shape[0] else torch.zeros(m.shape[1], dtype=m.dtype) for m, w in zip(maps, weights)]


def weight_of(name, log_prob, entropy):
    """The per-token weight of ViTOMR.uncertainty_maps: "entropy", "surprisal" = -log_prob, "error" = 1 - exp(log_prob)."""
    if name == "entropy":
        return entropy
    if name == "surprisal":
        return -log_prob
    if name == "error":
        return 1.0 - torch.exp(log_prob)
    raise ValueError(f"unknown weight {name!r}")
