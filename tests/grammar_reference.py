"""Float64 restatement of grammar-constrained token selection (acai_decode_grammar_step / acai_decode_grammar_sample_step and their slot
forms, DecodeEngine.greedy / sample / continuous(grammar=)), written from the statement of the step, not from the kernels.

A row in automaton state s (clamped to [0, S)) reads the table row next[s][:].  Token i takes part iff next[s][i] >= 0; a token that does not
counts as a -inf logit in everything that follows:
  greedy:  the arg-max (first index on ties); log-prob = log-softmax over the tokens that take part;
  sampled: the top_k largest of them in descending order (ties: lower index first) - with fewer than top_k the kept set is all of them -,
           the inverse-CDF draw over softmax(kept / temperature) with u (the first entry whose inclusive CDF exceeds u * sum; the last
           kept entry when rounding leaves none), log-prob = log_softmax(kept)[drawn] without the temperature.
The next state is next[s][token].  If NO token takes part the row is unconstrained at that step and the next state is resync[token].

The loops step a batch as the engine's static batch steps it: every row is written at every index (what follows a row's <eos> is junk that
the caller masks) and the automaton state goes on advancing."""
import torch

NEG_INF = float("-inf")


def _row(automaton, s):
    """(clamped state, allowed mask or None for a dead state)."""
    s = min(max(int(s), 0), automaton.states - 1)
    ok = automaton.next[s].cpu() >= 0
    return s, (ok if bool(ok.any()) else None)


def _advance(automaton, s, ok, tok):
    return int(automaton.resync[tok]) if ok is None else int(automaton.next[s, tok])


def select_greedy(logits, s, automaton):
    """logits (V,) float64 -> (token, log-prob, next state)."""
    lg = logits.double()
    s, ok = _row(automaton, s)
    if ok is not None:
        lg = lg.masked_fill(~ok, NEG_INF)
    m = lg.max()
    tok = int((lg == m).nonzero()[0])
    lp = float((lg[tok] - m) - torch.log(torch.exp(lg - m).sum()))
    return tok, lp, _advance(automaton, s, ok, tok)


def select_sample(logits, s, automaton, u, top_k, temperature):
    """logits (V,) float64, u in [0, 1) -> (token, log-prob, next state)."""
    lg = logits.double()
    s, ok = _row(automaton, s)
    if ok is not None:
        lg = lg.masked_fill(~ok, NEG_INF)
    val, idx = torch.sort(lg, descending=True, stable=True)   # ties: lower index first
    k = min(int(top_k), int((val > NEG_INF).sum()))
    val, idx = val[:k], idx[:k]
    p = torch.exp((val - val[0]) / temperature)
    hit = (torch.cumsum(p, 0) > float(u) * p.sum()).nonzero()
    r = int(hit[0]) if hit.numel() else k - 1
    lp = float((val[r] - val[0]) - torch.log(torch.exp(val - val[0]).sum()))
    tok = int(idx[r])
    return tok, lp, _advance(automaton, s, ok, tok)


def _run(logits_fn, automaton, B, max_len, bos, pick, start_states=None):
    seqs = torch.zeros(B, max_len, dtype=torch.int64)
    seqs[:, 0] = bos
    lps = torch.zeros(B, max_len, dtype=torch.float64)
    states = torch.zeros(B, max_len, dtype=torch.int64)   # states[b][t]: the state in which index t was chosen
    s = [automaton.start] * B if start_states is None else [int(v) for v in start_states]
    for t in range(1, max_len):
        lg = logits_fn(seqs[:, t - 1], t)
        for b in range(B):
            states[b, t] = min(max(s[b], 0), automaton.states - 1)
            tok, lp, s[b] = pick(lg[b], s[b], b, t)
            seqs[b, t] = tok
            lps[b, t] = lp
    return seqs, lps, states


def constrained_greedy(logits_fn, automaton, B, max_len, bos, start_states=None):
    """logits_fn(tokens of index t - 1 (B,), t) -> logits (B, V) of index t.  -> seqs (B, max_len) int64, log-probs float64 (0 at index 0),
    states (B, max_len), every index written."""
    return _run(logits_fn, automaton, B, max_len, bos, lambda lg, s, b, t: select_greedy(lg, s, automaton), start_states)


def constrained_sample(logits_fn, automaton, B, max_len, bos, uniforms, top_k, temperature, start_states=None):
    """The sampled form: row b draws index t with uniforms[b][t]."""
    return _run(logits_fn, automaton, B, max_len, bos,
                lambda lg, s, b, t: select_sample(lg, s, automaton, float(uniforms[b, t]), top_k, temperature), start_states)


def bigram_permissive(V, pad, bos, eos):
    """The table of the automaton whose state is the last token (S = V, start = <bos>'s row) and that allows every token but <bos> / <pad>
    everywhere: restrictive automata are cut out of it."""
    nxt = torch.arange(V, dtype=torch.long).repeat(V, 1)
    nxt[:, bos] = -1
    nxt[:, pad] = -1
    return nxt
