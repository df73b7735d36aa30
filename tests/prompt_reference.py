"""Plain-Python restatement of prompted decoding (acai_decode_prompt_step / acai_decode_spec_prompt_step, DecodeEngine.greedy(prompt=...) /
speculative(prompt=...)): the selection rule, the finishing rule and the speculative prompt step's bookkeeping.

A prompt is the list p[0 .. P-1] of a sequence's tokens of output indices 1 .. P (index 0 is <bos>), 0 <= P <= max_len - 1; <eos> only last.
Selection at index t from the step's logits: the token is p[t - 1] while t <= P, else the arg-max (first index on ties); its log-prob is
(logit[token] - max) - log(sum_j exp(logit[j] - max)) either way, so a forced token that IS the arg-max has the greedy step's log-prob.
A row finishes at <eos> - forced or chosen - or at index max_len - 1; a row with t < P counts as unfinished whatever its flag says.

Speculative form (tests/speculative_reference.py's state and accept rule): while the write index t <= P the drafts are the prompt's tokens
of indices t .. min(t + D - 1, P) and none beyond; a row predicting an index <= P emits the prompt's token, so those drafts are all accepted
and the first step past the prompt's end also emits the first free token: P prompt tokens plus that token take ceil((P + 1) / (D + 1))
steps.  Once t > P the drafts come from the usual source."""
import math

import speculative_reference as SR

NONE = SR.NONE


def log_prob(logits, tok):
    """(logit[tok] - max) - log(sum exp(logit - max)) in double precision."""
    m = max(logits)
    return (logits[tok] - m) - math.log(sum(math.exp(v - m) for v in logits))


def argmax_first(logits):
    m = max(logits)
    return next(i for i, v in enumerate(logits) if v == m)


def select(logits, t, prompt):
    """-> (token, log-prob, forced) of output index t."""
    forced = 1 <= t <= len(prompt)
    tok = prompt[t - 1] if forced else argmax_first(logits)
    return tok, log_prob(logits, tok), forced


def prompt_decode(step_logits, bos, eos, max_len, prompt):
    """One sequence: step_logits(seq) -> the logits of index len(seq).  -> (seq, log-probs (0 at index 0), forced flags)."""
    assert 0 <= len(prompt) <= max_len - 1
    seq, lps, forced = [bos], [0.0], [False]
    while len(seq) < max_len:
        tok, lp, f = select(step_logits(seq), len(seq), prompt)
        seq.append(tok)
        lps.append(lp)
        forced.append(f)
        if tok == eos:
            break
    return seq, lps, forced


def batch_decode(step_logits, bos, eos, max_len, prompts):
    """A ragged batch stepped together as the engine steps it: step_logits(i, seq) -> logits.  Every row is written at every step until
    the batch ends (the greedy step's behaviour: what follows a row's <eos> is masked by the caller); the batch ends after the step that
    leaves no row unfinished, or at max_len - 1.  -> (rows [(seq, lps)], unfinished count after each step)."""
    B = len(prompts)
    seqs, lps, fin, counts = [[bos] for _ in range(B)], [[0.0] for _ in range(B)], [False] * B, []
    for t in range(1, max_len):
        for i in range(B):
            tok, lp, _ = select(step_logits(i, seqs[i]), t, prompts[i])
            seqs[i].append(tok)
            lps[i].append(lp)
            fin[i] = fin[i] or tok == eos
        counts.append(sum(1 for i in range(B) if not fin[i] or t < len(prompts[i])))
        if counts[-1] == 0:
            break
    return list(zip(seqs, lps)), counts


def clip(seq, eos):
    """The row as the entry points return it: up to and including its first <eos>."""
    return seq[:seq.index(eos) + 1] if eos in seq else list(seq)


def prompted(next_token, prompt):
    """The token stream of a prompted sequence from the unprompted greedy choice next_token(prefix)."""
    return lambda prefix: prompt[len(prefix) - 1] if len(prefix) <= len(prompt) else next_token(prefix)


def prompt_source(prompt, fallback):
    """Draft source of the speculative prompt step: slot j (1-based) proposes index t - 1 + j."""
    P = len(prompt)

    def source(seq, D, max_len):
        t = len(seq)
        if t > P:
            return fallback(seq, D, max_len)
        return [prompt[t - 1 + j - 1] if t - 1 + j <= P else NONE for j in range(1, D + 1)]
    return source


def speculative_prompt_decode(next_token, bos, eos, max_len, D, prompt, fallback=SR.no_drafts):
    """-> (seq, steps, log) as speculative_reference.speculative_decode; next_token is the UNPROMPTED greedy choice."""
    return SR.speculative_decode(prompted(next_token, prompt), bos, eos, max_len, D, prompt_source(prompt, fallback))


def verify_steps(P, D):
    """Verify steps that P prompt tokens plus the first free token take (when max_len and <eos> do not cut them short)."""
    return -(-(P + 1) // (D + 1))
