"""Plain-Python restatement of speculative greedy decoding (acai_decode_spec_step / DecodeEngine.speculative): the drafter rule and the
accept rule, driven by an arbitrary `next_token(prefix) -> token` function (the greedy choice after `prefix`).

State: the sequence `seq` (seq[0] = <bos>), t = len(seq) the next index to write.  A step has D draft slots; slot j (1-based) proposes the
token at index t - 1 + j and is verified by row j, which predicts index t + j.  A slot whose row would predict an index >= max_len is idle
(none).  Accept rule: g_0 = next_token(seq); while draft j + 1 is not none and equals g_j: g_{j+1} = next_token(seq + drafts[:j+1]).  The
step writes g_0 .. g_n, cut at the first <eos> and at index max_len - 1.

Drafter rule (prompt lookup): for m = min(ngram, t - 1) .. 1 take the last m tokens; among their earlier occurrences seq[e-m:e] with
m <= e <= t - 1 take the most recent (largest e); the first m with an occurrence proposes seq[e : e + D] as far as it exists.  The rest is
none.  A table source proposes table[index] for each slot (negative = none)."""

NONE = -1


def ngram_proposals(seq, D, ngram):
    L = len(seq)
    for m in range(min(ngram, L - 1), 0, -1):
        suffix = seq[L - m:]
        for e in range(L - 1, m - 1, -1):
            if seq[e - m:e] == suffix:
                prop = list(seq[e:min(e + D, L)])
                return prop + [NONE] * (D - len(prop))
    return [NONE] * D


def table_proposals(table):
    def source(seq, D, max_len):
        t = len(seq)
        return [table[t - 1 + j] if t - 1 + j < len(table) and table[t - 1 + j] >= 0 else NONE for j in range(1, D + 1)]
    return source


def ngram_source(ngram):
    return lambda seq, D, max_len: ngram_proposals(seq, D, ngram)


def no_drafts(seq, D, max_len):
    return [NONE] * D


def greedy_decode(next_token, bos, eos, max_len):
    seq = [bos]
    while len(seq) < max_len:
        seq.append(next_token(seq))
        if seq[-1] == eos:
            break
    return seq


def speculative_decode(next_token, bos, eos, max_len, D, source):
    """-> (seq, steps, log): log[i] = (t, drafts as verified, tokens written) of step i."""
    seq, steps, log = [bos], 0, []
    finished = False
    while not finished and len(seq) < max_len:
        t = len(seq)
        drafts = list(source(seq, D, max_len))
        assert len(drafts) == D
        drafts = [d if t + j < max_len else NONE for j, d in enumerate(drafts, start=1)]   # a row that would predict index >= max_len is idle
        g = [next_token(seq)]
        n = 0
        while n < D and drafts[n] != NONE and drafts[n] == g[n]:
            g.append(next_token(seq + drafts[:n + 1]))
            n += 1
        written = []
        for tok in g:
            if len(seq) >= max_len:
                break
            seq.append(tok)
            written.append(tok)
            if tok == eos:
                finished = True
                break
        steps += 1
        log.append((t, drafts, written))
    return seq, steps, log
