"""Plain-Python restatement of speculative greedy decoding (acai_decode_spec_step / DecodeEngine.speculative): the drafter rule and the
accept rule, driven by an arbitrary `next_token(prefix) -> token` function (the greedy choice after `prefix`).

State: the sequence `seq` (seq[0] = <bos>), t = len(seq) the next index to write.  A step has D draft slots; slot j (1-based) proposes the
token at index t - 1 + j and is verified by row j, which predicts index t + j.  A slot whose row would predict an index >= max_len is idle
(none).  Accept rule: g_0 = next_token(seq); while draft j + 1 is not none and equals g_j: g_{j+1} = next_token(seq + drafts[:j+1]).  The
step writes g_0 .. g_n, cut at the first <eos> and at index max_len - 1.

Drafter rule (prompt lookup): for m = min(ngram, t - 1) .. 1 take the last m tokens; among their earlier occurrences seq[e-m:e] with
m <= e <= t - 1 take the most recent (largest e); the first m with an occurrence proposes seq[e : e + D] as far as it exists.  The rest is
none.  A table source proposes table[index] for each slot (negative = none).

ONE step as a pure state transition (SpecState / spec_step: what the launch acai_debug_decode_spec_accept makes must leave behind), written
from the statements in include/acai_omr_hip.h - the AcaiSpec block and the comments of acai_decode_spec_arm / _spec_step / _spec_prompt_arm /
_spec_prompt_step - not from the kernel.  Image i owns decode rows i * R .. i * R + D (R = D + 1) and row i of seqs / logprobs / t / cap /
steps / tab / next; with t its write index and next[i][1..D] the drafts the step verified, row j's logits predict index t + j:
  row       g_j = the arg-max (ties: lower index) with log-prob (logit - max) - log(sum exp(logit - max)); in a prompted run the prompt's token
            while t + j <= len (an id outside [0, V) is not forced), same formula;
  accept    g_0, then g_j while draft j is not none and equals g_{j-1}; written at t .. t + n, cut after the first <eos> and at cap - 1 (cap
            held to min(cap, max_len, pitch)); t' = t + what was written; the image finishes on <eos> or when t' reaches cap; steps += 1;
  skipped   an image whose flag is set has nothing of it written; one whose t is outside [1, cap - 1] gets its flag set and nothing else;
            an image that finishes in this step gets no drafts, next, tab or x either;
  drafts    of the next step, for every image unfinished afterwards: while t' <= len the prompt's tokens of indices t' .. min(t' + D - 1, len)
            and none beyond; else drafts[i][index] (ids outside [0, V): none); else ngram_proposals on seq[:t'] AFTER this step's writes; a
            slot whose prediction index t' + j would reach cap is none;
  next      next[i][0] = the token at t' - 1, next[i][1..D] the drafts (entries past D are not written);
  tab       tab[i][t' - 1 + j] = 8 * w + j for j = 0 .. D where the index is below pitch, w = min(step[1] + (0 if arm else 1), Tmax - 1);
  x         x[i * R + j] = emb[token, <pad> for none] + pos[min(t' + j, Tmax - 1)], one fp32 addition per element;
  counters  finished[B] = the unfinished images; step[1] = min(step[1] + 1, Tmax - 1) unless arm; step[0] is left alone.
arm: the launch that opens a run drafts and writes next / tab / x only - no logits are read, no token is written, steps and step[1] stay."""
import copy
from dataclasses import dataclass, field

import torch

NONE = -1


def ngram_match(seq, ngram):
    """-> (m, e): the suffix length that matched and the (exclusive) end of its most recent earlier occurrence seq[e - m:e]; None: no match."""
    L = len(seq)
    for m in range(min(ngram, L - 1), 0, -1):
        suffix = seq[L - m:]
        for e in range(L - 1, m - 1, -1):
            if seq[e - m:e] == suffix:
                return m, e
    return None


def ngram_proposals(seq, D, ngram):
    hit = ngram_match(seq, ngram)
    if hit is None:
        return [NONE] * D
    e = hit[1]
    prop = list(seq[e:min(e + D, len(seq))])
    return prop + [NONE] * (D - len(prop))


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


# ---- one step as a state transition ------------------------------------------------------------------------------------------------------
@dataclass
class SpecState:
    seqs: torch.Tensor       # [rows, max_len] int64, image i in row i
    logprobs: torch.Tensor   # [rows, max_len] float64
    finished: torch.Tensor   # [B + 1] int64: the images' flags in [0, images), then untouched entries, then the unfinished count at [B]
    step: list               # [unused, shared cache write index]
    t: torch.Tensor          # [rows] int64
    cap: torch.Tensor        # [rows] int64
    steps: torch.Tensor      # [rows] int64
    tab: torch.Tensor        # [rows, pitch] int64
    next: torch.Tensor       # [rows, 8] int64
    x: torch.Tensor          # [B, E] fp32
    touched: dict = field(default_factory=dict)   # of the LAST step: seqs (= logprobs) / tab / next bool masks of their shapes, x [B] bool
    written: list = field(default_factory=list)   # of the LAST step: per image the number of tokens written, None where it was skipped


def new_spec_state(cfg, D, pitch, rows=None, *, fill_tok=0, fill_lp=0.0, fill_x=0.0, fill_tab=0, fill_next=0, cache=0):
    """The armed state of the AcaiSpec block (<bos>, t = 1, cap = max_len, steps = 0, step = [1, cache]); everything not armed holds `fill_*`."""
    images = cfg.B // (D + 1)
    rows = images if rows is None else rows
    E = cfg.emb.shape[1]
    seqs = torch.full((rows, cfg.max_len), fill_tok, dtype=torch.int64)
    seqs[:, 0] = cfg.bos
    return SpecState(seqs=seqs, logprobs=torch.full((rows, cfg.max_len), float(fill_lp), dtype=torch.float64),
                     finished=torch.zeros(cfg.B + 1, dtype=torch.int64), step=[1, int(cache)], t=torch.ones(rows, dtype=torch.int64),
                     cap=torch.full((rows,), cfg.max_len, dtype=torch.int64), steps=torch.zeros(rows, dtype=torch.int64),
                     tab=torch.full((rows, pitch), fill_tab, dtype=torch.int64), next=torch.full((rows, 8), fill_next, dtype=torch.int64),
                     x=torch.full((cfg.B, E), float(fill_x), dtype=torch.float32))


def prompt_row(prompt, i, cfg):
    """-> (P, tok): image i's clamped prompt length and a function index -> forced token or NONE."""
    if prompt is None:
        return 0, lambda p: NONE
    tok, ln = prompt["tok"], prompt["len"]
    P = min(max(int(ln[i]), 0), min(tok.shape[1], cfg.max_len) - 1)

    def at(p):
        v = int(tok[i, p]) if 1 <= p <= P else NONE
        return v if 0 <= v < cfg.V else NONE
    return P, at


def row_choice(lg, forced):
    """The token and float64 log-prob of one row: `forced` when it is a token, else the arg-max (first index on ties)."""
    lg = lg.double()
    m = lg.max()
    tok = forced if forced != NONE else int((lg == m).nonzero()[0])
    return tok, float((lg[tok] - m) - torch.log(torch.exp(lg - m).sum()))


def spec_step(st, logits, cfg, D, *, arm, ngram=None, drafts=None, prompt=None):
    """One launch on logits [B, V] (None with arm).  drafts: [rows, pitch] table or None; prompt: dict(tok [rows, ppitch], len [rows]) or
    None.  -> the state after it."""
    n = copy.deepcopy(st)
    R, B = D + 1, cfg.B
    images = B // R
    pitch = st.tab.shape[1]
    w = min(st.step[1] + (0 if arm else 1), cfg.Tmax - 1)
    at, tabw, nxw = torch.zeros_like(st.seqs, dtype=torch.bool), torch.zeros_like(st.tab, dtype=torch.bool), torch.zeros_like(st.next, dtype=torch.bool)
    xw = torch.zeros(B, dtype=torch.bool)
    n.written = [None] * images
    for i in range(images):
        if int(st.finished[i]):
            continue
        cap, t = min(int(st.cap[i]), cfg.max_len, pitch), int(st.t[i])
        if t < 1 or t >= cap:
            n.finished[i] = 1
            continue
        P, forced = prompt_row(prompt, i, cfg)
        if not arm:
            wrote, fin, prev = 0, False, None
            for j in range(R):
                if j > 0 and (int(st.next[i, j]) < 0 or int(st.next[i, j]) != prev):
                    break
                if t + j >= cap:
                    break
                prev, lp = row_choice(logits[i * R + j], forced(t + j))
                n.seqs[i, t + j], n.logprobs[i, t + j], at[i, t + j] = prev, lp, True
                wrote += 1
                if prev == cfg.eos:
                    fin = True
                    break
            t += wrote
            n.t[i], n.steps[i], n.written[i] = t, int(st.steps[i]) + 1, wrote
            if fin or t >= cap:
                n.finished[i] = 1
                continue
        if t <= P:
            prop = [forced(t - 1 + j) for j in range(1, D + 1)]
        elif drafts is not None:
            prop = [int(drafts[i, t - 1 + j]) if t - 1 + j < pitch else NONE for j in range(1, D + 1)]
            prop = [v if 0 <= v < cfg.V else NONE for v in prop]
        else:
            prop = ngram_proposals([int(v) for v in n.seqs[i, :t]], D, ngram)
        prop = [v if t + j < cap else NONE for j, v in enumerate(prop, start=1)]
        row = [int(n.seqs[i, t - 1])] + prop
        for j in range(R):
            n.next[i, j], nxw[i, j] = row[j], True
            if t - 1 + j < pitch:
                n.tab[i, t - 1 + j], tabw[i, t - 1 + j] = 8 * w + j, True
            n.x[i * R + j] = cfg.emb[row[j] if row[j] != NONE else cfg.pad] + cfg.pos[min(t + j, cfg.Tmax - 1)]
            xw[i * R + j] = True
    n.finished[B] = int((n.finished[:images] == 0).sum())
    if not arm:
        n.step = [st.step[0], min(st.step[1] + 1, cfg.Tmax - 1)]
    n.touched = dict(seqs=at, tab=tabw, next=nxw, x=xw)
    return n
