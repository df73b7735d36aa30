"""Float64 restatement of ONE token-selection step of a decode step (acai_debug_decode_select: the selection launch of acai_decode_step /
_sample_step / _prompt_step / _grammar_step / _grammar_sample_step, their slot forms and acai_decode_beam_step), as a pure state transition.
Written from the statements in include/acai_omr_hip.h, not from the kernels.  The per-row choice is grammar_reference.select_greedy /
select_sample and prompt_reference.select; what is stated here is the step around it.

Static forms (every row at the shared time t = step[0]): every row - a finished one too - gets its token and log-prob at index t; a row
finishes on <eos> and stays finished; finished[B] = the rows that are unfinished (a prompted row with t < len counts as unfinished whatever
it emitted); step[0] and step[1] advance by 1; a chained step writes x[b] = emb[token] + pos[t + 1] (quirk Q1) while t + 1 < Tmax.
Slot forms (row b at its own time t[b]): a finished or idle row is skipped and nothing of it is written, its grammar state included; a row
finishes on <eos> or when t[b] = cap[b] - 1, otherwise t[b] advances and x[b] is written; finished[B] = the unfinished rows; step[1]
advances modulo Tmax and step[0] is left alone; a sampled row draws with uniforms[urow[b]][t[b]] (a static row with uniforms[b][t]).
Prompt: the token of index t is tok[b][t] while 1 <= t <= P, P = len[b] clamped to [0, min(pitch, max_len) - 1]; an id outside [0, V) is
not forced.  Grammar: grammar_reference's rule; the state vector takes next[s][token] (resync[token] out of a dead state).

`touched` names what a step wrote: everything else of seqs / logprobs / x (and of the beam lineage) must be left as it was."""
import copy
import math
from dataclasses import dataclass, field

import torch

import grammar_reference as GR
import prompt_reference as PR

NEG_INF = float("-inf")


class Table:
    """A bare transition table with the attributes grammar_reference reads (TokenAutomaton refuses the dead states these tests need)."""

    def __init__(self, next, start=0, resync=None):
        self.next = torch.as_tensor(next).to(torch.int16)
        self.start = int(start)
        self.resync = torch.zeros(self.next.shape[1], dtype=torch.int16) if resync is None else torch.as_tensor(resync).to(torch.int16)

    @property
    def states(self):
        return self.next.shape[0]


def allow_all(V):
    """One state that allows every token and leads to itself."""
    return Table(torch.zeros(1, V, dtype=torch.int16))


@dataclass
class Cfg:
    V: int
    B: int
    max_len: int
    Tmax: int
    eos: int
    bos: int = 0
    pad: int = 1
    emb: torch.Tensor = None   # [V, E] fp32
    pos: torch.Tensor = None   # [Tmax, E] fp32


@dataclass
class State:
    seqs: torch.Tensor         # [B, max_len] int64
    logprobs: torch.Tensor     # [B, max_len] float64
    finished: torch.Tensor     # [B + 1] int64: flags, then the unfinished count
    step: list                 # [t, cache length / ring index]
    x: torch.Tensor = None     # [B, E] fp32
    slot_t: torch.Tensor = None
    slot_cap: torch.Tensor = None
    gstate: torch.Tensor = None
    touched: dict = field(default_factory=dict)   # of the LAST step: seqs / logprobs [B, max_len] bool (one mask), x [B] bool
    margins: list = field(default_factory=list)   # of the LAST step: per row the draw's margin, None where no draw was made


def new_state(cfg, t=1, cache=0, slot_t=None, slot_cap=None, gstate=None, finished=None, fill=0):
    E = cfg.emb.shape[1] if cfg.emb is not None else 0
    fin = torch.zeros(cfg.B + 1, dtype=torch.int64)
    if finished is not None:
        fin[:cfg.B] = torch.as_tensor(finished, dtype=torch.int64)
    i64 = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.int64).clone()
    return State(seqs=torch.full((cfg.B, cfg.max_len), fill, dtype=torch.int64), logprobs=torch.full((cfg.B, cfg.max_len), float(fill), dtype=torch.float64),
                 finished=fin, step=[int(t), int(cache)], x=torch.full((cfg.B, E), float(fill), dtype=torch.float32), slot_t=i64(slot_t),
                 slot_cap=i64(slot_cap), gstate=i64(gstate))


def kept_cdf(logits, ok, top_k, temperature):
    """The kept entries of a draw in descending order (ties: lower index first) and their unnormalised CDF under the temperature."""
    lg = logits.double()
    if ok is not None:
        lg = lg.masked_fill(~ok, NEG_INF)
    val, idx = torch.sort(lg, descending=True, stable=True)
    k = min(int(top_k), int((val > NEG_INF).sum()))
    p = torch.exp((val[:k] - val[0]) / temperature)
    return idx[:k], torch.cumsum(p, 0), p


def draw_margin(logits, ok, u, top_k, temperature):
    """min_i |cdf_i - u * sum| / sum: how far u is from the nearest boundary of the inverse-CDF draw."""
    _, cdf, p = kept_cdf(logits, ok, top_k, temperature)
    return float((cdf - float(u) * p.sum()).abs().min() / p.sum())


def prompt_of(prompt, b, cfg):
    """Row b's prompt as prompt_reference takes it: the tokens of indices 1 .. P."""
    tok, ln = prompt["tok"], prompt["len"]
    P = min(max(int(ln[b]), 0), min(tok.shape[1], cfg.max_len) - 1)
    return [int(v) for v in tok[b, 1:P + 1]]


def step(st, logits, cfg, *, slot=False, table=None, prompt=None, draw=None, chained=True):
    """One selection step.  logits [B, V]; table: a transition table (grammar forms); prompt: dict(tok [B, pitch], len [B]) (static greedy
    only); draw: dict(uniforms [rows, ld], top_k, temperature, urow [B] for a slot form) (sampled forms).  -> the state after the step."""
    assert not (prompt is not None and (slot or table is not None or draw is not None))
    n = copy.deepcopy(st)
    B, V = cfg.B, cfg.V
    at = torch.zeros(B, cfg.max_len, dtype=torch.bool)
    xw = torch.zeros(B, dtype=torch.bool)
    n.margins = [None] * B
    unfinished = 0
    for b in range(B):
        if slot and int(st.finished[b]):
            continue
        t = int(st.slot_t[b]) if slot else st.step[0]
        lg = logits[b].double()
        in_prompt = False
        if draw is not None:
            tb = table if table is not None else allow_all(V)
            s = int(st.gstate[b]) if table is not None else 0
            u = float(draw["uniforms"][int(draw["urow"][b]) if slot else b, t])
            tok, lp, ns = GR.select_sample(lg, s, tb, u, draw["top_k"], draw["temperature"])
            n.margins[b] = draw_margin(lg, GR._row(tb, s)[1], u, draw["top_k"], draw["temperature"])
        elif table is not None:
            tok, lp, ns = GR.select_greedy(lg, int(st.gstate[b]), table)
        else:
            p = prompt_of(prompt, b, cfg) if prompt is not None else []
            in_prompt = t < len(p)
            if 1 <= t <= len(p) and not 0 <= p[t - 1] < V:
                p = []   # an id outside the vocabulary is not forced
            tok, lp, _ = PR.select(lg.tolist(), t, p)
        if table is not None:
            n.gstate[b] = ns
        n.seqs[b, t], n.logprobs[b, t], at[b, t] = tok, lp, True
        if slot:
            fin = tok == cfg.eos or t >= int(st.slot_cap[b]) - 1
            if fin:
                n.finished[b] = 1
            else:
                n.slot_t[b] = t + 1
            write_x = not fin
        else:
            fin = bool(st.finished[b]) or tok == cfg.eos
            n.finished[b] = int(fin)
            unfinished += 0 if (fin and not in_prompt) else 1
            write_x = chained and t + 1 < cfg.Tmax
        if write_x:
            n.x[b] = cfg.emb[tok] + cfg.pos[t + 1]   # one fp32 addition per element: exact
            xw[b] = True
    if slot:
        n.finished[B] = int((n.finished[:B] == 0).sum())
        n.step[1] = (st.step[1] + 1) % cfg.Tmax
    else:
        n.finished[B] = unfinished
        n.step = [st.step[0] + 1, st.step[1] + 1]
    n.touched = dict(seqs=at, logprobs=at, x=xw)
    return n


# ---- beam search -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Beam:
    cum: torch.Tensor        # [B] float64
    finished: torch.Tensor   # [B + 1] int64
    len: torch.Tensor        # [B] int64
    anc: torch.Tensor        # [2, B, pitch] int64: the two parity copies of the lineage
    tok: torch.Tensor        # [2, B, pitch] int64
    lp: torch.Tensor         # [2, B, pitch] float64
    step: list
    x: torch.Tensor = None
    touched: dict = field(default_factory=dict)   # lineage [2, B, pitch] bool, x [B] bool
    margin: float = math.inf                      # of the LAST step


def new_beam(cfg, K, pitch, fill=0):
    """The armed state: <bos> at 0, cum 0 for slot 0 of every image and -inf for the others, step = [1, 0]."""
    B = cfg.B
    anc = torch.full((2, B, pitch), fill, dtype=torch.int64)
    tok = torch.full((2, B, pitch), fill, dtype=torch.int64)
    lp = torch.full((2, B, pitch), float(fill), dtype=torch.float64)
    anc[1, :, 0], tok[1, :, 0], lp[1, :, 0] = torch.arange(B), cfg.bos, 0.0   # copy t & 1 = 1 is valid before step 1
    cum = torch.full((B,), NEG_INF, dtype=torch.float64)
    cum[::K] = 0.0
    E = cfg.emb.shape[1]
    return Beam(cum=cum, finished=torch.zeros(B + 1, dtype=torch.int64), len=torch.zeros(B, dtype=torch.int64), anc=anc, tok=tok, lp=lp,
                step=[1, 0], x=torch.full((B, E), float(fill), dtype=torch.float32))


def beam_candidates(logits, cum, finished, K, pad):
    """The candidates of one image, ranked: (score, candidate index parent * K + rank, token, lp), score descending, then index."""
    cands = []
    for k in range(K):
        c = float(cum[k])
        if c == NEG_INF:
            continue
        if int(finished[k]):
            cands.append((c, k * K, pad, 0.0))
            continue
        lg = logits[k].double()
        m = lg.max()
        lse = torch.log(torch.exp(lg - m).sum())
        order = torch.sort(lg, descending=True, stable=True).indices[:K].tolist()   # ties: lower index first; V < K: V of them
        for rank, v in enumerate(order):
            l = float((lg[v] - m) - lse)
            cands.append((c + l, k * K + rank, v, l))
    cands.sort(key=lambda c: (-c[0], c[1]))
    return cands


def beam_step(bm, logits, cfg, K):
    """One beam step t = step[0] on logits [B, V]: lineage copy (t & 1) is read, copy ((t + 1) & 1) written.  -> the state after it; its
    margin is the smallest gap between consecutively ranked candidates among the first K + 1 of any image."""
    n = copy.deepcopy(bm)
    B, t = cfg.B, bm.step[0]
    pitch = bm.anc.shape[2]
    cur, nxt = t & 1, (t + 1) & 1
    lin = torch.zeros(2, B, pitch, dtype=torch.bool)
    xw = torch.zeros(B, dtype=torch.bool)
    n.margin = math.inf
    for r0 in range(0, B, K):
        cands = beam_candidates(logits[r0:r0 + K], bm.cum[r0:r0 + K], bm.finished[r0:r0 + K], K, cfg.pad)
        top = cands[:K + 1]
        for a, b in zip(top, top[1:]):
            n.margin = min(n.margin, a[0] - b[0])
        for j in range(K):
            row = r0 + j
            if j < len(cands):
                sc, c, tk, l = cands[j]
                par = c // K
                if int(bm.finished[r0 + par]):
                    fin, ln = 1, int(bm.len[r0 + par])
                elif tk == cfg.eos:
                    fin, ln = 1, t
                else:
                    fin, ln = 0, 0
            else:   # a dead slot keeps its own lineage, extended by <pad>
                sc, par, tk, l, fin, ln = NEG_INF, j, cfg.pad, 0.0, 1, 0
            tc = min(t, pitch)
            for name in ("anc", "tok", "lp"):
                getattr(n, name)[nxt, row, :tc] = getattr(bm, name)[cur, r0 + par, :tc]
            lin[nxt, row, :tc] = True
            if t < pitch:
                n.anc[nxt, row, t], n.tok[nxt, row, t], n.lp[nxt, row, t] = row, tk, l
                lin[nxt, row, t] = True
            n.cum[row], n.finished[row], n.len[row] = sc, fin, ln
            if t + 1 < cfg.Tmax:
                n.x[row] = cfg.emb[tk] + cfg.pos[t + 1]
                xw[row] = True
    n.finished[B] = int((n.finished[:B] == 0).sum())
    n.step = [t + 1, bm.step[1] + 1]
    n.touched = dict(lineage=lin, x=xw)
    return n
