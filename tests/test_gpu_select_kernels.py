"""The token-selection kernels of a decode step (decode_select.hip: greedy_select_kernel<SLOT, GRAMMAR, PROMPT>, sample_select_kernel<SLOT,
GRAMMAR>, beam_select_kernel with their bookkeeping) launched ALONE through acai_debug_decode_select on logits each case writes itself, against
the float64 state transition of tests/select_reference.py.  No model is built.

Every launch: seqs, logprobs, x (and the beam lineage copy the step writes) are filled with sentinels first; afterwards what the reference
lists as written must hold the reference's value and everything else the sentinel.  Device and reference start from the same state and
evolve on their own; they are compared after every step.

Bars: tokens, flags, counters, slot times, grammar states, lineages integer-equal; x bit-equal (one fp32 addition per element);
log-probs by test_gpu_grammar._check_lps (fp32: |lp - lp64| / max(1, |lp|) <= 1e-5; ACAI_GEMM_ROUND_BF16: a bf16 number equal to the rounded
float64 value or its bf16 neighbour); beam cum within 1e-4 * max(1, |cum|) (test_gpu_beam.py's).
Margins: a draw is compared only through its token, so its u must not sit on a CDF boundary the fp32 CDF could cross.  The fp32 CDF of at
most 64 positive terms is off by about 64 * 2^-24 = 4e-6 relative; test_c_draw_at_interval_midpoints puts u at the midpoint of an entry of
probability > 1e-3 (margin >= 5e-4) and asserts margin > 1e-4, more than 20 times that error (derived, not measured).  The other sampled
cases take their u the same way, or are exact by construction (u = 0; equal logits with u = j / k, where the CDF is 1 .. k exactly; u = the
largest float below 1, where the hit and the rounding fallback name the same entry).  Random beam cases assert the reference's smallest
gap between consecutively ranked candidates among the first K + 1 above 1e-3 (test_gpu_beam.py's fp32 bar) for their hard-coded seeds.

Every live row has a finite allowed logit and there is no NaN: a row without one is outside the selection launches' contract."""
import itertools
import math

import pytest
import torch

import grammar_reference as GR
import select_reference as SR
from acai_omr_amd import ops
from decode_support import dev  # noqa: F401
from test_gpu_grammar import _check_lps

pytestmark = pytest.mark.gpu

F = ops
GREEDY = [F.SELECT_ARGMAX, F.SELECT_PROMPT, F.SELECT_GRAMMAR_ARGMAX, F.SELECT_SLOT_ARGMAX, F.SELECT_SLOT_GRAMMAR_ARGMAX]
SAMPLED = [F.SELECT_SAMPLE, F.SELECT_GRAMMAR_SAMPLE, F.SELECT_SLOT_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE]
SLOT = {F.SELECT_SLOT_ARGMAX, F.SELECT_SLOT_GRAMMAR_ARGMAX, F.SELECT_SLOT_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE}
GRAMMAR = {F.SELECT_GRAMMAR_ARGMAX, F.SELECT_SLOT_GRAMMAR_ARGMAX, F.SELECT_GRAMMAR_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE}
NAMES = {F.SELECT_ARGMAX: "argmax", F.SELECT_PROMPT: "prompt", F.SELECT_GRAMMAR_ARGMAX: "grammar_argmax", F.SELECT_SLOT_ARGMAX: "slot_argmax",
         F.SELECT_SLOT_GRAMMAR_ARGMAX: "slot_grammar_argmax", F.SELECT_SAMPLE: "sample", F.SELECT_GRAMMAR_SAMPLE: "grammar_sample",
         F.SELECT_SLOT_SAMPLE: "slot_sample", F.SELECT_SLOT_GRAMMAR_SAMPLE: "slot_grammar_sample", F.SELECT_BEAM: "beam"}
SENT_TOK, SENT_LP, SENT_X = -4242, 777.25, -555.5
U_TOP = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))   # the largest float below 1
STATS = dict(draw_margin=math.inf, beam_margin=math.inf, lp_err=0.0, cum_err=0.0, launches=0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\nselection kernels: {STATS['launches']} launches; smallest draw margin {STATS['draw_margin']:.3g}, smallest beam margin "
          f"{STATS['beam_margin']:.3g}; largest fp32 log-prob error {STATS['lp_err']:.3g} (bar 1e-5), largest cum error {STATS['cum_err']:.3g} (bar 1e-4)")


def _gen(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _cfg(V, B, max_len, Tmax=None, E=8, eos=2, seed=0):
    g = _gen(V, B, E, seed)
    Tmax = Tmax or max_len
    return SR.Cfg(V=V, B=B, max_len=max_len, Tmax=Tmax, eos=eos, bos=0, pad=min(1, V - 1), emb=torch.randn(V, E, generator=g),
                  pos=torch.randn(Tmax, E, generator=g))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lp_check(got, want, live, bf):
    """_check_lps on the positions `live`; everything else must still hold the sentinel."""
    got = got.cpu()
    assert bool((got[~live] == SENT_LP).all()), "a log-prob outside the step's writes was touched"
    if bool(live.any()):
        _check_lps(got, want, live, bf)
        if not bf:
            w = want[live]
            STATS["lp_err"] = max(STATS["lp_err"], float(((got[live].double() - w).abs() / w.abs().clamp(min=1.0)).max()))


class Sel:
    """The device buffers of one selection case beside the reference state; step() launches once and compares everything."""

    def __init__(self, dev, cfg, st, form, *, table=None, prompt=None, draw=None, tickets=False, round_lp=False, chained=True):
        self.dev, self.cfg, self.ref, self.form = dev, cfg, st, form
        self.table, self.prompt, self.draw, self.bf, self.chained = table, prompt, draw, round_lp, chained
        i32 = lambda v: torch.as_tensor(v).to(torch.int32).to(dev).contiguous()
        B = cfg.B
        self.d = dict(logits=torch.empty(B, cfg.V, device=dev), seqs=torch.empty(B, cfg.max_len, dtype=torch.int64, device=dev),
                      logprobs=torch.empty(B, cfg.max_len, device=dev), step=i32(st.step), finished=i32(st.finished),
                      x=torch.empty(B, cfg.emb.shape[1], device=dev), emb=cfg.emb.to(dev), pos=cfg.pos.to(dev))
        self.tickets = torch.zeros(4, dtype=torch.int32, device=dev) if tickets else None
        self.slots = dict(t=i32(st.slot_t), cap=i32(st.slot_cap)) if form in SLOT else None
        self.gram = None
        if form in GRAMMAR:
            self.gram = dict(next=table.next.to(dev).contiguous(), resync=table.resync.to(dev).contiguous(), state=i32(st.gstate), start=table.start)
        self.pr = dict(tok=i32(prompt["tok"]), len=i32(prompt["len"])) if form == F.SELECT_PROMPT else None
        self.uni = draw["uniforms"].to(dev).contiguous() if draw is not None else None
        self.urow = i32(draw["urow"]) if draw is not None and form in SLOT else None

    def launch(self, logits):
        d, c = self.d, self.cfg
        d["seqs"].fill_(SENT_TOK), d["logprobs"].fill_(SENT_LP), d["x"].fill_(SENT_X), d["logits"].copy_(logits)
        dr = self.draw or {}
        ops.debug_decode_select(self.form, d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], max_len=c.max_len, Tmax=c.Tmax,
                                eos=c.eos, bos=c.bos, pad=c.pad, emb=d["emb"], pos=d["pos"], x=d["x"], tickets=self.tickets, round_lp=self.bf,
                                chained=self.chained, slots=self.slots, grammar=self.gram, prompt=self.pr, uniforms=self.uni, urow=self.urow,
                                top_k=dr.get("top_k", 1), temperature=dr.get("temperature", 1.0))
        torch.cuda.synchronize()
        STATS["launches"] += 1

    def mid_uniforms(self, logits, shift=0):
        """Puts the u of every live row's coming draw on `logits` at an interval midpoint (the caller rewrites the table between launches)."""
        dr, r, slot = self.draw, self.ref, self.form in SLOT
        for b in range(self.cfg.B):
            if slot and int(r.finished[b]):
                continue
            t = int(r.slot_t[b]) if slot else r.step[0]
            ok = GR._row(self.table, int(r.gstate[b]))[1] if self.form in GRAMMAR else None
            dr["uniforms"][dr["urow"][b] if slot else b, t] = _mid_u(logits[b], ok, dr["top_k"], dr["temperature"], b + shift)
        self.uni.copy_(dr["uniforms"])

    def step(self, logits):
        """logits: CPU fp32 [B, V].  -> the reference state after the step (the device agreed with all of it)."""
        slot = self.form in SLOT
        self.ref = r = SR.step(self.ref, logits, self.cfg, slot=slot, table=self.table if self.form in GRAMMAR else None, prompt=self.prompt,
                               draw=self.draw, chained=self.chained)
        self.launch(logits)
        d, name = self.d, NAMES[self.form]
        at = r.touched["seqs"]
        want = torch.where(at, r.seqs, torch.full_like(r.seqs, SENT_TOK))
        got = d["seqs"].cpu()
        assert torch.equal(got, want), (name, "tokens", (got != want).nonzero().tolist()[:8], got[got != want][:8], want[got != want][:8])
        _lp_check(d["logprobs"], r.logprobs, at, self.bf)
        wx = torch.where(r.touched["x"][:, None], r.x, torch.full_like(r.x, SENT_X))
        assert torch.equal(_bits(d["x"].cpu()), _bits(wx)), (name, "x", (d["x"].cpu() != wx).any(1).nonzero().flatten().tolist())
        assert d["finished"].cpu().tolist() == r.finished.tolist(), (name, "finished", d["finished"].cpu().tolist(), r.finished.tolist())
        assert d["step"].cpu().tolist() == r.step, (name, "step", d["step"].cpu().tolist(), r.step)
        if slot:
            assert self.slots["t"].cpu().tolist() == r.slot_t.tolist(), (name, "slot t")
            assert self.slots["cap"].cpu().tolist() == r.slot_cap.tolist(), (name, "slot cap")
        if self.gram is not None:
            assert self.gram["state"].cpu().tolist() == r.gstate.tolist(), (name, "grammar state", self.gram["state"].cpu().tolist(), r.gstate.tolist())
        if self.tickets is not None:
            assert self.tickets.cpu().tolist() == [0, 0, 0, 0], (name, "the arrival counter must read 0 between launches")
        return r


def _margins(r):
    """Every draw of the step sits more than 1e-4 from a CDF boundary (see the module's note on margins)."""
    ms = [m for m in r.margins if m is not None]
    assert all(m > 1e-4 for m in ms), ("u too close to a boundary of the draw for an fp32 CDF", ms)
    STATS["draw_margin"] = min([STATS["draw_margin"]] + ms)


def _mid_u(lg, ok, top_k, temperature, want):
    """u (an fp32 value) at the midpoint of the CDF interval of a kept entry with probability > 1e-3: the want-th such entry (cyclic)."""
    _, cdf, p = SR.kept_cdf(lg, ok, top_k, temperature)
    tot = float(p.sum())
    good = [r for r in range(len(p)) if float(p[r]) / tot > 1e-3]
    r = good[want % len(good)]
    lo = float(cdf[r - 1]) if r else 0.0
    return float(torch.tensor((lo + float(cdf[r])) / 2 / tot, dtype=torch.float32))


def _planted(V):
    """The indices the layout rows (_layout_logits) are built around: no test table may forbid them."""
    return sorted({p for p in (0, 1, 2, 3, 5, 63, 64, 67, V - 2, V - 1) if 0 <= p < V})


def _thirds_table(V):
    """Two states: 0 allows every token, 1 forbids the tokens i % 3 == 1 - but none of the planted indices, so that a row in state 1 keeps
    every placement and tie it was built for and loses only tokens around them."""
    nxt = torch.zeros(2, V, dtype=torch.int16)
    nxt[0, ::2] = 1
    nxt[1, 1::3] = -1
    nxt[1, _planted(V)] = 0
    return SR.Table(nxt, start=0, resync=torch.zeros(V, dtype=torch.int16))


def _setup(dev, form, cfg, logits, *, t=2, slot_t=None, caps=None, finished=None, table=None, gstate=None, prompt=None, top_k=4, temperature=1.0,
           want_rank=None, u=None, urow=None, cache=0, **kw):
    """A Sel for any of the nine forms on one logit matrix: the draw's u at interval midpoints (rank want_rank[b], default b) unless given."""
    B = cfg.B
    if form in GRAMMAR:
        table = table if table is not None else _thirds_table(cfg.V)
        gstate = gstate if gstate is not None else [b % table.states for b in range(B)]
    else:
        table = gstate = None
    if form in SLOT:
        slot_t = slot_t if slot_t is not None else [1 + b % 3 for b in range(B)]
        caps = caps if caps is not None else [cfg.max_len] * B
    if form == F.SELECT_PROMPT and prompt is None:
        prompt = dict(tok=torch.full((B, cfg.max_len), -1, dtype=torch.int64), len=torch.zeros(B, dtype=torch.int64))
    st = SR.new_state(cfg, t=t, cache=cache, slot_t=slot_t if form in SLOT else None, slot_cap=caps if form in SLOT else None, gstate=gstate,
                      finished=finished)
    draw = None
    if form in SAMPLED:
        rows = B if form not in SLOT else B + (3 if (B + 3) % 7 else 4)
        urow = urow if urow is not None else [(b * 7 + 3) % rows for b in range(B)]   # (distinct: rows is no multiple of 7)
        uni = torch.full((rows, cfg.max_len + (2 if form in SLOT else 0)), 0.5, dtype=torch.float32)
        for b in range(B):
            tb = int(slot_t[b]) if form in SLOT else t
            ok = GR._row(table, gstate[b])[1] if table is not None else None
            ub = u[b] if u is not None else _mid_u(logits[b], ok, top_k, temperature, b if want_rank is None else want_rank[b])
            uni[urow[b] if form in SLOT else b, tb] = ub
        draw = dict(uniforms=uni, top_k=top_k, temperature=temperature, urow=urow)
    return Sel(dev, cfg, st, form, table=table, prompt=prompt if form == F.SELECT_PROMPT else None, draw=draw, **kw)


# ---- a. vocabulary and row layout --------------------------------------------------------------------------------------------------------
def _layout_logits(V):
    """One row per placement of the maximum at 0 / 63 / 64 / V - 1, one per tie of two of them (across lanes; 0 and 64 share a lane), and
    rows whose 4th and 5th largest entries tie - inside a lane (3, 67) and across lanes (1, V - 1): top_k = 4 keeps the lower index."""
    g = _gen(V, 11)
    P = sorted({p for p in (0, 63, 64, V - 1) if p < V})
    rows, rank = [], []
    for hot in [(p,) for p in P] + list(itertools.combinations(P, 2)):
        lg = torch.randn(V, generator=g)
        lg[list(hot)] = 5.0
        rows.append(lg)
        rank.append(0)   # (u at the midpoint of the first entry: a sampled form draws the maximum)
    for pair in ((3, 67), (1, V - 1)):
        if V >= 68 or (V >= 8 and pair[0] == 1):
            lg = 0.3 * torch.randn(V, generator=g)
            lg[2], lg[5], lg[V - 2] = 3.0, 2.9, 2.8
            lg[list(pair)] = 2.7
            rows.append(lg)
            rank.append(3)
    return torch.stack(rows), rank


_VS = [1, 2, 63, 64, 65, 227, 448, 449, 511, 512]
_LAYOUT = [(f, v) for f in GREEDY for v in _VS + [513, 1000]] + [(f, v) for f in SAMPLED for v in _VS]   # (the sampled forms refuse V > 512)


@pytest.mark.parametrize("form,V", _LAYOUT, ids=[f"{NAMES[f]}-V{v}" for f, v in _LAYOUT])
def test_a_vocabulary_layout(dev, form, V):
    logits, rank = _layout_logits(V)
    cfg = _cfg(V, logits.shape[0], max_len=6, eos=2 if V > 2 else V)
    s = _setup(dev, form, cfg, logits, want_rank=rank, tickets=form in SLOT)
    r = s.step(logits)
    _margins(r)
    # what the inputs were built for, stated without the reference, for EVERY form (the grammar forms' rows alternate between the state that
    # allows everything and the restrictive one, which forbids none of the planted indices): the planted maximum; the lower index of a tie;
    # in the rows whose 4th and 5th entries tie, the arg-max 2 (greedy) or the 4th kept entry = the tie's lower index (sampled, top_k 4)
    P = sorted({p for p in (0, 63, 64, V - 1) if p < V})
    want = P + [a for a, _ in itertools.combinations(P, 2)]
    want += [(2 if form in GREEDY else 3)] * (V >= 68) + [(2 if form in GREEDY else 1)] * (V >= 8)
    assert r.seqs[r.touched["seqs"]].tolist() == want
    if form in GRAMMAR:
        assert s.table.states == 2 and int((s.table.next[1] < 0).sum()) == len(range(1, V, 3)) - len([p for p in _planted(V) if p % 3 == 1])


# ---- b. launch edges ----------------------------------------------------------------------------------------------------------------------
def _rand_logits(B, V, *key, scale=3.0):
    return scale * torch.randn(B, V, generator=_gen(B, V, *key))


_BATCH = [(f, b) for f in GREEDY for b in (1, 4, 5, 8, 9, 16, 17, 33, 40)] + [(f, b) for f in SAMPLED for b in (1, 4, 5, 18, 33)]


@pytest.mark.parametrize("round_lp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form,B", _BATCH, ids=[f"{NAMES[f]}-B{b}" for f, b in _BATCH])
def test_b_batch_sizes(dev, form, B, round_lp):
    V = 65
    cfg = _cfg(V, B, max_len=7, Tmax=9)
    logits = _rand_logits(B, V, form)
    logits[::5, cfg.eos] = 12.0   # some rows finish
    fin = [1 if b % 4 == 3 else 0 for b in range(B)]   # finished (static) / idle (slot) rows
    s = _setup(dev, form, cfg, logits, t=3, finished=fin, slot_t=[1 + b % 5 for b in range(B)], caps=[2 + (3 * b) % 5 for b in range(B)], cache=8,
               tickets=form in SLOT, round_lp=round_lp)
    _margins(s.step(logits))


@pytest.mark.parametrize("form", [F.SELECT_SLOT_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE], ids=lambda f: NAMES[f])
@pytest.mark.parametrize("tickets,B", [(True, 18), (False, 9)], ids=["tickets", "one_workgroup"])
def test_b_slot_sampling_closes_the_step(dev, form, tickets, B):
    """With the arrival counter (ceil(B / 4) workgroups) it reads 0 after each of three consecutive steps; without, one workgroup loops."""
    V, T = 65, 8
    cfg = _cfg(V, B, max_len=T, Tmax=T)
    s = None
    for k in range(3):
        logits = _rand_logits(B, V, form, k)
        if s is None:
            s = _setup(dev, form, cfg, logits, slot_t=[1 + b % 3 for b in range(B)], caps=[T - b % 3 for b in range(B)], cache=T - 2, tickets=tickets)
        s.mid_uniforms(logits, shift=k)
        r = s.step(logits)
        _margins(r)
    assert r.step[1] == 1, "the ring index wrapped"


@pytest.mark.parametrize("E", [4, 252, 256, 260, 1024])
@pytest.mark.parametrize("form", [F.SELECT_ARGMAX, F.SELECT_SLOT_ARGMAX, F.SELECT_SAMPLE, F.SELECT_SLOT_SAMPLE], ids=lambda f: NAMES[f])
def test_b_next_input_widths(dev, form, E):
    B, V = 5, 65
    cfg = _cfg(V, B, max_len=6, Tmax=8, E=E)
    logits = _rand_logits(B, V, E)
    logits[:, cfg.eos] = -9.0   # (a slot row that ends writes no next input)
    r = _setup(dev, form, cfg, logits, tickets=form in SLOT).step(logits)
    _margins(r)
    assert bool(r.touched["x"].all())


@pytest.mark.parametrize("form", [f for f in GREEDY + SAMPLED if f not in SLOT], ids=lambda f: NAMES[f])
def test_b_unchained_leaves_x(dev, form):
    B, V = 6, 65
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, 3)
    r = _setup(dev, form, cfg, logits, chained=False).step(logits)
    _margins(r)
    assert not bool(r.touched["x"].any())


# ---- c. the draw --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [40, 512])
@pytest.mark.parametrize("temperature", [0.05, 1.0, 100.0])
@pytest.mark.parametrize("top_k", [1, 2, 63, 64])
@pytest.mark.parametrize("form", SAMPLED, ids=lambda f: NAMES[f])
def test_c_draw_at_interval_midpoints(dev, form, top_k, temperature, V):
    """u at the midpoint of a random entry of probability > 1e-3 (V = 40: top_k above V; temperature 0.05: the tail's expf underflows)."""
    B = 8
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, top_k, scale=5.0)
    g = _gen(V, top_k, 17)
    s = _setup(dev, form, cfg, logits, top_k=top_k, temperature=temperature, want_rank=torch.randint(0, 64, (B,), generator=g).tolist(),
               tickets=form in SLOT)
    r = s.step(logits)
    _margins(r)
    assert len([m for m in r.margins if m is not None]) == B
    if temperature == 0.05 and top_k >= 63 and V == 512:
        lg = logits.double().sort(1, descending=True).values
        assert float(((lg[:, top_k - 1] - lg[:, 0]) / temperature).max()) < -104, "the tail must underflow in fp32 (expf(-104) = 0)"


@pytest.mark.parametrize("form", SAMPLED, ids=lambda f: NAMES[f])
def test_c_fixed_edge_draws(dev, form):
    """u = 0 gives rank 0; u = the largest float below 1 gives the last kept entry (its probability is above 1e-3 here: logits of small spread)."""
    B, V, k = 8, 227, 8
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, 23, scale=0.5)
    table = SR.allow_all(V)
    u = [0.0 if b % 2 == 0 else U_TOP for b in range(B)]
    r = _setup(dev, form, cfg, logits, table=table, gstate=[0] * B, top_k=k, u=u, tickets=form in SLOT).step(logits)
    for b in range(B):
        idx, _, p = SR.kept_cdf(logits[b], None, k, 1.0)
        assert float(p[-1] / p.sum()) > 1e-3
        assert int(r.seqs[b][r.touched["seqs"][b]]) == int(idx[0] if b % 2 == 0 else idx[-1])


@pytest.mark.parametrize("form", [F.SELECT_SAMPLE, F.SELECT_SLOT_SAMPLE], ids=lambda f: NAMES[f])
def test_c_unmasked_draw_at_the_top_of_an_underflowed_cdf(dev, form):
    """temperature 0.05, top_k 64, u = the largest float below 1: the tail's expf is 0 in fp32, so which tail entry the draw names is a
    matter of rounding (a trailing prefix that rounds above u * sum, or the fallback k - 1) and is not compared with the reference's.  What
    must hold: the token is a kept entry at the top of the CDF - the entry hit has an fp32 prefix above u * sum >= sum * (1 - 2^-22), and
    an fp32 prefix of at most 64 terms is within 64 * 2^-24 of the true one, so its float64 inclusive CDF is at least 1 - 5e-6 of the sum
    (4.1e-6 derived, rounded up; the fallback k - 1 has CDF 1) - and its log-prob is log_softmax(kept)[token]."""
    B, V, k, T = 8, 512, 64, 0.05
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, 83, scale=5.0)
    logits[:, cfg.eos] = -40.0
    s = _setup(dev, form, cfg, logits, top_k=k, temperature=T, u=[U_TOP] * B, slot_t=[2] * B, tickets=form in SLOT)
    s.ref = SR.step(s.ref, logits, cfg, slot=form in SLOT, draw=s.draw)   # (only for the positions the step writes)
    s.launch(logits)
    at = s.ref.touched["seqs"]
    toks, lps = s.d["seqs"].cpu()[at].tolist(), s.d["logprobs"].cpu()[at].double()
    want = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        idx, cdf, p = SR.kept_cdf(logits[b], None, k, T)
        val = logits[b].double()[idx]
        assert int(((val - val[0]) / T > -87.0).sum()) < k - 8, "the tail must underflow (expf below -87 is 0 or a denormal)"
        assert toks[b] in idx.tolist(), (b, toks[b], idx.tolist())
        assert float(cdf[idx.tolist().index(toks[b])] / p.sum()) >= 1 - 5e-6, (b, toks[b])
        want[b] = (logits[b, toks[b]].double() - val[0]) - torch.log(torch.exp(val - val[0]).sum())
    assert float(((lps - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-5


@pytest.mark.parametrize("k,part", [(2, 0), (4, 0), (64, 0), (64, 1)])
@pytest.mark.parametrize("form", SAMPLED, ids=lambda f: NAMES[f])
def test_c_exact_boundaries(dev, form, k, part):
    """k equal logits, u = j / k: the CDF is 1 .. k exactly and u * sum = j exactly, so the strict > gives rank j."""
    V = 227
    js = list(range(k))[part * 32:(part + 1) * 32]
    B = len(js)
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    g = _gen(k, 29)
    logits = -1.0 - torch.rand(B, V, generator=g)
    hot = [sorted(torch.randperm(V, generator=g)[:k].tolist()) for _ in range(B)]
    for b in range(B):
        logits[b, hot[b]] = 3.0
    r = _setup(dev, form, cfg, logits, table=SR.allow_all(V), gstate=[0] * B, top_k=k, u=[j / k for j in js], tickets=form in SLOT).step(logits)
    for b, j in enumerate(js):
        assert int(r.seqs[b][r.touched["seqs"][b]]) == hot[b][j], (b, j)


def _narrow_table(V):
    """0: one token; 1: three tokens; 2: dead (allows nothing); 3: everything."""
    nxt = torch.full((4, V), -1, dtype=torch.int16)
    nxt[0, 70] = 1
    nxt[1, [5, 69, V - 1]] = torch.tensor([2, 2, 2], dtype=torch.int16)
    nxt[3] = 0
    return SR.Table(nxt, start=3, resync=torch.arange(V) % 4)


@pytest.mark.parametrize("form", sorted(GRAMMAR), ids=lambda f: NAMES[f])
def test_c_grammar_rows(dev, form):
    """One allowed token; fewer than top_k (at u = the largest float below 1 the fallback is the last entry that holds a token); a dead
    state (unconstrained, then resync); states outside [0, states) are clamped.  Two steps, so that every next state is read back."""
    V, T = 227, 6
    states = [0, 1, 1, 1, 2, 2, 3, -5, 99]
    B = len(states)
    cfg = _cfg(V, B, max_len=T, Tmax=T + 2)
    table = _narrow_table(V)
    logits = _rand_logits(B, V, 31, scale=1.0)
    u = None
    if form in SAMPLED:
        u = [_mid_u(logits[b], GR._row(table, states[b])[1], 8, 1.0, b) for b in range(B)]
        u[0], u[2], u[3] = 0.77, U_TOP, 0.0
    s = _setup(dev, form, cfg, logits, table=table, gstate=states, top_k=8, u=u, slot_t=[2] * B, tickets=form in SLOT)
    r = s.step(logits)
    got = r.seqs[r.touched["seqs"]].tolist()
    assert got[0] == 70 and float(r.logprobs[r.touched["seqs"]][0]) == 0.0 and got[7] == 70 and set(got[1:4]) <= {5, 69, V - 1}
    assert r.gstate.tolist()[:4] == [1, 2, 2, 2] and r.gstate.tolist()[4:6] == [got[4] % 4, got[5] % 4]
    if form in SAMPLED:
        assert got[2] == int(SR.kept_cdf(logits[2], GR._row(table, 1)[1], 8, 1.0)[0][-1]), "the fallback is the last entry that holds a token"
        assert got[3] == int(SR.kept_cdf(logits[3], GR._row(table, 1)[1], 8, 1.0)[0][0])
        s.mid_uniforms(logits * 0.5, shift=1)   # the second step's u, for the states the first step left
    s.step(logits * 0.5)


@pytest.mark.parametrize("top_k", [8, 64])
@pytest.mark.parametrize("form", [F.SELECT_GRAMMAR_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE], ids=lambda f: NAMES[f])
def test_c_masked_draw_at_the_top_of_the_cdf(dev, form, top_k):
    """2 .. 7 allowed tokens under top_k 8 / 64 with u = the largest float below 1 and u = 1 - 2^-12: the drawn entry is the last one that
    holds a token.  The lanes past the allowed set carry the same prefix sum plus zeros, added in another order; one of them rounding above
    u * sum must not be hit (it holds the token 0x7fffffff, and the next input would be read far outside emb)."""
    V, S = 227, 6
    B = 36
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    g = _gen(73)
    nxt = torch.full((S, V), -1, dtype=torch.int16)
    for s in range(S):
        nxt[s, torch.randperm(V, generator=g)[:s + 2]] = 0
    table = SR.Table(nxt, start=0)
    states = [b % S for b in range(B)]
    logits = _rand_logits(B, V, 79, scale=1.0)
    u = [U_TOP if b % 3 else 1.0 - 2.0 ** -12 for b in range(B)]
    # (the static form runs unchained, so that a lane past the allowed set being hit shows as a token mismatch, not as a fault in the read
    # of emb; a slot step always writes the next input)
    r = _setup(dev, form, cfg, logits, table=table, gstate=states, top_k=top_k, u=u, slot_t=[2] * B, tickets=form in SLOT,
               chained=form in SLOT).step(logits)
    for b in range(B):
        idx, _, p = SR.kept_cdf(logits[b], GR._row(table, states[b])[1], top_k, 1.0)
        assert len(idx) == states[b] + 2 and float(p[-1] / p.sum()) > 1e-3
        assert int(r.seqs[b][r.touched["seqs"][b]]) == int(idx[-1])


@pytest.mark.parametrize("plain,masked", [(F.SELECT_ARGMAX, F.SELECT_GRAMMAR_ARGMAX), (F.SELECT_SLOT_ARGMAX, F.SELECT_SLOT_GRAMMAR_ARGMAX),
                                          (F.SELECT_SAMPLE, F.SELECT_GRAMMAR_SAMPLE), (F.SELECT_SLOT_SAMPLE, F.SELECT_SLOT_GRAMMAR_SAMPLE)],
                         ids=lambda f: NAMES[f])
@pytest.mark.parametrize("round_lp", [False, True], ids=["fp32", "bf16"])
def test_c_table_that_allows_everything_is_the_plain_form(dev, plain, masked, round_lp):
    B, V = 9, 227
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, 37)
    u = [_mid_u(logits[b], None, 50, 1.1, b) for b in range(B)]
    kw = dict(top_k=50, temperature=1.1, u=u, round_lp=round_lp)
    a = _setup(dev, plain, cfg, logits, tickets=plain in SLOT, **kw)
    b = _setup(dev, masked, cfg, logits, table=SR.allow_all(V), gstate=[0] * B, tickets=masked in SLOT, **kw)
    _margins(a.step(logits)), _margins(b.step(logits))
    for name in ("seqs", "finished", "step"):
        assert torch.equal(a.d[name], b.d[name]), name
    assert torch.equal(_bits(a.d["logprobs"]), _bits(b.d["logprobs"])) and torch.equal(_bits(a.d["x"]), _bits(b.d["x"]))


# ---- d. bookkeeping over consecutive steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [F.SELECT_ARGMAX, F.SELECT_GRAMMAR_ARGMAX, F.SELECT_SAMPLE, F.SELECT_GRAMMAR_SAMPLE], ids=lambda f: NAMES[f])
def test_d_static_bookkeeping(dev, form):
    """Finished rows are still written and stay finished; finished[B], step[0], step[1] after every step; no x at t + 1 == Tmax."""
    B, V, T = 6, 65, 6
    cfg = _cfg(V, B, max_len=T, Tmax=T)
    table = SR.allow_all(V) if form in GRAMMAR else None
    run = {t: _rand_logits(B, V, form, t) for t in range(1, T)}
    run[2][2, cfg.eos] = run[3][4, cfg.eos] = 25.0
    s = _setup(dev, form, cfg, run[1], t=1, finished=[0, 1, 0, 0, 0, 0], table=table, gstate=[0] * B, cache=3)
    for t in range(1, T):
        if form in SAMPLED:
            s.mid_uniforms(run[t], shift=t)
        r = s.step(run[t])
        _margins(r)
        assert bool(r.touched["seqs"][:, t].all()) and bool(r.touched["x"].all()) == (t + 1 < T)
    assert r.finished.tolist()[1] == 1 and r.finished.tolist()[2] == 1 and r.finished.tolist()[4] == 1 and r.step == [T, 3 + T - 1]


@pytest.mark.parametrize("form", sorted(SLOT), ids=lambda f: NAMES[f])
def test_d_slot_bookkeeping(dev, form):
    """Rows at different t with caps in 2 .. T; one ends by <eos>, others by cap - 1; finished and idle rows write nothing; step[1] wraps at
    Tmax; urow is a permutation."""
    B, V, T = 7, 65, 7
    cfg = _cfg(V, B, max_len=T, Tmax=T)
    table = SR.allow_all(V) if form in GRAMMAR else None
    t0, caps, fin = [1, 2, 1, 3, 1, 1, 2], [2, T, 5, T, 3, T, 4], [0, 0, 0, 0, 0, 1, 0]
    urow = [4, 2, 6, 0, 5, 1, 3]
    s, by_eos = None, False
    for k in range(T):
        logits = _rand_logits(B, V, 41, k)
        logits[:, cfg.eos] = -9.0
        if k == 1:
            logits[1, cfg.eos] = 15.0
        if s is None:
            s = _setup(dev, form, cfg, logits, slot_t=t0, caps=caps, finished=fin, table=table, gstate=[0] * B, cache=T - 2, urow=urow, tickets=True)
        if form in SAMPLED:
            s.mid_uniforms(logits, shift=k)
        before = s.ref
        r = s.step(logits)
        _margins(r)
        for b in range(B):
            if int(before.finished[b]):
                assert not bool(r.touched["seqs"][b].any()) and not bool(r.touched["x"][b])
        by_eos = by_eos or (int(r.finished[1]) == 1 and int(before.finished[1]) == 0 and int(r.slot_t[1]) < caps[1] - 1)
        if int(r.finished[B]) == 0:
            break
    assert by_eos and int(r.finished[B]) == 0 and int(r.slot_t[3]) == T - 1 and int(r.slot_t[0]) == 1
    assert r.step[0] == 2 and r.step[1] < T - 2, "step[0] is left alone and the ring index wrapped"


def test_d_prompt_bookkeeping(dev):
    """Lengths 0, 1, max_len - 1 and one above the clamp; an id outside [0, V) (the arg-max is used); forced tokens that are not the arg-max;
    <eos> inside the prompt: the flag is set and the row still counts as unfinished."""
    V, T = 65, 7
    g = _gen(47)
    lens = [0, 1, T - 1, 99, 3, 4, 2]
    B = len(lens)
    cfg = _cfg(V, B, max_len=T, Tmax=T)
    tok = torch.randint(3, V, (B, T + 2), generator=g)   # pitch above max_len
    tok[4, 2], tok[5, 2] = V + 5, cfg.eos
    tok[6, 1] = -1
    s, forced_other, eos_inside = None, 0, False
    for t in range(1, T):
        logits = _rand_logits(B, V, 53, t)
        logits[:, cfg.eos] = -9.0
        if s is None:
            s = _setup(dev, F.SELECT_PROMPT, cfg, logits, t=1, prompt=dict(tok=tok, len=torch.tensor(lens)))
        r = s.step(logits)
        am = logits.argmax(1)
        for b in range(B):
            P = min(max(lens[b], 0), T - 1)
            if t <= P and 0 <= int(tok[b, t]) < V:
                assert int(r.seqs[b, t]) == int(tok[b, t])
                forced_other += int(tok[b, t]) != int(am[b])
            else:
                assert int(r.seqs[b, t]) == int(am[b])
        if t == 2:
            eos_inside = int(r.finished[5]) == 1 and int(r.finished[B]) == B
    assert forced_other >= 10 and eos_inside and r.finished.tolist() == [0, 0, 0, 0, 0, 1, 0, B - 1]


# ---- e. beam ------------------------------------------------------------------------------------------------------------------------------
class BeamRun:
    def __init__(self, dev, cfg, K, bm, round_lp=False):
        self.dev, self.cfg, self.K, self.ref, self.bf = dev, cfg, K, bm, round_lp
        to = lambda v, dt: v.to(dt).to(dev).contiguous()
        lp = torch.where(torch.isfinite(bm.lp), bm.lp, torch.zeros_like(bm.lp))
        self.d = dict(logits=torch.empty(cfg.B, cfg.V, device=dev), step=to(torch.tensor(bm.step), torch.int32), finished=to(bm.finished, torch.int32),
                      x=torch.empty(cfg.B, cfg.emb.shape[1], device=dev), emb=cfg.emb.to(dev), pos=cfg.pos.to(dev))
        self.b = dict(K=K, anc=to(bm.anc, torch.int32), tok=to(bm.tok, torch.int64), lp=to(lp, torch.float32), cum=to(bm.cum, torch.float32),
                      len=to(bm.len, torch.int32))

    def launch(self):
        c, d = self.cfg, self.d
        ops.debug_decode_select(F.SELECT_BEAM, d["logits"], None, None, d["step"], d["finished"], max_len=c.max_len, Tmax=c.Tmax, eos=c.eos,
                                bos=c.bos, pad=c.pad, emb=d["emb"], pos=d["pos"], x=d["x"], round_lp=self.bf, beam=self.b)
        torch.cuda.synchronize()
        STATS["launches"] += 1

    def step(self, logits):
        c, d, b = self.cfg, self.d, self.b
        t = self.ref.step[0]
        cur, nxt = t & 1, (t + 1) & 1
        self.ref = r = SR.beam_step(self.ref, logits, c, self.K)
        b["anc"][nxt].fill_(SENT_TOK), b["tok"][nxt].fill_(SENT_TOK), b["lp"][nxt].fill_(SENT_LP), d["x"].fill_(SENT_X), d["logits"].copy_(logits)
        keep = {n: b[n][cur].clone() for n in ("anc", "tok", "lp")}
        self.launch()
        lin = r.touched["lineage"][nxt]
        for n in ("anc", "tok"):
            want = torch.where(lin, getattr(r, n)[nxt], torch.full_like(r.anc[nxt], SENT_TOK))
            assert torch.equal(b[n][nxt].cpu().long(), want), ("beam", n, (b[n][nxt].cpu().long() != want).nonzero().tolist()[:8])
        _lp_check(b["lp"][nxt], r.lp[nxt], lin, self.bf)
        for n in keep:
            assert torch.equal(b[n][cur], keep[n]), ("beam", "the copy the step reads was written", n)
        got, want = b["cum"].cpu().double(), r.cum
        dead = want == -math.inf
        assert torch.equal(got == -math.inf, dead), ("beam", "dead slots", got.tolist(), want.tolist())
        if bool((~dead).any()):
            err = (got[~dead] - want[~dead]).abs() / want[~dead].abs().clamp(min=1.0)
            STATS["cum_err"] = max(STATS["cum_err"], float(err.max()))
            assert float(err.max()) <= 1e-4, ("beam", "cum", got.tolist(), want.tolist())
        assert b["len"].cpu().tolist() == r.len.tolist(), ("beam", "len", b["len"].cpu().tolist(), r.len.tolist())
        assert d["finished"].cpu().tolist() == r.finished.tolist(), ("beam", "finished", d["finished"].cpu().tolist(), r.finished.tolist())
        assert d["step"].cpu().tolist() == r.step
        wx = torch.where(r.touched["x"][:, None], r.x, torch.full_like(r.x, SENT_X))
        assert torch.equal(_bits(d["x"].cpu()), _bits(wx)), ("beam", "x")
        return r


BEAM_STEPS = 6


def _beam_logits(seed, n, K, V, step):
    return 4.0 * torch.randn(n * K, V, generator=_gen(seed, n, K, V, step))


def beam_margin(seed, n, K, V):
    """The smallest reference margin of the random case (CPU only: the seeds below were chosen with it)."""
    cfg = _cfg(V, n * K, max_len=BEAM_STEPS + 2, Tmax=BEAM_STEPS + 3, eos=2)
    bm, m = SR.new_beam(cfg, K, cfg.max_len), math.inf
    for k in range(BEAM_STEPS):
        bm = SR.beam_step(bm, _beam_logits(seed, n, K, V, k), cfg, K)
        m = min(m, bm.margin)
    return m


# (n, K, V) -> the first seed whose smallest margin (beam_margin, on the CPU) is above 2e-3; seed 0 where not listed
BEAM_SEEDS = {(1, 15, 64): 4, (1, 16, 3): 1, (1, 16, 65): 1, (1, 16, 512): 7, (3, 5, 512): 2, (3, 8, 3): 1, (3, 8, 64): 5, (3, 8, 512): 1,
              (3, 15, 64): 20, (3, 15, 65): 83, (3, 15, 512): 34, (3, 16, 64): 16, (3, 16, 65): 66, (3, 16, 512): 100}


@pytest.mark.parametrize("V", [3, 64, 65, 512])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 15, 16])
@pytest.mark.parametrize("n", [1, 3])
def test_e_beam_random(dev, n, K, V):
    seed = BEAM_SEEDS.get((n, K, V), 0)
    cfg = _cfg(V, n * K, max_len=BEAM_STEPS + 2, Tmax=BEAM_STEPS + 3, eos=2)
    run = BeamRun(dev, cfg, K, SR.new_beam(cfg, K, cfg.max_len, fill=SENT_TOK))
    dead = False
    for k in range(BEAM_STEPS):
        r = run.step(_beam_logits(seed, n, K, V, k))
        assert r.margin > 1e-3, f"seed {seed} (n={n} K={K} V={V}) step {k}: margin {r.margin} - decisions not separated enough for fp32"
        STATS["beam_margin"] = min(STATS["beam_margin"], r.margin)
        dead = dead or bool((r.cum == -math.inf).any())
    if V < K:
        assert dead, "V < K must leave dead slots"


def _beam_state(cfg, K, pitch, t, cum, fin, ln, seed=59):
    g = _gen(seed)
    B = cfg.B
    bm = SR.new_beam(cfg, K, pitch, fill=SENT_TOK)
    cp = t & 1
    bm.anc[cp, :, :t] = (torch.arange(B) // K * K)[:, None] + torch.randint(0, K, (B, t), generator=g)
    bm.tok[cp, :, :t] = torch.randint(3, cfg.V, (B, t), generator=g)
    bm.lp[cp, :, :t] = -torch.rand(B, t, generator=g).to(torch.bfloat16).double()   # (bf16 numbers: a bf16 run copies them unchanged)
    bm.anc[1 - cp], bm.tok[1 - cp], bm.lp[1 - cp] = SENT_TOK, SENT_TOK, SENT_LP
    bm.cum, bm.len = torch.tensor(cum, dtype=torch.float64), torch.tensor(ln)
    bm.finished[:B] = torch.tensor(fin)
    bm.step = [t, t - 1]
    return bm


@pytest.mark.parametrize("t", [3, 5], ids=["t3", "t_pitch_minus_1"])
@pytest.mark.parametrize("round_lp", [False, True], ids=["fp32", "bf16"])
def test_e_beam_constructed(dev, t, round_lp):
    """Image 0: exact ties across parents (equal cum, equal logit rows) and within a row; image 1: a finished parent that outranks every live
    extension, a parent at cum = -inf, <eos> as a chosen token; image 2: every row finished.  At t = 3 and at t = pitch - 1."""
    K, V, pitch = 4, 16, 6
    inf = math.inf
    cfg = _cfg(V, 3 * K, max_len=pitch, Tmax=pitch + 2)
    cum = [-1.0, -1.0, -1.0, -2.5, -3.0, -0.25, -inf, -3.0, -1.0, -2.0, -0.5, -4.0]
    fin = [0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1]
    ln = [0, 0, 0, 0, 0, 2, 0, 0, 1, 2, 2, 1]
    bm = _beam_state(cfg, K, pitch, t, cum, fin, ln)
    row = torch.tensor([0.0, 2.0, -1.0, 2.0, 1.0, 1.0, 1.0] + [-3.0] * (V - 7))   # ties inside the row: 1 and 3; 4, 5 and 6
    logits = _rand_logits(3 * K, V, 61)
    logits[0], logits[1], logits[2], logits[3] = row, row, row, row
    logits[4, cfg.eos] = 9.0
    r = BeamRun(dev, cfg, K, bm, round_lp).step(logits)
    assert r.margin == 0.0
    cp = (t + 1) & 1
    assert r.tok[cp, :4, t].tolist() == [1, 3, 1, 3] and r.anc[cp, :4, t - 1].tolist() == bm.anc[t & 1, [0, 0, 1, 1], t - 1].tolist()
    assert int(r.tok[cp, 4, t]) == cfg.pad and float(r.cum[4]) == -0.25 and int(r.len[4]) == 2, "the finished parent ranks first"
    assert int(r.tok[cp, 5, t]) == cfg.eos and int(r.len[5]) == t and int(r.finished[5]) == 1
    assert r.tok[cp, 8:, t].tolist() == [cfg.pad] * 4 and r.cum[8:].tolist() == [-0.5, -1.0, -2.0, -4.0] and r.len[8:].tolist() == [2, 1, 2, 1]
    assert bool(r.touched["x"].all()) and bool(r.touched["lineage"][cp, :, t].all())


def test_e_beam_width_one_is_greedy_bit_for_bit(dev):
    B, V = 5, 65
    cfg = _cfg(V, B, max_len=6, Tmax=8)
    logits = _rand_logits(B, V, 67)
    logits[3, cfg.eos] = 9.0
    g = _setup(dev, F.SELECT_ARGMAX, cfg, logits, t=1)
    g.step(logits)
    run = BeamRun(dev, cfg, 1, SR.new_beam(cfg, 1, cfg.max_len, fill=SENT_TOK))
    run.step(logits)
    assert torch.equal(run.b["tok"][0, :, 1], g.d["seqs"][:, 1]) and torch.equal(_bits(run.b["lp"][0, :, 1]), _bits(g.d["logprobs"][:, 1]))
    assert torch.equal(_bits(run.d["x"]), _bits(g.d["x"])) and torch.equal(run.d["finished"], g.d["finished"])
    assert torch.equal(_bits(run.b["cum"]), _bits(g.d["logprobs"][:, 1]))


@pytest.mark.parametrize("E", [4, 252, 256, 260, 1024])
def test_e_beam_next_input_widths(dev, E):
    K, V = 2, 65
    cfg = _cfg(V, 2 * K, max_len=6, Tmax=8, E=E)
    r = BeamRun(dev, cfg, K, SR.new_beam(cfg, K, cfg.max_len, fill=SENT_TOK)).step(_rand_logits(2 * K, V, E, 71))
    assert bool(r.touched["x"].all())


# ---- f. refusals --------------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    S, G, P, D, Bm = F.SELECT_SLOT_ARGMAX, F.SELECT_GRAMMAR_ARGMAX, F.SELECT_PROMPT, F.SELECT_SLOT_SAMPLE, F.SELECT_BEAM
    return [
        ("form_low", F.SELECT_ARGMAX, dict(form=-1)), ("form_high", F.SELECT_ARGMAX, dict(form=10)),
        ("null_logits", F.SELECT_ARGMAX, dict(logits=None)), ("null_step", F.SELECT_ARGMAX, dict(step=None)),
        ("null_finished", F.SELECT_ARGMAX, dict(finished=None)), ("null_seqs", F.SELECT_ARGMAX, dict(seqs=None)),
        ("null_logprobs", F.SELECT_SAMPLE, dict(logprobs=None)), ("B_zero", F.SELECT_ARGMAX, dict(B=0)), ("V_zero", F.SELECT_ARGMAX, dict(V=0)),
        ("E_zero", F.SELECT_ARGMAX, dict(E=0)), ("max_len_one", F.SELECT_ARGMAX, dict(max_len=1)), ("Tmax_zero", F.SELECT_ARGMAX, dict(Tmax=0)),
        ("chained_null_emb", F.SELECT_ARGMAX, dict(emb=None)), ("chained_null_pos", F.SELECT_SAMPLE, dict(pos=None)),
        ("chained_null_x", G, dict(x=None)), ("chained_E_not_4", F.SELECT_ARGMAX, dict(E=6)),
        ("slot_unchained", S, dict(chained=False)), ("beam_unchained", Bm, dict(chained=False)),
        ("null_slots", S, dict(slots=None)), ("null_slot_t", S, dict(slots=("t", None))), ("null_slot_cap", D, dict(slots=("cap", None))),
        ("slot_rows", S, dict(slots=("rows", 3))), ("slot_max_len_above_Tmax", S, dict(Tmax=5)),
        ("null_grammar", G, dict(grammar=None)), ("null_next", G, dict(grammar=("next", None))), ("null_resync", G, dict(grammar=("resync", None))),
        ("null_state", G, dict(grammar=("state", None))), ("states_zero", G, dict(grammar=("states", 0))),
        ("states_high", G, dict(grammar=("states", 32768))), ("start_low", G, dict(grammar=("start", -1))),
        ("start_high", G, dict(grammar=("start", 2))), ("grammar_rows", G, dict(grammar=("rows", 3))),
        ("null_prompt", P, dict(prompt=None)), ("null_prompt_tok", P, dict(prompt=("tok", None))), ("null_prompt_len", P, dict(prompt=("len", None))),
        ("prompt_pitch", P, dict(prompt=("pitch", 5))), ("prompt_rows", P, dict(prompt=("rows", 3))),
        ("null_uniforms", F.SELECT_SAMPLE, dict(uniforms=None)), ("null_urow", D, dict(urow=None)), ("ld_uniforms", D, dict(ld_uniforms=5)),
        ("top_k_zero", F.SELECT_SAMPLE, dict(top_k=0)), ("top_k_65", F.SELECT_GRAMMAR_SAMPLE, dict(top_k=65)),
        ("temperature_zero", F.SELECT_SAMPLE, dict(temperature=0.0)), ("temperature_negative", D, dict(temperature=-1.0)),
        ("sampled_V_513", F.SELECT_SAMPLE, dict(V=513)),
        ("null_beam", Bm, dict(beam=None)), ("null_beam_cum", Bm, dict(beam=("cum", None))), ("null_beam_anc", Bm, dict(beam=("anc", None))),
        ("null_beam_tok", Bm, dict(beam=("tok", None))), ("null_beam_lp", Bm, dict(beam=("lp", None))), ("null_beam_len", Bm, dict(beam=("len", None))),
        ("K_zero", Bm, dict(beam=("K", 0))), ("K_17", Bm, dict(beam=("K", 17))), ("K_not_dividing_B", Bm, dict(beam=("K", 3))),
        ("beam_rows", Bm, dict(beam=("rows", 3))), ("beam_pitch", Bm, dict(beam=("pitch", 5))), ("beam_V_513", Bm, dict(V=513)),
    ]


@pytest.mark.parametrize("name,form,change", _refusal_cases(), ids=[c[0] for c in _refusal_cases()])
def test_f_refusals(dev, name, form, change):
    """Every condition the entry validates raises with the entry's name, and nothing is launched (every buffer keeps its content)."""
    B, V, T, E = 4, 16, 6, 8
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    i32 = torch.int32
    args = dict(logits=z(B, V), seqs=z(B, T, dt=torch.int64), logprobs=z(B, T), step=torch.tensor([1, 0], dtype=i32, device=dev),
                finished=z(B + 1, dt=i32))
    kw = dict(max_len=T, Tmax=T, eos=2, emb=z(V, E), pos=z(T, E), x=z(B, E), chained=True, top_k=4, temperature=1.0,
              slots=dict(t=torch.ones(B, dtype=i32, device=dev), cap=torch.full((B,), T, dtype=i32, device=dev)),
              grammar=dict(next=z(2, V, dt=torch.int16), resync=z(V, dt=torch.int16), state=z(B, dt=i32), start=0),
              prompt=dict(tok=z(B, T, dt=i32), len=z(B, dt=i32)), uniforms=z(B, T), urow=z(B, dt=i32),
              beam=dict(K=2, anc=z(2, B, T, dt=i32), tok=z(2, B, T, dt=torch.int64), lp=z(2, B, T), cum=z(B), len=z(B, dt=i32)))
    for k, v in change.items():
        if k == "form":
            form = v
        elif k in args:
            args[k] = v
        elif isinstance(v, tuple):
            kw[k] = dict(kw[k], **{v[0]: v[1]})
        else:
            kw[k] = v
    if args["logits"] is None:
        kw.update(B=B, V=V)
    with pytest.raises(RuntimeError, match=r"\): acai_debug_decode_select: "):
        ops.debug_decode_select(form, args["logits"], args["seqs"], args["logprobs"], args["step"], args["finished"], **kw)
    torch.cuda.synchronize()
    assert args["step"] is None or args["step"].tolist() == [1, 0]
    assert int(kw["x"].abs().sum()) == 0 if kw["x"] is not None else True
