"""tests/select_reference.py (one selection step as a float64 state transition, one beam step) against independent statements: the chained
references of grammar_reference / prompt_reference, the greedy step, full enumeration, and the static step row by row.  No GPU."""
import itertools
import math

import pytest
import torch

import grammar_reference as GR
import prompt_reference as PR
import select_reference as SR

V, B, T, E = 11, 5, 9, 8
PAD, BOS, EOS = 1, 0, 2


def _cfg(V=V, B=B, T=T, Tmax=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    Tmax = Tmax or T
    return SR.Cfg(V=V, B=B, max_len=T, Tmax=Tmax, eos=EOS, bos=BOS, pad=PAD, emb=torch.randn(V, E, generator=g), pos=torch.randn(Tmax, E, generator=g))


def _logit_table(V=V, T=T, rows=B, seed=1, scale=3.0):
    """logits of index t for row b after token k: a fixed table [T][rows][V][V]."""
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(T, rows, V, V, generator=g, dtype=torch.float64)


def _table(seed=2):
    """A restrictive table with a dead state (3, reached through token 5) that grammar_reference leaves through resync."""
    g = torch.Generator().manual_seed(seed)
    nxt = torch.randint(0, 4, (4, V), generator=g)
    nxt[torch.rand(4, V, generator=g) < 0.4] = -1
    nxt[:, EOS] = 0
    nxt[0, 5] = 3
    nxt[3] = -1
    return SR.Table(nxt, start=0, resync=torch.randint(0, 3, (V,), generator=g))


def _chain(cfg, tab, steps, **kw):
    st, out = SR.new_state(cfg, gstate=[kw["table"].start] * cfg.B if kw.get("table") is not None else None), []
    st.seqs[:, 0] = cfg.bos
    for _ in range(steps):
        t = st.step[0]
        lg = torch.stack([tab[t, b, int(st.seqs[b, t - 1])] for b in range(cfg.B)])
        st = SR.step(st, lg, cfg, **kw)
        out.append(st)
    return out


def _fn(tab):
    return lambda prev, t: torch.stack([tab[t, b, int(prev[b])] for b in range(len(prev))])


def test_chained_grammar_greedy_is_constrained_greedy():
    cfg, tab, a = _cfg(), _logit_table(), _table()
    st = _chain(cfg, tab, T - 1, table=a)[-1]
    seqs, lps, states = GR.constrained_greedy(_fn(tab), a, B, T, BOS)
    assert torch.equal(st.seqs, seqs) and torch.equal(st.logprobs, lps)
    assert int((states == 3).sum()) > 0, "the dead state must be visited"
    assert st.step == [T, T - 1]


def test_chained_grammar_sample_is_constrained_sample():
    cfg, tab, a = _cfg(), _logit_table(seed=3), _table()
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(4))
    hist = _chain(cfg, tab, T - 1, table=a, draw=dict(uniforms=u, top_k=3, temperature=0.7))
    seqs, lps, _ = GR.constrained_sample(_fn(tab), a, B, T, BOS, u, 3, 0.7)
    assert torch.equal(hist[-1].seqs, seqs) and torch.equal(hist[-1].logprobs, lps)
    assert all(m is not None and 0 <= m <= 1 for s in hist for m in s.margins)
    # and the plain sampled form is the constrained one under a table that allows everything
    hist = _chain(cfg, tab, T - 1, draw=dict(uniforms=u, top_k=3, temperature=0.7))
    seqs, lps, _ = GR.constrained_sample(_fn(tab), SR.allow_all(V), B, T, BOS, u, 3, 0.7)
    assert torch.equal(hist[-1].seqs, seqs) and torch.equal(hist[-1].logprobs, lps)


def test_chained_prompt_step_is_batch_decode():
    cfg, tab = _cfg(), _logit_table(seed=5)
    prompts = [[], [4], [5, 6, EOS], [7, 3, 4, 5, 6, 7, 8, 9], [3, 4]]
    tok = torch.full((B, T), -7, dtype=torch.int64)
    for b, p in enumerate(prompts):
        tok[b, 1:len(p) + 1] = torch.tensor(p, dtype=torch.int64)
    pr = dict(tok=tok, len=torch.tensor([len(p) for p in prompts]))
    hist = _chain(cfg, tab, T - 1, prompt=pr)
    rows, counts = PR.batch_decode(lambda i, seq: tab[len(seq), i, seq[-1]].tolist(), BOS, EOS, T, prompts)
    n = len(counts)
    assert [int(s.finished[B]) for s in hist[:n]] == counts
    for b, (seq, lps) in enumerate(rows):
        assert hist[n - 1].seqs[b, :n + 1].tolist() == seq
        assert hist[n - 1].logprobs[b, :n + 1].tolist() == pytest.approx(lps, abs=1e-12)
    # the clamp: a length above max_len - 1 forces indices 1 .. max_len - 1 only; a negative one forces nothing
    assert SR.prompt_of(dict(tok=tok, len=torch.tensor([99, -3, 0, 0, 0])), 0, cfg) == tok[0, 1:].tolist()
    assert SR.prompt_of(dict(tok=tok, len=torch.tensor([99, -3, 0, 0, 0])), 1, cfg) == []


def test_static_bookkeeping():
    cfg = _cfg(Tmax=T)
    st = SR.new_state(cfg, t=T - 1, cache=4, finished=[0, 1, 0, 0, 0], fill=-5)
    lg = torch.zeros(B, V, dtype=torch.float64)
    lg[0, EOS] = lg[1, 4] = lg[2, 5] = lg[3, 6] = lg[4, 7] = 1.0
    n = SR.step(st, lg, cfg)
    assert n.seqs[:, T - 1].tolist() == [EOS, 4, 5, 6, 7] and n.finished.tolist() == [1, 1, 0, 0, 0, 3] and n.step == [T, 5]
    assert not bool(n.touched["x"].any()) and bool((n.x == -5).all()), "no next input at t + 1 == Tmax"
    assert int(n.touched["seqs"].sum()) == B and bool((n.seqs[:, :T - 1] == -5).all())
    n = SR.step(SR.new_state(cfg, t=2, fill=-5), lg, cfg)
    assert torch.equal(n.x, cfg.emb[n.seqs[:, 2]] + cfg.pos[3]) and bool(n.touched["x"].all())
    assert not bool(SR.step(SR.new_state(cfg, t=2, fill=-5), lg, cfg, chained=False).touched["x"].any())


def test_beam_width_one_is_the_greedy_step():
    cfg, tab = _cfg(Tmax=T + 1), _logit_table(seed=6)
    g = SR.new_state(cfg)
    g.seqs[:, 0] = BOS
    bm = SR.new_beam(cfg, 1, T)
    for _ in range(T - 1):
        t = g.step[0]
        lg = torch.stack([tab[t, b, int(g.seqs[b, t - 1])] for b in range(B)])
        g, bm = SR.step(g, lg, cfg), SR.beam_step(bm, lg, cfg, 1)
        cp = (t + 1) & 1
        assert bm.tok[cp, :, :t + 1].tolist() == g.seqs[:, :t + 1].tolist()
        live = bm.tok[cp, :, 1:t + 1] != PAD   # a finished beam row is extended by <pad> with log-prob 0; greedy goes on emitting
        assert float((bm.lp[cp, :, 1:t + 1][live] - g.logprobs[:, 1:t + 1][live]).abs().max()) < 1e-12
        done = (g.seqs[:, 1:t + 1] == EOS).any(1)
        if not bool(done.any()):
            assert torch.equal(bm.x, g.x) and bm.finished.tolist() == g.finished.tolist()
        if bool(done.any()):
            break
    assert bm.step == g.step


@pytest.mark.parametrize("Vs,steps,K", [(3, 2, 9), (2, 4, 16), (3, 2, 12)])
def test_beam_wide_enough_is_full_enumeration(Vs, steps, K):
    """With K at least the number of hypotheses nothing is pruned: the slots are ALL hypotheses sorted by score."""
    eos, pad = 1, 0
    cfg = SR.Cfg(V=Vs, B=K, max_len=steps + 1, Tmax=steps + 2, eos=eos, bos=0, pad=pad, emb=torch.zeros(Vs, 4), pos=torch.zeros(steps + 2, 4))
    g = torch.Generator().manual_seed(Vs * 100 + steps)
    lg_of = {}

    def logits_of(prefix):
        if prefix not in lg_of:
            lg_of[prefix] = 2.0 * torch.randn(Vs, generator=g, dtype=torch.float64)
        return lg_of[prefix]

    bm = SR.new_beam(cfg, K, steps + 1)
    for t in range(1, steps + 1):
        rows = [tuple(bm.tok[t & 1, r, :t].tolist()) for r in range(K)]
        bm = SR.beam_step(bm, torch.stack([logits_of(p) for p in rows]), cfg, K)
    hyps = []   # (score, tokens after <bos>, length or 0)
    for n in range(1, steps + 1):
        for toks in itertools.product(range(Vs), repeat=n):
            if eos in toks[:-1] or (n < steps and toks[-1] != eos):
                continue
            sc, pre = 0.0, (0,)
            for k in toks:
                sc += float(torch.log_softmax(logits_of(pre), 0)[k])
                pre += (k,)
            hyps.append((sc, toks, n if toks[-1] == eos else 0))
    hyps.sort(key=lambda h: -h[0])
    assert len(hyps) <= K
    cp = (steps + 1) & 1
    for j, (sc, toks, ln) in enumerate(hyps):
        assert float(bm.cum[j]) == pytest.approx(sc, abs=1e-12)
        assert bm.tok[cp, j, 1:len(toks) + 1].tolist() == list(toks) and bool((bm.tok[cp, j, len(toks) + 1:] == pad).all())
        assert int(bm.len[j]) == ln and int(bm.finished[j]) == (1 if ln else 0)
    for j in range(len(hyps), K):
        assert float(bm.cum[j]) == -math.inf and int(bm.finished[j]) == 1
    assert int(bm.finished[K]) == sum(1 for h in hyps if h[2] == 0)


def test_beam_ties_and_dead_slots():
    cfg = _cfg(V=3, B=5, T=4, Tmax=6)
    bm = SR.new_beam(cfg, 5, 4)
    lg = torch.zeros(5, 3, dtype=torch.float64)   # exact ties within the row: the lower token first
    n = SR.beam_step(bm, lg, cfg, 5)
    assert n.tok[0, :, 1].tolist() == [0, 1, EOS, PAD, PAD] and n.anc[0, :, 0].tolist() == [0, 0, 0, 3, 4]
    assert n.cum[3:].tolist() == [-math.inf] * 2 and n.finished.tolist() == [0, 0, 1, 1, 1, 2] and n.len.tolist() == [0, 0, 1, 0, 0]
    assert n.margin == 0.0 and bool((n.tok[1] == bm.tok[1]).all())
    # exact ties across parents: the lower parent slot first; a finished parent is one candidate that outranks live extensions
    n.cum[:3] = torch.tensor([-1.0, -1.0, -1.5])
    m = SR.beam_step(n, lg, cfg, 5)
    assert m.anc[1, :, 1].tolist() == [2, 0, 0, 0, 1] and m.tok[1, :, 2].tolist() == [PAD, 0, 1, EOS, 0]
    assert m.len.tolist() == [1, 0, 0, 2, 0] and m.cum[0] == -1.5 and m.finished.tolist() == [1, 0, 0, 1, 0, 3]


def test_slot_step_gives_each_row_its_static_tokens():
    """Rows armed at different times with different caps: row b's tokens are the static step's, up to <eos> or cap - 1."""
    cfg, tab = _cfg(Tmax=T), _logit_table(seed=8)
    a = _table()
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(9))
    urow = torch.tensor([3, 0, 4, 1, 2])
    for kw, skw in ((dict(), dict()), (dict(table=a), dict(table=a)),
                    (dict(draw=dict(uniforms=u, top_k=4, temperature=1.3, urow=urow)), dict(draw=dict(uniforms=u[urow], top_k=4, temperature=1.3)))):
        static = _chain(cfg, tab, T - 1, **skw)[-1]
        caps = [2, T, 5, 3, T]
        arm_at = [0, 0, 2, 4, 1]   # the slot step at which row b starts
        st = SR.new_state(cfg, t=-9, cache=T - 3, slot_t=[1] * B, slot_cap=caps, finished=[1] * B, gstate=[a.start] * B if "table" in kw else None)
        st.seqs[:, 0] = BOS
        ring = []
        for s in range(2 * T):
            for b in range(B):
                if arm_at[b] == s:
                    st.finished[b] = 0
            lg = torch.stack([tab[int(st.slot_t[b]), b, int(st.seqs[b, int(st.slot_t[b]) - 1])] for b in range(B)])
            before = st
            st = SR.step(st, lg, cfg, slot=True, **kw)
            ring.append(st.step[1])
            for b in range(B):
                if int(before.finished[b]):
                    assert not bool(st.touched["seqs"][b].any()) and not bool(st.touched["x"][b])
            assert int(st.finished[B]) == int((st.finished[:B] == 0).sum()) and st.step[0] == -9
        assert ring[:4] == [T - 2, T - 1, 0, 1], "the ring index wraps at Tmax"
        assert bool(st.finished[:B].all())
        for b in range(B):
            row = static.seqs[b, 1:caps[b]].tolist()
            n = 1 + (row.index(EOS) + 1 if EOS in row else len(row))
            assert int(st.slot_t[b]) == n - 1
            assert st.seqs[b, :n].tolist() == static.seqs[b, :n].tolist() and torch.equal(st.logprobs[b, :n], static.logprobs[b, :n])
            assert bool((st.seqs[b, n:] == 0).all())


def test_draw_margin():
    lg = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.125], dtype=torch.float64))
    assert SR.draw_margin(lg, None, 0.6, 4, 1.0) == pytest.approx(0.1)
    assert SR.draw_margin(lg, None, 0.5, 4, 1.0) == pytest.approx(0.0, abs=1e-15)
    assert SR.draw_margin(lg, torch.tensor([False, True, True, True]), 0.25, 2, 1.0) == pytest.approx(2 / 3 - 0.25)
    idx, cdf, _ = SR.kept_cdf(torch.tensor([1.0, 3.0, 3.0, 2.0]), None, 3, 1.0)
    assert idx.tolist() == [1, 2, 3]
