"""Token automata on the CPU (acai_omr_amd/grammar.py), the float64 restatement of constrained selection (tests/grammar_reference.py) and
the well-formedness term of the token reward.  Nothing here needs a GPU."""
import io

import pytest
import torch

import grammar_reference as GR
from acai_omr_amd.grammar import TokenAutomaton

V, PAD, BOS, EOS = 12, 0, 1, 2
KW = dict(pad_idx=PAD, bos_idx=BOS, eos_idx=EOS)
CORPUS = [[BOS, EOS], [BOS, 3, 4, 5, EOS], [BOS, 3, 3, 4, EOS], [BOS, 5, 4, 3, EOS], torch.tensor([BOS, 6, 7, 6, 7, 8, EOS])]


def _table(S=3):
    nxt = torch.full((S, V), -1, dtype=torch.long)
    nxt[0, 3], nxt[0, 4], nxt[1, 5], nxt[1, EOS] = 1, 0, 0, 2
    nxt[2, EOS] = 2
    return nxt


# ---- from_transitions ---------------------------------------------------------------------------------------------------------------------
def test_from_transitions_validates():
    a = TokenAutomaton.from_transitions(_table(), 0, **KW)
    assert a.next.dtype == torch.int16 and a.resync.dtype == torch.int16 and (a.states, a.vocab_size, a.start) == (3, V, 0)
    assert a.resync.tolist() == [0, 0, 0, 1, 0] + [0] * (V - 5)   # next[start][k] where allowed, else start
    for bad, msg in ((3, "outside"), (40000, "outside")):
        t = _table()
        t[0, 5] = bad
        with pytest.raises(ValueError, match=msg):
            TokenAutomaton.from_transitions(t, 0, **KW)
    for k, msg in ((BOS, "<bos>"), (PAD, "<pad>")):
        t = _table()
        t[1, k] = 0
        with pytest.raises(ValueError, match=f"state 1 allows {msg}"):
            TokenAutomaton.from_transitions(t, 0, **KW)
    with pytest.raises(ValueError, match="start"):
        TokenAutomaton.from_transitions(_table(), 3, **KW)
    with pytest.raises(ValueError, match="resync"):
        TokenAutomaton.from_transitions(_table(), 0, torch.full((V,), 3), **KW)
    with pytest.raises(ValueError, match="resync"):
        TokenAutomaton.from_transitions(_table(), 0, torch.zeros(V - 1, dtype=torch.long), **KW)
    with pytest.raises(ValueError, match="states"):
        TokenAutomaton.from_transitions(torch.zeros(0, V, dtype=torch.long), 0, **KW)
    with pytest.raises(ValueError, match="integer table"):
        TokenAutomaton.from_transitions(torch.zeros(2, V), 0, **KW)


def test_from_transitions_dead_states():
    t = _table(4)
    t[1, 6] = 3                                   # state 3 allows nothing and is reachable through 0 -3-> 1 -6-> 3
    with pytest.raises(ValueError, match="state 3 is reachable"):
        TokenAutomaton.from_transitions(t, 0, **KW)
    a = TokenAutomaton.from_transitions(_table(4), 0, **KW)   # the same empty state, unreachable: accepted
    assert a.states == 4 and not bool((a.next[3] >= 0).any())
    with pytest.raises(ValueError, match="state 3 is reachable"):
        TokenAutomaton.from_transitions(_table(4), 3, **KW)   # the start state itself


def test_permissive():
    a = TokenAutomaton.permissive(V, **KW)
    assert a.states == 1 and a.start == 0
    assert [k for k in range(V) if a.next[0, k] < 0] == sorted([PAD, BOS])
    assert a.accepts([BOS, 5, 5, EOS]) and not a.accepts([BOS, 5, 5]) and not a.accepts([BOS, BOS, EOS])


# ---- from_corpus --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_from_corpus(order):
    a = TokenAutomaton.from_corpus(CORPUS, order, V=V, **KW)
    viol, comp = a.violations(CORPUS)
    assert viol.tolist() == [0] * len(CORPUS) and comp.tolist() == [True] * len(CORPUS)
    assert all(a.accepts(s) for s in CORPUS)
    assert a.start == 0
    end = int(a.next[a.start, EOS])               # [<bos>, <eos>] is in the corpus
    assert end >= 0 and [k for k in range(V) if a.next[end, k] >= 0] == [EOS] and int(a.next[end, EOS]) == end
    assert bool((a.next[:, EOS][a.next[:, EOS] >= 0] == end).all())
    # one unseen n-gram: one violation, and the count goes on from the token that was emitted
    if order == 1:
        seq = [BOS, 3, 5, 4, 3, EOS]              # (3, 5) is not in the corpus; (5, 4), (4, 3) and (3, <eos>) are
    else:
        seq = [BOS, 5, 4, 5, EOS]                 # (5, 4, 5) is not; resync[5] is the context (4, 5), where <eos> is allowed
    viol, comp = a.violations([seq])
    assert viol.tolist() == [1] and comp.tolist() == [True] and not a.accepts(seq)
    # an order-2 automaton tells contexts apart that the bigram automaton merges
    if order == 2:
        assert int(a.violations([[BOS, 3, 4, 3, EOS]])[0]) >= 1                # (3, 4, 3) is not in the corpus
        assert TokenAutomaton.from_corpus(CORPUS, 1, V=V, **KW).accepts([BOS, 3, 4, 3, EOS])
    # state_dict round trip, through torch.save
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    b = TokenAutomaton.from_state_dict(torch.load(buf))
    assert torch.equal(a.next, b.next) and torch.equal(a.resync, b.resync)
    assert (a.start, a.pad_idx, a.bos_idx, a.eos_idx) == (b.start, b.pad_idx, b.bos_idx, b.eos_idx)
    assert all(isinstance(v, (int, torch.Tensor)) for v in a.state_dict().values())


def test_from_corpus_numbers_contexts_in_order_of_first_appearance():
    a = TokenAutomaton.from_corpus([[BOS, 7, 3, EOS], [BOS, 3, EOS]], 1, V=V, **KW)
    # <bos> 0, (7) 1, (3) 2, end 3
    assert a.states == 4 and int(a.next[0, 7]) == 1 and int(a.next[1, 3]) == 2 and int(a.next[2, EOS]) == 3 and int(a.next[0, 3]) == 2


def test_from_corpus_rejects():
    for bad in ([[BOS, 3]], [[3, EOS]], [[BOS, PAD, EOS]], [[BOS, EOS, 3, EOS]], [[BOS, V, EOS]], []):
        with pytest.raises(ValueError):
            TokenAutomaton.from_corpus(bad, 1, V=V, **KW)
    with pytest.raises(ValueError, match="order"):
        TokenAutomaton.from_corpus(CORPUS, 3, V=V, **KW)
    big = 211   # (prime) 211 * 210 distinct bigram contexts exceed 32767 states at order 2
    seq = [BOS] + [3 + (i * j) % big for j in range(1, big) for i in range(big)] + [EOS]
    with pytest.raises(ValueError, match="32767"):
        TokenAutomaton.from_corpus([seq], 2, V=big + 3, **KW)


# ---- violations() against a plain loop ---------------------------------------------------------------------------------------------------------
def _loop(a, seqs, lens):
    out_v, out_c = [], []
    ld = seqs.shape[1]
    for r in range(seqs.shape[0]):
        n = min(max(int(lens[r]), 0), ld)
        s, v, ended = a.start, 0, False
        for p in range(1, n):
            k = int(seqs[r, p])
            if not 0 <= k < a.vocab_size:
                v, s, ended = v + 1, a.start, False
            elif int(a.next[s, k]) < 0:
                v, s, ended = v + 1, int(a.resync[k]), False
            else:
                s, ended = int(a.next[s, k]), k == EOS
        out_v.append(v)
        out_c.append(n >= 2 and ended)
    return out_v, out_c


@pytest.mark.parametrize("order", [1, 2])
def test_violations_against_a_plain_loop(order):
    a = TokenAutomaton.from_corpus(CORPUS, order, V=V, **KW)
    g = torch.Generator().manual_seed(4)
    R, ld = 40, 9
    seqs = torch.randint(2, 9, (R, ld), generator=g)
    seqs[:, 0] = BOS
    lens = torch.randint(0, ld + 1, (R,), generator=g)
    lens[:6] = torch.tensor([0, 1, 2, 2, ld, ld + 5])          # (the last is clamped to ld)
    seqs[2, 1] = EOS                                           # <bos> <eos>: complete
    seqs[3, 1] = 3                                             # length 2 without <eos>
    seqs[4] = torch.tensor([BOS, 3, 4, EOS, 3, 4, 5, EOS, 7])  # <eos> in the middle, then more
    seqs[5, 3], seqs[5, 5] = V, -1                             # ids outside [0, V)
    seqs[6, :5], lens[6] = torch.tensor([BOS, 3, 4, 5, EOS]), 5
    want_v, want_c = _loop(a, seqs, lens)
    viol, comp = a.violations(seqs, lens)
    assert viol.dtype == torch.int32 and comp.dtype == torch.bool
    assert viol.tolist() == want_v and comp.tolist() == want_c
    assert want_v[0] == want_v[1] == 0 and want_c[:4] == [False, False, True, False] and want_c[6] and want_v[6] == 0
    assert want_v[5] >= 2 and want_v[4] >= 1
    # a bool prefix mask in place of the lengths
    mask = torch.arange(ld).unsqueeze(0) < lens.clamp(max=ld).unsqueeze(1)
    v2, c2 = a.violations(seqs, mask)
    assert torch.equal(v2, viol) and torch.equal(c2, comp)


# ---- the restatement of constrained selection ---------------------------------------------------------------------------------------------------
def _unmasked_greedy(lg):
    m = lg.max()
    tok = int((lg == m).nonzero()[0])
    return tok, float(torch.log_softmax(lg, 0)[tok])


def _unmasked_sample(lg, u, top_k, temperature):
    """The sampler's rule as the sampled decode tests restate it: stable descending sort, top_k, inverse CDF, log_softmax(kept)."""
    val, idx = torch.sort(lg, descending=True, stable=True)
    k = min(top_k, lg.numel())
    p = torch.exp((val[:k] - val[0]) / temperature)
    hit = (torch.cumsum(p, 0) / p.sum() > u).nonzero()
    r = int(hit[0]) if hit.numel() else k - 1
    return int(idx[r]), float(torch.log_softmax(val[:k], 0)[r])


def _logits_fn(seed, B, bias_off=(PAD, BOS)):
    """Deterministic float64 logits that depend on the previous token and the index; <pad> and <bos> far below everything else."""
    def fn(prev, t):
        g = torch.Generator().manual_seed(seed * 1000 + t)
        lg = torch.randn(B, V, generator=g, dtype=torch.float64) + 0.3 * prev.double().unsqueeze(1)
        lg[:, list(bias_off)] -= 50.0
        lg[:, 5] = lg[:, 6]                                   # a tie: the lower index wins
        return lg
    return fn


def test_restatement_with_the_permissive_automaton_is_the_unmasked_rule():
    B, T = 3, 10
    U = torch.rand(B, T, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for a in (TokenAutomaton.permissive(V, **KW), TokenAutomaton.from_transitions(GR.bigram_permissive(V, PAD, BOS, EOS), BOS, **KW)):
        fn = _logits_fn(3, B)
        seqs, lps, _ = GR.constrained_greedy(fn, a, B, T, BOS)
        for t in range(1, T):
            lg = fn(seqs[:, t - 1], t)
            for b in range(B):
                tok, lp = _unmasked_greedy(lg[b])
                assert int(seqs[b, t]) == tok and abs(float(lps[b, t]) - lp) < 1e-12
        for top_k in (1, 5, 50):
            seqs, lps, _ = GR.constrained_sample(fn, a, B, T, BOS, U, top_k, 1.1)
            for t in range(1, T):
                lg = fn(seqs[:, t - 1], t)
                for b in range(B):
                    tok, lp = _unmasked_sample(lg[b], float(U[b, t]), min(top_k, V), 1.1)
                    # (<pad> / <bos> sit 50 below: inside the top 50 of 12 tokens their mass is exp(-50), never drawn)
                    assert int(seqs[b, t]) == tok and abs(float(lps[b, t]) - lp) < 1e-9, (top_k, b, t)


def test_restatement_masks_draws_and_falls_back():
    nxt = torch.full((4, V), -1, dtype=torch.long)
    nxt[0, 7] = 1                     # one allowed token
    nxt[1, [3, 4, 5]] = 2             # three allowed tokens
    nxt[2, EOS] = 2                   # only <eos>
    a = TokenAutomaton.from_transitions(nxt, 0, torch.full((V,), 2), **KW)   # state 3 is dead and unreachable
    lg = torch.linspace(-1, 1, V, dtype=torch.float64)
    for u in (0.0, 0.5, 0.999999):
        assert GR.select_sample(lg, 0, a, u, 50, 1.1) == (7, 0.0, 1)
    assert GR.select_greedy(lg, 0, a) == (7, 0.0, 1)
    kept = torch.log_softmax(lg[[5, 4, 3]], 0)
    p = torch.softmax(lg[[5, 4, 3]] / 1.1, 0).cumsum(0)
    for u, r in ((0.0, 0), (float(p[0]) + 1e-9, 1), (float(p[1]) + 1e-9, 2), (0.999999999, 2)):
        tok, lp, s = GR.select_sample(lg, 1, a, u, 50, 1.1)
        assert (tok, s) == ([5, 4, 3][r], 2) and abs(lp - float(kept[r])) < 1e-12
    tok, lp, s = GR.select_greedy(lg, 1, a)
    assert (tok, s) == (5, 2) and abs(lp - float(kept[0])) < 1e-12
    assert GR.select_greedy(lg, 2, a)[::2] == (EOS, 2)
    # the dead state: unconstrained, next state resync[token]; states outside [0, S) are clamped
    for s in (3, 99):
        assert GR.select_greedy(lg, s, a) == _unmasked_greedy(lg) + (2,)
        assert GR.select_sample(lg, s, a, 0.3, 4, 1.1)[:2] == pytest.approx(_unmasked_sample(lg, 0.3, 4, 1.1))
    assert GR.select_greedy(lg, -5, a) == (7, 0.0, 1)
    seqs, _, states = GR.constrained_greedy(lambda prev, t: lg.repeat(2, 1), a, 2, 5, BOS)
    assert seqs.tolist() == [[BOS, 7, 5, EOS, EOS]] * 2 and states[0].tolist() == [0, 0, 1, 2, 2]
    assert a.violations(seqs[:, :4])[0].tolist() == [0, 0]


# ---- the reward ------------------------------------------------------------------------------------------------------------------------------
def test_token_reward_wellformedness(monkeypatch):
    from acai_omr_amd.train import grpo as G
    monkeypatch.setattr(G, "calc_token_edit_costs", lambda rollouts, mask, tgt, pad, group_size=1: torch.zeros(rollouts.shape[0]))
    a = TokenAutomaton.from_corpus(CORPUS, 1, V=V, **KW)
    rollouts = torch.tensor([[BOS, 3, 4, 5, EOS, PAD], [BOS, 3, 5, 5, 3, EOS], [BOS, 3, 4, 5, 5, 5], [BOS, EOS, PAD, PAD, PAD, PAD]])
    mask = torch.tensor([[1, 1, 1, 1, 1, 0], [1] * 6, [1] * 6, [1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    targets = torch.tensor([[BOS, 3, 4, 5, EOS]] * 4)
    cfg = G.RewardConfig(lambda_tedn=7, lambda_well_formed=1.5, lambda_f1=2.5, lambda_repeat=2, lambda_len=2, alpha_tedn=0.01,
                         alpha_well_formed=0.25, gamma=3, delta=5, tau=50)
    batch = [None, None]
    viol, comp = a.violations(rollouts, mask)
    assert viol.tolist() == [0, 3, 2, 0] and comp.tolist() == [True, True, False, True]
    want = torch.exp(-0.25 * viol.float()).masked_fill(~comp, -3.0)
    rewards, comps = G.make_token_reward_fn(cfg, PAD, grammar=a)(rollouts, mask, targets, batch)
    assert torch.equal(comps.wellformedness_scores, want)
    assert torch.equal(comps.wellformedness_scores, G.calc_wellformedness(~comp, viol.float(), 3, 0.25))
    plain_rewards, plain = G.make_token_reward_fn(cfg, PAD)(rollouts, mask, targets, batch)
    assert torch.equal(plain.wellformedness_scores, torch.zeros(4))
    assert rewards.shape == (2, 2) and torch.allclose(rewards - plain_rewards, (1.5 * want).view(2, 2))
    for x, y in zip(comps._vals(), plain._vals()):
        if x is not comps.wellformedness_scores:
            assert torch.equal(x, y)
