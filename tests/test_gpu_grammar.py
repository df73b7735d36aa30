"""Grammar-constrained decoding and the grammar scan on the GPU (acai_decode_grammar_step and its sampled / slot forms through
DecodeEngine.greedy / sample / continuous(grammar=), the model and inference entry points, acai_grammar_scan through ops.grammar_scan, and
the GRPO well-formedness term).

Shapes (tests/test_gpu_prompt.py's): the golden fixtures vitomr_small, vitomr_dh64b, vitomr_odd (three images each, the generic GEMV path)
and the random decoder decode_support._decoder(T=48, L=2, E=1024, H=16, Fd=4096) on memories of 40, 17 and 64 rows (the chain-GEMV /
fused-LayerNorm path), whose <eos> logit is biased so that one greedy row ends before max_len; fp32 and bf16.

The restrictive automaton of a case is cut out of the bigram-permissive table (S = V, the state is the last token) with the case's own plain
greedy result: the greedy path's bigram (seq[t-1], seq[t]) is forbidden at t in {1, 2, L // 2, L - 1} of every row, and for one row that
ended in <eos> the <eos> is forbidden where greedy emitted it.  Every state keeps more than 200 allowed tokens; the greedy result has at
least 3 violations per row under it (asserted on the CPU, before the GPU run).

Bars:
  1. automata that allow every token in every state (one state; bigram, S = 227): constrained greedy / sampling torch.equal to plain
     greedy / sampling (top_k 1 and 50, temperature 1.1), also for a group-of-3 rollout.  These tables come from the plain constructor:
     the builders refuse a table that allows <bos> or <pad>, and under TokenAutomaton.permissive the log-probs are renormalised over the
     other 225 tokens (measured on the MI355X: up to 0.0156 above the plain ones on vitomr_dh64b in bf16, 0.0049 in fp32, 0.078 on the
     random decoder), so they
     cannot be bitwise the plain ones; for those the tokens and the mask are torch.equal and the log-probs are not below the plain ones;
  2. the restrictive automaton against the host-stepped path (cached_set_up_inference + one decoder.cached_generate per token) with the
     float64 restatement (tests/grammar_reference.py) applied to its logits: tokens equal; log-probs fp32 within 1e-5 * max(1, |lp|), bf16
     equal to the float64 value rounded to bf16 or its bf16 neighbour; the output differs from greedy's, has no violation and every <eos>
     is an allowed one;
  3. narrow states (one token; three tokens under top_k 50; only <eos>) and a dead state reached through the C ABI;
  4. S = 32767 (a chain automaton started 30 states before its end, 40 steps): equal to the restatement;
  5. slot modes, greedy and sampled: 7 images through 3 slots, each as in a constrained static batch alone; an idle slot's poisoned state
     stays untouched;
  6. graph replay == eager launches; a grammar run leaves the other modes as on a fresh engine; a second, larger automaton gets its own
     result; inference(grammar=) == streamed_inference(grammar=); FP8 memory cache;
  7. the scan kernel against TokenAutomaton.violations, LDS path and global path;
  8. the C ABI's argument checks;
  9. one grpo_update with constrained rollouts and the automaton's well-formedness term;
 10. every selection form (greedy / sampled x static / slot x plain / grammar, prompted greedy) at 18 rows - more than the 16 waves of the
     workgroup that closes a greedy step, five sampling workgroups - on a one-layer decoder, against the restatements, bar 2's bounds."""
import ctypes
import math

import pytest
import torch
from torch.amp import autocast

import grammar_reference as GR
from conftest import VOCAB, load_golden
from decode_support import _decoder, _memory, _models, _same, _vit, _vocab, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURES = ["vitomr_small", "vitomr_dh64b", "vitomr_odd"]
CASES = FIXTURES + ["random"]
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]
RAND_T, RAND_LENS = 48, [40, 17, 64]
TEMPERATURE = 1.1
_CACHE = {}


def _ctx(bf):
    return autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf)


def _TA():
    from acai_omr_amd.grammar import TokenAutomaton
    return TokenAutomaton


def _ids(m):
    dec = m.decoder
    return dict(pad_idx=dec.pad_idx, bos_idx=dec.bos_idx, eos_idx=dec.eos_idx)


def _host_logits(m, lat, mask, T):
    """The host-stepped path as a grammar_reference logits_fn: (tokens of index t - 1, t) -> float64 logits of index t on the CPU.  The
    calls must come in order t = 1, 2, ... (each one appends to the KV cache)."""
    m.cached_set_up_inference(lat, T)
    return lambda prev, t: m.decoder.cached_generate(prev.to(lat.device).unsqueeze(1), t, mask).squeeze(1).double().cpu()


def _case(name, cdt, dev):
    """(model, memory (B, S, E), padding mask, max_len) of a test shape, built once per (shape, dtype)."""
    key = (name, cdt)
    if key in _CACHE:
        return _CACHE[key]
    bf = cdt == torch.bfloat16
    if name != "random":
        fx = load_golden(name)
        m = build_vitomr(fx["cfg"], fx["state_dict"], dev, cdt, max_batch=24)
        lat, mask = _memory(m, fx["imgs"], bf)
        out = (m, lat, mask, fx["cfg"]["gen_len"])
    else:
        dec = _decoder(T=RAND_T, L=2, E=1024, H=16, Fd=4096)
        g = torch.Generator().manual_seed(21)
        lat = torch.zeros(len(RAND_LENS), max(RAND_LENS), 1024)
        mask = torch.ones(len(RAND_LENS), max(RAND_LENS), dtype=torch.bool)
        for i, n in enumerate(RAND_LENS):
            lat[i, :n] = torch.randn(n, 1024, generator=g).to(torch.bfloat16).float()
            mask[i, :n] = False
        lat, mask = lat.to(dev), mask.to(dev)
        # bias the <eos> logit half way between the two smallest per-row minima of (max logit - <eos> logit) along the unbiased greedy path:
        # exactly one row's greedy run then ends before max_len (tests/test_gpu_prompt.py)
        m0 = _vit(dec, 24, cdt, dev)
        gap = torch.zeros(len(RAND_LENS), RAND_T, dtype=torch.float64)
        with torch.no_grad(), _ctx(bf):
            fn = _host_logits(m0, lat, mask, RAND_T)
            prev = torch.full((len(RAND_LENS),), dec.bos_idx, dtype=torch.int64)
            for t in range(1, RAND_T):
                lg = fn(prev, t)
                prev = torch.argmax(lg, dim=-1)
                gap[:, t] = lg.max(dim=-1).values - lg[:, dec.eos_idx]
        lo = gap[:, 1:RAND_T - 1].min(dim=1).values.sort().values
        with torch.no_grad():
            dec.unembed.bias[dec.eos_idx] += float(lo[0] + lo[1]) / 2
        out = (_vit(dec, 24, cdt, dev), lat, mask, RAND_T)
    _CACHE[key] = out
    return out


def _greedy(m, lat, mask, T, bf, **kw):
    with torch.no_grad(), _ctx(bf):
        return m.cached_greedy_generate(lat, mask, max_len=T, **kw)


def _sample(m, lat, mask, T, bf, U, top_k, G=1, **kw):
    """DecodeEngine.sample on the memories (each serving G rows), masked and clipped as the entry points return it."""
    from acai_omr_amd import engine as EG
    blocks = m.decoder.decoder_blocks
    with torch.no_grad(), _ctx(bf):
        mem32, lens = EG.unpad_rows(lat, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=G)
        s, lp, _ = blocks.engine(lat.device).sample(T, top_k, TEMPERATURE, uniforms=U, **kw)
        return m.mask_and_clip_seqs(s.clone(), lp.clone())


def _permissive(m, bigram, builders=False):
    """An automaton that allows EVERY token in every state - one state, or S = V with the last token as the state.  The builders refuse a
    table that allows <bos> or <pad>, so these come from the plain constructor.  builders=True: what TokenAutomaton.permissive /
    from_transitions give instead, every token but <bos> and <pad>."""
    ids = _ids(m)
    V = m.decoder.vocab_size
    if builders:
        if not bigram:
            return _TA().permissive(V, **ids)
        return _TA().from_transitions(GR.bigram_permissive(V, ids["pad_idx"], ids["bos_idx"], ids["eos_idx"]), ids["bos_idx"], **ids)
    if not bigram:
        return _TA()(torch.zeros(1, V, dtype=torch.int16), 0, torch.zeros(V, dtype=torch.int16), **ids)
    return _TA()(torch.arange(V, dtype=torch.int16).repeat(V, 1).contiguous(), ids["bos_idx"], torch.arange(V, dtype=torch.int16), **ids)


def _bigram_resync(V, ids):
    rs = torch.arange(V)
    rs[ids["bos_idx"]] = rs[ids["pad_idx"]] = ids["bos_idx"]
    return rs


def _restrictive(m, g, extra=()):
    """The case's restrictive automaton from its plain greedy result g (module docstring); extra: more (state, token) pairs to forbid."""
    ids = _ids(m)
    V, bos, eos = m.decoder.vocab_size, ids["bos_idx"], ids["eos_idx"]
    nxt = GR.bigram_permissive(V, ids["pad_idx"], bos, eos)
    seqs, _, mk = (x.cpu() for x in g)
    Ls = (mk.sum(dim=1) - 1).tolist()
    for i, L in enumerate(Ls):
        for t in {1, 2, L // 2, L - 1}:
            if 1 <= t <= L:
                nxt[int(seqs[i, t - 1]), int(seqs[i, t])] = -1
    ended = [i for i, L in enumerate(Ls) if int(seqs[i, L]) == eos]
    if ended:
        i = ended[0]
        nxt[int(seqs[i, Ls[i] - 1]), eos] = -1
    for s, k in extra:
        nxt[s, k] = -1
    assert int((nxt >= 0).sum(dim=1).min()) > 200
    a = _TA().from_transitions(nxt, bos, _bigram_resync(V, ids), **ids)
    viol, _ = a.violations(seqs, mk)
    assert int(viol.min()) >= 3, (viol.tolist(), Ls)   # on the CPU, before the GPU run: the constraint binds on every row
    return a, bool(ended)


def _check_lps(got, want, live, bf):
    """The log-prob bars of tests/test_gpu_prompt.py bar 2 on the positions `live`."""
    want, got = want[live], got.cpu()[live]
    if bf:
        assert torch.equal(got, got.to(torch.bfloat16).float())                    # rounded where the greedy step rounds
        wb = want.to(torch.bfloat16)
        ulps = (got.to(torch.bfloat16).view(torch.int16).int() - wb.view(torch.int16).int()).abs()
        bad = (ulps > 1) & (got != wb.float())
        print(f"bf16: {int((ulps == 1).sum())} of {ulps.numel()} log-probs are the bf16 neighbour of the rounded float64 value")
        assert not bool(bad.any()), (got[bad], want[bad])
    else:
        err = (got.double() - want).abs() / want.abs().clamp(min=1.0)
        print(f"fp32: max |lp - float64| / max(1, |lp|) = {float(err.max()):.3g}")
        assert float(err.max()) <= 1e-5


def _check_against_restatement(m, lat, mask, T, bf, a, out, tokens_only=False, pick=None):
    """out = the entry point's (seqs, lps, mask) against the restatement on the host-stepped logits.  -> the restatement's (seqs, lps)."""
    B = lat.shape[0]
    with torch.no_grad(), _ctx(bf):
        fn = _host_logits(m, lat, mask, T)
        rs, rlp, _ = (pick or GR.constrained_greedy)(fn, a, B, T, m.decoder.bos_idx)
    rmask = m.create_inference_mask(rs)
    n = int(rmask.sum(dim=-1).max())
    seqs, lps, mk = (x.cpu() for x in out)
    assert seqs.shape[1] == n and torch.equal(mk, rmask[:, :n])
    assert torch.equal(seqs, rs.masked_fill(~rmask, m.decoder.pad_idx)[:, :n])
    if not tokens_only:
        live = rmask[:, :n].clone()
        live[:, 0] = False
        _check_lps(lps, rlp[:, :n], live, bf)
        assert bool((lps[~mk] == 0).all())
    return rs, rlp


# ---- 1. permissive automata -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_permissive_automaton_is_unconstrained_decoding(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    g = _greedy(m, lat, mask, T, bf)
    U = torch.rand(lat.shape[0], T, generator=torch.Generator().manual_seed(7)).to(dev)
    plain = {k: _sample(m, lat, mask, T, bf, U, k) for k in (1, 50)}
    for bigram in (False, True):
        a = _permissive(m, bigram)
        assert a.states == (227 if bigram else 1)
        c = _greedy(m, lat, mask, T, bf, grammar=a)
        assert torch.equal(c[0], g[0]) and torch.equal(c[2], g[2]), (name, bigram)
        assert torch.equal(c[1], g[1]), (name, bigram, float((c[1] - g[1]).abs().max()))
        for k in (1, 50):
            _same(plain[k], _sample(m, lat, mask, T, bf, U, k, grammar=a))
        # the builders' permissive automata leave <bos> and <pad> out: the same tokens (the model never prefers those two), and log-probs
        # renormalised over the rest - never below the plain ones, up to the rounding of the format
        b = _permissive(m, bigram, builders=True)
        c = _greedy(m, lat, mask, T, bf, grammar=b)
        assert torch.equal(c[0], g[0]) and torch.equal(c[2], g[2]), (name, bigram)
        slack = (2.0 ** -7 if bf else 1e-5) * g[1].abs().clamp(min=1.0)
        assert bool((c[1] >= g[1] - slack).all()), (name, bigram, float((g[1] - c[1]).max()))
        print(f"{name} {'bf16' if bf else 'fp32'} S={b.states}: log-probs without <bos> / <pad> exceed the plain ones by up to {float((c[1] - g[1]).max()):.3g}")
    _same(g, _greedy(m, lat, mask, T, bf))   # and plain greedy after the grammar runs


def test_permissive_automaton_group_of_three_rollouts(dev):
    fx, old, _, G, cfg = _models(dev)
    T = cfg["max_len"] - 2
    lat, mask = _memory(old, fx["imgs"], True)
    U = torch.rand(lat.shape[0] * G, T, generator=torch.Generator().manual_seed(8)).to(dev)
    xl, xm = old.expand_img_latent_for_rollout(lat, mask, G)
    for k in (1, 50):
        with torch.no_grad(), _ctx(True):
            plain = old.cached_forward_rollout_policy(xl, xm, T, k, TEMPERATURE, group_size=G, uniforms=U)
            for bigram in (False, True):
                _same(plain, old.cached_forward_rollout_policy(xl, xm, T, k, TEMPERATURE, group_size=G, uniforms=U, grammar=_permissive(old, bigram)))


# ---- 2. the restrictive automaton against the host-stepped path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_restrictive_automaton_against_host_stepped_restatement(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    g = _greedy(m, lat, mask, T, bf)
    a, ended = _restrictive(m, g)
    if name == "random":
        assert ended                           # the row the <eos> bias ends: its <eos> is forbidden where greedy emitted it
    out = _greedy(m, lat, mask, T, bf, grammar=a)
    _check_against_restatement(m, lat, mask, T, bf, a, out)
    seqs, _, mk = (x.cpu() for x in out)
    n = min(seqs.shape[1], g[0].shape[1])
    assert seqs.shape != g[0].shape or not torch.equal(seqs, g[0].cpu())
    assert all(not torch.equal(seqs[i, :n], g[0][i, :n].cpu()) for i in range(seqs.shape[0]))   # every row was diverted
    viol, comp = a.violations(seqs, mk)
    assert viol.tolist() == [0] * seqs.shape[0]
    has_eos = (seqs == m.decoder.eos_idx).any(dim=1)
    assert torch.equal(comp, has_eos)          # every <eos> sits in a state that allows it
    dv, dc = _scan(seqs.to(dev), mk.to(dev), a)
    assert torch.equal(dv.cpu(), viol) and torch.equal(dc.cpu(), comp)


def _scan(rollouts, mask, a):
    from acai_omr_amd import ops
    return ops.grammar_scan(rollouts, mask, a)


# ---- 3. narrow states ------------------------------------------------------------------------------------------------------------------------
def _narrow(m):
    """0 -A-> 1 -{B1, B2, B3}-> 2 -(anything but <eos>)-> 3 -<eos>-> 4 -<eos>-> 4; 5 allows nothing and is unreachable."""
    ids = _ids(m)
    V, eos = m.decoder.vocab_size, ids["eos_idx"]
    ok = [k for k in range(V) if k not in ids.values()]
    A, Bs = ok[17], [ok[5], ok[90], ok[200]]
    nxt = torch.full((6, V), -1, dtype=torch.long)
    nxt[0, A] = 1
    nxt[1, Bs] = 2
    nxt[2, ok] = 3
    nxt[3, eos] = nxt[4, eos] = 4
    resync = torch.full((V,), 2, dtype=torch.long)
    resync[ok[::2]] = 4
    return _TA().from_transitions(nxt, 0, resync, **ids), A, Bs


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_narrow_states(dev, cdt):
    m, lat, mask, T = _case("vitomr_dh64b", cdt, dev)
    bf = cdt == torch.bfloat16
    B, eos, bos = lat.shape[0], m.decoder.eos_idx, m.decoder.bos_idx
    a, A, Bs = _narrow(m)
    U = torch.rand(B, T, generator=torch.Generator().manual_seed(9)).to(dev)
    U[0, :3], U[1, :3] = 0.0, 0.99999
    s, lp, mk = _sample(m, lat, mask, T, bf, U, 50, grammar=a)
    assert s.shape == (B, 5) and bool(mk.all())
    assert s[:, 0].tolist() == [bos] * B and s[:, 1].tolist() == [A] * B and s[:, 4].tolist() == [eos] * B
    assert lp[:, 1].tolist() == [0.0] * B and lp[:, 4].tolist() == [0.0] * B        # one allowed token: log-prob 0 whatever u is
    # the three-token state against the restatement on the host-stepped logits, fed the run's own tokens
    with torch.no_grad(), _ctx(bf):
        fn = _host_logits(m, lat, mask, T)
        fn(s[:, 0].cpu(), 1)
        lg = fn(s[:, 1].cpu(), 2)
    kept = lg[:, Bs]
    order = torch.argsort(kept, dim=1, descending=True, stable=True)
    assert int(s[0, 2]) == Bs[int(order[0, 0])]                           # u = 0: the best of the three
    assert all(int(v) in Bs for v in s[:, 2])                             # top_k = 50, and the kept set is those three
    # the restatement's draw, unless u sits next to a boundary of its CDF: one bf16 ulp of a logit moves a boundary by up to
    # 0.25 (exp(ulp / temperature) - 1) (tests/test_gpu_continuous_sample.py), 0.03 at the ulp of 0.125 of logits of 16 .. 32
    margin = 0.25 * (math.exp(0.125 / TEMPERATURE) - 1.0) if bf else 1e-5
    for b in range(B):
        p = torch.softmax(kept[b][order[b]] / TEMPERATURE, 0).cumsum(0)
        tok, _, _ = GR.select_sample(lg[b], 1, a, float(U[b, 2]), 50, TEMPERATURE)
        if float((p[:-1] - float(U[b, 2])).abs().min()) > margin:
            assert int(s[b, 2]) == tok, (b, float(U[b, 2]), p.tolist())
    want = torch.stack([torch.log_softmax(kept[b], 0)[Bs.index(int(s[b, 2]))] for b in range(B)])
    live = torch.ones(B, dtype=torch.bool)
    _check_lps(lp[:, 2], want, live, bf)
    assert not any(int(v) == eos for v in s[:, 3])
    # greedy under the same automaton, and the batch exits once every row is done: four steps
    gs, glp, gmk = _greedy(m, lat, mask, T, bf, grammar=a)
    assert gs.shape == (B, 5) and gs[:, 1].tolist() == [A] * B and gs[:, 4].tolist() == [eos] * B
    assert [int(v) for v in gs[:, 2]] == [Bs[int(order[b, 0])] for b in range(B)]
    eng = m.decoder.decoder_blocks.engine(dev)
    with torch.no_grad(), _ctx(bf):
        _greedy(m, lat, mask, T, bf)            # (re-prepares the caches)
        _, _, done = eng.greedy(T, poll=1, grammar=a)
    assert done == 4 and int(eng.finished[eng.B]) == 0
    assert eng.gram_state[:B].tolist() == [4] * B


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_dead_state_through_the_c_abi(dev, cdt):
    from acai_omr_amd import _lib
    m, lat, mask, T = _case("vitomr_dh64b", cdt, dev)
    bf = cdt == torch.bfloat16
    B = lat.shape[0]
    a, _, _ = _narrow(m)
    g = _greedy(m, lat, mask, T, bf)            # prepares the caches; index 1 of the plain result is the unconstrained choice
    eng = m.decoder.decoder_blocks.engine(dev)
    L = _lib.lib()
    eng._mode = ("grammar",)
    try:
        with torch.no_grad():
            eng._set_grammar(a)
            eng.arm(B)
            eng.gram_state[:B] = torch.tensor([5, 99, 5][:B], dtype=torch.int32, device=dev)   # the dead state; 99 is clamped to it
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(L.acai_decode_grammar_step(ctypes.byref(eng._desc), ctypes.byref(eng._gram_desc), st), "acai_decode_grammar_step")
            torch.cuda.synchronize()
            tok, lp, state = eng.seqs[:B, 1].clone(), eng.logprobs[:B, 1].clone(), eng.gram_state[:B].clone()
    finally:
        eng._mode = ("greedy",)
    assert torch.equal(tok, g[0][:, 1]) and torch.equal(lp, g[1][:, 1])     # the unconstrained step, bit for bit
    assert state.tolist() == [int(a.resync[int(k)]) for k in tok]
    _same(g, _greedy(m, lat, mask, T, bf))


# ---- 4. table sizes: S = 32767 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_chain_automaton_of_32767_states(dev, cdt):
    m, lat, mask, _ = _case("random", cdt, dev)
    bf = cdt == torch.bfloat16
    ids = _ids(m)
    V, S, T = m.decoder.vocab_size, 32767, 41
    key = ("chain", V)
    if key not in _CACHE:
        ok = torch.tensor([k for k in range(V) if k not in ids.values()])
        i = torch.arange(S)
        nxt = torch.full((S, V), -1, dtype=torch.long)
        to = (i + 1).clamp(max=S - 1)
        nxt[i, ok[i % 97]] = to
        nxt[i, ok[100 + (7 * i + 13) % 89]] = to
        _CACHE[key] = _TA().from_transitions(nxt, S - 30, **ids)      # 30 states before the end: the run reaches the clamp at S - 1
    a = _CACHE[key]
    assert a.start * V > 2 ** 22 and int(a.next.max()) == S - 1        # row offsets past 2^22 elements, entries that need 15 bits
    out = _greedy(m, lat, mask, T, bf, grammar=a)
    rs, _ = _check_against_restatement(m, lat, mask, T, bf, a, out)
    eng = m.decoder.decoder_blocks.engine(dev)
    assert a.violations(rs)[0].tolist() == [0] * rs.shape[0]
    assert out[0].shape[1] == T and eng.gram_state[:rs.shape[0]].tolist() == [S - 1] * rs.shape[0]
    # a smaller automaton afterwards runs in the larger buffer
    _same(_greedy(m, lat, mask, T, bf), _greedy(m, lat, mask, T, bf, grammar=_permissive(m, True)))


# ---- 5. slot modes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_slot_modes_each_image_as_alone(dev, cdt):
    m, lat, mask, T = _case("vitomr_dh64b", cdt, dev)
    bf = cdt == torch.bfloat16
    a, _ = _restrictive(m, _greedy(m, lat, mask, T, bf))
    order = [0, 1, 2, 0, 1, 2, 0]
    caps = [T, 5, T - 3, 9, T, 2, 12]
    lat7, mask7 = lat[order], mask[order]
    U = torch.rand(7, T, generator=torch.Generator().manual_seed(12)).to(dev)
    eng = m.decoder.decoder_blocks.engine(dev)
    alone_g = [_greedy(m, lat7[i:i + 1], mask7[i:i + 1], caps[i], bf, grammar=a) for i in range(7)]
    alone_s = [_sample(m, lat7[i:i + 1], mask7[i:i + 1], caps[i], bf, U[i:i + 1, :caps[i]], 50, grammar=a) for i in range(7)]

    def check(got, alone, what):
        seqs, lps, mk = got
        for i, (rs, rl, rk) in enumerate(alone):
            n = rs.shape[1]
            assert torch.equal(seqs[i, :n], rs[0]) and torch.equal(mk[i, :n], rk[0]) and not bool(mk[i, n:].any()), (what, i)
            assert torch.equal(lps[i, :n], rl[0]), (what, i, float((lps[i, :n] - rl[0]).abs().max()))

    with torch.no_grad(), _ctx(bf):
        got = m.cached_continuous_generate(lat7, mask7, max_len=caps, slots=3, grammar=a)
    check(got, alone_g, "greedy")
    assert eng.slot_steps < sum(c - 1 for c in caps)                    # rows were refilled while others went on
    viol, _ = a.violations(got[0].cpu(), got[2].cpu())
    assert viol.tolist() == [0] * 7
    from acai_omr_amd import engine as EG
    with torch.no_grad(), _ctx(bf):
        mem32, lens = EG.unpad_rows(lat7, mask7)
        got = m._continuous_packed(mem32, None, lens, caps, 3, sample=(50, TEMPERATURE), uniforms=U, grammar=a)
    check(got, alone_s, "sampled")
    assert a.violations(got[0].cpu(), got[2].cpu())[0].tolist() == [0] * 7
    # two images through three slots: slot 2 stays idle, and its (poisoned) state is neither read out of bounds nor written
    eng.gram_state[2] = 2 ** 30
    with torch.no_grad(), _ctx(bf):
        two = m.cached_continuous_generate(lat7[:2], mask7[:2], max_len=caps[:2], slots=3, grammar=a)
        mem32, lens = EG.unpad_rows(lat7[:2], mask7[:2])
        two_s = m._continuous_packed(mem32, None, lens, caps[:2], 3, sample=(50, TEMPERATURE), uniforms=U[:2, :max(caps[:2])], grammar=a)
    check(two, alone_g[:2], "greedy, idle slot")
    check(two_s, alone_s[:2], "sampled, idle slot")
    assert int(eng.gram_state[2]) == 2 ** 30
    with torch.no_grad(), _ctx(bf):                                     # the unconstrained slot modes afterwards
        _same(m.cached_continuous_generate(lat7, mask7, max_len=caps, slots=3),
              m.cached_continuous_generate(lat7, mask7, max_len=caps, slots=3, grammar=_permissive(m, False)))


# ---- 6. hygiene ------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_a_larger_automaton_gets_its_own_graphs(dev):
    from acai_omr_amd import engine as EG
    m, lat, mask, T = _case("vitomr_dh64b", torch.bfloat16, dev)
    g = _greedy(m, lat, mask, T, True)
    a, _ = _restrictive(m, g)
    want = _greedy(m, lat, mask, T, True, grammar=a)
    eng = m.decoder.decoder_blocks.engine(dev)
    mem32, lens = EG.unpad_rows(lat, mask)
    for form in (dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False)):
        with torch.no_grad():
            m.decoder.decoder_blocks.prepare_caches_packed(mem32, None, lens)
            s, lp, _ = eng.greedy(T, grammar=a, **form)
            _same(want, m.mask_and_clip_seqs(s.clone(), lp.clone()))
    U = torch.rand(lat.shape[0], T, generator=torch.Generator().manual_seed(13)).to(dev)
    _same(_sample(m, lat, mask, T, True, U, 50, grammar=a), _sample(m, lat, mask, T, True, U, 50, grammar=a, use_graph=False))
    # one state, then 227 states (reallocation: the one-state graphs are dropped), then another 227-state automaton, then one state again
    fresh = build_vitomr(load_golden("vitomr_dh64b")["cfg"], load_golden("vitomr_dh64b")["state_dict"], dev, torch.bfloat16, max_batch=24)
    ids = _ids(m)
    second, _ = _restrictive(m, g, extra=[(int(want[0][i, 1]), int(want[0][i, 2])) for i in range(lat.shape[0])])
    want2 = _greedy(m, lat, mask, T, True, grammar=second)
    assert want2[0].shape != want[0].shape or not torch.equal(want2[0], want[0])
    _same(g, _greedy(fresh, lat, mask, T, True, grammar=_permissive(fresh, False)))
    _same(want, _greedy(fresh, lat, mask, T, True, grammar=a))
    _same(want2, _greedy(fresh, lat, mask, T, True, grammar=second))
    _same(g, _greedy(fresh, lat, mask, T, True, grammar=_permissive(fresh, False)))
    _same(want, _greedy(fresh, lat, mask, T, True, grammar=a))
    _check_against_restatement(m, lat, mask, T, True, second, want2)
    assert ids == _ids(fresh)


def test_grammar_runs_leave_other_modes_alone(dev):
    from acai_omr_amd import engine as EG
    from acai_omr_amd.inference.vitomr_inference import inference
    fx = load_golden("vitomr_dh64b")
    cfg = fx["cfg"]
    T = cfg["gen_len"]
    u = torch.rand(len(fx["imgs"]) * 2, T, generator=torch.Generator().manual_seed(3)).to(dev)

    def setup():
        m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
        mem, mask = _memory(m, fx["imgs"], True)
        return m, mem, mask

    def others(m, mem, mask):
        g = inference(m, fx["imgs"], "cuda", max_inference_len=T)
        pre = [g[0][i, 1:4] for i in range(len(fx["imgs"]))]
        with torch.no_grad(), _ctx(True):
            b = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
            c = m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2)
            sp = m.cached_speculative_generate(mem, mask, max_len=T, draft_len=4)
            p = m.cached_greedy_generate(mem, mask, max_len=T, prefix=pre)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return g + b + c + sp + p + s

    def constrained(m, mem, mask, a):
        with torch.no_grad(), _ctx(True):
            mem32, lens = EG.unpad_rows(mem, mask)
            return m.cached_greedy_generate(mem, mask, max_len=T, grammar=a) + \
                m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2, grammar=a) + \
                m._continuous_packed(mem32, None, lens, [T, T - 3, 5], 2, sample=(5, 1.3), uniforms=u[:3], grammar=a) + \
                _sample(m, mem, mask, T, True, u, 5, G=2, grammar=a)

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    a, _ = _restrictive(m0, fresh_others[:3])
    m1, mem1, mask1 = setup()
    fresh_constrained = constrained(m1, mem1, mask1, a)
    _same(fresh_others, others(m1, mem1, mask1))                 # grammar runs, then greedy / beam / slot / speculative / prompted / sampling
    _same(fresh_constrained, constrained(m1, mem1, mask1, a))    # and the reverse, on captured graphs of both
    _same(fresh_constrained, constrained(m0, mem0, mask0, a))
    assert m1.decoder.decoder_blocks.engine(dev)._mode == ("greedy",)


def test_entry_points(dev):
    from acai_omr_amd.config import InferenceEvent
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, inference, iter_continuous_inference, streamed_inference
    fx = load_golden("vitomr_dh64b")
    cfg, imgs = fx["cfg"], fx["imgs"]
    T = cfg["max_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
    plain = inference(m, imgs, "cuda", max_inference_len=T)
    a, _ = _restrictive(m, plain)
    batch = inference(m, imgs, "cuda", max_inference_len=T, grammar=a)
    assert a.violations(batch[0].cpu(), batch[2].cpu())[0].tolist() == [0] * len(imgs)
    _same(plain, inference(m, imgs, "cuda", max_inference_len=T, grammar=None))
    _same(batch, continuous_inference(m, imgs, "cuda", max_inference_len=T, slots=2, grammar=a))
    got = {i: r for i, *r in iter_continuous_inference(m, imgs, "cuda", max_inference_len=T, slots=2, grammar=a)}
    for i, img in enumerate(imgs):
        one = inference(m, [img], "cuda", max_inference_len=T, grammar=a)
        _same(one, tuple(got[i]))
        ev = list(streamed_inference([img], m, "cuda", max_inference_len=T, flush_interval=5, grammar=a))
        fin = ev[-1]["payload"]
        _same(one, (fin["sequence"], fin["log_probs"], fin["mask"]))
        steps = [e["payload"]["tokens"] for e in ev if e["type"] == InferenceEvent.STEP.value]
        if steps:
            cat = torch.cat(steps, dim=1)
            assert torch.equal(cat.long(), one[0][:, 1:1 + cat.shape[1]])
    pre = [plain[0][i, 1:3] for i in range(len(imgs))]
    for kw, msg in ((dict(beam_width=2), "beam"), (dict(speculative=2), "speculative"), (dict(prefix=pre), "prefix")):
        with pytest.raises(ValueError, match=f"grammar.*{msg}"):
            inference(m, imgs, "cuda", max_inference_len=T, grammar=a, **kw)
    with pytest.raises(ValueError, match="grammar.*prefix"):
        list(streamed_inference([imgs[0]], m, "cuda", max_inference_len=T, grammar=a, prefix=[pre[0]]))
    with pytest.raises(TypeError, match="TokenAutomaton"):
        inference(m, imgs, "cuda", max_inference_len=T, grammar=a.next)
    lat, mask = _memory(m, imgs, True)
    small = _TA().permissive(m.decoder.vocab_size + 1, **_ids(m))
    with pytest.raises(ValueError, match="vocabulary"), torch.no_grad():
        m.cached_greedy_generate(lat, mask, max_len=T, grammar=small)
    _same(plain, inference(m, imgs, "cuda", max_inference_len=T))
    # an automaton that already lives on the device
    _same(batch, inference(m, imgs, "cuda", max_inference_len=T, grammar=a.to(dev)))


def test_fp8_memory_cache(dev):
    fx = load_golden("vitomr_small")
    T = fx["cfg"]["gen_len"]
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16, max_batch=8, memory_cache_dtype=torch.float8_e4m3fn)
    lat, mask = _memory(m, fx["imgs"], True)
    g = _greedy(m, lat, mask, T, True)
    a, _ = _restrictive(m, g)
    out = _greedy(m, lat, mask, T, True, grammar=a)
    assert m.decoder.decoder_blocks.engine(dev).cross_fp8
    _check_against_restatement(m, lat, mask, T, True, a, out, tokens_only=True)
    assert a.violations(out[0].cpu(), out[2].cpu())[0].tolist() == [0] * lat.shape[0]
    _same(g, _greedy(m, lat, mask, T, True, grammar=_permissive(m, True)))


# ---- 7. the scan kernel ------------------------------------------------------------------------------------------------------------------------
def _scan_automata():
    if "scan" in _CACHE:
        return _CACHE["scan"]
    V, pad, eos = _vocab()
    toks = [ln.strip() for ln in open(VOCAB) if ln.strip()]
    bos = toks.index("<bos>")
    ids = dict(pad_idx=pad, bos_idx=bos, eos_idx=eos)
    g = torch.Generator().manual_seed(17)
    nxt = GR.bigram_permissive(V, pad, bos, eos)
    nxt[torch.rand(V, V, generator=g) < 0.3] = -1
    nxt[:, 3] = 3                                   # (no state dies)
    small = _TA().from_transitions(nxt, bos, _bigram_resync(V, ids), **ids)
    S = 4096
    big = torch.randint(0, S, (S, V), generator=g)
    big[torch.rand(S, V, generator=g) < 0.3] = -1
    big[:, 3] = torch.randint(0, S, (S,), generator=g)
    big[:, bos] = big[:, pad] = -1
    large = _TA().from_transitions(big, 5, torch.randint(0, S, (V,), generator=g), **ids)
    assert small.states * V * 2 <= 156 * 1024 < large.states * V * 2      # one fits the LDS path, the other does not
    _CACHE["scan"] = (small, large, ids)
    return _CACHE["scan"]


@pytest.mark.parametrize("ld", [48, 1536])
@pytest.mark.parametrize("R", [1, 65, 257])
def test_scan_kernel_against_the_cpu_statement(dev, R, ld):
    from acai_omr_amd import ops
    small, large, ids = _scan_automata()
    V, eos = small.vocab_size, ids["eos_idx"]
    g = torch.Generator().manual_seed(100 * R + ld)
    rows = torch.randint(0, V, (R, ld), generator=g)
    rows[:, 0] = ids["bos_idx"]
    lens = torch.randint(0, ld + 1, (R,), generator=g, dtype=torch.int32)
    special = [0, 1, 2, ld, ld + 7, -3]                                    # (the last two are clamped to ld and 0)
    for i, n in enumerate(special[:R] if R > 1 else [ld]):
        lens[i] = n
    last = (lens.long().clamp(0, ld) - 1).clamp(min=1)
    ends = torch.rand(R, generator=g) < 0.6
    rows[ends, last[ends]] = eos                                           # most rows end in <eos> ...
    rows[torch.arange(R), last // 2] = torch.where(torch.rand(R, generator=g) < 0.3, torch.full((R,), eos), rows[torch.arange(R), last // 2])   # ... some hold one mid-row
    rows[R - 1, ld // 3], rows[R - 1, ld // 2], rows[R - 1, ld - 2] = V, -1, 2 ** 40    # ids outside [0, V)
    lens[R - 1] = ld
    if R > 2:
        rows[2, 1] = eos                                                   # <bos> <eos>
    for a, path in ((small, "LDS"), (large, "global")):
        want_v, want_c = a.violations(rows, lens)
        ad = a.to(dev)
        viol, comp = ops.grammar_scan(rows.to(dev), lens.to(dev), ad)
        assert viol.dtype == torch.int32 and comp.dtype == torch.bool
        assert torch.equal(viol.cpu(), want_v) and torch.equal(comp.cpu(), want_c), (path, R, ld)
        mask = torch.arange(ld).unsqueeze(0) < lens.long().clamp(0, ld).unsqueeze(1)
        v2, c2 = ops.grammar_scan(rows.to(dev), mask.to(dev), a)              # a bool mask, tables still on the CPU
        assert torch.equal(v2.cpu(), want_v) and torch.equal(c2.cpu(), want_c), (path, R, ld)
        print(f"scan {path} R={R} ld={ld}: {int(want_v.sum())} violations, {int(want_c.sum())} complete rows")
        assert int(want_v.sum()) > 0 and (R == 1 or 0 < int(want_c.sum()) < R)


# ---- 8. the C ABI's argument checks ---------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks(dev):
    from acai_omr_amd import _lib
    m, lat, mask, T = _case("vitomr_dh64b", torch.bfloat16, dev)
    a = _permissive(m, True)
    U = torch.rand(lat.shape[0], T, generator=torch.Generator().manual_seed(5)).to(dev)
    from acai_omr_amd import engine as EG
    with torch.no_grad(), _ctx(True):
        mem32, lens = EG.unpad_rows(lat, mask)
        m._continuous_packed(mem32, None, lens, [T] * len(lens), 2, sample=(5, TEMPERATURE), uniforms=U, grammar=a)   # leaves the slot descriptors behind
    _sample(m, lat, mask, T, True, U, 5, grammar=a)                        # and the static batch's descriptors
    eng = m.decoder.decoder_blocks.engine(dev)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    d, gr, sl = ctypes.byref(eng._desc), ctypes.byref(eng._gram_desc), ctypes.byref(eng._slot_desc)
    u, su, ur = eng.uniforms.data_ptr(), eng.slot_uniforms.data_ptr(), eng.slot_urow.data_ptr()
    calls = {
        b"acai_decode_grammar_step": lambda g: L.acai_decode_grammar_step(d, g, st),
        b"acai_decode_grammar_sample_step": lambda g: L.acai_decode_grammar_sample_step(d, g, u, 5, TEMPERATURE, st),
        b"acai_decode_slot_grammar_step": lambda g: L.acai_decode_slot_grammar_step(d, sl, g, st),
        b"acai_decode_slot_grammar_sample_step": lambda g: L.acai_decode_slot_grammar_sample_step(d, sl, g, su, eng.Tmax, ur, 5, TEMPERATURE, st),
    }
    step_before = eng.step.tolist()
    for name, call in calls.items():
        assert call(None) < 0 and name in L.acai_last_error() and b"null grammar" in L.acai_last_error()
        for field, bad, msg in (("next", None, b"null grammar"), ("resync", None, b"null grammar"), ("state", None, b"null grammar"),
                                ("states", 0, b"states"), ("states", 32768, b"states"), ("start", -1, b"start"),
                                ("start", eng._gram_desc.states, b"start"), ("rows", eng.B - 1, b"rows")):
            keep = getattr(eng._gram_desc, field)
            setattr(eng._gram_desc, field, bad)
            try:
                assert call(gr) < 0, (name, field)
                assert name in L.acai_last_error() and msg in L.acai_last_error(), (name, field, L.acai_last_error())
            finally:
                setattr(eng._gram_desc, field, keep)
    assert L.acai_decode_grammar_sample_step(d, gr, None, 5, TEMPERATURE, st) < 0 and b"acai_decode_grammar_sample_step" in L.acai_last_error()
    assert L.acai_decode_grammar_sample_step(d, gr, u, 65, TEMPERATURE, st) < 0 and b"top_k" in L.acai_last_error()
    assert L.acai_decode_slot_grammar_sample_step(d, sl, gr, su, eng.Tmax - 1, ur, 5, TEMPERATURE, st) < 0 and b"ld_uniforms" in L.acai_last_error()
    assert L.acai_decode_slot_grammar_step(d, None, gr, st) < 0 and b"acai_decode_slot_grammar_step" in L.acai_last_error()
    torch.cuda.synchronize()
    assert eng.step.tolist() == step_before                                # errors, not launches
    eng.logits_step(torch.zeros(eng.B, dtype=torch.int64, device=dev), 1)   # overwrites x
    for name, call in calls.items():
        assert call(gr) < 0 and name in L.acai_last_error() and b"x does not hold" in L.acai_last_error(), name
    # the scan
    ad = a.to(dev)
    rows = torch.zeros(4, 8, dtype=torch.int64, device=dev)
    lens = torch.full((4,), 8, dtype=torch.int32, device=dev)
    out = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    args = [rows.data_ptr(), 8, lens.data_ptr(), 4, ad.next.data_ptr(), ad.resync.data_ptr(), ad.states, ad.start, ad.vocab_size, ad.eos_idx,
            out[0].data_ptr(), out[1].data_ptr(), st]
    assert L.acai_grammar_scan(*args) == 0
    for pos, bad in ((2, None), (4, None), (5, None), (10, None), (11, None), (3, 0), (6, 0), (6, 32768), (7, -1), (7, ad.states), (8, 0)):
        b = list(args)
        b[pos] = bad
        assert L.acai_grammar_scan(*b) < 0 and b"acai_grammar_scan" in L.acai_last_error(), pos
    torch.cuda.synchronize()


# ---- 9. GRPO ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [None, 4])
def test_grpo_update_with_a_grammar(dev, slots):
    from acai_omr_amd.models.models import OMRCELoss
    from acai_omr_amd.train import grpo as G
    fx, old, theta, Gs, cfg = _models(dev)
    V, pad, eos = _vocab()
    ids = _ids(old)
    g = torch.Generator().manual_seed(71)
    nxt = GR.bigram_permissive(V, pad, ids["bos_idx"], eos)
    nxt[torch.rand(V, V, generator=g) < 0.08] = -1
    assert int((nxt >= 0).sum(dim=1).min()) > 180
    a = _TA().from_transitions(nxt, ids["bos_idx"], _bigram_resync(V, ids), **ids)
    max_actions = cfg["max_len"] - 2
    R = len(fx["imgs"]) * Gs
    uniforms = torch.rand(R, max_actions, generator=g).to(dev)
    targets = [torch.randint(3, 227, (n,), generator=g) for n in (9, 5, 12)]
    batch = [(img, t, "") for img, t in zip(fx["imgs"], targets)]
    conf = G.GRPOConfig(G.RolloutConfig(Gs, max_actions, 20, 1.1), G.INITIAL_REWARD_CONFIG, G.LossConfig(0.05, 0.1), G.UpdateConfig(0.2, 1, 1.0),
                        100, 100)
    seen = {}
    inner = G.make_token_reward_fn(conf.reward_config, pad, grammar=a.to(dev))

    def reward_fn(rollouts, rollout_mask, target_lmx_seqs, b):
        out = inner(rollouts, rollout_mask, target_lmx_seqs, b)
        seen.update(rollouts=rollouts.cpu(), mask=rollout_mask.cpu(), comps=out[1])
        return out

    # without the grammar the same draws break the automaton somewhere (the check is not vacuous)
    with torch.no_grad(), _ctx(True):
        lat, lmask = _memory(old, fx["imgs"], True)
        xl, xm = old.expand_img_latent_for_rollout(lat, lmask, Gs)
        free = old.cached_forward_rollout_policy(xl, xm, max_actions, 20, 1.1, group_size=Gs, uniforms=uniforms)
    assert int(a.violations(free[0].cpu(), free[2].cpu())[0].sum()) > 0
    opt = torch.optim.SGD(theta.parameters(), lr=1e-4)
    loss, ce, rew, comps = G.grpo_update(old, theta, opt, batch, conf, OMRCELoss(pad), "cuda", reward_fn=reward_fn, uniforms=uniforms,
                                         rollout_slots=slots, grammar=a)
    assert all(math.isfinite(v) for v in (loss, ce, rew) + comps._vals())
    viol, comp = a.violations(seen["rollouts"], seen["mask"])
    assert viol.tolist() == [0] * R                                        # the rollouts are constrained
    rc = conf.reward_config
    want = G.calc_wellformedness(~comp, viol.float(), rc.gamma, rc.alpha_well_formed)
    assert torch.equal(seen["comps"].wellformedness_scores.cpu(), want)
    assert bool(((want == 1.0) | (want == -rc.gamma)).all())
    print(f"grpo_update(grammar=, rollout_slots={slots}): {int(comp.sum())} of {R} rollouts end with an allowed <eos>; loss {loss:.4g}")
    if slots is not None:   # validation_loop: constrained rollouts and the default reward's well-formedness term
        torch.manual_seed(3)
        r2, c2, ce2 = G.validation_loop([batch], old, rc, G.RolloutConfig(1, max_actions, 20, 1.1), OMRCELoss(pad), pad, "cuda", slots=slots,
                                        grammar=a)
        assert all(math.isfinite(v) for v in (r2, ce2) + c2._vals()) and -rc.gamma <= c2.wellformedness_scores <= 1.0
        assert c2.wellformedness_scores != 0.0


# ---- 10. every selection form at more rows than the closing workgroup has waves ---------------------------------------------------------------
WIDE_B, WIDE_T, WIDE_K = 18, 10, 5
WIDE_CAPS = [WIDE_T, 3, WIDE_T - 2, 5, 2, WIDE_T, 7, 4, WIDE_T - 1, 6, WIDE_T, 3, 8, 2, WIDE_T, 5, WIDE_T - 3, WIDE_T]


def _wide_case(cdt, dev):
    """A one-layer decoder (E 1024, 16 heads) on 18 memories of 9 .. 60 rows, max_len 10."""
    key = ("wide", cdt)
    if key not in _CACHE:
        dec = _decoder(T=WIDE_T, L=1, E=1024, H=16, Fd=4096)
        g = torch.Generator().manual_seed(23)
        lens = [9 + 3 * i for i in range(WIDE_B)]
        lat = torch.zeros(WIDE_B, max(lens), 1024)
        mask = torch.ones(WIDE_B, max(lens), dtype=torch.bool)
        for i, n in enumerate(lens):
            lat[i, :n] = torch.randn(n, 1024, generator=g).to(torch.bfloat16).float()
            mask[i, :n] = False
        _CACHE[key] = (_vit(dec, 24, cdt, dev), lat.to(dev), mask.to(dev))
    return _CACHE[key]


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_every_selection_form_at_18_rows(dev, cdt):
    """The nine selection forms (greedy / sampled x static / slot x plain / grammar, and prompted greedy) at B = 18 - rows 16 and 17 are the
    second pass of a wave of the one workgroup that closes a greedy step, and the fifth sampling workgroup is half empty - against the
    float64 restatements on the host-stepped logits at the same B: tests/grammar_reference.py with the case's restrictive automaton for the
    grammar forms and a table that allows everything for the plain ones, tests/prompt_reference.py's selection rule for the prompted
    form.  A slot run (18 slots, caps 2 .. 10) must give every row what the restatement gives it up to its cap.  Tokens and masks equal;
    log-probs within bar 2's bounds (_check_lps)."""
    import prompt_reference as PR
    from acai_omr_amd import engine as EG
    m, lat, mask = _wide_case(cdt, dev)
    bf = cdt == torch.bfloat16
    B, T, K, caps = WIDE_B, WIDE_T, WIDE_K, WIDE_CAPS
    bos, pad = m.decoder.bos_idx, m.decoder.pad_idx
    free = _permissive(m, False)
    tight, _ = _restrictive(m, _greedy(m, lat, mask, T, bf))
    U = torch.rand(B, T, generator=torch.Generator().manual_seed(14))
    # prompts of seeded random ids without the specials: row 0 none, row 1 max_len - 1, the rest 1 .. max_len - 2 tokens
    ok = torch.tensor([i for i in range(m.decoder.vocab_size) if i not in _ids(m).values()])
    g = torch.Generator().manual_seed(33)
    prompts = [ok[torch.randint(len(ok), (n,), generator=g)] for n in [0, T - 1] + [1 + (4 * i) % (T - 2) for i in range(2, B)]]
    eng = m.decoder.decoder_blocks.engine(dev)
    assert eng.tickets is not None     # a slot sampling step is five workgroups closed by the last to arrive

    def restated(a, sampled):
        with torch.no_grad(), _ctx(bf):
            fn = _host_logits(m, lat, mask, T)
            if sampled:
                return GR.constrained_sample(fn, a, B, T, bos, U, K, TEMPERATURE)[:2]
            return GR.constrained_greedy(fn, a, B, T, bos)[:2]

    def restated_prompt():
        rs = torch.full((B, T), bos, dtype=torch.int64)
        rlp = torch.zeros(B, T, dtype=torch.float64)
        with torch.no_grad(), _ctx(bf):
            fn = _host_logits(m, lat, mask, T)
            for t in range(1, T):
                lg = fn(rs[:, t - 1], t)
                for b in range(B):
                    rs[b, t], rlp[b, t], _ = PR.select(lg[b].tolist(), t, [int(v) for v in prompts[b]])
        return rs, rlp

    def check(what, out, ref, row_caps):
        rs, rlp = ref
        rmask = m.create_inference_mask(rs) & (torch.arange(T) < torch.tensor(row_caps).unsqueeze(1))
        n = int(rmask.sum(dim=-1).max())
        seqs, lps, mk = (x.cpu() for x in out)
        assert seqs.shape[1] == n and torch.equal(mk, rmask[:, :n]), what
        assert torch.equal(seqs, rs.masked_fill(~rmask, pad)[:, :n]), (what, (seqs != rs.masked_fill(~rmask, pad)[:, :n]).nonzero().tolist())
        live = rmask[:, :n].clone()
        live[:, 0] = False
        print(what, end=": ")
        _check_lps(lps, rlp[:, :n], live, bf)
        assert bool((lps[~mk] == 0).all()), what

    def slots(**kw):
        with torch.no_grad(), _ctx(bf):
            mem32, lens = EG.unpad_rows(lat, mask)
            return m._continuous_packed(mem32, None, lens, caps, B, **kw)

    full = [T] * B
    for a, name in ((free, "plain"), (tight, "grammar")):
        kw = {} if a is free else {"grammar": a}
        ref = restated(a, False)
        check(f"{name} greedy", _greedy(m, lat, mask, T, bf, **kw), ref, full)
        check(f"{name} slot greedy", slots(**kw), ref, caps)
        ref = restated(a, True)
        check(f"{name} sampled", _sample(m, lat, mask, T, bf, U.to(dev), K, **kw), ref, full)
        check(f"{name} slot sampled", slots(sample=(K, TEMPERATURE), uniforms=U.to(dev), **kw), ref, caps)
    check("prompted greedy", _greedy(m, lat, mask, T, bf, prefix=prompts), restated_prompt(), full)
