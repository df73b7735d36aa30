"""Prompt prefill on the GPU (acai_decode_prefill_self_kv / acai_decode_prefill_arm through DecodeEngine.greedy(prompt=, prefill=True) /
greedy_chunks, ViTOMR.cached_greedy_generate(prefix=, prefill=True), inference(prefix=, prefill=True) and streamed_inference).

Shapes: tests 1 and 2 call the two entry points on engines of small random decoders (Tmax = 72, Bmax = 5, three rows armed) with dh = 32,
64 and the odd fixture's 12 (dhp = 16 > dh); tests 3 and 4 use test_gpu_prompt's cases - the golden fixtures vitomr_small, vitomr_dh64b,
vitomr_odd and the random decoder _decoder(T=48, L=2, E=1024, H=16, Fd=4096) on memories of 40 / 17 / 64 rows - in fp32 and bf16.

Bars:
  1. the scatter is torch.equal to the restatement (tests/prefill_reference.py), and everything it must not write keeps its sentinel;
  2. arm: seqs, step, finished[0..B] and x torch.equal to the restatement; log-probs against float64 log_softmax of the same logits: fp32
     within 1e-5 * max(1, |lp|), bf16 equal to the float64 value rounded to bf16 or its bf16 neighbour (bar 2 of test_gpu_prompt.py);
  3. the engine after prefill + arm at depth C against the engine after C prompt steps: integers and x equal, log-probs within the
     project's pass-versus-decode bars (1e-4 fp32, 0.07 bf16: test_gpu_confidence.py);
  4. end to end against the same call without prefill: mask and forced tokens equal, log-probs within the bars of 3, free tokens equal up to
     the row's first index where the host-stepped top-1 minus top-2 logit gap is below twice the bar (two logits, each off by at most the
     bar, cannot flip a larger gap).  fp32: every row is comparable to its end; bf16: at least half of the free (row, index) pairs are;
  5. prefill without a prefix, or with an empty prompt in the batch, is the call without it and prefills nothing;
  6. a prefilled run leaves the other modes as on a fresh engine and the reverse; graph replay == eager launches; poll = 1 == poll = 16;
  7. inference == streamed_inference; the refusals; the C ABI's argument checks return errors and launch nothing."""
import ctypes

import pytest
import torch

import prefill_reference as FR
from conftest import load_golden
from decode_support import _decoder, _memory, _same, _vit, build_vitomr, dev  # noqa: F401
from test_gpu_prompt import CASES, DTYPES, IDS, RAND_LENS, RAND_T, _ctx, _greedy, _random_prompts
from test_gpu_prompt import _case as _prompt_case

pytestmark = pytest.mark.gpu

BAR = {True: 0.07, False: 1e-4}     # pass-versus-decode log-prob bars, by "is bf16"
_TINY = {}
_RANDOM = {}
# The random decoder's seed.  Test 4 compares free tokens only while the top two logits are further apart than twice the log-prob bar, so it
# needs a decoder whose decisions are well separated in bf16 (logits near 10 are 0.0625 apart there: a gap must be three such steps).  On
# the CPU oracle (oracle.vitomr_oracle.decode_step, float64 and its bf16 emulation alike) seed 7 keeps 332 of the 388 free (row, index)
# pairs of test 4's prompts comparable and its smallest fp32 gap is 7e-3; decode_support's default seed 5 keeps 126 of 388, seeds 1 - 4, 6
# and 8 between 51 and 186.
RAND_SEED = 7


def _case(name, cdt, dev):
    """test_gpu_prompt's cases: its fixtures as they are; the random decoder with RAND_SEED and without the <eos> bias, on the same memories."""
    if name != "random":
        return _prompt_case(name, cdt, dev)
    if cdt not in _RANDOM:
        g = torch.Generator().manual_seed(21)
        lat = torch.zeros(len(RAND_LENS), max(RAND_LENS), 1024)
        mask = torch.ones(len(RAND_LENS), max(RAND_LENS), dtype=torch.bool)
        for i, n in enumerate(RAND_LENS):
            lat[i, :n] = torch.randn(n, 1024, generator=g).to(torch.bfloat16).float()
            mask[i, :n] = False
        dec = _decoder(T=RAND_T, L=2, E=1024, H=16, Fd=4096, seed=RAND_SEED)
        _RANDOM[cdt] = (_vit(dec, 24, cdt, dev), lat.to(dev), mask.to(dev), RAND_T)
    return _RANDOM[cdt]


def _tiny(dev, cdt, E, H):
    """(model, engine) of a small random decoder, Tmax = 72, Bmax = 5, prepared with three memories of 4 / 5 / 3 rows."""
    key = (cdt, E, H)
    if key not in _TINY:
        m = _vit(_decoder(T=72, L=2, E=E, H=H, Fd=2 * E), 5, cdt, dev)
        blocks = m.decoder.decoder_blocks
        mem = torch.randn(12, E, generator=torch.Generator().manual_seed(1)).to(dev)
        with torch.no_grad():
            blocks.prepare_caches_packed(mem, None, [4, 5, 3])
        _TINY[key] = (m, blocks.engine(dev))
    return _TINY[key]


def _ok_ids(m):
    dec = m.decoder
    return torch.tensor([i for i in range(dec.vocab_size) if i not in (dec.bos_idx, dec.pad_idx, dec.eos_idx)])


# ---- 1. the scatter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("E,H", [(128, 4), (128, 2), (12, 1)], ids=["dh32", "dh64", "dh12"])
def test_scatter_is_exact(dev, E, H, cdt):
    from acai_omr_amd import _lib
    m, eng = _tiny(dev, cdt, E, H)
    B, Tmax, dh = 3, eng.Tmax, E // H
    assert (eng.B, eng.Bmax, eng.L, eng.dh) == (B, 5, 2, dh) and (eng.dhp > dh) == (dh == 12)
    L, d, st = _lib.lib(), ctypes.byref(eng._desc), torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7)
    caches = eng.k_self + eng.v_self
    for C in (1, 2, 63, 64, 65, Tmax - 1):
        # qkv where the pass leaves it (row stride 3E), as columns of a wider matrix at a 16-byte offset, and at an offset that allows none
        for form, off, extra in (("plain", 0, 0), ("wide", 16, 32), ("shifted", 1, 32)):
            big = torch.randn(B * C, 3 * E + extra, generator=g).to(device=dev, dtype=cdt)
            qkv = big[:, off:off + 3 * E]
            for t in caches:
                t.copy_(torch.randn(t.shape, generator=g).to(device=dev, dtype=cdt))      # sentinel
            before = [t.clone() for t in caches]
            assert L.acai_decode_prefill_self_kv(d, 1, qkv.data_ptr(), qkv.stride(0), C, st) == 0, L.acai_last_error()
            torch.cuda.synchronize()
            k, v = FR.scatter(before[1], before[3], qkv, B, C, E, H, dh)
            where = (E, H, C, form)
            assert torch.equal(eng.k_self[1], k) and torch.equal(eng.v_self[1], v), where
            assert torch.equal(eng.k_self[0], before[0]) and torch.equal(eng.v_self[0], before[2]), where     # the other layer
            # written at all, and only where it may: positions < C, columns < dh, rows < B
            assert not torch.equal(eng.k_self[1][:B, :, :C, :dh], before[1][:B, :, :C, :dh]), where
            for got, was in ((eng.k_self[1], before[1]), (eng.v_self[1], before[3])):
                assert torch.equal(got[B:], was[B:]) and torch.equal(got[:, :, C:], was[:, :, C:]) and torch.equal(got[..., dh:], was[..., dh:])


# ---- 2. the arm kernel ------------------------------------------------------------------------------------------------------------------------
def _check_lps(got, want, bf):
    """Bar 2 of test_gpu_prompt.py: got fp32 from the device, want float64."""
    if bf:
        assert torch.equal(got, got.to(torch.bfloat16).float())          # rounded where the prompt step rounds
        wb = want.to(torch.bfloat16)
        ulps = (got.to(torch.bfloat16).view(torch.int16).int() - wb.view(torch.int16).int()).abs()
        bad = (ulps > 1) & (got != wb.float())
        print(f"bf16: {int((ulps == 1).sum())} of {ulps.numel()} log-probs are the bf16 neighbour of the rounded float64 value")
        assert not bool(bad.any()), (got[bad], want[bad])
    else:
        err = (got.double() - want).abs() / want.abs().clamp(min=1.0)
        print(f"fp32: max |lp - float64| / max(1, |lp|) = {float(err.max()):.3g}")
        assert float(err.max()) <= 1e-5


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_arm_state(dev, cdt):
    from acai_omr_amd import _lib
    m, eng = _tiny(dev, cdt, 128, 4)
    dec, bf = m.decoder, cdt == torch.bfloat16
    B, Tmax, V = 3, eng.Tmax, eng.V
    L, d, st = _lib.lib(), ctypes.byref(eng._desc), torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(11)
    ok, eos = _ok_ids(m), torch.tensor([dec.eos_idx])
    ids = lambda n: ok[torch.randint(len(ok), (n,), generator=g)]   # noqa: E731
    emb, pos = dec.vocab_embedding.weight.detach().cpu(), dec.pos_embedding.detach().cpu()
    for C in (1, 2, 7, 64, Tmax - 1):
        more = min(C + 3, Tmax - 1)
        for kind, prompts in (("ragged", [ids(C), ids(more), ids(min(C + 1, Tmax - 1))]),                 # rows with P_b > C where C allows
                              ("eos at C", [torch.cat([ids(C - 1), eos]), ids(more), ids(C)]),            # a prompt-final <eos> at index C
                              ("all done", [torch.cat([ids(C - 1), eos]) for _ in range(B)])):            # ... in every row: nothing is left
            logits = (torch.randn(B * C, V, generator=g) * 3).to(dev)
            with torch.no_grad():
                eng._set_prompt(prompts, B, Tmax)
                eng.arm(B)
                x0 = eng.ws["x"][:B].clone()
                assert L.acai_decode_prefill_arm(d, ctypes.byref(eng._prompt_desc), logits.data_ptr(), C, st) == 0, L.acai_last_error()
                torch.cuda.synchronize()
            want = FR.arm_state(logits, prompts, C, dec.bos_idx, dec.pad_idx, dec.eos_idx, Tmax, emb, pos, x0.cpu())
            where = (C, kind)
            assert torch.equal(eng.seqs[:B].cpu(), want["seqs"]), where
            assert eng.step.tolist() == want["step"], where
            assert torch.equal(eng.finished[:B + 1].cpu(), want["finished"]), (where, eng.finished[:B + 1].tolist())
            assert (int(want["finished"][B]) == 0) == (kind == "all done")
            assert torch.equal(eng.ws["x"][:B].cpu(), want["x"]), where
            lps = eng.logprobs[:B].cpu()
            assert bool((lps[:, 0] == 0).all()) and bool((lps[:, C + 1:] == 0).all())
            _check_lps(lps[:, 1:C + 1].reshape(-1), want["logprobs"][:, 1:C + 1].reshape(-1), bf)
        eng._x_valid = False      # (the arm entry point was called behind the engine's back)


# ---- 3. prefill + arm against C prompt steps ----------------------------------------------------------------------------------------------
def _engine_state(m, lat, mask, T, bf, prompts, C, prefill):
    """The engine's device state after the C common prompt tokens, taken by one prefill or by C prompt steps."""
    from acai_omr_amd import engine as EG
    blocks = m.decoder.decoder_blocks
    with torch.no_grad(), _ctx(bf):
        mem32, lens = EG.unpad_rows(lat, mask)
        blocks.prepare_caches_packed(mem32, None, lens)
        eng = blocks.engine(lat.device)
        B = eng.B
        with eng._run(T, ("prompt",)):
            eng._set_prompt(prompts, B, T)
            eng._arm_and_capture(B)
            if prefill:
                eng._prefill(C)
            else:
                eng.launch_steps(C)
        torch.cuda.synchronize()
    return dict(seqs=eng.seqs[:B, :C + 1].cpu(), lps=eng.logprobs[:B, :C + 1].cpu(), step=eng.step.tolist(),
                fin=eng.finished[:B + 1].tolist(), x=eng.ws["x"][:B].cpu())


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_state_after_prefill_is_the_state_after_C_steps(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    B, eng = lat.shape[0], m.decoder.decoder_blocks.engine(dev)
    eos = torch.tensor([m.decoder.eos_idx])
    for C in sorted({1, 2, T // 2, T - 1}):
        lens = [C, min(C + 3, T - 1), min(C + 1, T - 1)][:B]
        prompts = _random_prompts(m, B, T, seed=50 + C, lens=lens)
        if C > 1:
            prompts[0] = torch.cat([prompts[0][:-1], eos])       # a prompt-final <eos> at index C
        a = _engine_state(m, lat, mask, T, bf, prompts, C, False)
        b = _engine_state(m, lat, mask, T, bf, prompts, C, True)
        where = (name, C)
        assert torch.equal(a["seqs"], b["seqs"]) and a["step"] == b["step"] == [C + 1, C] and a["fin"] == b["fin"], (where, a["fin"], b["fin"])
        if C + 1 < eng.Tmax:      # (at C = Tmax - 1 there is no position C + 1: neither path writes an input that nothing would read)
            assert torch.equal(a["x"], b["x"]), where
        err = float((a["lps"].double() - b["lps"].double()).abs().max())
        print(f"{name} {'bf16' if bf else 'fp32'} C={C}: max |log-prob of the pass - of the steps| = {err:.3g}")
        assert err <= BAR[bf], where


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------
def _host_gaps(m, lat, mask, T, prompts):
    """test_gpu_prompt._host_stepped's path (one decoder.cached_generate call per token, fed the forced tokens, arg-max on the CPU after the
    prompt) -> seqs (B, T) and the top-1 minus top-2 logit gap at every index (B, T), on the CPU."""
    B = lat.shape[0]
    seqs, _, _ = m.cached_set_up_inference(lat, T)
    gap = torch.zeros(B, T, dtype=torch.float64)
    for t in range(1, T):
        lg = m.decoder.cached_generate(seqs[:, t - 1].unsqueeze(1), t, mask).squeeze(1).double().cpu()
        top = lg.topk(2, dim=-1).values
        gap[:, t] = top[:, 0] - top[:, 1]
        tok = torch.argmax(lg, dim=-1)
        for i, p in enumerate(prompts):
            if t <= len(p):
                tok[i] = int(p[t - 1])
        seqs[:, t] = tok.to(seqs.device)
    return seqs.cpu(), gap


def _compare(want, got, prompts, gap, bf, where):
    """-> (free (row, index) pairs compared, free pairs in all, rows comparable to their end)."""
    bar = BAR[bf]
    (ws, wl, wm), (gs, gl, gm) = ((x.cpu() for x in want), (x.cpu() for x in got))
    compared = total = whole = 0
    limits = []
    for b, p in enumerate(prompts):
        n, P = int(wm[b].sum()), len(p)
        low = [t for t in range(P + 1, n) if float(gap[b, t]) < 2 * bar]
        limits.append(low[0] if low else n)
    if all(limits[b] == int(wm[b].sum()) for b in range(len(prompts))):
        assert gs.shape == ws.shape and torch.equal(gm, wm), where             # nothing may differ: the mask as a whole
    for b, p in enumerate(prompts):
        n, P, lim = int(wm[b].sum()), len(p), limits[b]
        w = min(lim, gs.shape[1])
        assert w == lim, (where, b)
        assert torch.equal(gm[b, :lim], wm[b, :lim]), (where, b)
        assert gs[b, 1:min(P, n - 1) + 1].tolist() == [int(v) for v in p[:n - 1]], (where, b)                # every forced token
        assert torch.equal(gs[b, :lim], ws[b, :lim]), (where, b, lim, gs[b].tolist(), ws[b].tolist())         # free tokens up to the limit
        err = float((gl[b, :lim].double() - wl[b, :lim].double()).abs().max())
        assert err <= bar, (where, b, err)
        total += max(0, n - 1 - P)
        compared += max(0, lim - 1 - P)
        whole += lim == n
    return compared, total, whole


def _end_to_end(dev, name, cdt):
    """One case: -> (free pairs compared, free pairs, rows comparable to their end, rows) over its prompt sets."""
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    B = lat.shape[0]
    g = _greedy(m, lat, mask, T, bf)
    Ls = (g[2].sum(dim=1) - 1).tolist()
    L = min(Ls)
    with torch.no_grad(), _ctx(bf):
        hs, own_gap = _host_gaps(m, lat, mask, T, [[]] * B)
    assert all(hs[i, :Ls[i] + 1].tolist() == g[0][i, :Ls[i] + 1].tolist() for i in range(B))      # the gaps are those of greedy's own path
    sets = []
    for C in sorted(c for c in {1, 2, L // 2, L - 1} if 1 <= c <= L):          # the model's own output, common depth C, ragged tails
        sets.append((f"own C={C}", [g[0][i, 1:1 + min(Ls[i], C + 2 * i)].clone().cpu() for i in range(B)], own_gap))
    rnd = _random_prompts(m, B, T, seed=61, lens=[T // 3, T // 3 + 2, T - 1][:B])
    with torch.no_grad(), _ctx(bf):
        _, rnd_gap = _host_gaps(m, lat, mask, T, rnd)
    sets.append(("random ids", rnd, rnd_gap))
    compared = total = whole = rows = 0
    eng = m.decoder.decoder_blocks.engine(dev)
    for label, prompts, gap in sets:
        C = min(len(p) for p in prompts)
        want = _greedy(m, lat, mask, T, bf, prefix=prompts)
        before = eng.prefilled_tokens
        got = _greedy(m, lat, mask, T, bf, prefix=prompts, prefill=True)
        assert eng.prefilled_tokens - before == B * C
        c, t, w = _compare(want, got, prompts, gap, bf, (name, label))
        free = [gap[b, len(p) + 1:int(want[2][b].sum())] for b, p in enumerate(prompts)]
        print(f"{name} {'bf16' if bf else 'fp32'} {label}: free pairs compared {c} of {t}; smallest top-1 - top-2 gap per row "
              f"{[round(float(f.min()), 4) if f.numel() else None for f in free]}")
        compared, total, whole, rows = compared + c, total + t, whole + w, rows + B
    assert total > 0
    return compared, total, whole, rows


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_end_to_end_against_the_stepwise_prompt_run(dev, cdt):
    """Every case is checked as far as its gaps allow; how far that must be is a condition on the cases, not on the code: in fp32 every row
    of every case to its end, in bf16 at least half of all free (row, index) pairs, counted over the four cases together (the golden
    fixtures are what they are: vitomr_small's greedy path holds an exact bf16 tie of the top two logits early in row 0, which ends that
    row's comparison for the prompts that stop before it)."""
    tot = [0, 0, 0, 0]
    for name in CASES:
        r = _end_to_end(dev, name, cdt)
        print(f"{name}: compared {r[0]} of {r[1]} free pairs, {r[2]} of {r[3]} rows to their end")
        tot = [a + b for a, b in zip(tot, r)]
    compared, total, whole, rows = tot
    if cdt == torch.bfloat16:
        assert 2 * compared >= total, (compared, total)
    else:
        assert whole == rows and compared == total, (whole, rows, compared, total)


# ---- 5. no-ops ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_prefill_without_a_common_prompt_token_changes_nothing(dev, cdt):
    m, lat, mask, T = _case("vitomr_dh64b", cdt, dev)
    bf = cdt == torch.bfloat16
    eng = m.decoder.decoder_blocks.engine(dev)
    before = eng.prefilled_tokens
    _same(_greedy(m, lat, mask, T, bf), _greedy(m, lat, mask, T, bf, prefill=True))
    prompts = _random_prompts(m, 3, T, seed=71, lens=[5, 0, 9])
    _same(_greedy(m, lat, mask, T, bf, prefix=prompts), _greedy(m, lat, mask, T, bf, prefix=prompts, prefill=True))
    with torch.no_grad(), _ctx(bf):
        one = list(m.streamed_cached_greedy_generate(lat[:1], mask[:1], max_len=T, flush_interval=5, prefill=True))[-1]["payload"]
        ref = list(m.streamed_cached_greedy_generate(lat[:1], mask[:1], max_len=T, flush_interval=5))[-1]["payload"]
    _same((one["sequence"], one["log_probs"], one["mask"]), (ref["sequence"], ref["log_probs"], ref["mask"]))
    assert eng.prefilled_tokens == before


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------------------------
def test_prefill_leaves_other_modes_alone(dev):
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
        with torch.no_grad(), _ctx(True):
            p = m.cached_greedy_generate(mem, mask, max_len=T, prefix=_random_prompts(m, 3, T, seed=9))     # un-prefilled prompt mode
            b = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
            c = m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2)
            sp = m.cached_speculative_generate(mem, mask, max_len=T, draft_len=4)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return g + p + b + c + sp + s

    def prefilled(m, mem, mask):
        prompts, two = _random_prompts(m, 3, T, seed=9, lens=[4, T - 1, 6]), _random_prompts(m, 2, T - 2, seed=10, lens=[3, 2])
        with torch.no_grad(), _ctx(True):
            return m.cached_greedy_generate(mem, mask, max_len=T, prefix=prompts, prefill=True) + \
                m.cached_greedy_generate(mem[:2], mask[:2], max_len=T - 2, prefix=two, prefill=True)

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    m1, mem1, mask1 = setup()
    fresh_prefilled = prefilled(m1, mem1, mask1)
    assert m1.decoder.decoder_blocks.engine(dev).prefilled_tokens == 3 * 4 + 2 * 2
    _same(fresh_others, others(m1, mem1, mask1))           # prefilled runs, then every other mode
    _same(fresh_prefilled, prefilled(m1, mem1, mask1))     # and the reverse, on captured graphs of both
    _same(fresh_prefilled, prefilled(m0, mem0, mask0))
    # graph replay and eager launches, poll = 1 and poll = 16
    eng = m1.decoder.decoder_blocks.engine(dev)
    prompts = _random_prompts(m1, 3, T, seed=9, lens=[4, T - 1, 6])
    mem32, lens = EG.unpad_rows(mem1, mask1)
    for form in (dict(), dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False)):
        with torch.no_grad():
            m1.decoder.decoder_blocks.prepare_caches_packed(mem32, None, lens)
            s, lp, _ = eng.greedy(T, prompt=prompts, prefill=True, **form)
            _same(fresh_prefilled[:3], m1.mask_and_clip_seqs(s.clone(), lp.clone()))


# ---- 7. entry points, refusals, the C ABI's argument checks -----------------------------------------------------------------------------------
def test_entry_points_refusals_and_c_abi_checks(dev):
    from acai_omr_amd import _lib
    from acai_omr_amd.config import InferenceEvent
    from acai_omr_amd.inference.vitomr_inference import inference, streamed_inference
    fx = load_golden("vitomr_dh64b")
    cfg, imgs = fx["cfg"], fx["imgs"]
    T = cfg["max_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
    prompts = _random_prompts(m, 3, T, seed=11, lens=[12, 9, 4])
    batch = inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, prefill=True)
    assert all(batch[0][i, 1:1 + len(p)].tolist() == p.tolist() for i, p in enumerate(prompts))
    eng = m.decoder.decoder_blocks.engine(dev)
    assert eng.prefilled_tokens == 3 * 4
    with pytest.raises(ValueError, match=r"outside \[0, "):       # the engine's own check (the entry points' _check_prefix comes first)
        eng.greedy(T, prompt=[[5, eng.V], [5], [5]], prefill=True)
    for i, img in enumerate(imgs):
        one = inference(m, [img], "cuda", max_inference_len=T, prefix=[prompts[i]], prefill=True)
        ev = list(streamed_inference([img], m, "cuda", max_inference_len=T, flush_interval=5, prefix=[prompts[i]], prefill=True))
        fin = ev[-1]["payload"]
        _same(one, (fin["sequence"], fin["log_probs"], fin["mask"]))
        steps = [e["payload"]["tokens"] for e in ev if e["type"] == InferenceEvent.STEP.value]
        assert len(steps) >= 2
        cat = torch.cat(steps, dim=1)
        assert torch.equal(cat.long(), one[0][:, 1:1 + cat.shape[1]]) and one[0].shape[1] - 1 - cat.shape[1] < 5   # prefilled tokens included
    # refusals, each naming the mode
    with pytest.raises(ValueError, match="speculative"):
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, prefill=True, speculative=3)
    with pytest.raises(ValueError, match="beam"):
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, prefill=True, beam_width=2)
    fx8 = load_golden("vitomr_small")
    m8 = build_vitomr(fx8["cfg"], fx8["state_dict"], dev, torch.bfloat16, max_batch=8, memory_cache_dtype=torch.float8_e4m3fn)
    lat8, mask8 = _memory(m8, fx8["imgs"], True)
    with pytest.raises(ValueError, match="FP8 memory cache"):
        _greedy(m8, lat8, mask8, fx8["cfg"]["gen_len"], True, prefix=_random_prompts(m8, 3, fx8["cfg"]["gen_len"], seed=3, lens=[2, 2, 3]),
                prefill=True)
    # the C ABI: the engine's descriptors as the last prefilled run left them
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, prefill=True)
        d, pr, B, E, C = ctypes.byref(eng._desc), ctypes.byref(eng._prompt_desc), eng.B, eng.E, 4
        qkv = torch.zeros(B * C, 3 * E, dtype=torch.bfloat16, device=dev)
        logits = torch.zeros(B * C, eng.V, device=dev)
        torch.cuda.synchronize()
        state = [t.clone() for t in [eng.step, eng.seqs, eng.logprobs, eng.finished, eng.ws["x"]] + eng.k_self + eng.v_self]
        kv = lambda layer=0, q=qkv.data_ptr(), ld=3 * E, c=C: L.acai_decode_prefill_self_kv(d, layer, q, ld, c, st)   # noqa: E731
        arm = lambda p=pr, lg=logits.data_ptr(), c=C: L.acai_decode_prefill_arm(d, p, lg, c, st)                       # noqa: E731
        for call, msg in ((lambda: kv(q=None), b"null qkv"), (lambda: kv(layer=-1), b"layer"), (lambda: kv(layer=eng.L), b"layer"),
                          (lambda: kv(c=0), b"depth"), (lambda: kv(c=eng.Tmax), b"depth"), (lambda: kv(ld=3 * E - 1), b"below 3E"),
                          (lambda: arm(lg=None), b"null logits"), (lambda: arm(p=None), b"null prompt"), (lambda: arm(c=0), b"depth"),
                          (lambda: arm(c=eng.Tmax), b"depth")):
            assert call() != 0 and msg in L.acai_last_error(), (msg, L.acai_last_error())
        for field, bad, msg in (("tok", None, b"null prompt"), ("len", None, b"null prompt"), ("pitch", eng.Tmax - 1, b"pitch"),
                                ("rows", B - 1, b"rows")):
            keep = getattr(eng._prompt_desc, field)
            setattr(eng._prompt_desc, field, bad)
            try:
                assert arm() != 0 and msg in L.acai_last_error(), (field, L.acai_last_error())
            finally:
                setattr(eng._prompt_desc, field, keep)
        keep = eng._desc.V
        eng._desc.V = 513
        try:
            assert arm() != 0 and b"above 512" in L.acai_last_error()
        finally:
            eng._desc.V = keep
        torch.cuda.synchronize()
        now = [eng.step, eng.seqs, eng.logprobs, eng.finished, eng.ws["x"]] + eng.k_self + eng.v_self
        assert all(torch.equal(a, b) for a, b in zip(state, now))                # errors, not launches
