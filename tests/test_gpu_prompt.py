"""Prompted decoding on the GPU (acai_decode_prompt_step / acai_decode_spec_prompt_step through DecodeEngine.greedy(prompt=) /
speculative(prompt=), ViTOMR.cached_greedy_generate(prefix=) / cached_speculative_generate(prefix=), inference(prefix=) and
streamed_inference(prefix=)).

Shapes: the golden fixtures vitomr_small, vitomr_dh64b, vitomr_odd (three images each, the generic GEMV path) and the random decoder
decode_support._decoder(T=48, L=2, E=1024, H=16, Fd=4096) on memories of 40, 17 and 64 rows (the chain-GEMV / fused-LayerNorm path), whose
<eos> logit is biased so that one greedy row ends before max_len.

Bars:
  1. the model's own greedy output as the prompt, split at P in {0, 1, 2, L // 2, L - 1, L} mixed over the rows: seqs, log-probs and mask
     torch.equal to greedy's (a forced arg-max has the greedy step's log-prob bit for bit);
  2. random forced ids against the host-stepped path (cached_set_up_inference + decoder.cached_generate fed the forced tokens, arg-max after
     the prompt, float64 log_softmax of its logits): tokens equal; log-probs fp32 within 1e-5 * max(1, |lp|), bf16 equal to the float64 value
     rounded to bf16 or its bf16 neighbour;
  3. a prompt-final <eos> and a full-length prompt end the row, and the batch exits once every row is done;
  4. speculative prompt mode, D in {1, 4, 7}: torch.equal to prompt mode, verify steps equal to the restatement's (tests/prompt_reference.py);
  5. FP8 memory cache: tokens equal to the host-stepped FP8 path's;
  6. a prompt run leaves greedy, sampling, beam, slot and speculative decoding as on a fresh engine; graph replay == eager launches;
  7. inference(prefix=) == streamed_inference(prefix=); the C ABI's argument checks return errors."""
import ctypes

import pytest
import torch
from torch.amp import autocast

import prompt_reference as PR
import speculative_reference as SR
from conftest import load_golden
from decode_support import _decoder, _memory, _same, _vit, build_vitomr, dev  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURES = ["vitomr_small", "vitomr_dh64b", "vitomr_odd"]
CASES = FIXTURES + ["random"]
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]
RAND_T, RAND_LENS = 48, [40, 17, 64]
_CACHE = {}


def _ctx(bf):
    return autocast(device_type="cuda", dtype=torch.bfloat16, enabled=bf)


def _host_stepped(m, lat, mask, T, prompts):
    """The path that exists without the feature: one decoder.cached_generate call per token, fed the forced tokens, arg-max (first index,
    taken on the CPU) after the prompt.  -> seqs (B, T) int64 with every index written, float64 log_softmax of the chosen token (B, T),
    the arg-max at every index (B, T), and max logit - <eos> logit (B, T).  All on the CPU."""
    B = lat.shape[0]
    eos = m.decoder.eos_idx
    seqs, _, _ = m.cached_set_up_inference(lat, T)
    lp = torch.zeros(B, T, dtype=torch.float64)
    am = torch.zeros(B, T, dtype=torch.int64)
    gap = torch.zeros(B, T, dtype=torch.float64)
    for t in range(1, T):
        lg = m.decoder.cached_generate(seqs[:, t - 1].unsqueeze(1), t, mask).squeeze(1).double().cpu()
        am[:, t] = torch.argmax(lg, dim=-1)
        tok = am[:, t].clone()
        for i, p in enumerate(prompts):
            if t <= len(p):
                tok[i] = int(p[t - 1])
        lp[:, t] = torch.log_softmax(lg, dim=-1).gather(1, tok.unsqueeze(1)).squeeze(1)
        gap[:, t] = lg.max(dim=-1).values - lg[:, eos]
        seqs[:, t] = tok.to(seqs.device)
    return seqs.cpu(), lp, am, gap


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
        # bias the <eos> logit so that exactly one row's greedy run ends before max_len: along the unbiased greedy path <eos> first wins
        # where its distance to the row maximum drops below the bias (earlier tokens do not depend on the <eos> logit), so a bias half way
        # between the two smallest per-row minima of that distance ends the one row and no other
        with torch.no_grad(), _ctx(bf):
            _, _, _, gap = _host_stepped(_vit(dec, 24, cdt, dev), lat, mask, RAND_T, [[]] * len(RAND_LENS))
        lo = gap[:, 1:RAND_T - 1].min(dim=1).values.sort().values
        print(f"random decoder {'bf16' if bf else 'fp32'}: per-row minimum of max logit - <eos> logit {lo.tolist()}")
        with torch.no_grad():
            dec.unembed.bias[dec.eos_idx] += float(lo[0] + lo[1]) / 2
        out = (_vit(dec, 24, cdt, dev), lat, mask, RAND_T)
    _CACHE[key] = out
    return out


def _greedy(m, lat, mask, T, bf, **kw):
    with torch.no_grad(), _ctx(bf):
        return m.cached_greedy_generate(lat, mask, max_len=T, **kw)


def _spec_run(m, lat, mask, T, bf, D, prefix, **kw):
    """cached_speculative_generate(prefix=), or with kw (poll, use_graph) the packed form under it -> the triple and the verify steps per
    image."""
    from acai_omr_amd import engine as EG
    with torch.no_grad(), _ctx(bf):
        if kw:
            mem32, lens = EG.unpad_rows(lat, mask)
            out = m._speculative_packed(mem32, None, lens, T, D, prefix=prefix, **kw)
        else:
            out = m.cached_speculative_generate(lat, mask, max_len=T, draft_len=D, prefix=prefix)
    return out, m.decoder.decoder_blocks.engine(lat.device).spec_steps[:lat.shape[0]].tolist()


def _restated_steps(out, prompts, T, D, m, ngram=3):
    """Verify steps of the restatement per image when the token stream is the run's own result."""
    seqs, _, mk = out
    steps = []
    for i, p in enumerate(prompts):
        toks = seqs[i, :int(mk[i].sum())].tolist()
        nxt = lambda prefix, toks=toks: toks[len(prefix)] if len(prefix) < len(toks) else m.decoder.eos_idx   # noqa: E731
        seq, st, _ = SR.speculative_decode(nxt, toks[0], m.decoder.eos_idx, T, D, PR.prompt_source([int(v) for v in p], SR.ngram_source(ngram)))
        assert seq == toks
        steps.append(st)
    return steps


def _splits(L):
    return [0, 1, 2, L // 2, L - 1, L]


def _own_prompts(g, k):
    """Prompts cut from a greedy result, a different split per row: row i at _splits(L_i)[(k + i) % 6]."""
    seqs, _, mk = g
    Ls = (mk.sum(dim=1) - 1).tolist()   # tokens after <bos>, a final <eos> included
    return [seqs[i, 1:1 + min(max(0, _splits(L)[(k + i) % 6]), L)].clone() for i, L in enumerate(Ls)], Ls


def _random_prompts(m, B, T, seed, lens=None):
    """Seeded random ids without the specials: row 0 none, row 1 max_len - 1, the rest in between."""
    dec = m.decoder
    ok = torch.tensor([i for i in range(dec.vocab_size) if i not in (dec.bos_idx, dec.pad_idx, dec.eos_idx)])
    g = torch.Generator().manual_seed(seed)
    lens = lens or [0, T - 1] + [max(1, T // 3 + i) for i in range(B - 2)]
    return [ok[torch.randint(len(ok), (n,), generator=g)] for n in lens[:B]]


# ---- 1. the model's own output as the prompt ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_replays_greedy_bit_for_bit(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    g = _greedy(m, lat, mask, T, bf)
    _, Ls = _own_prompts(g, 0)
    assert max(Ls) >= 8, Ls
    if name == "random":   # a row that ends in <eos> before max_len
        assert any((g[0][i] == m.decoder.eos_idx).any().item() and L < T - 1 for i, L in enumerate(Ls)), Ls
    for k in range(6):
        prompts, _ = _own_prompts(g, k)
        p = _greedy(m, lat, mask, T, bf, prefix=prompts)
        where = (name, k, [len(x) for x in prompts], Ls)
        assert torch.equal(p[0], g[0]) and torch.equal(p[2], g[2]), where
        assert torch.equal(p[1], g[1]), (where, float((p[1] - g[1]).abs().max()))
    _same(g, _greedy(m, lat, mask, T, bf, prefix=[[] for _ in Ls]))   # P = 0 everywhere, through the prompt kernel
    _same(g, _greedy(m, lat, mask, T, bf))                            # and greedy after prompt runs
    print(f"{name} {'bf16' if bf else 'fp32'}: greedy lengths {Ls}")


# ---- 2. tokens the model would not choose ---------------------------------------------------------------------------------------------------
def _check_against_host(m, lat, mask, T, bf, prompts, out, tokens_only=False):
    with torch.no_grad(), _ctx(bf):
        rs, rlp, am, _ = _host_stepped(m, lat, mask, T, prompts)
    rmask = m.create_inference_mask(rs)
    n = int(rmask.sum(dim=-1).max())
    seqs, lps, mk = (x.cpu() for x in out)
    assert seqs.shape[1] == n and torch.equal(mk, rmask[:, :n])
    assert torch.equal(seqs, rs.masked_fill(~rmask, m.decoder.pad_idx)[:, :n])
    forced = torch.zeros_like(rmask)
    for i, p in enumerate(prompts):
        forced[i, 1:1 + len(p)] = True
    forced &= rmask
    differ = int((forced & (rs != am)).sum())
    assert 2 * differ >= int(forced.sum()) > 0, (differ, int(forced.sum()))   # on the reference alone: the prompts do force something
    if tokens_only:
        return
    live = rmask[:, :n].clone()
    live[:, 0] = False
    want, got = rlp[:, :n][live], lps[live]
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
    assert bool((lps[~mk.cpu()] == 0).all())


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_forces_tokens_the_model_would_not_choose(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    prompts = _random_prompts(m, lat.shape[0], T, seed=31)
    assert len(prompts[0]) == 0 and len(prompts[1]) == T - 1
    _check_against_host(m, lat, mask, T, bf, prompts, _greedy(m, lat, mask, T, bf, prefix=prompts))


# ---- 3. prompt-final <eos>, a full-length prompt ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_prompt_final_eos_and_full_length_prompt(dev, cdt):
    m, lat, mask, T = _case("vitomr_dh64b", cdt, dev)
    bf = cdt == torch.bfloat16
    dec = m.decoder
    eos, pad, bos = dec.eos_idx, dec.pad_idx, dec.bos_idx
    a, b, c = (int(v) for v in _random_prompts(m, 3, T, seed=5, lens=[0, 3, 0])[1])
    prompts = [[a, b, eos], [c, eos], [eos]]
    s, lp, mk = _greedy(m, lat, mask, T, bf, prefix=prompts)
    assert s.tolist() == [[bos, a, b, eos], [bos, c, eos, pad], [bos, eos, pad, pad]]
    assert mk.tolist() == [[True] * 4, [True] * 3 + [False], [True] * 2 + [False] * 2]
    assert bool((lp[~mk] == 0).all()) and bool((lp[:, 1:][mk[:, 1:]] < 0).all())
    _check_against_host(m, lat, mask, T, bf, prompts, (s, lp, mk), tokens_only=True)
    # the batch exits as soon as every row is done: three steps, and the longest row has nothing after its <eos>
    eng = dec.decoder_blocks.engine(dev)
    with torch.no_grad(), _ctx(bf):
        _, _, done = eng.greedy(T, poll=1, prompt=prompts)
    assert done == 3 and int(eng.finished[eng.B]) == 0
    assert eng.seqs[0, :T].tolist() == [bos, a, b, eos] + [pad] * (T - 4)
    # one row inside a longer prompt keeps the batch going although the others are done
    long = [int(v) for v in _random_prompts(m, 3, T, seed=6, lens=[0, 0, 7])[2]]
    with torch.no_grad(), _ctx(bf):
        _, _, done = eng.greedy(T, poll=1, prompt=[[eos], [c, eos], long + [eos]])
    assert done == 8
    # a full-length prompt: every index is forced, nothing is free
    full = _random_prompts(m, 3, T, seed=7, lens=[T - 1, T - 1, T - 2])
    full[2] = torch.cat([full[2], torch.tensor([eos])])
    s, lp, mk = _greedy(m, lat, mask, T, bf, prefix=full)
    assert s.shape == (3, T) and bool(mk.all())
    assert all(s[i, 1:].tolist() == full[i].tolist() for i in range(3)) and bool((s[:, 0] == bos).all())
    _check_against_host(m, lat, mask, T, bf, full, (s, lp, mk))


# ---- 4. speculative prompt mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_speculative_prompt_mode(dev, name, cdt):
    m, lat, mask, T = _case(name, cdt, dev)
    bf = cdt == torch.bfloat16
    B, eos = lat.shape[0], m.decoder.eos_idx
    g = _greedy(m, lat, mask, T, bf)
    sets = [_own_prompts(g, k)[0] for k in (1, 3, 5)]           # case 1: every split appears in some row
    sets.append(_random_prompts(m, B, T, seed=31))              # case 2
    mid = _random_prompts(m, B, T, seed=32, lens=[5, 0, 10])    # a prompt-final <eos> inside an accepted run (D = 7), one ending mid-step
    mid[0] = torch.cat([mid[0], torch.tensor([eos])])
    sets.append(mid)
    for prompts in sets:
        want = _greedy(m, lat, mask, T, bf, prefix=prompts)
        for D in (1, 4, 7):
            got, steps = _spec_run(m, lat, mask, T, bf, D, prompts)
            where = (name, D, [len(p) for p in prompts])
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), where
            assert torch.equal(got[1], want[1]), (where, float((got[1] - want[1]).abs().max()))
            assert steps == _restated_steps(want, prompts, T, D, m), where
            for i, p in enumerate(prompts):   # the prompt and the first free token: ceil((P + 1) / (D + 1)) steps, or the whole run
                Tn = int(want[2][i].sum())
                assert steps[i] >= min(PR.verify_steps(len(p), D), -(-(Tn - 1) // (D + 1))), where
                if len(p) + 1 >= Tn - 1:
                    assert steps[i] == -(-(Tn - 1) // (D + 1)), (where, i)
    got, steps = _spec_run(m, lat, mask, T, bf, 4, sets[3], poll=1, use_graph=False)
    _same(_greedy(m, lat, mask, T, bf, prefix=sets[3]), got)
    with torch.no_grad(), _ctx(bf):   # unprompted speculative decoding after the prompted runs
        _same(g, m.cached_speculative_generate(lat, mask, max_len=T, draft_len=4))


# ---- 5. FP8 memory cache -------------------------------------------------------------------------------------------------------------------
def test_fp8_memory_cache(dev):
    fx = load_golden("vitomr_small")
    T = fx["cfg"]["gen_len"]
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16, max_batch=8, memory_cache_dtype=torch.float8_e4m3fn)
    lat, mask = _memory(m, fx["imgs"], True)
    prompts = _random_prompts(m, 3, T, seed=41)
    out = _greedy(m, lat, mask, T, True, prefix=prompts)
    assert m.decoder.decoder_blocks.engine(dev).cross_fp8
    _check_against_host(m, lat, mask, T, True, prompts, out, tokens_only=True)
    g = _greedy(m, lat, mask, T, True)
    _same(g, _greedy(m, lat, mask, T, True, prefix=_own_prompts(g, 3)[0]))
    with torch.no_grad(), pytest.raises(ValueError, match="FP8"):
        m.cached_speculative_generate(lat[:1], mask[:1], max_len=T, draft_len=2, prefix=prompts[:1])


# ---- 6. isolation ----------------------------------------------------------------------------------------------------------------------------
def test_prompt_mode_leaves_other_modes_alone(dev):
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
            b = m.cached_beam_generate(mem, mask, beam_width=4, max_len=T)
            c = m.cached_continuous_generate(mem, mask, max_len=[T, T - 3, 5], slots=2)
            sp = m.cached_speculative_generate(mem, mask, max_len=T, draft_len=4)
        blocks = m.decoder.decoder_blocks
        mem32, lens = EG.unpad_rows(mem, mask)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=2)
        s = tuple(x.clone() for x in blocks.engine(dev).sample(T, 5, 1.3, uniforms=u)[:2])
        return g + b + c + sp + s

    def prompted(m, mem, mask):
        prompts, two = _random_prompts(m, 3, T, seed=9), _random_prompts(m, 2, T - 2, seed=10)
        with torch.no_grad(), _ctx(True):
            return m.cached_greedy_generate(mem, mask, max_len=T, prefix=prompts) + \
                m.cached_speculative_generate(mem, mask, max_len=T, draft_len=4, prefix=prompts) + \
                m.cached_greedy_generate(mem[:2], mask[:2], max_len=T - 2, prefix=two)

    m0, mem0, mask0 = setup()
    fresh_others = others(m0, mem0, mask0)
    m1, mem1, mask1 = setup()
    fresh_prompted = prompted(m1, mem1, mask1)
    _same(fresh_others, others(m1, mem1, mask1))         # prompt runs, then greedy / beam / slot / speculative / sampling
    _same(fresh_prompted, prompted(m1, mem1, mask1))     # and the reverse, on captured graphs of both
    _same(fresh_prompted, prompted(m0, mem0, mask0))
    # graph replay and eager launches
    eng = m1.decoder.decoder_blocks.engine(dev)
    prompts = _random_prompts(m1, 3, T, seed=9)
    mem32, lens = EG.unpad_rows(mem1, mask1)
    runs = []
    for form in (dict(), dict(use_graph=False), dict(poll=1), dict(poll=1, use_graph=False)):
        with torch.no_grad():
            m1.decoder.decoder_blocks.prepare_caches_packed(mem32, None, lens)
            s, lp, _ = eng.greedy(T, prompt=prompts, **form)
            runs.append(m1.mask_and_clip_seqs(s.clone(), lp.clone()))
    for r in runs:
        _same(fresh_prompted[:3], r)


# ---- 7. entry points and the C ABI's argument checks ----------------------------------------------------------------------------------------
def test_entry_points_and_c_abi_checks(dev):
    from acai_omr_amd import _lib
    from acai_omr_amd.config import InferenceEvent
    from acai_omr_amd.inference.vitomr_inference import inference, streamed_inference
    fx = load_golden("vitomr_dh64b")
    cfg, imgs = fx["cfg"], fx["imgs"]
    T = cfg["max_len"]
    m = build_vitomr(cfg, fx["state_dict"], dev, torch.bfloat16, max_batch=16)
    prompts = _random_prompts(m, 3, T, seed=11, lens=[0, 9, 4])
    batch = inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts)
    assert all(batch[0][i, 1:1 + len(p)].tolist() == p.tolist() for i, p in enumerate(prompts))
    _same(batch, inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, speculative=3))
    _same(inference(m, imgs, "cuda", max_inference_len=T), inference(m, imgs, "cuda", max_inference_len=T, prefix=None))
    for i, img in enumerate(imgs):
        one = inference(m, [img], "cuda", max_inference_len=T, prefix=[prompts[i]])
        _same(one, inference(m, img, "cuda", max_inference_len=T, prefix=prompts[i]))   # a single 1-D tensor for one image
        ev = list(streamed_inference([img], m, "cuda", max_inference_len=T, flush_interval=5, prefix=[prompts[i]]))
        fin = ev[-1]["payload"]
        _same(one, (fin["sequence"], fin["log_probs"], fin["mask"]))
        steps = [e["payload"]["tokens"] for e in ev if e["type"] == InferenceEvent.STEP.value]
        assert len(steps) >= 2
        cat = torch.cat(steps, dim=1)
        assert torch.equal(cat.long(), one[0][:, 1:1 + cat.shape[1]]) and one[0].shape[1] - 1 - cat.shape[1] < 5   # forced tokens included
    with pytest.raises(ValueError, match="beam"):
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, beam_width=2)
    with pytest.raises(ValueError, match="entries for 3 images"):
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts[:2])
    # the C ABI: the engine's descriptors as the last prompted runs left them
    eng = m.decoder.decoder_blocks.engine(dev)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts)
        d, pr = ctypes.byref(eng._desc), ctypes.byref(eng._prompt_desc)
        step_before = eng.step.tolist()
        for field, bad, msg in (("tok", None, b"null prompt"), ("len", None, b"null prompt"), ("pitch", eng.Tmax - 1, b"pitch"),
                                ("rows", eng.B - 1, b"rows")):
            keep = getattr(eng._prompt_desc, field)
            setattr(eng._prompt_desc, field, bad)
            try:
                assert L.acai_decode_prompt_step(d, pr, st) != 0 and msg in L.acai_last_error(), (field, L.acai_last_error())
            finally:
                setattr(eng._prompt_desc, field, keep)
        assert L.acai_decode_prompt_step(d, None, st) != 0 and b"null prompt" in L.acai_last_error()
        torch.cuda.synchronize()
        assert eng.step.tolist() == step_before                                # errors, not launches
        eng.logits_step(torch.zeros(eng.B, dtype=torch.int64, device=dev), 1)   # overwrites x
        assert L.acai_decode_prompt_step(d, pr, st) != 0 and b"x does not hold" in L.acai_last_error()
        inference(m, imgs, "cuda", max_inference_len=T, prefix=prompts, speculative=3)
        d, sp = ctypes.byref(eng._desc), ctypes.byref(eng._spec_desc)
        n = eng.B // 4
        for fn in (L.acai_decode_spec_prompt_arm, L.acai_decode_spec_prompt_step):
            for field, bad, msg in (("tok", None, b"null prompt"), ("pitch", eng.Tmax - 1, b"pitch"), ("rows", n - 1, b"rows")):
                keep = getattr(eng._prompt_desc, field)
                setattr(eng._prompt_desc, field, bad)
                try:
                    assert fn(d, sp, pr, st) != 0 and msg in L.acai_last_error(), (field, L.acai_last_error())
                finally:
                    setattr(eng._prompt_desc, field, keep)
            assert fn(d, sp, None, st) != 0 and b"null prompt" in L.acai_last_error()
        torch.cuda.synchronize()
