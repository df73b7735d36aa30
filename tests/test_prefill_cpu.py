"""Prompt prefill without a GPU: the torch restatement (tests/prefill_reference.py) against the plain-Python prompt steps
(tests/prompt_reference.py) run C steps on the same logits, the scatter's index map written out by hand, the ValueErrors that need no
device, and the C ABI declarations against the ctypes mirror."""
import re
import os
import types

import pytest
import torch

import prefill_reference as FR
import prompt_reference as PR
from conftest import ROOT, VOCAB

BOS, PAD, EOS, V = 0, 2, 1, 13


def _prompts(C, kind):
    if kind == "ragged":
        return [[3 + (i * 5) % 9 for i in range(C)], [4 + (i * 3) % 8 for i in range(C + 3)], [5 + i % 7 for i in range(C + 1)]]
    if kind == "eos_at_C":
        return [[3 + i % 9 for i in range(C - 1)] + [EOS], [4 + i % 8 for i in range(C + 2)], [6 + i % 5 for i in range(C)]]
    return [[3 + i % 9 for i in range(C - 1)] + [EOS], [7 + i % 4 for i in range(C - 1)] + [EOS]]   # every row ends at C


@pytest.mark.parametrize("kind", ["ragged", "eos_at_C", "all_done"])
@pytest.mark.parametrize("C", [1, 2, 7, 15])
def test_arm_state_is_what_C_prompt_steps_leave(C, kind):
    max_len, E = 16, 8
    prompts = _prompts(C, kind)
    B = len(prompts)
    g = torch.Generator().manual_seed(100 * C + len(kind))
    logits = torch.randn(B * C, V, generator=g, dtype=torch.float64) * 3
    emb, pos = torch.randn(V, E, generator=g), torch.randn(max_len, E, generator=g)
    x0 = torch.randn(B, E, generator=g)
    st = FR.arm_state(logits, prompts, C, BOS, PAD, EOS, max_len, emb, pos, x0)
    # the prompt steps of the restatement, stopped after index C (max_len = C + 1), reading the pass's logits row by row
    rows, counts = PR.batch_decode(lambda i, seq: logits[i * C + len(seq) - 1].tolist(), BOS, EOS, C + 1, prompts)
    assert len(counts) == C
    for b, (seq, lps) in enumerate(rows):
        assert st["seqs"][b, :C + 1].tolist() == seq and st["seqs"][b, C + 1:].tolist() == [PAD] * (max_len - C - 1)
        assert torch.allclose(st["logprobs"][b, :C + 1], torch.tensor(lps, dtype=torch.float64), atol=1e-12, rtol=0)
        assert bool((st["logprobs"][b, C + 1:] == 0).all())
        assert int(st["finished"][b]) == int(EOS in seq)
    assert int(st["finished"][B]) == counts[-1]
    assert (counts[-1] == 0) == (kind == "all_done")
    assert st["step"] == [C + 1, C]
    if C + 1 < max_len:
        assert torch.equal(st["x"], torch.stack([emb[rows[b][0][C]] + pos[C + 1] for b in range(B)]))
    else:
        assert torch.equal(st["x"], x0)     # index max_len - 1 was the last: no position max_len to embed with


def test_scatter_index_map():
    B, Bmax, C, H, dh, dhp, Tmax = 2, 3, 3, 2, 3, 4, 5
    E = H * dh
    qkv = torch.arange(B * C * 3 * E, dtype=torch.float32).reshape(B * C, 3 * E)
    k0, v0 = torch.full((Bmax, H, Tmax, dhp), -1.0), torch.full((Bmax, H, Tmax, dhp), -2.0)
    k, v = FR.scatter(k0, v0, qkv, B, C, E, H, dh)
    kf, vf = k.reshape(-1), v.reshape(-1)
    written = torch.zeros(Bmax * H * Tmax * dhp, dtype=torch.bool)
    for b in range(B):
        for h in range(H):
            for p in range(C):
                for d in range(dh):
                    at = ((b * H + h) * Tmax + p) * dhp + d
                    assert kf[at] == qkv.reshape(-1)[(b * C + p) * 3 * E + E + h * dh + d]
                    assert vf[at] == qkv.reshape(-1)[(b * C + p) * 3 * E + 2 * E + h * dh + d]
                    written[at] = True
    assert bool((kf[~written] == -1).all()) and bool((vf[~written] == -2).all())      # positions >= C, pad columns, rows >= B
    assert torch.equal(k0, torch.full_like(k0, -1.0))                                  # the inputs are left alone


def _cpu_vit(max_batch, memory_cache_dtype=None):
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    dec = OMRDecoder(16, VOCAB, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64)
    return ViTOMR(None, None, dec.to_cached_version(max_batch, torch.bfloat16, memory_cache_dtype=memory_cache_dtype).eval())


def test_refusals_that_need_no_gpu():
    from acai_omr_amd.engine import DecodeEngine
    from acai_omr_amd.inference import vitomr_inference as VI
    m = _cpu_vit(8)
    dec = m.decoder
    ok = next(i for i in range(dec.vocab_size) if i not in (dec.bos_idx, dec.pad_idx, dec.eos_idx))
    lat = torch.zeros(2, 4, 32)
    for call, mode in ((lambda: VI.inference(m, None, "cuda", max_inference_len=8, prefix=[[ok]], prefill=True, speculative=3), "speculative"),
                       (lambda: VI.inference(m, None, "cuda", max_inference_len=8, prefill=True, beam_width=2), "beam search"),
                       (lambda: VI._check_decode_kwargs("aligned_inference", dict(prefix=[[ok]], prefill=True, speculative=2)), "speculative"),
                       (lambda: VI._check_decode_kwargs("confident_inference", dict(prefill=True, beam_width=3)), "beam search")):
        with pytest.raises(ValueError, match=r"prefill \(prompt prefill\) cannot be combined with " + mode):
            call()
    VI._check_decode_kwargs("diagnosed_inference", dict(prefix=[[ok]], prefill=True))       # on the allow-list
    with pytest.raises(TypeError, match="unexpected decode arguments"):
        VI._check_decode_kwargs("diagnosed_inference", dict(prefil=True))
    from acai_omr_amd.grammar import TokenAutomaton
    gram = TokenAutomaton.__new__(TokenAutomaton)       # refused by name before anything looks inside it
    for call in (lambda: VI.inference(m, None, "cuda", max_inference_len=8, prefill=True, grammar=gram),
                 lambda: m.cached_greedy_generate(lat, None, max_len=8, prefill=True, grammar=gram),
                 lambda: next(m.streamed_cached_greedy_generate(lat[:1], None, max_len=8, prefill=True, grammar=gram))):
        with pytest.raises(ValueError, match=r"prefill \(prompt prefill\) cannot be combined with grammar"):
            call()
    # the prefix is validated as without prefill, before anything reaches the device
    with pytest.raises(ValueError, match="outside"):
        m.cached_greedy_generate(lat, None, max_len=8, prefix=[[ok], [dec.vocab_size]], prefill=True)
    with pytest.raises(ValueError, match="entries for 2 images"):
        m.cached_greedy_generate(lat, None, max_len=8, prefix=[[ok]], prefill=True)
    # continuous batching and beam search take no prefix, with or without prefill
    with pytest.raises(ValueError, match="out of scope here"):
        m.cached_continuous_generate(lat, None, max_len=8, prefix=[[ok], [ok]])
    # the engine's own plan: what a prefilled run cannot do, and when there is nothing to prefill
    plan = DecodeEngine._prefill_plan
    eng = types.SimpleNamespace(cross_fp8=False, B=2, group=1, omr=dec, _mem=(lat, None), V=dec.vocab_size)
    eos = dec.eos_idx
    assert plan(eng, [[ok, ok, ok], [ok, ok]], 8) == (2, True)
    assert plan(eng, [torch.tensor([ok, eos]), [ok, ok]], 8) == (2, True)
    assert plan(eng, [[ok, eos], [ok, ok, eos]], 8) == (2, True)         # a row inside its prompt is live
    assert plan(eng, [[ok, eos], [ok, eos]], 8) == (2, False)            # every prompt ends at C with <eos>: no step is left
    assert plan(eng, [[ok], []], 8) is None                              # an empty prompt: the plain prompt run
    assert plan(eng, [[ok]], 8) is None and plan(eng, [[ok] * 8, [ok]], 8) is None   # left to _set_prompt's errors
    for bad in ([[ok, dec.vocab_size], [ok]], [[ok], [-1, ok]]):
        with pytest.raises(ValueError, match=r"outside \[0, "):
            plan(eng, bad, 8)
    eng.cross_fp8 = True
    with pytest.raises(ValueError, match="FP8 memory cache"):
        plan(eng, [[ok], [ok]], 8)
    eng.cross_fp8, eng.group = False, 2
    with pytest.raises(ValueError, match="one memory per row"):
        plan(eng, [[ok], [ok]], 8)
    eng.group, eng.V = 1, 513
    with pytest.raises(ValueError, match="at most 512"):
        plan(eng, [[ok], [ok]], 8)


def test_symbols_match_header_and_sources():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for fn, nargs in (("acai_decode_prefill_self_kv", 6), ("acai_decode_prefill_arm", 5)):
        m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and fn in _lib.exported_symbols()
        res, args = _lib._SIGNATURES[fn]
        assert len(m.group(1).split(",")) == len(args) == nargs
        src = open(os.path.join(_lib.CSRC, "decode.hip")).read()
        assert re.search(r'extern "C" int ' + fn + r"\(", src)
    assert "decode_prefill.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "decode_prefill.hip"))
    internal = open(os.path.join(_lib.CSRC, "decode_internal.h")).read()
    assert "launch_prefill_self_kv(" in internal and "launch_prefill_arm(" in internal
    assert "AcaiPrefill" not in hdr      # plain arguments and AcaiPrompt: no new struct
