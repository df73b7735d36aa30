"""Speculative greedy decoding without a GPU: the plain-Python restatement (tests/speculative_reference.py) reproduces plain greedy for every
draft source, its step counts are the ones the design states, and the host-side argument checks raise as documented."""
import ctypes
import math
import os
import random
import re

import pytest
import torch

import speculative_reference as SR
from conftest import ROOT, VOCAB

BOS, EOS, V = 0, 1, 11


def _toy(seed, period=None, eos_at=None):
    """A deterministic next_token(prefix): a hash of the last two tokens (never <eos>), or a periodic pattern; <eos> once the prefix has
    eos_at tokens."""
    def nxt(prefix):
        if eos_at is not None and len(prefix) == eos_at:
            return EOS
        if period is not None:
            return 2 + (len(prefix) % period + seed) % (V - 2)
        h = (prefix[-1] * 31 + (prefix[-2] if len(prefix) > 1 else 7) * 17 + seed * 13 + (len(prefix) // 9)) % (V - 2)
        return 2 + h
    return nxt


def _oracle_table(greedy, max_len):
    return list(greedy) + [SR.NONE] * (max_len - len(greedy))


def _adversarial_table(greedy, max_len):
    return [2 + (tok - 2 + 1) % (V - 2) if tok >= 2 else 2 for tok in greedy] + [3] * (max_len - len(greedy))   # every token changed


CASES = [(seed, period, eos_at, max_len) for seed in (0, 3) for period in (None, 3, 5) for eos_at in (None, 2, 7, 12, 13) for max_len in (2, 3, 9, 14, 24)]


@pytest.mark.parametrize("D", range(1, 8))
def test_restatement_reproduces_greedy_for_every_draft_source(D):
    for seed, period, eos_at, max_len in CASES:
        nxt = _toy(seed, period, eos_at)
        greedy = SR.greedy_decode(nxt, BOS, EOS, max_len)
        T = len(greedy)
        rnd = random.Random(seed * 100 + D)
        half = [tok if rnd.random() < 0.5 else 2 + (tok - 1) % (V - 2) for tok in _oracle_table(greedy, max_len)]
        sources = {"none": SR.no_drafts, "oracle": SR.table_proposals(_oracle_table(greedy, max_len)),
                   "adversarial": SR.table_proposals(_adversarial_table(greedy, max_len)), "half": SR.table_proposals(half),
                   "ngram1": SR.ngram_source(1), "ngram3": SR.ngram_source(3), "ngram8": SR.ngram_source(8)}
        for name, src in sources.items():
            seq, steps, log = SR.speculative_decode(nxt, BOS, EOS, max_len, D, src)
            assert seq == greedy, (name, D, seed, period, eos_at, max_len)
            assert sum(len(w) for _, _, w in log) == T - 1
            if name in ("none", "adversarial"):
                assert steps == T - 1
            if name == "oracle":
                assert steps == math.ceil((T - 1) / (D + 1))
            assert math.ceil((T - 1) / (D + 1)) <= steps <= T - 1


def test_no_accepted_draft_takes_max_len_minus_one_steps():
    for D in (1, 4, 7):
        seq, steps, _ = SR.speculative_decode(_toy(1), BOS, EOS, 24, D, SR.no_drafts)
        assert len(seq) == 24 and steps == 23


def test_ngram_drafter_rule():
    P = SR.ngram_proposals
    assert P([0], 3, 3) == [-1, -1, -1]                       # nothing earlier
    assert P([0, 5, 6, 7, 5, 6], 3, 3) == [7, 5, 6]          # suffix (5, 6) occurred at 1..2: what followed
    assert P([0, 5, 6, 7, 5, 6], 5, 3) == [7, 5, 6, -1, -1]  # only as far as the sequence goes
    assert P([0, 5, 6, 5, 7, 5], 2, 3) == [7, 5]             # most recent earlier occurrence of (5): index 3
    assert P([0, 5, 6, 9, 6], 2, 3) == [9, 6]                # m = 3, 2 fail, m = 1 matches
    assert P([0, 5, 5, 5], 2, 3) == [5, -1]                  # overlapping occurrence: e = 3
    assert P([0, 4, 5, 6], 2, 3) == [-1, -1]
    # a periodic sequence is drafted perfectly once one period is seen
    nxt = _toy(0, period=4)
    seq, steps, log = SR.speculative_decode(nxt, BOS, EOS, 40, 4, SR.ngram_source(3))
    assert seq == SR.greedy_decode(nxt, BOS, EOS, 40) and steps < 20
    assert all(len(w) == 5 for _, _, w in log[8:-1])


def test_struct_and_symbols_match_header():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} AcaiSpec;")):hdr.index("} AcaiSpec;")]
    names = re.findall(r"\b([A-Za-z_]+)\s*;", body)
    assert [f for f, _ in _lib.AcaiSpec._fields_] == names == ["D", "ngram", "pitch", "rows", "t", "cap", "steps", "tab", "next", "drafts"]
    assert ctypes.sizeof(_lib.AcaiSpec) == 4 * 4 + 6 * 8
    for fn in ("acai_decode_spec_step", "acai_decode_spec_arm"):
        assert fn in _lib.exported_symbols() and re.search(r"\b" + fn + r"\s*\(", hdr)


def _cpu_vit(max_batch, memory_cache_dtype=None):
    from acai_omr_amd.models.models import OMRDecoder, ViTOMR
    dec = OMRDecoder(16, VOCAB, num_layers=1, hidden_dim=32, num_heads=2, mlp_dim=64)
    return ViTOMR(None, None, dec.to_cached_version(max_batch, torch.bfloat16, memory_cache_dtype).eval())


def test_host_argument_checks_raise_without_a_gpu():
    m = _cpu_vit(8)
    lat = torch.zeros(2, 4, 32)
    for D in (0, 8, -1):
        with pytest.raises(ValueError, match="draft_len"):
            m.cached_speculative_generate(lat, None, max_len=8, draft_len=D)
    with pytest.raises(ValueError, match="max batch size"):
        m.cached_speculative_generate(lat, None, max_len=8, draft_len=4)      # 2 x 5 rows > 8
    with pytest.raises(ValueError, match="max batch size"):
        _cpu_vit(4).cached_speculative_generate(lat[:1], None, max_len=8, draft_len=4)
    with pytest.raises(ValueError, match="FP8"):
        _cpu_vit(8, torch.float8_e4m3fn).cached_speculative_generate(lat[:1], None, max_len=8, draft_len=2)
    from acai_omr_amd.inference.vitomr_inference import inference
    with pytest.raises(ValueError, match="beam"):
        inference(m, [torch.zeros(1, 32, 32)], "cpu", speculative=2, beam_width=2)
    import inspect
    sig = inspect.signature(inference)
    assert sig.parameters["speculative"].default == 0
