"""The loop guard as far as it can be checked without a device: the rule's brute-force statement (tests/loop_reference.py) pinned on the
committed golden sequences, LoopGuard's validation, the ValueErrors of the combinations that are out of scope, the mask / trim arithmetic,
and the declarations (header, ctypes, sources)."""
import inspect
import os
import re

import pytest
import torch

import loop_reference as LR
from acai_omr_amd.loops import LoopGuard, LoopReport, check_guard, refuse_guard, scan_repeats

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# (stop, period, start) per row, None = no loop; rows of ref_fp32 and ref_bf16 alike
PINNED_3_4_8 = {
    "vitomr_small": [(8, 2, 3), None, None],
    "vitomr_dh64b": [None, None, (7, 2, 2)],
    "vitomr_dh64": [None, None],
    "vitomr_odd": [(5, 1, 1)] * 3,
}
PINNED_2_2_4 = {"vitomr_dh64b": [(4, 1, 2), (7, 1, 5), (5, 2, 2)]}


@pytest.mark.parametrize("precision", ["ref_fp32", "ref_bf16"])
@pytest.mark.parametrize("name", sorted(PINNED_3_4_8))
def test_reference_on_golden_sequences_r3_m4_p8(name, precision):
    rows = LR.golden_rows(name, precision)
    assert [LR.first_loop(r, P=8, R=3, M=4) for r in rows] == PINNED_3_4_8[name]


@pytest.mark.parametrize("precision", ["ref_fp32", "ref_bf16"])
def test_reference_on_golden_sequences_r2_m2_p4(precision):
    rows = LR.golden_rows("vitomr_dh64b", precision)
    assert [LR.first_loop(r, P=4, R=2, M=2) for r in rows] == PINNED_2_2_4["vitomr_dh64b"]


def test_reference_by_hand():
    #       0  1  2  3  4  5  6  7  8
    seq = [0, 5, 6, 7, 5, 6, 7, 5, 6]
    # period 3, R = 2: need 3 - indices 4, 5, 6 repeat 1, 2, 3: fires at 6, the cycle began at index 1
    assert LR.first_loop(seq, P=8, R=2, M=1) == (6, 3, 1)
    assert LR.loop_end(seq, 6, 3) == 8
    assert LR.first_loop(seq, P=2, R=2, M=1) is None                  # no period up to 2
    assert LR.first_loop(seq, P=8, R=2, M=5) == (8, 3, 1)             # min_tokens lifts the need to 5: indices 4 .. 8
    assert LR.first_loop(seq, P=8, R=3, M=1) is None                  # a third copy is not there
    assert LR.first_loop([0, 9, 9], P=4, R=2, M=1) == (2, 1, 1)       # index 0 never takes part: 9 9 is the shortest loop there is
    assert LR.first_loop([9, 9, 3], P=4, R=2, M=1) is None
    # two periods due at the same index: 4 4 4 4 is period 1 (need 3 at R = 2, M = 3) and period 2 (need 3): the smaller wins
    assert LR.first_loop([0, 4, 4, 4, 4], P=8, R=2, M=3) == (4, 1, 1)
    assert LR.run_counters(seq, 8, 64)[:4] == [0, 0, 5, 0]
    assert LR.run_counters(seq, 8, 2) == [0] * 64
    assert LR.decode_stop([0, 5, 5, 2, 2], 4, 2, 1, eos=2) == ("loop", 2, 1, 1)
    assert LR.decode_stop([0, 5, 2, 2, 2], 4, 2, 1, eos=2) == ("eos", 2)
    assert LR.decode_stop([0, 2, 2], 4, 2, 1, eos=2) == ("eos", 1)
    assert LR.decode_stop([0, 5, 6, 7], 4, 2, 1, eos=2, cap=3) == ("cap", 2)
    assert LR.scan_rows([[0, 7, 7, 7, 1], [0, 1, 2, 3, 4]], 4, 2, 1, lens=[5, 5]) == ([2, 0], [1, 0], [1, 0], [3, 0])
    assert LR.scan_rows([[0, 7, 7, 7, 1]], 4, 2, 1, lens=[2]) == ([0], [0], [0], [0])


def test_loop_guard_validation():
    g = LoopGuard(3, 4)
    assert g.params == (64, 3, 4) and g.trim is False and g.need(1) == 4 and g.need(5) == 10
    assert LoopGuard(min_repeats=2, min_tokens=1, max_period=1, trim=True).params == (1, 2, 1)
    p = inspect.signature(LoopGuard).parameters
    assert p["min_repeats"].default is inspect.Parameter.empty and p["min_tokens"].default is inspect.Parameter.empty   # no shipped threshold
    for kw in (dict(min_repeats=1, min_tokens=4), dict(min_repeats=3, min_tokens=0), dict(min_repeats=3, min_tokens=4, max_period=0),
               dict(min_repeats=3, min_tokens=4, max_period=65), dict(min_repeats=1 << 24, min_tokens=4)):
        with pytest.raises(ValueError):
            LoopGuard(**kw)
    for kw in (dict(min_repeats=3.0, min_tokens=4), dict(min_repeats=3, min_tokens=True), dict(min_repeats=3, min_tokens=4, max_period="8")):
        with pytest.raises(TypeError):
            LoopGuard(**kw)
    assert check_guard(None) is None and check_guard(g) is g
    with pytest.raises(TypeError):
        check_guard((3, 4))
    refuse_guard(None, "beam search")
    with pytest.raises(ValueError, match="beam search"):
        refuse_guard(g, "beam search")
    with pytest.raises(TypeError):
        scan_repeats(torch.zeros(1, 4, dtype=torch.int64), (3, 4))
    with pytest.raises(RuntimeError):   # no CPU fallback
        scan_repeats(torch.zeros(1, 4, dtype=torch.int64), g)


def test_mask_and_trim_arithmetic():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    rep = LoopReport(stop=i32(8, 0, 7), period=i32(2, 0, 2), start=i32(3, 0, 2))
    assert rep.looped.tolist() == [True, False, True]
    assert rep.caps([12, 12, 12]) == [9, 12, 8]                 # the token at stop is the row's last: stop + 1 tokens
    assert rep.caps([12, 12, 12], trim=True) == [5, 12, 4]      # one copy of the cycle: through start + period - 1
    assert rep.caps([6, 3, 12]) == [6, 3, 8]                    # never above the row's own cap
    # trim never keeps more than the untrimmed cut: start + period <= stop + 1 because need(p) >= p
    for R in (2, 3, 5):
        for M in (1, 4, 9):
            for p in (1, 2, 7):
                g = LoopGuard(R, M)
                stop = 40
                assert (stop - g.need(p) - p + 1) + p <= stop + 1


def _model_shell():
    from acai_omr_amd.models.models import ViTOMR
    return ViTOMR.__new__(ViTOMR)


def test_combinations_raise_value_error_naming_the_mode():
    from acai_omr_amd.engine import DecodeEngine
    from acai_omr_amd.models.models import ViTOMR
    g = LoopGuard(3, 4)
    for what in ("prefix (prompted decoding)", "grammar (constrained decoding)", "prefill (prompt prefill)", "sample (sampled rollouts)"):
        with pytest.raises(ValueError, match=re.escape(what)):
            ViTOMR._check_loop_guard(g, **{what: object()})
        assert ViTOMR._check_loop_guard(g, **{what: None}) is g
        assert ViTOMR._check_loop_guard(None, **{what: object()}) is None
    assert ViTOMR._check_loop_guard(g, **{"prefill (prompt prefill)": False}) is g
    with pytest.raises(TypeError):
        ViTOMR._check_loop_guard((3, 4))
    m = _model_shell()
    lat = torch.zeros(1, 2, 4)
    for call, mode in ((lambda: m.cached_beam_generate(lat, loop_guard=g), "beam search"),
                       (lambda: m.cached_speculative_generate(lat, loop_guard=g), "speculative decoding"),
                       (lambda: m.streamed_continuous_generate(lat, loop_guard=g), "streamed"),
                       (lambda: next(m.streamed_cached_greedy_generate(lat, loop_guard=g)), "streamed")):
        with pytest.raises(ValueError, match=mode):
            call()
    for fn in (DecodeEngine.greedy, DecodeEngine.greedy_chunks, DecodeEngine.continuous, ViTOMR.cached_greedy_generate,
               ViTOMR.cached_continuous_generate):
        p = inspect.signature(fn).parameters["loop_guard"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn


def test_inference_entry_points_take_loop_guard_keyword_only():
    from acai_omr_amd.inference import vitomr_inference as VI
    from acai_omr_amd.page import PageResult
    for fn in (VI.inference, VI.continuous_inference, VI.iter_continuous_inference, VI.page_inference):
        p = inspect.signature(fn).parameters["loop_guard"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert inspect.signature(PageResult.__init__).parameters["loops"].default is None


def test_declared_built_and_documented():
    from acai_omr_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for name in ("acai_decode_loop_step", "acai_decode_slot_loop_step", "acai_debug_decode_loop_select", "acai_repeat_scan"):
        assert re.search(r"int " + name + r"\(", hdr), name
        assert name in _lib._SIGNATURES, name
    m = re.search(r"int acai_repeat_scan\(([^;]*)\);", hdr)
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["tokens", "lens", "N", "ld", "max_period", "min_repeats", "min_tokens", "stop", "period", "start", "end", "stream"]
    assert len(_lib._SIGNATURES["acai_repeat_scan"][1]) == len(params)
    fields = re.search(r"typedef struct \{([^}]*)\} AcaiLoop;", hdr).group(1)
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in fields.strip().splitlines()]
    assert names == [f for f, _ in _lib.AcaiLoop._fields_]
    assert "loops.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "loops.hip"))
    assert callable(ops.repeat_scan) and callable(ops.debug_decode_loop_select)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "loop guard" in open(os.path.join(ROOT, doc)).read().lower(), doc
