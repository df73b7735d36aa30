"""Page assessment without a GPU: the numpy restatement (tests/assess_reference.py) on pages whose answer is known, the host rule
`page.choose_staff_scale`, the `AssessConfig` gate, and `DetectConfig.resolved` sized from a staff space."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import assess_reference as A
import page_reference as R

DENSE = dict(seed=1, H=1600, W=200, systems_at=tuple((60 + 60 * i, 1) for i in range(24)))   # 24 one-staff systems, 3 rows from line to line


def _scale(s):
    return None if s is None else dict(line=s.line, space=s.space, pitch_bin=s.pitch_bin, pitch=s.pitch, confidence=s.confidence)


def test_restatement_reads_the_synthetic_page():
    from acai_omr_amd.page import choose_staff_scale
    hists = A.runs(R.synthetic_page()[0])
    want = A.choose_staff_scale(hists)
    assert (want["line"], want["space"], want["pitch_bin"]) == (1, 2, 3) and want["pitch"] == pytest.approx(3.0, abs=0.05)
    assert want["confidence"] == pytest.approx(0.81, abs=0.01)
    assert hists[:, 0].tolist() == [0, 0, 0]
    got = choose_staff_scale(torch.from_numpy(hists))
    assert _scale(got) == want and got.staff_space == 2
    assert _scale(choose_staff_scale(hists.tolist())) == want


def test_runs_of_hand_made_columns():
    col = lambda *v: np.array(v, dtype=np.uint8)[:, None] * 255   # noqa: E731   1 = paper, 0 = ink
    # paper(open) ink 2 paper 3 ink 1 paper(open): two closed ink runs, one closed paper run, one pair (2 + 3); the last ink's paper is open
    h = A.runs(col(1, 0, 0, 1, 1, 1, 0, 1))
    assert h[0].nonzero()[0].tolist() == [1, 2] and h[1].nonzero()[0].tolist() == [3] and h[2].nonzero()[0].tolist() == [5] and h.sum() == 4
    assert A.runs(col(0, 0, 0, 0)).sum() == 0 and A.runs(col(1, 1, 1)).sum() == 0                 # open runs only
    assert A.runs(col(0, 1, 1, 0)).tolist() == (np.eye(256, dtype=np.int64)[2][None] * np.array([[0], [1], [0]])).tolist()   # open ink: no pair
    long = np.full((302, 1), 255, dtype=np.uint8)
    long[1:301] = 0
    assert A.runs(long)[0, 255] == 1 and A.runs(long).sum() == 1                                  # 300 rows: the clamp bin


def test_blank_page_has_no_scale():
    from acai_omr_amd.page import choose_staff_scale, page_quality
    blank = np.full((40, 30), 255, dtype=np.uint8)
    assert A.choose_staff_scale(A.runs(blank)) is None and choose_staff_scale(A.runs(blank).tolist()) is None
    only_clamped = np.zeros((3, 256), dtype=np.int64)
    only_clamped[:, 255] = 7                                                                      # bins 2 .. 254 empty
    assert choose_staff_scale(only_clamped.tolist()) is None and A.choose_staff_scale(only_clamped) is None
    stats, levels = A.sharpness(blank)
    q = page_quality(A.runs(blank).tolist(), stats.tolist(), levels.tolist())
    assert q.scale is None and q.ok and q.reasons == () and q.sharpness == 0.0 and q.contrast == 0 and q.ink_share == 0.0


def test_ties_take_the_lowest_bin_and_the_pitch_is_a_weighted_mean():
    from acai_omr_amd.page import choose_staff_scale
    h = np.zeros((3, 256), dtype=np.int64)
    h[2, 9], h[2, 12], h[2, 20] = 5, 5, 4              # a tie of the pair bins: 9
    h[0, 2], h[0, 3], h[0, 8], h[0, 10] = 6, 6, 1, 99   # a tie of the ink bins below 9: 2 (bin 10 is not below the pitch)
    h[2, 8], h[2, 10] = 1, 2
    s = choose_staff_scale(h.tolist())
    assert (s.line, s.space, s.pitch_bin, s.staff_space) == (2, 7, 9, 7)
    assert s.pitch == (8 * 1 + 9 * 5 + 10 * 2) / 8 and s.confidence == 8 / 17
    assert _scale(s) == A.choose_staff_scale(h)
    with pytest.raises(ValueError):
        choose_staff_scale([[0] * 256] * 2)


def test_assess_config_is_validated():
    from acai_omr_amd.page import AssessConfig
    cfg = AssessConfig()
    assert all(getattr(cfg, n) is None for n in ("min_staff_space", "min_model_staff_space", "min_sharpness", "min_focus", "min_contrast",
                                                 "min_scale_confidence"))
    assert (cfg.ink_threshold, cfg.paper_percent, cfg.ink_percent) == (0.5, 50, 2)
    for bad in (dict(paper_percent=0), dict(ink_percent=101), dict(paper_percent=50.0), dict(ink_percent=True), dict(ink_threshold="x"),
                dict(min_sharpness=-1.0), dict(min_focus=float("nan")), dict(min_contrast="3"), dict(min_staff_space=float("inf")),
                dict(min_scale_confidence=1.5), dict(min_model_staff_space=True)):
        with pytest.raises(ValueError):
            AssessConfig(**bad)
    cfg.min_contrast = -3                               # spoilt after it was made: refused when it is used
    with pytest.raises(ValueError):
        cfg.check()


def test_gate_reports_every_missed_bound_and_nothing_when_unset():
    from acai_omr_amd.page import AssessConfig, page_quality
    page = R.synthetic_page()[0]
    counts = (A.runs(page).tolist(), *(v.tolist() for v in A.sharpness(page)))
    want = A.quality(page)
    q = page_quality(*counts)
    assert q.ok and q.reasons == ()
    assert _scale(q.scale) == want["scale"]
    assert {k: getattr(q, k) for k in ("sharpness", "paper_level", "ink_level", "contrast", "ink_share", "focus")} == {k: v for k, v in want.items() if k != "scale"}
    passing = AssessConfig(min_staff_space=3, min_sharpness=1.0, min_focus=0.1, min_contrast=100, min_scale_confidence=0.5, min_model_staff_space=2)
    assert page_quality(*counts, passing).ok and page_quality(*counts, passing, 2.0).ok
    failing = AssessConfig(min_staff_space=3.5, min_sharpness=1e9, min_focus=50, min_contrast=250, min_scale_confidence=0.9, min_model_staff_space=6)
    q = page_quality(*counts, failing)
    assert not q.ok and len(q.reasons) == 5 and all(isinstance(r, str) for r in q.reasons)       # the model bound needs the resize: not applied
    for r, name in zip(q.reasons, ("min_staff_space", "min_sharpness", "min_focus", "min_contrast", "min_scale_confidence")):
        assert name in r
    q = page_quality(*counts, failing, 5.5)
    assert len(q.reasons) == 6 and "min_model_staff_space" in q.reasons[1]
    one = page_quality(*counts, AssessConfig(min_contrast=209))
    assert not one.ok and len(one.reasons) == 1 and "contrast 208" in one.reasons[0]
    blank = np.full((20, 20), 255, dtype=np.uint8)
    bq = page_quality(A.runs(blank).tolist(), *(v.tolist() for v in A.sharpness(blank)), AssessConfig(min_staff_space=1, min_scale_confidence=0.1))
    assert not bq.ok and len(bq.reasons) == 2           # no scale: both bounds on it fail


def test_dense_page_needs_the_staff_space():
    from acai_omr_amd.page import DetectConfig
    page, truth = R.synthetic_page(**DENSE)
    H, W = page.shape
    cfg = DetectConfig()
    by_canvas, by_music = cfg.resolved(H, W), cfg.resolved(H, W, staff_space=3)
    assert by_canvas == (1, 8, 17, 100, 16) and by_music == (1, 2, 6, 100, 5)

    def found(prm):
        min_ink, merge_gap, min_height, line_len, margin = prm
        return R.systems(page, cfg.ink_threshold, min_ink, merge_gap, min_height, line_len, cfg.min_line_rows, margin, cfg.max_systems)

    assert found(by_canvas) == (0, [])
    assert found(by_music) == (24, R.truth_boxes_with_margin(truth, 5, H, W))
    scale = A.choose_staff_scale(A.runs(page))
    assert (scale["line"], scale["space"], scale["pitch_bin"]) == (1, 2, 3)                    # what page_inference hands to resolved()


def test_resolved_is_unchanged_without_a_staff_space_and_caller_fields_win():
    from acai_omr_amd.page import DetectConfig
    for H, W in ((240, 200), (3508, 2480), (1600, 200), (90, 40), (1, 1)):
        want = (max(1, W // 500), max(1, H // 200), max(1, H // 90), int(np.ceil(0.5 * W)), max(1, H // 100))
        assert DetectConfig().resolved(H, W) == want == DetectConfig().resolved(H, W, None) == DetectConfig().resolved(H, W, staff_space=None)
    # an engraved A4 page at 300 dpi has about H / 180 between its lines: sized from that it resolves to what it resolved to anyway
    assert DetectConfig().resolved(3508, 2480, staff_space=3508 / 180) == DetectConfig().resolved(3508, 2480)
    assert DetectConfig().resolved(560, 200, staff_space=3) == DetectConfig().resolved(560, 200)
    assert DetectConfig(merge_gap=4, margin=0).resolved(1600, 200, staff_space=3) == (1, 4, 6, 100, 0)
    assert DetectConfig(min_ink=2, min_height=9).resolved(1600, 1000, staff_space=2.5) == (2, 2, 9, 500, 4)
    for bad in (0, -1.0, True, "3"):
        with pytest.raises(ValueError):
            DetectConfig().resolved(100, 100, staff_space=bad)


def test_page_result_carries_quality_and_staff_spaces():
    from acai_omr_amd.page import PageResult, StaffScale, system_staff_spaces
    plans = [(0, (0, 10, 50, 30), (32, 80), (0, 0, 32, 80)), (1, (0, 0, 9, 9), (16, 16), (0, 0, 16, 16)), (0, (0, 40, 50, 50), (16, 80), (0, 0, 16, 80))]
    spaces = system_staff_spaces([StaffScale(1, 2, 3, 3.25, 0.9), None], plans)
    assert spaces == [3.25 * 32 / 20, None, 3.25 * 16 / 10]
    res = PageResult([[(0, 10, 50, 30), (0, 40, 50, 50)], [(0, 0, 9, 9)]], None, None, None, [0, 0, 1], [(32, 80), (16, 80), (16, 16)],
                     [(0, 0, 32, 80), (0, 0, 16, 80), (0, 0, 16, 16)], quality=["q0", None], system_staff_space=[5.2, 5.2, None])
    assert res.quality == ["q0", None] and res.system_staff_space == [5.2, 5.2, None]
    plain = PageResult([[]], None, None, None, [], [], [])
    assert plain.quality == [None] and plain.system_staff_space == []
    with pytest.raises(ValueError):
        PageResult([[]], None, None, None, [], [], [], quality=[None, None])


def test_ops_refuse_bad_pages_before_any_launch():
    from acai_omr_amd import ops
    for fn in (ops.page_runs, ops.page_sharpness):
        with pytest.raises(TypeError):
            fn([[0, 1], [1, 0]])
        with pytest.raises(RuntimeError):
            fn(torch.zeros(4, 4, dtype=torch.uint8))                                                 # a CPU tensor: no fallback


def test_the_walk_joins_chunks_and_segments_as_the_whole_column_counts(tmp_path):
    """The C++ the kernels run for their bookkeeping (csrc/assess_walk.h, no HIP in it), compiled for the host with the sanitizers that
    the compiler at hand offers, on 27648 columns against a direct count."""
    from acai_omr_amd import _lib
    rocm = os.path.dirname(os.path.dirname(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"))
    cxx = next((c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
                            os.path.join(rocm, "bin", "amdclang++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler next to the one build() uses"
    src, exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assess_walk_host.cpp"), str(tmp_path / "assess_walk_host")
    base = [cxx, "-std=c++17", "-O1", "-I", _lib.CSRC, src, "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
