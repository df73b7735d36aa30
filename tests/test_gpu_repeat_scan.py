"""ops.repeat_scan (csrc/loops.hip: acai_repeat_scan) against the brute-force statement of the loop guard's rule (tests/loop_reference.py)
on random rows over a 3-token alphabet, where loops are frequent: N in {1, 4, 5} (one wave, a full workgroup of four, a second workgroup),
ragged lengths read on the device, a row-strided view, a bool mask, and lengths around the eight-index look-ahead of the sweep.  Integer
outputs: torch.equal."""
import pytest
import torch

import loop_reference as LR
from acai_omr_amd import ops
from acai_omr_amd.loops import LoopGuard, scan_repeats
from decode_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _rows(N, T, seed, alphabet=3):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(3, 3 + alphabet, (N, T), generator=g)
    t[:, 0] = 0
    return t


def _check(dev, tok, P, R, M, lens=None, view=None):
    dtok = tok.to(dev) if view is None else view
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    got = ops.repeat_scan(dtok, P, R, M, lens=dl)
    want = LR.scan_rows(tok.tolist(), P, R, M, lens=lens)
    for name, g, w in zip(("stop", "period", "start", "end"), got, want):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), torch.tensor(w, dtype=torch.int32)), (name, g.tolist(), w)
    return want


@pytest.mark.parametrize("N", [1, 4, 5])
@pytest.mark.parametrize("prm", [(8, 3, 4), (4, 2, 2), (64, 2, 1), (1, 2, 3)])
def test_random_rows(dev, N, prm):
    P, R, M = prm
    fired = 0
    for seed, T in ((1, 40), (2, 9), (3, 17), (4, 2), (5, 1), (8, 96)):
        want = _check(dev, _rows(N, T, seed * 10 + N), P, R, M)
        fired += sum(1 for p in want[1] if p)
    assert fired >= 1


def test_ragged_lengths_mask_and_view(dev):
    tok = _rows(5, 48, 7)
    lens = [48, 0, 1, 11, 30]
    _check(dev, tok, 8, 2, 3, lens=lens)
    _check(dev, tok, 8, 2, 3, lens=[60, -4, 2, 3, 48])           # clamped to [0, T] where they are read
    mask = torch.arange(48).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
    got = ops.repeat_scan(tok.to(dev), 8, 2, 3, lens=mask.to(dev))
    assert [g.tolist() for g in got] == list(LR.scan_rows(tok.tolist(), 8, 2, 3, lens=lens))
    wide = torch.full((5, 64), 3, dtype=torch.int64)              # the columns past the view would loop at once: they must not be read
    wide[:, 5:53] = tok
    view = wide.to(dev)[:, 5:53]
    assert view.stride(0) == 64 and not view.is_contiguous()
    _check(dev, tok, 8, 2, 3, view=view)
    _check(dev, tok, 8, 2, 3, lens=lens, view=view)
    rep = scan_repeats(tok.to(dev), LoopGuard(2, 3, max_period=8), lens=torch.tensor(lens, dtype=torch.int32, device=dev))
    stop, period, start, _ = LR.scan_rows(tok.tolist(), 8, 2, 3, lens=lens)
    assert rep.stop.tolist() == stop and rep.period.tolist() == period and rep.start.tolist() == start
    assert rep.looped.tolist() == [p > 0 for p in period]


def test_grpo_loop_rate_is_the_share_of_flagged_rollouts(dev):
    from acai_omr_amd.train.grpo import loop_rate
    tok = _rows(5, 48, 7)
    lens = [48, 0, 1, 11, 30]
    mask = torch.arange(48).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
    rate = loop_rate(tok.to(dev), mask.to(dev), LoopGuard(2, 3, max_period=8))
    period = LR.scan_rows(tok.tolist(), 8, 2, 3, lens=lens)[1]
    assert rate.shape == () and rate.is_cuda and 0 < sum(1 for p in period if p) < 5
    assert float(rate) == pytest.approx(sum(1 for p in period if p) / 5)


def test_by_hand_and_end(dev):
    #                    0  1  2  3  4  5  6  7  8  9
    tok = torch.tensor([[0, 5, 6, 7, 5, 6, 7, 5, 6, 9],      # period 3 fires at 6, holds through 8
                        [0, 4, 4, 4, 4, 4, 4, 4, 4, 4],      # period 1 fires at 3, holds to the end of the row
                        [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]])     # nothing
    got = ops.repeat_scan(tok.to(dev), 8, 2, 2)
    assert [g.tolist() for g in got] == [[6, 3, 0], [3, 1, 0], [1, 1, 0], [8, 9, 0]]
    golden = torch.tensor(LR.golden_rows("vitomr_dh64b"))
    got = ops.repeat_scan(golden.to(dev), 4, 2, 2)
    assert [g.tolist() for g in got[:3]] == [[4, 7, 5], [1, 1, 2], [2, 5, 2]]
    long = torch.full((1, 700), 8, dtype=torch.int64)             # `end` found across several 64-index rounds
    long[0, 0], long[0, 650] = 0, 9
    assert [g.tolist() for g in ops.repeat_scan(long.to(dev), 64, 3, 4)] == [[5], [1], [1], [649]]


def test_refusals(dev):
    tok = _rows(2, 8, 1).to(dev)
    for prm in ((0, 2, 1), (65, 2, 1), (8, 1, 1), (8, 2, 0)):
        with pytest.raises(ValueError):
            ops.repeat_scan(tok, *prm)
    with pytest.raises(TypeError):
        ops.repeat_scan(tok.int(), 8, 2, 1)
    with pytest.raises(ValueError):
        ops.repeat_scan(tok, 8, 2, 1, lens=torch.zeros(3, dtype=torch.int32, device=dev))
    empty = ops.repeat_scan(tok[:0], 8, 2, 1)
    assert all(e.shape == (0,) for e in empty)
