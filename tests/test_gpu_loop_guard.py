"""The loop guard end to end (ViTOMR.cached_greedy_generate / cached_continuous_generate / page_inference with loop_guard=) on the committed
fixture models, fp32 and bf16.  The baseline is always the UNGUARDED call: a guarded row must be that row, bit for bit, cut where the
brute-force statement of the rule (tests/loop_reference.py) stops it.  The fixtures' greedy rows loop (tests/test_loops_cpu.py pins where):
with R = 3, M = 4, P = 8 vitomr_small row 0 stops at 8, vitomr_dh64b row 2 at 7, every row of vitomr_odd at 5, and the other rows do not."""
import pytest
import torch

import loop_reference as LR
import page_reference as R
from acai_omr_amd.loops import LoopGuard
from conftest import load_golden
from decode_support import build_vitomr, dev, _memory  # noqa: F401

pytestmark = pytest.mark.gpu

G348 = LoopGuard(min_repeats=3, min_tokens=4, max_period=8)
G224 = LoopGuard(min_repeats=2, min_tokens=2, max_period=4)
FIXTURES = ["vitomr_small", "vitomr_dh64b", "vitomr_odd"]
TRUTH = [(14, 37, 191, 74), (14, 107, 191, 123), (14, 167, 191, 204)]


def _model(dev, name, bf):
    fx = load_golden(name)
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16 if bf else torch.float32, max_batch=8)
    mem, mask = _memory(m, fx["imgs"], bf)
    return fx["cfg"], m, mem, mask


def _expected(m, base, guard, caps):
    """Per row of the unguarded result `base`: (tokens kept, report) by the reference."""
    seqs, _, smask = base
    out = []
    for i in range(seqs.shape[0]):
        n = int(smask[i].sum())
        kind = LR.decode_stop(seqs[i, :n].tolist(), *guard.params, m.decoder.eos_idx, cap=caps[i])
        if kind[0] == "loop":
            _, stop, period, start = kind
            out.append(((start + period) if guard.trim else stop + 1, (stop, period, start)))
        else:
            out.append((min(n, caps[i]), (0, 0, 0)))
    return out


def _check_rows(m, got, base, want):
    seqs, lps, smask, rep = got
    for i, (keep, report) in enumerate(want):
        assert (int(rep.stop[i]), int(rep.period[i]), int(rep.start[i])) == report, i
        assert int(smask[i].sum()) == keep and bool(smask[i, :keep].all()), i
        assert torch.equal(seqs[i, :keep], base[0][i, :keep]), i
        assert torch.equal(lps[i, :keep].view(torch.int32), base[1][i, :keep].view(torch.int32)), i     # bitwise
        assert bool((seqs[i, keep:] == m.decoder.pad_idx).all()) and float(lps[i, keep:].abs().sum()) == 0.0, i
    assert seqs.shape[1] == max(k for k, _ in want)
    assert rep.looped.tolist() == [r[1] > 0 for _, r in want]


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_guarded_greedy_is_the_unguarded_row_cut_at_stop(dev, bf):
    fired = quiet = 0
    for name in FIXTURES:
        cfg, m, mem, mask = _model(dev, name, bf)
        T = cfg["gen_len"]
        with torch.no_grad():
            base = m.cached_greedy_generate(mem, mask, max_len=T)
            assert len(base) == 3
            for guard in (G348, LoopGuard(3, 4, 8, trim=True)):
                got = m.cached_greedy_generate(mem, mask, max_len=T, loop_guard=guard)
                want = _expected(m, base, guard, [T] * mem.shape[0])
                _check_rows(m, got, base, want)
            # a guard that cannot fire: greedy, bit for bit, and an empty report
            off = m.cached_greedy_generate(mem, mask, max_len=T, loop_guard=LoopGuard(2, T + 1))
            again = m.cached_greedy_generate(mem, mask, max_len=T)
        for a, b, c in zip(base, off, again):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert not bool(off[3].looped.any()) and int(off[3].stop.abs().sum()) == 0
        want = _expected(m, base, G348, [T] * mem.shape[0])
        fired += sum(1 for _, r in want if r[1])
        quiet += sum(1 for _, r in want if not r[1])
        pinned = {"vitomr_small": [(8, 2, 3), (0, 0, 0), (0, 0, 0)], "vitomr_dh64b": [(0, 0, 0), (0, 0, 0), (7, 2, 2)],
                  "vitomr_odd": [(5, 1, 1)] * 3}[name]
        assert [r for _, r in want] == pinned, name
    assert fired >= 1 and quiet >= 1


def test_a_looping_batch_ends_early(dev):
    from acai_omr_amd.engine import unpad_rows
    cfg, m, mem, mask = _model(dev, "vitomr_odd", False)
    T = cfg["max_len"]
    blocks = m.decoder._cached_blocks()
    mem32, lens = unpad_rows(mem, mask)
    with torch.no_grad():
        blocks.prepare_caches_packed(mem32, None, lens)
        eng = blocks.engine(dev)
        _, _, done = eng.greedy(T, poll=1, loop_guard=G348)
        stop, period, start = (t.tolist() for t in eng.loop_report())
        blocks.prepare_caches_packed(mem32, None, lens)
        _, _, plain = eng.greedy(T, poll=1)
    assert (stop, period, start) == ([5] * 3, [1] * 3, [1] * 3)
    assert done == 5 and done < T - 1          # every row stopped at index 5: the batch ends there
    assert plain > done                        # the unguarded batch went on repeating itself
    assert eng._mode == ("greedy",)


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_continuous_rows_free_their_slots_at_stop(dev, bf):
    cfg, m, mem, mask = _model(dev, "vitomr_dh64b", bf)
    # the cache's length, 24: the host looks at the slots every 16 steps (or at a cap), so the rows must be longer than that for a slot
    # freed at index 4 or 7 to be seen - and refilled - before its cap would have freed it anyway
    T = cfg["max_len"]
    eng = m.decoder._cached_blocks().engine(dev)
    with torch.no_grad():
        base = m.cached_continuous_generate(mem, mask, max_len=T, slots=2)
        plain_steps = eng.slot_steps
        got = m.cached_continuous_generate(mem, mask, max_len=T, slots=2, loop_guard=G224)
        steps = eng.slot_steps
        want = _expected(m, base, G224, [T] * 3)
        assert [r for _, r in want] == [(4, 1, 2), (7, 1, 5), (5, 2, 2)]
        _check_rows(m, got, base, want)
        for i in range(3):   # each image is its guarded static result, decoded alone
            alone = m.cached_greedy_generate(mem[i:i + 1], mask[i:i + 1], max_len=T, loop_guard=G224)
            n = alone[0].shape[1]
            assert n == want[i][0]
            assert torch.equal(got[0][i, :n], alone[0][0]) and torch.equal(got[2][i, :n], alone[2][0]) and not bool(got[2][i, n:].any())
            assert torch.equal(got[1][i, :n].view(torch.int32), alone[1][0].view(torch.int32))
            assert (int(alone[3].stop[0]), int(alone[3].period[0]), int(alone[3].start[0])) == want[i][1]
        # per-image caps below a stop: the cap ends the row and nothing is reported
        capped = m.cached_continuous_generate(mem, mask, max_len=[T, 5, T], slots=1, loop_guard=G224)
    assert steps < plain_steps, (steps, plain_steps)
    assert capped[3].period.tolist() == [1, 0, 2] and int(capped[2][1].sum()) == 5


def test_page_inference_reports_loops_per_system(dev):
    from acai_omr_amd.inference.vitomr_inference import continuous_inference, page_inference
    from acai_omr_amd.utils import DynamicResize
    fx = load_golden("vitomr_dh64b")
    m = build_vitomr(fx["cfg"], fx["state_dict"], dev, torch.bfloat16, max_batch=2)
    tr = DynamicResize(16, 32, 4, 8, True)
    page = torch.from_numpy(R.synthetic_page()[0]).float() / 255.0
    boxes = TRUTH[:2]
    crops = [tr(page[y0:y1, x0:x1][None]) for x0, y0, x1, y1 in boxes]
    plain = continuous_inference(m, crops, "cuda", max_inference_len=12)
    want = continuous_inference(m, crops, "cuda", max_inference_len=12, loop_guard=G224)
    assert len(plain) == 3 and len(want) == 4
    res = page_inference(m, page, "cuda", tr, boxes=boxes, max_inference_len=12, loop_guard=G224)
    assert len(res) == 2 and res.loops is not None
    for a, b in zip((res.seqs, res.log_probs, res.seq_mask, res.loops.stop, res.loops.period, res.loops.start),
                    want[:3] + (want[3].stop, want[3].period, want[3].start)):
        assert torch.equal(a, b)
    assert res.loops.period.shape == (2,)
    expect = _expected(m, plain, G224, [12, 12])
    assert [(int(res.loops.stop[i]), int(res.loops.period[i]), int(res.loops.start[i])) for i in range(2)] == [r for _, r in expect]
    assert page_inference(m, page, "cuda", tr, boxes=boxes, max_inference_len=12).loops is None
    with pytest.raises(ValueError, match="streamed"):
        m.streamed_continuous_generate(torch.zeros(1, 2, 4), loop_guard=G224)
