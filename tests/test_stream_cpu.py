"""CPU checks of streamed continuous batching's reference statements (tests/stream_reference.py): the numpy statement of the flush
contract on hand-worked slot states, and predict_events - the event skeleton the GPU tests hold the engine to - on hand-worked runs.
They pin the scheduler model the GPU tests are judged against; the device is not needed."""
import os
import random
import re

import numpy as np

from conftest import ROOT
from stream_reference import flatten_events, flush_reference, predict_events


# ---- the flush contract -----------------------------------------------------------------------------------------------------------------
def _state(rows, pitch):
    seqs = (np.arange(rows * pitch, dtype=np.int64).reshape(rows, pitch) * 7 + 3) % 200
    lps = -np.arange(rows * pitch, dtype=np.float32).reshape(rows, pitch) / 8
    return seqs, lps


def test_flush_reference_by_hand():
    seqs, lps = _state(4, 12)
    t = np.array([5, 5, 1, 9], dtype=np.int32)
    fin = np.array([0, 1, 1, 0], dtype=np.int32)       # slot 1 ended at index 5; slot 2 is parked (finished at t = 1)
    mark = np.array([1, 3, 2, 2], dtype=np.int32)
    tok0, lp0, hdr0 = np.full((4, 3), -9, np.int32), np.full((4, 3), -9, np.float32), np.full((4, 4), -9, np.int32)
    tok, lp, hdr, m1 = flush_reference(seqs, lps, t, fin, mark, 4, 3, tok0, lp0, hdr0)
    # slot 0: running, indices 1 .. 4 are new, three fit; slot 1: finished, its last token is at t: indices 3 .. 5; slot 2: nothing;
    # slot 3: indices 2 .. 8, three fit
    assert hdr.tolist() == [[3, 1, 0, 0], [3, 3, 1, 0], [0, 2, 1, 0], [3, 2, 0, 0]]
    assert m1.tolist() == [4, 6, 2, 5]
    assert tok[0].tolist() == seqs[0, 1:4].tolist() and tok[1].tolist() == seqs[1, 3:6].tolist() and tok[3].tolist() == seqs[3, 2:5].tolist()
    assert tok[2].tolist() == [-9, -9, -9] and lp[2].tolist() == [-9, -9, -9]       # what was there stays
    assert lp[1].tolist() == lps[1, 3:6].tolist()
    assert mark.tolist() == [1, 3, 2, 2] and tok0.min() == tok0.max() == -9          # the inputs are not written
    # the second call delivers what did not fit: slot 0 index 4, slot 1 nothing, slot 3 indices 5 .. 7
    tok2, lp2, hdr2, m2 = flush_reference(seqs, lps, t, fin, m1, 4, 3, tok, lp, hdr)
    assert hdr2.tolist() == [[1, 4, 0, 0], [0, 6, 1, 0], [0, 2, 1, 0], [3, 5, 0, 0]] and m2.tolist() == [5, 6, 2, 8]
    assert tok2[0].tolist() == [int(seqs[0, 4])] + tok[0, 1:].tolist() and tok2[3].tolist() == seqs[3, 5:8].tolist()
    # only the first B slots are touched
    tokb, _, hdrb, mb = flush_reference(seqs, lps, t, fin, mark, 2, 3, tok0, lp0, hdr0)
    assert hdrb[2:].min() == hdrb[2:].max() == -9 and tokb[2:].max() == -9 and mb.tolist() == [4, 6, 2, 2]
    # a mark past the end (never produced by the engine) sends nothing and stays
    _, _, hdrc, mc = flush_reference(seqs, lps, t, fin, np.array([7, 9, 5, 9], np.int32), 4, 3, tok0, lp0, hdr0)
    assert [h[0] for h in hdrc.tolist()] == [0, 0, 0, 0] and mc.tolist() == [7, 9, 5, 9]


def test_flush_reference_refusals():
    seqs, lps = _state(3, 8)
    z = np.zeros(3, np.int32)
    out = (np.zeros((3, 8), np.int32), np.zeros((3, 8), np.float32), np.zeros((3, 4), np.int32))
    assert flush_reference(seqs, lps, z, z, z, 3, 8, *out) is not None
    for B, ld in ((3, 0), (3, 9), (4, 2), (0, 2)):
        assert flush_reference(seqs, lps, z, z, z, B, ld, *out) is None
    assert flush_reference(seqs, lps, z, z, z[:2], 3, 2, *out) is None              # rows < B


# ---- the event skeleton ------------------------------------------------------------------------------------------------------------------
def test_one_slot():
    # image 0 (3 tokens, cap 4): 2 steps, then the chunk is cut to the 1 step its cap leaves; image 1 ends on <eos> after 1 of its 2 steps
    assert predict_events([3, 1], [4, 3], slots=1, flush_interval=2) == [
        ([(0, 1, 2)], []), ([(0, 3, 1)], [0]), ([(1, 1, 1)], [1])]


def test_more_slots_than_images():
    # slots 2 and 3 stay parked and never emit; image 1 ends at step 2 and waits for the poll after step 3
    assert predict_events([4, 2], [5, 5], slots=4, flush_interval=3) == [
        ([(0, 1, 3), (1, 1, 2)], [1]), ([(0, 4, 1)], [0])]


def test_end_on_a_poll_boundary_and_one_step_after_it():
    # image 0 ends exactly at the poll after step 4: its last chunk and its finish come together; image 1 ends one step later
    assert predict_events([4, 5], [20, 20], slots=2, flush_interval=4) == [
        ([(0, 1, 4), (1, 1, 4)], [0]), ([(1, 5, 1)], [1])]
    # with a queue behind them: image 2 takes slot 0 at that poll and is one chunk in when image 1 finishes
    assert predict_events([4, 5, 6], [20, 20, 20], slots=2, flush_interval=4) == [
        ([(0, 1, 4), (1, 1, 4)], [0]), ([(2, 1, 4), (1, 5, 1)], [1]), ([(2, 5, 2)], [2])]


def test_caps_of_0_1_and_2():
    # caps 0 and 1: no token, finished up front; cap 2: one token, one step
    assert predict_events([0, 0, 1, 1], [0, 1, 2, 2], slots=1, flush_interval=5) == [
        ([], [0, 1]), ([(2, 1, 1)], [2]), ([(3, 1, 1)], [3])]
    assert predict_events([0], [1], slots=3, flush_interval=5) == [([], [0])]


def test_flush_interval_1_and_larger_than_every_cap():
    assert predict_events([3], [4], slots=2, flush_interval=1) == [([(0, 1, 1)], []), ([(0, 2, 1)], []), ([(0, 3, 1)], [0])]
    # the chunk is cut at the first cap (3 steps), where both rows have already ended
    assert predict_events([3, 2], [4, 6], slots=2, flush_interval=100) == [([(0, 1, 3), (1, 1, 2)], [0, 1])]
    # ... and a row that outlives that cut goes on in chunks cut at ITS cap
    assert predict_events([3, 5], [4, 6], slots=2, flush_interval=100) == [([(0, 1, 3), (1, 1, 3)], [0]), ([(1, 4, 2)], [1])]


def test_flatten_order():
    assert flatten_events(predict_events([4, 2], [5, 5], slots=4, flush_interval=3)) == [
        ("step", 0, 1, 3), ("step", 1, 1, 2), ("finish", 1), ("step", 0, 4, 1), ("finish", 0)]


def test_chunks_tile_every_row():
    rng = random.Random(11)
    for trial in range(200):
        n, slots, F = rng.randint(1, 25), rng.randint(1, 7), rng.choice([1, 2, 5, 16, 25, 64])
        caps = [rng.choice([0, 1, 2, 3, 5, 17, 40]) for _ in range(n)]
        lengths = [rng.randint(1, c - 1) if c >= 2 else 0 for c in caps]
        ev = flatten_events(predict_events(lengths, caps, slots, F))
        nxt, done = [1] * n, []
        for e in ev:
            if e[0] == "step":
                _, i, start, k = e
                assert i not in done and start == nxt[i] and 1 <= k <= F, (trial, e)     # no gap, no overlap, after no finish
                nxt[i] += k
            else:
                done.append(e[1])
                assert nxt[e[1]] == 1 + lengths[e[1]], (trial, e)                        # complete when it finishes
        assert sorted(done) == list(range(n)), trial                                    # every image finishes exactly once


def test_flush_export_is_declared():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    assert "acai_decode_slot_flush" in _lib.exported_symbols() and re.search(r"\bacai_decode_slot_flush\s*\(", hdr)
    proto = hdr[hdr.index("int acai_decode_slot_flush("):]
    assert proto[:proto.index(";")].count(",") + 1 == len(_lib._SIGNATURES["acai_decode_slot_flush"][1])
    from acai_omr_amd.config import InferenceEvent
    assert InferenceEvent.SYSTEMS_FOUND.value == "systems_found"
