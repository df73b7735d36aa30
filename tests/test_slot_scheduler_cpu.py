"""CPU checks of continuous batching's slot scheduler (acai_omr_amd/scheduler.py), driven by a fake device whose rows finish at given
lengths, and of the slot-mode C-ABI mirror."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


class FakeDevice:
    """Slot s decodes image i for stop[i] steps (its <eos> step, or cap - 1 at the latest), then raises its finished flag."""

    def __init__(self, stop, slots):
        self.stop, self.row, self.done = stop, [None] * slots, [0] * slots
        self.finished = [1] * slots

    def arm(self, s, i):
        self.row[s], self.done[s], self.finished[s] = i, 0, 0

    def steps(self, n):
        for s, i in enumerate(self.row):
            if i is not None and not self.finished[s]:
                self.done[s] = min(self.done[s] + n, self.stop[i])
                self.finished[s] = int(self.done[s] == self.stop[i])


def drive(caps, stop, slots, poll):
    """The engine's loop (DecodeEngine.continuous) against the fake device.  Returns the admissions, the completion order and, per poll,
    the idle slots and the queue length left after the refill."""
    from acai_omr_amd.scheduler import SlotScheduler
    sc = SlotScheduler(caps, slots)
    dev = FakeDevice(stop, slots)
    admitted, order, polls = [], list(sc.skipped), []
    for s, i in sc.admit():
        dev.arm(s, i)
        admitted.append((s, i))
    n = sc.chunk(poll)
    while n > 0:
        dev.steps(n)
        freed = sc.advance(n, list(dev.finished))
        for s, i in sc.admit():
            dev.arm(s, i)
            admitted.append((s, i))
        polls.append((sc.idle(), len(sc.queue)))
        order += [i for _, i in freed]
        n = sc.chunk(poll)
    assert sc.done
    return admitted, order, polls


def test_admission_order_and_lowest_free_slot():
    caps = [10, 4, 6, 3, 8, 2, 5]
    stop = [c - 1 for c in caps]
    admitted, order, _ = drive(caps, stop, slots=3, poll=16)
    assert [i for _, i in admitted] == list(range(7))            # input order
    assert admitted[:3] == [(0, 0), (1, 1), (2, 2)]
    # image 1 (3 steps) frees slot 1 first; image 3 goes there; then image 2 (5 steps) and image 3 (2 more) free slots 2 and 1 together:
    # images 4 and 5 go to the LOWER free slot first
    assert admitted[3] == (1, 3)
    assert admitted[4:6] == [(1, 4), (2, 5)]
    assert sorted(order) == list(range(7)) and len(order) == 7   # every image harvested exactly once


def test_no_idle_slot_while_images_are_queued():
    import random
    rng = random.Random(7)
    for trial in range(50):
        n, slots, poll = rng.randint(1, 30), rng.randint(1, 8), rng.choice([1, 3, 16])
        caps = [rng.randint(1, 40) for _ in range(n)]
        stop = [rng.randint(1, c - 1) if c >= 2 else 0 for c in caps]   # <eos> anywhere up to the cap
        admitted, order, polls = drive(caps, stop, slots, poll)
        assert sorted(order) == list(range(n)) and len(set(order)) == n
        assert [i for _, i in admitted] == [i for i in range(n) if caps[i] >= 2]
        for idle, queued in polls:
            assert not (idle and queued), (trial, idle, queued)


def test_completion_order_indices():
    """Completion order: by the step each image finishes at; images freed at the same poll come out in slot order."""
    caps = [30, 30, 30, 30]
    stop = [20, 5, 12, 5]
    _, order, _ = drive(caps, stop, slots=4, poll=1)
    assert order == [1, 3, 2, 0]
    _, order, _ = drive(caps, stop, slots=4, poll=16)
    assert order == [1, 2, 3, 0]                                 # 1, 2, 3 at the poll after step 16 (slot order), 0 at step 29
    _, order, _ = drive(caps, stop, slots=2, poll=16)
    assert order == [1, 0, 2, 3]                                 # 2 refills slot 1 at step 16; 0 and 2 at step 29; 3 refills slot 0
    _, order, _ = drive([1, 5, 1], [0, 4, 0], slots=1, poll=16)
    assert order == [0, 2, 1]                                    # cap 1: no token to decode, reported first


def test_chunk_stops_at_the_first_cap():
    from acai_omr_amd.scheduler import SlotScheduler
    sc = SlotScheduler([9, 40, 17], 3)
    sc.admit()
    assert sc.chunk(16) == 8                                     # image 0 ends after 8 steps: the poll comes then
    sc.advance(8, [1, 0, 0])
    assert sc.chunk(16) == 8 and sc.idle() == [0]
    with pytest.raises(RuntimeError):
        sc.advance(8, [0, 0, 0])                                 # image 2 is at its cap: the device must have finished it
    with pytest.raises(ValueError):
        SlotScheduler([3], 0)


def test_slot_abi_mirror_matches_header():
    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} AcaiSlots;")):hdr.index("} AcaiSlots;")]
    names = re.findall(r"\b([a-z_]+);", body)
    assert [f for f, _ in _lib.AcaiSlots._fields_] == names == ["t", "first", "cap", "rows", "pad_"]
    assert ctypes.sizeof(_lib.AcaiSlots) == 3 * 8 + 2 * 4
    for fn in ("acai_decode_slot_step", "acai_decode_slot_arm"):
        assert fn in _lib.exported_symbols() and re.search(r"\b" + fn + r"\s*\(", hdr)
