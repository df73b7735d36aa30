"""Slot scheduling of continuous-batching greedy decode (DecodeEngine.continuous), in plain Python so that it can be driven without a device.

A fixed set of decode rows ("slots") works through a queue of images.  Admission order is input order, into the lowest free slot.  The
engine polls the device's per-slot finished flags between runs of decode steps; at every poll it harvests the finished slots and refills
them at once, so no slot is idle at a poll boundary while images are still queued."""
from collections import deque


class SlotScheduler:
    def __init__(self, caps, slots):
        """caps[i]: image i's cap (its row ends after writing token index caps[i] - 1); images with a cap below 2 produce no token and are
        never queued (`skipped`)."""
        if slots < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        self.caps = [int(c) for c in caps]
        self.slots = int(slots)
        self.skipped = [i for i, c in enumerate(self.caps) if c < 2]
        self.queue = deque(i for i, c in enumerate(self.caps) if c >= 2)
        self.image = [None] * self.slots   # image decoding in each slot (None: idle)
        self.left = [0] * self.slots       # steps until the slot's image reaches its cap

    @property
    def done(self):
        return not self.queue and all(i is None for i in self.image)

    def idle(self):
        return [s for s, i in enumerate(self.image) if i is None]

    def admit(self):
        """Fill every free slot, lowest first, with the next queued image.  Returns [(slot, image)]."""
        out = []
        for s in range(self.slots):
            if not self.queue:
                break
            if self.image[s] is None:
                i = self.queue.popleft()
                self.image[s], self.left[s] = i, self.caps[i] - 1
                out.append((s, i))
        return out

    def chunk(self, poll):
        """Steps to run before the next poll: `poll`, or fewer when a busy slot reaches its cap sooner (0 when every slot is idle)."""
        busy = [self.left[s] for s, i in enumerate(self.image) if i is not None]
        return min([int(poll)] + busy) if busy else 0

    def advance(self, n, finished):
        """`n` steps ran; finished[s] is the device's flag of slot s.  Frees the finished busy slots and returns them as [(slot, image)] in
        slot order (the order they are harvested in)."""
        out = []
        for s, i in enumerate(self.image):
            if i is None:
                continue
            self.left[s] -= n
            if finished[s]:
                out.append((s, i))
                self.image[s] = None
            elif self.left[s] <= 0:
                raise RuntimeError(f"slot {s} (image {i}) is past its cap but the device did not finish it")
        return out
