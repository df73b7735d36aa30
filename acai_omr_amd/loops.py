"""The loop guard (an extension: the reference lets a row that fell into a repeat cycle run to its cap).

One rule, stated once (include/acai_omr_hip.h at AcaiLoop; tests/loop_reference.py restates it by brute force): with P = max_period,
R = min_repeats, M = min_tokens and need(p) = max((R - 1) p, M), a row fires at the first index t at which the last need(p) tokens repeat
the tokens p indices before them, for some p in 1 .. P (index 0, <bos>, never takes part); the smallest such p wins.  The report is
stop = t, period = p and start = t - need(p) - p + 1, the first index of the periodic stretch.

LoopGuard carries the parameters to the decoding entry points that take loop_guard= (greedy and continuous-batching greedy decoding: the
check runs inside the selection launch of the replayed graphs and frees the row at `stop`); scan_repeats applies the same rule to token
rows of any origin after the fact.

How often trained checkpoints loop, and which (R, M, P) separate a runaway row from a genuine ostinato, has not been measured: that is why
min_repeats and min_tokens have no defaults."""
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class LoopGuard:
    """min_repeats R >= 2: copies of the cycle that must stand, the first included.  min_tokens M >= 1: repeated tokens that must stand at
    least, whatever the period (it keeps a short period from firing on a few equal tokens).  max_period P in [1, 64].  trim: the entry
    points' mask keeps one copy of the cycle (through start + period - 1) instead of everything up to `stop`."""
    min_repeats: int
    min_tokens: int
    max_period: int = 64
    trim: bool = False

    def __post_init__(self):
        for name in ("min_repeats", "min_tokens", "max_period"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"LoopGuard: {name} must be an int, got {v!r}")
        if not 1 <= self.max_period <= 64:
            raise ValueError(f"LoopGuard: max_period must be in [1, 64], got {self.max_period}")
        if self.min_repeats < 2:
            raise ValueError(f"LoopGuard: min_repeats must be at least 2, got {self.min_repeats}")
        if self.min_tokens < 1:
            raise ValueError(f"LoopGuard: min_tokens must be at least 1, got {self.min_tokens}")
        if self.min_repeats >= 1 << 24 or self.min_tokens >= 1 << 24:
            raise ValueError("LoopGuard: min_repeats and min_tokens must be below 2^24")

    @property
    def params(self):
        """(P, R, M), as the engine's modes and the C ABI take them."""
        return self.max_period, self.min_repeats, self.min_tokens

    def need(self, period):
        return max((self.min_repeats - 1) * period, self.min_tokens)


def check_guard(guard):
    """`loop_guard` as the entry points take it: None, or a LoopGuard (TypeError otherwise)."""
    if guard is not None and not isinstance(guard, LoopGuard):
        raise TypeError(f"loop_guard must be a loops.LoopGuard, got {type(guard).__name__}")
    return guard


def refuse_guard(guard, mode):
    """The decoding modes that do not take a loop guard name themselves here (scan_repeats covers their outputs after the fact)."""
    if check_guard(guard) is not None:
        raise ValueError(f"loop_guard (loop detection) cannot be combined with {mode}: out of scope here; scan_repeats covers its output")


@dataclass
class LoopReport:
    """Per row: stop (the index of the row's last token), period (0 = the row did not loop) and start (the first index of the periodic
    stretch) - int32 tensors of N entries; stop and start are 0 where period is."""
    stop: torch.Tensor
    period: torch.Tensor
    start: torch.Tensor

    @property
    def looped(self):
        return self.period > 0

    def caps(self, caps, trim=False):
        """The rows' effective caps (tokens kept, <bos> included): caps[i] where row i did not loop, else stop + 1 - with trim
        start + period, one copy of the cycle - and never above caps[i]."""
        out = []
        for c, st, p, s in zip(caps, self.stop.tolist(), self.period.tolist(), self.start.tolist()):
            out.append(int(c) if p == 0 else min(int(c), s + p if trim else st + 1))
        return out


def scan_repeats(tokens, guard, lens=None):
    """The guard's rule over finished rows -> LoopReport.  tokens (N, T) int64; lens: None (every row holds T tokens), int32 lengths (N,) or
    a bool prefix mask of tokens' shape.  On the device one launch (ops.repeat_scan), no host sync."""
    from . import ops
    if not isinstance(guard, LoopGuard):
        raise TypeError(f"guard must be a loops.LoopGuard, got {type(guard).__name__}")
    stop, period, start, _ = ops.repeat_scan(tokens, *guard.params, lens=lens)
    return LoopReport(stop, period, start)
