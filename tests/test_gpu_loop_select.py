"""The loop guard's selection launches alone (decode_select.hip: greedy_select_kernel<SLOT, false, false, LOOP = true>) through
acai_debug_decode_loop_select, on one-hot logits that script every row's tokens step by step, against the brute-force statement of the rule
in tests/loop_reference.py.  No model is built.  Device and reference start from the same state and evolve on their own; after EVERY launch
the rows, the report (stop, period, start), the finished flags, the unfinished count, step / the slots' t and all 64 run counters of every
row are compared with torch.equal.

Shapes are the smallest that can go wrong: B in {1, 5, 9, 17} (one row per wave at 256 / 512 / 1024 threads, and rows wrapping onto the 16
waves), P in {1, 7, 64} with max_len = 140 so that a period of 64 can fire at R = 2 (two copies from index 1 end at index 128 at the earliest).

Two periods due at the same index: on a row guarded from index 1 the FIRST firing never has two (run_p reaches need(p) exactly, so the
periodic stretch of the smaller period is preceded by a token that breaks it, which the longer period's stretch would have to repeat), so
the tie is staged the one way the launch can meet it: counters zeroed at a later index of a row that is already periodic, which is what
loop_reference's `armed` states.  The ballot then has several bits and the lowest must win."""
import pytest
import torch

import loop_reference as LR
from acai_omr_amd import ops
from decode_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

V, E, EOS, BOS, PAD, MAX_LEN = 96, 8, 2, 0, 1, 140
SENT = -77   # sentinel of rows the launch must not touch


class Guarded:
    """Device state of one case beside the reference's; step(tokens) scripts one launch and compares everything."""

    def __init__(self, dev, B, P, R, M, slot=False, caps=None, live=None, armed=1):
        g = torch.Generator().manual_seed(B * 1000 + P)
        self.dev, self.B, self.prm, self.slot, self.armed = dev, B, (P, R, M), slot, armed
        self.emb, self.pos = torch.randn(V, E, generator=g).to(dev), torch.randn(MAX_LEN, E, generator=g).to(dev)
        live = [True] * B if live is None else live
        # reference state
        self.seq = [[BOS] + [PAD] * (MAX_LEN - 1) for _ in range(B)]
        self.fin = [0 if l else 1 for l in live]
        self.rep = [[0, 0, 0] for _ in range(B)]
        self.run = [[0] * 64 for _ in range(B)]
        self.t = [1] * B
        self.cap = [MAX_LEN] * B if caps is None else list(caps)
        self.stp = [1, 0]
        # device state
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
        self.d = dict(logits=torch.zeros(B, V, device=dev), seqs=torch.tensor(self.seq, dtype=torch.int64, device=dev),
                      logprobs=torch.zeros(B, MAX_LEN, device=dev), step=i32(self.stp), finished=i32(self.fin + [sum(live)]),
                      x=torch.zeros(B, E, device=dev))
        self.slots = dict(t=i32(self.t), cap=i32(self.cap)) if slot else None
        self.loop = dict(run=torch.zeros(B, 64, dtype=torch.int32, device=dev), stop=torch.zeros(B, dtype=torch.int32, device=dev),
                         period=torch.zeros(B, dtype=torch.int32, device=dev), start=torch.zeros(B, dtype=torch.int32, device=dev),
                         max_period=P, min_repeats=R, min_tokens=M)

    def preset(self, b, tokens, t):
        """Row b already holds `tokens` at indices 1 .. and stands at index t (device and reference alike); counters stay zero."""
        for i, k in enumerate(tokens):
            self.seq[b][1 + i] = k
        self.d["seqs"][b] = torch.tensor(self.seq[b], dtype=torch.int64)
        if self.slot:
            self.t[b] = t
            self.slots["t"][b] = t
        else:
            self.stp[0] = t
            self.d["step"][0] = t

    def rearm(self, b, cap=None):
        """What the engine does when it refills slot b: the row, the flag, the local time and the guard's words back to the armed state."""
        self.seq[b] = [BOS] + [PAD] * (MAX_LEN - 1)
        self.fin[b], self.t[b], self.rep[b], self.run[b] = 0, 1, [0, 0, 0], [0] * 64
        self.d["seqs"][b] = torch.tensor(self.seq[b], dtype=torch.int64)
        self.d["finished"][b] = 0
        self.slots["t"][b] = 1
        if cap is not None:
            self.cap[b] = cap
            self.slots["cap"][b] = cap
        self.loop["run"][b].zero_()
        for k in ("stop", "period", "start"):
            self.loop[k][b] = 0

    def _reference(self, toks):
        P, R, M = self.prm
        for b in range(self.B):
            if self.fin[b] and self.slot:
                continue                                 # a finished or idle slot is skipped: nothing of it is read or written
            t = self.t[b] if self.slot else self.stp[0]
            self.seq[b][t] = toks[b]                     # (a finished static row goes on emitting, as without a guard)
            if self.fin[b]:
                continue                                 # ... but is not examined again: counters and report stand
            self.run[b] = LR.run_counters(self.seq[b], t, P, self.armed)
            hit = LR.fires_at(self.seq[b], t, P, R, M, self.armed)
            fin = False
            if toks[b] == EOS:
                fin = True                               # the row ends as it does without a guard; period stays 0
            elif hit:
                fin, self.rep[b] = True, [t, hit[0], hit[1]]
            if self.slot:
                fin = fin or t >= self.cap[b] - 1
                if not fin:
                    self.t[b] = t + 1
            self.fin[b] = 1 if fin else 0
        if self.slot:
            self.stp[1] = (self.stp[1] + 1) % MAX_LEN
        else:
            self.stp = [self.stp[0] + 1, self.stp[1] + 1]

    def step(self, toks):
        d = self.d
        d["logits"].zero_()
        d["logits"][torch.arange(self.B), torch.tensor(toks)] = 12.0
        ops.debug_decode_loop_select(self.slot, d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], loop=self.loop,
                                     max_len=MAX_LEN, Tmax=MAX_LEN, eos=EOS, bos=BOS, pad=PAD, emb=self.emb, pos=self.pos, x=d["x"], slots=self.slots)
        self._reference(toks)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
        where = f"after index {self.stp[0] - 1 if not self.slot else self.t}"
        assert torch.equal(d["seqs"].cpu(), torch.tensor(self.seq, dtype=torch.int64)), where
        rep = torch.stack([self.loop["stop"], self.loop["period"], self.loop["start"]], dim=1).cpu()
        assert torch.equal(rep, i32(self.rep)), (where, rep.tolist(), self.rep)
        assert torch.equal(d["finished"].cpu(), i32(self.fin + [self.B - sum(self.fin)])), where
        assert torch.equal(self.loop["run"].cpu(), i32(self.run)), where
        if self.slot:
            assert torch.equal(self.slots["t"].cpu(), i32(self.t)), where
            assert int(d["step"][1]) == self.stp[1]
        else:
            assert torch.equal(d["step"].cpu(), i32(self.stp)), where


def _row_script(b, P, n):
    """Row b's tokens of indices 1 .. n: `lead` tokens that never repeat, then a cycle of q distinct tokens - q from 1 up to P + 1, which no
    period up to P matches, so that row runs on."""
    q = [1, 2, P, max(1, P // 2), P + 1][b % 5]
    lead = b % 3   # 0: the cycle begins at index 1
    return [90 + i for i in range(lead)] + [3 + (i % q) for i in range(n - lead)]


@pytest.mark.parametrize("P", [1, 7, 64])
@pytest.mark.parametrize("B", [1, 5, 9, 17])
def test_static_rows_fire_where_the_reference_fires(dev, B, P):
    n = min(MAX_LEN - 1, 2 * P + 12)
    rows = [_row_script(b, P, n) for b in range(B)]
    g = Guarded(dev, B, P, R=2, M=3)
    for i in range(n):
        g.step([r[i] for r in rows])
    want = [LR.first_loop([BOS] + r, P, 2, 3) for r in rows]
    assert [tuple(r) if r[1] else None for r in g.rep] == want
    assert any(w is not None for w in want)
    if B >= 5:
        assert any(w is None for w in want) and g.fin.count(0) >= 1   # the row of period P + 1 is still running
    if P == 64 and B >= 3:
        assert (130, 64, 3) in want   # row 2: the longest period there is, behind two lead tokens (indices 3 .. 130 hold two copies)
    if P == 64 and B == 17:
        assert (128, 64, 1) in want   # row 12: from index 1, at the first index at which period 64 can fire


@pytest.mark.parametrize("B", [1, 5, 17])
def test_slot_rows_fire_skip_and_rearm(dev, B):
    P, R, M = 7, 2, 3
    n = 2 * P + 12
    rows = [_row_script(b, P, n) for b in range(B)]
    live = [b % 4 != 3 for b in range(B)]                        # idle slots from the start
    caps = [MAX_LEN if b % 5 != 4 else 9 for b in range(B)]      # the row that never loops ends at its cap (index 8)
    g = Guarded(dev, B, P, R, M, slot=True, caps=caps, live=live)
    for b in range(B):
        if not live[b]:
            g.d["seqs"][b].fill_(SENT)
            g.seq[b] = [SENT] * MAX_LEN
    for i in range(n):
        g.step([r[i] for r in rows])
    for b in range(B):
        kind = LR.decode_stop([BOS] + rows[b], P, R, M, EOS, cap=caps[b])
        if not live[b]:
            assert g.rep[b] == [0, 0, 0] and g.t[b] == 1
        elif kind[0] == "loop":
            assert g.rep[b] == list(kind[1:]) and g.t[b] == kind[1] and g.fin[b] == 1   # t is left at the row's last token
        else:
            assert kind == ("cap", 8) and g.rep[b] == [0, 0, 0] and g.t[b] == 8 and g.fin[b] == 1
    assert all(g.fin)
    # slot 0 stopped on a loop; re-armed it starts from zeroed counters: the same tokens fire at the same index again, not earlier
    first = list(g.rep[0])
    assert first[1] > 0
    g.rearm(0)
    for i in range(first[0]):
        g.step([r[i] for r in rows])
        assert (g.fin[0] == 1) == (i == first[0] - 1)
    assert g.rep[0] == first


def test_near_miss_eos_and_tie(dev):
    P, R, M = 8, 2, 6
    a, b_, x = 10, 11, 12
    # period 2 needs 6: indices 3 .. 8.  Row 0 breaks it at index 8, one token before the need is met, and fires six tokens later at the
    # earliest; row 1 goes through; row 2 puts <eos> where the rule would fire: it ends as any row does and reports nothing.
    rows = [[a, b_, a, b_, a, b_, a, x, a, x, a, x, a, x, a],
            [a, b_, a, b_, a, b_, a, b_, a, b_, a, b_, a, b_, a],
            [a, b_, a, b_, a, b_, a, EOS, a, b_, a, b_, a, b_, a]]
    g = Guarded(dev, 3, P, R, M)
    for i in range(len(rows[0])):
        g.step([r[i] for r in rows])
    assert g.rep[1] == [8, 2, 1] and g.rep[2] == [0, 0, 0] and g.rep[0] == [14, 2, 7]
    assert g.run[2] == LR.run_counters([BOS] + rows[2], 8, P)   # the <eos> step updated the counters, then they stood
    # the tie: a row that is already all one token when its counters are zeroed at index 6; periods 1, 2 and 3 all need 3 (R = 2, M = 3)
    # and are due together at index 8 - the smallest wins
    g = Guarded(dev, 2, 3, 2, 3, armed=6)
    for b in range(2):
        g.preset(b, [20 + b] * 5, 6)
    for t in range(6, 9):
        assert g.fin == [0, 0]
        g.step([20, 21])
    assert LR.due_at(g.seq[0], 8, 3, 2, 3, armed=6) == [1, 2, 3]
    assert g.rep == [[8, 1, 5], [8, 1, 5]] and g.fin == [1, 1]


@pytest.mark.parametrize("slot", [False, True])
def test_a_guard_that_cannot_fire_is_the_plain_launch_bit_for_bit(dev, slot):
    B = 9
    gen = torch.Generator().manual_seed(5)
    form = ops.SELECT_SLOT_ARGMAX if slot else ops.SELECT_ARGMAX
    out = []
    for guarded in (False, True):
        g = Guarded(dev, B, 64, R=2, M=MAX_LEN + 1, slot=slot)
        gen.manual_seed(5)
        for _ in range(6):
            logits = torch.randn(B, V, generator=gen)
            logits[:, EOS] = -30.0
            logits[:, :6] += 3.0          # few candidates: rows repeat themselves, and still nothing may fire
            d = g.d
            d["logits"].copy_(logits)
            if guarded:
                ops.debug_decode_loop_select(slot, d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], loop=g.loop, max_len=MAX_LEN,
                                             Tmax=MAX_LEN, eos=EOS, bos=BOS, pad=PAD, emb=g.emb, pos=g.pos, x=d["x"], slots=g.slots)
            else:
                ops.debug_decode_select(form, d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], max_len=MAX_LEN, Tmax=MAX_LEN,
                                        eos=EOS, bos=BOS, pad=PAD, emb=g.emb, pos=g.pos, x=d["x"], slots=g.slots)
        out.append([d[k].clone() for k in ("seqs", "logprobs", "step", "finished", "x")] + ([g.slots["t"].clone()] if slot else []))
        if guarded:
            assert int(g.loop["period"].abs().sum()) == 0 and int(g.loop["run"].max()) >= 1
    for u, w in zip(*out):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, w.view(torch.int32) if w.dtype == torch.float32 else w)


def test_refusals(dev):
    g = Guarded(dev, 2, 8, 2, 3)
    d = g.d

    def launch(**over):
        loop = dict(g.loop, **over)
        ops.debug_decode_loop_select(False, d["logits"], d["seqs"], d["logprobs"], d["step"], d["finished"], loop=loop, max_len=MAX_LEN,
                                     Tmax=MAX_LEN, eos=EOS, emb=g.emb, pos=g.pos, x=d["x"])
    for over, msg in ((dict(max_period=0), "max_period"), (dict(max_period=65), "max_period"), (dict(min_repeats=1), "min_repeats"),
                      (dict(min_tokens=0), "min_tokens"), (dict(rows=1), "rows"), (dict(run=None), "null loop")):
        with pytest.raises(RuntimeError, match=msg):
            launch(**over)
    assert torch.equal(d["step"].cpu(), torch.tensor([1, 0], dtype=torch.int32))   # nothing was launched
