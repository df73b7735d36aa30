"""The loop guard's rule by brute force (not a test module): direct comparison of index ranges, no run counters, so that it shares nothing
with the kernels' method (csrc/decode_select.hip loop_check, csrc/loops.hip).

The rule (include/acai_omr_hip.h at AcaiLoop): need(p) = max((R - 1) p, M); index 0 is <bos> and never takes part; a row fires at the first t
for which some p in 1 .. P has seq[i] == seq[i - p] for the need(p) indices i = t - need(p) + 1 .. t, with i - p >= 1; the smallest p wins;
the report is (stop = t, period = p, start = t - need(p) - p + 1)."""


def need(p, R, M):
    return max((R - 1) * p, M)


def due_at(seq, t, P, R, M, armed=1):
    """The periods due at index t of seq (a list of ints), ascending.  armed: the first index whose comparison counts - 1 for a row guarded
    from its start (the rule); a later index states what counters zeroed at that index see (the selection test stages a tie with it)."""
    out = []
    for p in range(1, P + 1):
        n = need(p, R, M)
        lo = t - n + 1                      # the need(p) indices lo .. t against lo - p .. t - p
        if lo >= armed and lo - p >= 1 and seq[lo:t + 1] == seq[lo - p:t + 1 - p]:
            out.append(p)
    return out


def fires_at(seq, t, P, R, M, armed=1):
    """(period, start) of the smallest period due at index t, or None."""
    due = due_at(seq, t, P, R, M, armed)
    return (due[0], t - need(due[0], R, M) - due[0] + 1) if due else None


def first_loop(seq, P, R, M):
    """(stop, period, start) of the first firing over the whole of seq, or None.  Every token is a token like any other (acai_repeat_scan)."""
    for t in range(1, len(seq)):
        hit = fires_at(seq, t, P, R, M)
        if hit:
            return (t,) + hit
    return None


def loop_end(seq, stop, period):
    """The last index up to which seq[i] == seq[i - period] keeps holding from stop on (acai_repeat_scan's `end`)."""
    e = stop
    while e + 1 < len(seq) and seq[e + 1] == seq[e + 1 - period]:
        e += 1
    return e


def scan_rows(rows, P, R, M, lens=None):
    """acai_repeat_scan over a list of rows -> four lists (stop, period, start, end), zeros for a row that never fires."""
    out = ([], [], [], [])
    for n, row in enumerate(rows):
        seq = list(row) if lens is None else list(row)[:max(0, min(int(lens[n]), len(row)))]
        hit = first_loop(seq, P, R, M)
        vals = (0, 0, 0, 0) if hit is None else hit + (loop_end(seq, hit[0], hit[1]),)
        for o, v in zip(out, vals):
            o.append(v)
    return out


def decode_stop(seq, P, R, M, eos, cap=None):
    """How a guarded greedy row ends, given the tokens the unguarded row emits: ("loop", stop, period, start) at the first firing whose token
    is not <eos>, ("eos", t) at the first <eos>, else ("cap", cap - 1): index cap - 1 was reached first (cap None: len(seq))."""
    cap = len(seq) if cap is None else min(cap, len(seq))
    for t in range(1, cap):
        if seq[t] == eos:
            return ("eos", t)
        hit = fires_at(seq, t, P, R, M)
        if hit:
            return ("loop", t) + hit
    return ("cap", cap - 1)


def run_counters(seq, t, P, armed=1):
    """run_p(t) for p = 1 .. 64 by direct comparison (0 past P): the 64 counters the selection kernel holds after index t of a live row
    (armed: as in due_at)."""
    out = []
    for p in range(1, 65):
        k = 0
        while p <= P and t - k >= armed and t - k - p >= 1 and seq[t - k] == seq[t - k - p]:
            k += 1
        out.append(k)
    return out


def golden_rows(name, precision="ref_fp32"):
    """The reference's greedy rows of a committed fixture, as lists."""
    import os

    import torch
    fx = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".pt"), map_location="cpu", weights_only=False)
    return fx[precision]["seqs"].tolist()
