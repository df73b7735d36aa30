"""Probe inputs for the variable-length attention kernels, and a float64 reference that can be broken on purpose.

On randn data every key holds about 1/lk of a row's probability, so an addressing defect at an edge (a zero-filled key past the ragged end
that is not masked, the neighbouring packed sequence's first key read into this one, the last key of a ragged tile skipped, a tail query
row lost to dK / dV) moves the result by about 1/lk: at or below what a bf16 comparison must allow.  The inputs built here give up the first
four columns of every head so that each of those defects moves the result by many times the tolerance instead:

  columns 0, 1  parity  queries of sequence s carry A_q in column s % 2, its keys carry A_k in column 1 - s % 2: scores inside a sequence
                        are unchanged, any key of a neighbouring sequence scores A_q A_k / sqrt(dh) ~ 30 nats more and takes the whole row
  column 2      shift   queries carry +A_q, keys -A_k: every real score drops by ~30 nats, which softmax ignores; a zero-filled phantom key
                        scores 0 and takes the whole row (-43 in the log2 domain: far inside the zero-reference kernels' 2^+-100 window)
  column 3      edge    queries carry C = 2.  Not causal: the keys at the tile edges carry boost sqrt(dh) / C, boost = ln(lk / (2 n_edges)) nats,
                        so that together they hold about a third of each row.  Causal: key j carries slope (j - (lk - 1)) sqrt(dh) / C,
                        slope = min(0.25, 40 / lk) nats per key, a ramp on which the diagonal key is the heaviest visible one and the
                        key just past the diagonal would be heavier still.

A few query rows at the block edges get a loud `dout`, so that one of them going missing from dK / dV shows.

How the amplitudes were set (tests/test_attn_probe_cpu.py holds every shape to the factor of four they were set for):
  * A_k = 2 and A_q = 30 sqrt(dh) / 2, not A_q = A_k: in dQ = dS K a component common to all keys of a row multiplies the bf16 rounding of
    dS, while the exact sum cancels (rows of dS sum to zero).  With A on both sides, an emulation of bf16 dS rounding alone came to 0.9 of the
    backward tolerance in the reserved columns of dq on the smallest shape; with the small factor on the keys it is 0.15.
  * the ordinary query columns are randn / 2: with scores spread by a whole nat, equally boosted keys differ by e^+-1 in weight, and the
    lighter ones' dK / dV fell short of four tolerances of the heaviest one's.
  * four loud rows (first, 64, 256, last) with a factor of 32: dK / dV of an edge key sum over the loud rows, so one row lost out of n
    changes them by ~1 / sqrt(n) of their maximum; eleven rows at 16 reached 3.8.
  * causal: the ramp ends at zero instead of starting there, and the loud rows are 0 and the last two.  With the ramp rising from zero the
    loud last row's keys shared ~16 nats of column 3; times the rounding of the bf16 output in delta that came to 1.9 backward tolerances
    in dq's reserved columns on the MI355X (0.5 - 0.9 in a CPU emulation of the bf16 roundings alone), from a correct kernel.

Everything is CPU torch."""
import math

import torch

A_KEY = 2.0             # the keys' parity and shift amplitude
Q_STD = 0.5             # the queries' ordinary columns: scores spread by ~0.5 nat, so that equally boosted keys weigh about the same
C_EDGE = 2.0            # the queries' column 3
LOUD = 32.0             # dout factor of the loud edge query rows
SLOPE_MAX = 0.25        # nats per key of the causal ramp, at most (40 nats over the whole sequence)
FILL = 7.0              # what guarded outputs hold before the kernel runs
EDGE_KEYS = (0, 1, 31, 32, 63, 64, 127, 128, -2, -1)
LOUD_ROWS = (0, 64, 256, -1)
LOUD_ROWS_CAUSAL = (0, -2, -1)


def amplitude(dh):
    """(A_q, A_k) with A_q A_k / sqrt(dh) ~ 30 nats, small integers that bf16 holds exactly.  The keys carry the small factor: a component
    common to all keys of a row multiplies the rounding of dS into dQ, where the exact sum over the keys cancels to zero."""
    return float(round(30.0 * math.sqrt(dh) / A_KEY)), A_KEY


def _edges(positions, n):
    return sorted({p % n for p in positions if -n <= p < n})


def edge_keys(lk):
    return _edges(EDGE_KEYS, lk)


def loud_rows(lq, causal=False):
    """(Causal: row 0 and the last two rows.  The ramp is zero at the last key, so the last rows' keys carry no large common component
    in column 3: a loud row's would multiply the rounding of its bf16 output, through delta, into dQ.  Row 0 sees one key, P = 1 and dS = 0
    exactly.  The last row but one is there because a mask that is off by one cannot show in the last row.)"""
    return _edges(LOUD_ROWS_CAUSAL if causal else LOUD_ROWS, lq)


def reserved_columns(H, dh):
    return torch.tensor([h * dh + c for h in range(H) for c in range(4)], dtype=torch.long)


def build(lens_q, lens_k, H, dh, dtype, causal, seed):
    """Packed q [sum(lens_q), H*dh], k, v [sum(lens_k), H*dh], dout like q: float32 tensors holding values of `dtype` exactly, so the
    reference and the kernel see the same numbers.  Also returns the indices of the reserved columns."""
    assert dh >= 8, "four reserved columns must leave ordinary ones"
    E = H * dh
    g = torch.Generator().manual_seed(seed)
    q, dout = torch.randn(sum(lens_q), E, generator=g) * Q_STD, torch.randn(sum(lens_q), E, generator=g)
    k, v = torch.randn(sum(lens_k), E, generator=g), torch.randn(sum(lens_k), E, generator=g)
    (Aq, Ak), rt, C = amplitude(dh), math.sqrt(dh), C_EDGE
    qh, kh = q.view(-1, H, dh), k.view(-1, H, dh)
    qh[:, :, :4] = 0.0
    kh[:, :, :4] = 0.0
    qh[:, :, 2], kh[:, :, 2] = Aq, -Ak
    qh[:, :, 3] = C
    oq = ok = 0
    for s, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        qh[oq:oq + lq, :, s % 2] = Aq
        kh[ok:ok + lk, :, 1 - s % 2] = Ak
        if causal:
            slope = min(SLOPE_MAX, 40.0 / lk)
            kh[ok:ok + lk, :, 3] = (slope * rt / C * (torch.arange(lk, dtype=torch.float32) - (lk - 1)))[:, None]
        else:
            ed = edge_keys(lk)
            boost = max(0.0, math.log(lk / (2.0 * len(ed))))
            kh[[ok + j for j in ed], :, 3] = boost * rt / C
        dout[[oq + i for i in loud_rows(lq, causal)]] *= LOUD
        oq += lq
        ok += lk
    q, k, v, dout = (t.to(dtype).float() for t in (q, k, v, dout))
    return q, k, v, dout, reserved_columns(H, dh)


def guarded(t, rows=64, kind="out", dh=None, fill=FILL):
    """`t` in the middle of an allocation with `rows` guard rows in front of it and behind it; returns the middle as a view (the whole is
    its `_base`, see guards_hold).  The guards are finite and hostile: kind "k" (needs dh): keys with A in both parity columns and 0 in the
    shift column, which outweigh every real key by ~60 nats, +-1 elsewhere; "q", "v", "dout": +-8; "out": `fill` everywhere, the middle
    included (pass an empty tensor of the output's shape and dtype).  Never NaN or Inf: a kernel may load past the end and multiply by a
    probability that is exactly zero."""
    n = t.shape[0]
    whole = torch.empty((n + 2 * rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    if kind == "out":
        whole.fill_(fill)
        return whole[rows:rows + n]
    g = torch.Generator().manual_seed(n + rows)
    guard = (torch.randint(0, 2, (2 * rows,) + tuple(t.shape[1:]), generator=g).float() * 2.0 - 1.0) * (1.0 if kind == "k" else 8.0)
    if kind == "k":
        gh = guard.view(2 * rows, -1, dh)
        gh[:, :, 0] = gh[:, :, 1] = amplitude(dh)[1]
        gh[:, :, 2] = 0.0
    else:
        assert kind in ("q", "v", "dout"), kind
    guard = guard.to(t.dtype).to(t.device)
    whole[:rows], whole[rows + n:] = guard[:rows], guard[rows:]
    mid = whole[rows:rows + n]
    mid.copy_(t)
    return mid


def guards_hold(view, rows=64, fill=FILL):
    """No guard row of a guarded output was written."""
    whole, n = view._base, view.shape[0]
    return bool((whole[:rows] == fill).all()) and bool((whole[rows + n:] == fill).all())


def all_written(view, fill=FILL):
    """Every row of a guarded output was written: none still holds the fill in all its elements."""
    return not bool((view.reshape(view.shape[0], -1) == fill).all(dim=1).any())


def reference(q, k, v, lens_q, lens_k, H, dh, causal, defect=None):
    """Float64 softmax attention over packed sequences in differentiable torch (q, k, v that require grad receive gradients through the
    result).  Returns out [sum(lens_q), H*dh] and lse [H, sum(lens_q)], the log2 of the row sums of 2^(score log2 e).  `defect` breaks it:
      ("drop_key", seq, j)        key j of sequence seq (negative: from the end) is not attended to
      ("leak_key_after", seq)     the first key of sequence seq + 1 is attended to as well
      ("leak_key_before", seq)    the last key of sequence seq - 1 is attended to as well
      ("phantom_zero_key", seq)   an all-zero key with an all-zero value is attended to as well
      ("lose_query_row", seq, i)  row i's output is zero, so under any loss its contribution to dK / dV (and its dQ) vanishes
      ("causal_offset", d)        key j is visible to row i when j <= i + d"""
    kind = defect[0] if defect else None
    assert kind in (None, "drop_key", "leak_key_after", "leak_key_before", "phantom_zero_key", "lose_query_row", "causal_offset"), kind
    q, k, v = q.double(), k.double(), v.double()
    B = len(lens_q)
    off_k = [0]
    for lk in lens_k:
        off_k.append(off_k[-1] + lk)
    outs, lses = [], []
    oq = 0
    for s, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        ok = off_k[s]
        hit = defect is not None and kind != "causal_offset" and defect[1] == s
        ks, vs = k[ok:ok + lk], v[ok:ok + lk]
        vis = torch.ones(lq, lk, dtype=torch.bool)
        if causal:
            vis = vis.tril(defect[1] if kind == "causal_offset" else 0)
        extra = None
        if hit and kind == "drop_key":
            vis[:, defect[2] % lk] = False
        elif hit and kind == "leak_key_after":
            assert s + 1 < B
            extra = off_k[s + 1]
        elif hit and kind == "leak_key_before":
            assert s > 0
            extra = ok - 1
        if extra is not None:
            ks, vs = torch.cat([ks, k[extra:extra + 1]]), torch.cat([vs, v[extra:extra + 1]])
        elif hit and kind == "phantom_zero_key":
            ks, vs = torch.cat([ks, torch.zeros_like(ks[:1])]), torch.cat([vs, torch.zeros_like(vs[:1])])
        if ks.shape[0] > lk:
            vis = torch.cat([vis, torch.ones(lq, 1, dtype=torch.bool)], 1)
        empty = ~vis.any(-1, keepdim=True)       # (a row that sees no key gives zeros)
        row_o, row_l = [], []
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            sc = q[oq:oq + lq, sl] @ ks[:, sl].t() / math.sqrt(dh)
            sc = sc.masked_fill(~vis, float("-inf")).masked_fill(empty, 0.0)
            o = (torch.softmax(sc, -1) * (~empty)) @ vs[:, sl]
            if hit and kind == "lose_query_row":
                keep = torch.ones(lq, 1, dtype=torch.float64)
                keep[defect[2] % lq] = 0.0
                o = o * keep
            row_o.append(o)
            row_l.append(torch.logsumexp(sc, -1) / math.log(2.0))
        outs.append(torch.cat(row_o, 1))
        lses.append(torch.stack(row_l))
        oq += lq
    return torch.cat(outs), torch.cat(lses, 1)


def gradients(q, k, v, dout, lens_q, lens_k, H, dh, causal, defect=None):
    """out, lse, dq, dk, dv of `reference` under the loss sum(out * dout), by autograd in float64."""
    qr, kr, vr = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    out, lse = reference(qr, kr, vr, lens_q, lens_k, H, dh, causal, defect)
    (out * dout.double()).sum().backward()
    return out.detach(), lse.detach(), qr.grad, kr.grad, vr.grad


def compare(got, ref, tol, reserved):
    """The worst |got - ref| / (tol max(1, max |ref|)), taken separately over the ordinary and over the reserved columns, each against
    its own maximum: the parity and shift columns of dK are genuinely ~10 times larger than the rest and must not loosen the tolerance
    of the ordinary columns."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and got.dim() == 2
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    res = torch.zeros(ref.shape[1], dtype=torch.bool)
    res[reserved] = True
    worst = 0.0
    for cols in (res, ~res):
        if bool(cols.any()):
            g, r = got[:, cols], ref[:, cols]
            worst = max(worst, float((g - r).abs().max()) / (tol * max(1.0, float(r.abs().max()))))
    return worst


# The shapes of tests/test_gpu_attn_edges.py, (H, dh, lens_q, lens_k or None, causal): the smallest that reach each kernel form.
# tests/test_attn_probe_cpu.py shows on each of them that every defect above moves the reference by at least four times the tolerance.
FWD_GENERIC = [
    (2, 16, [65, 64], None, True),
    (3, 32, [130, 1, 77], None, False),
    (4, 12, [7, 12], [20, 13], False),
    (4, 16, [7, 12], [20, 13], False),
    (2, 64, [300], None, True),
    (2, 8, [130, 1, 77], None, False),          # the four reserved columns still leave ordinary ones
]
FWD_TWO_BLOCK = [                               # bf16, prescaled, d_h <= 32, max_q >= 512
    (3, 32, [513, 640, 1], None, False),
    (2, 32, [600, 513], [1000, 577], False),
    (2, 24, [520], [64], False),
]
FWD_64 = [                                      # bf16, prescaled, d_h = 64, no mask: attn_fwd64.hip, wide + tail
    (2, 64, [513, 130], [1100, 64], False),
    (1, 64, [40, 129, 192], [40, 65, 191], False),          # (the tail kernel is launched and finds no last block of <= 32 rows)
    (1, 64, [256], [1], False),                             # (equal lengths, a multiple of 256: the wide kernel alone)
    (2, 64, [288, 289, 20], [700, 64, 1], False),
    (1, 64, [513] * 3, [1100] * 3, False),
]
BWD_GENERIC = [
    (2, 16, [65, 64], None, True),
    (2, 32, [333, 128], None, False),
    (1, 64, [256], [400], False),
    (4, 12, [7, 12], [20, 13], False),
    (2, 8, [130, 77], None, False),
]
BWD_TWO_BLOCK = [                               # bf16, prescaled, d_h <= 32, max_q, max_k >= 512
    (2, 32, [513, 700], None, False),
    (2, 32, [600, 513], [1000, 577], False),
    (1, 24, [1025], [512], False),
]
BWD_ONE_PASS_EQUAL = [                          # attn_bwd1p.hip with equal lengths (the above reach its ragged launches)
    (2, 32, [1024, 1024], None, False),
    (2, 32, [600, 600], [1536, 1536], False),
]
BWD_64 = [                                      # bf16, prescaled, d_h = 64, max_q >= 256: attn_bwd64w.hip + the one-block tails
    (2, 64, [513, 700], None, False),
    (2, 64, [600, 256, 40], [1000, 577, 300], False),
    (2, 64, [768], [129], False),                           # (no rows past the full query blocks, no full key block: never the wide dK / dV)
]
BWD_ACCUMULATE = [(2, 64, [300], [513], False)]
FWD_CASES = FWD_GENERIC + FWD_TWO_BLOCK + FWD_64
BWD_CASES = BWD_GENERIC + BWD_TWO_BLOCK + BWD_ONE_PASS_EQUAL + BWD_64 + BWD_ACCUMULATE


def case_id(c):
    H, dh, lq, lk, causal = c
    return f"H{H}-dh{dh}-q{'_'.join(map(str, lq))}" + (f"-k{'_'.join(map(str, lk))}" if lk else "") + ("-causal" if causal else "")


def case_seed(c):
    H, dh, lq, lk, causal = c
    return H * dh + sum(lq) + 3 * sum(lk or lq) + (1 if causal else 0)
