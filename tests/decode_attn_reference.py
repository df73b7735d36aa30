"""Float64 reference of the decode self-attention forms and of the rollout-group cross attention, the builders that lay their caches out,
and the cases of tests/test_gpu_decode_self_attn.py.  Everything is CPU torch.

A case holds the operands exactly as acai_debug_decode_self_attn / acai_debug_decode_attn_group take them, and `reference` resolves logical
key p of row b to a cache location from THOSE operands alone, as include/acai_omr_hip.h and csrc/decode_internal.h state it:

  plain      [b][h][p], len = step[1] + 1
  ancestor   cache row anc[step[0] & 1][b][p], position p, len = step[1] + 1
  ring       position (first[b] + p) % Tmax of row b, len = row_len[b]
  spec       image i = b / R, table entry e = tab[i][p]: cache row i R + (e & 7), position e >> 3;
             row j of the image attends over max(1, min(t[i] + j, pitch, chunk nsplit)) keys
  group      row b attends over the ragged K/V of image b / group: key p of head h at seq_off + (h len + p) dhp

The builders start from logical sequences (SEQS of them, each with its keys, values and up to eight queries) and lay the same logical keys
out in each form's way, so that a table form and the plain form can be compared bit for bit.  What they guarantee:
  * every cache element no logical key maps to is NaN in its first dh columns - positions at and past the length, rows no lineage points to,
    the targets of the unused parity copy - so a wrong read poisons the result;
  * the pad columns d >= dh of K and V are zero everywhere, as in the engine's caches (0 * NaN in a score would poison a correct kernel);
  * table entries past the length name an in-range location that holds NaN, never a wild index: a wrong read must not fault the card;
  * outputs are built by `guarded_out`: pre-filled with a sentinel, between guard rows.

`reference(case, defect=...)` breaks the reference on purpose (tests/test_decode_attn_reference_cpu.py measures what each defect moves):
  drop_last_key             every row attends over one key fewer (a row of one key is left with none: 0 / 0)
  one_key_past_len          every row attends over logical key `len` as well (where the table has such an entry)
  ring_no_wrap              ring positions first + p are not reduced modulo Tmax
  other_parity              the ancestor form reads the other parity copy of its table
  spec_row_len_not_offset   every row of an image attends over t keys, not t + j
  group_rows_swapped        rows 2i and 2i + 1 of an image exchange their queries
A location past the cache's end reads as NaN, and a result that is not finite counts as moved without bound."""
import math

import torch

import attn_probe

H, TMAX = 2, 130
LENGTHS = [1, 7, 8, 9, 32, 33, 63, 64, 65, 127, 128, 129, 130]   # edges of keys per wave / workgroup pass / unrolled iteration / split, Tmax
FORMS = [("bf16", 64), ("bf16", 32), ("bf16", 12), ("fp32", 64), ("fp32", 12)]   # lanes per key 8, 4, 2, 16, 4
SPLITS = [(256, 1), (64, 3)]
BAR = 2e-5              # absolute; q = 2 randn, k, v = randn (tests/test_gpu_kernels.py::test_decode_attn, test_cross_form_vs_float64)
SEQS, SEQ_LEN = 4, 264  # logical sequences; the longest speculative row attends over chunk nsplit = 256 keys
GUARD_ROWS = 8
DEFECTS = {
    "plain": ["drop_last_key", "one_key_past_len"],
    "ancestor": ["drop_last_key", "one_key_past_len", "other_parity"],
    "ring": ["drop_last_key", "one_key_past_len", "ring_no_wrap"],
    "spec": ["drop_last_key", "one_key_past_len", "spec_row_len_not_offset"],
    "group_mean": ["drop_last_key", "one_key_past_len"],
    "group_onehot": ["group_rows_swapped"],
}


def defects_for(case):
    """The defects that apply to a case (a group of one row has no rows to swap)."""
    fam = "group_" + case.kind if case.form == "group" else case.form
    return [d for d in DEFECTS[fam] if not (d == "group_rows_swapped" and case.group < 2)], fam


GROUP_MEMS = {1: [1, 31, 32, 33, 63, 65, 300], 2: [1, 31, 32, 33, 63, 65, 300], 16: [1, 32, 33, 300], 17: [31, 33, 65, 300], 33: [1, 63, 300]}
GROUP_SPLITS = [(64, 5), (512, 1)]   # chunk 64 with tickets; one split
ONE_HOT_NATS = 40.0


def form_id(f):
    return f"{f[0]}_dh{f[1]}"


def dhp_of(dh):
    return max(16, 1 << (dh - 1).bit_length())


def rb(x):
    return x.to(torch.bfloat16).float()


class Case:
    """Operands of one launch (CPU tensors; caches float32 holding values of `dtype` exactly) and `logical`: per row (q [H, dh], k [H, len,
    dh], v [H, len, dh]), what the row attends over however the form lays it out."""

    def __init__(self, **kw):
        self.step = self.row_len = self.table = self.seq_off = self.seq_len = None
        self.pitch = self.stride = self.group = 0
        self.__dict__.update(kw)


_LOGICAL = {}


def logical(dtype, dh):
    """q [SEQS, 8, H, dh] = 2 randn; k, v [SEQS, H, SEQ_LEN, dh] = randn rounded to the cache dtype."""
    if (dtype, dh) not in _LOGICAL:
        g = torch.Generator().manual_seed(1000 * dh + (1 if dtype == "bf16" else 0))
        q = torch.randn(SEQS, 8, H, dh, generator=g) * 2
        k, v = torch.randn(SEQS, H, SEQ_LEN, dh, generator=g), torch.randn(SEQS, H, SEQ_LEN, dh, generator=g)
        if dtype == "bf16":
            k, v = rb(k), rb(v)
        _LOGICAL[(dtype, dh)] = (q, k, v)
    return _LOGICAL[(dtype, dh)]


def _empty_cache(rows, dh):
    dhp = dhp_of(dh)
    c = torch.zeros(rows, H, TMAX, dhp)
    c[..., :dh] = float("nan")
    return c, c.clone()


def _rows_of(dtype, dh, rows, lens):
    """rows: (sequence, query) per launch row -> q [B, H * dh] and the logical triples."""
    q, k, v = logical(dtype, dh)
    qq = torch.stack([q[s, j].reshape(H * dh) for s, j in rows])
    return qq, [(q[s, j], k[s, :, :n], v[s, :, :n]) for (s, j), n in zip(rows, lens)]


def build_plain(dtype, dh, L, rows=((0, 0), (1, 0), (2, 0))):
    """Every row has L keys (step[1] is the launch's)."""
    kc, vc = _empty_cache(len(rows), dh)
    q, log = _rows_of(dtype, dh, rows, [L] * len(rows))
    for b, (_, k, v) in enumerate(log):
        kc[b, :, :L, :dh], vc[b, :, :L, :dh] = k, v
    return Case(form="plain", dtype=dtype, dh=dh, q=q, kc=kc, vc=vc, step=torch.tensor([L - 1, L - 1], dtype=torch.int32), logical=log,
                rows=list(rows), lens=[L] * len(rows))


def build_ancestor(dtype, dh, L, parity, identity=False, rows=((0, 0), (1, 0), (2, 0))):
    """B rows over a cache of 2 B rows.  Scattered: the key at position p of row b sits in cache row (2 b + p // 3) % 2B - the lineages hop
    every three positions and never meet - and the other parity copy names the row after it, which holds NaN there.  pitch = Tmax + 6."""
    B, R2, pitch = len(rows), 2 * len(rows), TMAX + 6
    kc, vc = _empty_cache(R2, dh)
    q, log = _rows_of(dtype, dh, rows, [L] * B)
    tab = torch.empty(2, R2, pitch, dtype=torch.int32)
    p = torch.arange(pitch)
    for r in range(R2):
        live = ((torch.full_like(p, r) if identity else 2 * r + p // 3) % R2).to(torch.int32) if r < B else torch.full((pitch,), R2 - 1, dtype=torch.int32)
        tab[parity, r] = live
        tab[1 - parity, r] = (live + (B if identity else 1)) % R2   # (identity: rows B .. 2B - 1 are never written)
    for b, (_, k, v) in enumerate(log):
        rr, pp = tab[parity, b, :L].long(), torch.arange(L)
        kc[rr, :, pp, :dh], vc[rr, :, pp, :dh] = k.transpose(0, 1), v.transpose(0, 1)
    return Case(form="ancestor", dtype=dtype, dh=dh, q=q, kc=kc, vc=vc, step=torch.tensor([4 + parity, L - 1], dtype=torch.int32), table=tab,
                pitch=pitch, stride=R2 * pitch, logical=log, rows=list(rows), lens=[L] * B)


def ring_firsts(lens, variant):
    """The ring starts: by turns a window that fits without wrapping, one that wraps in its middle, one that starts at Tmax - 1 and one that
    ends exactly at Tmax - 1; a row of full length starts at 77."""
    first = []
    for i, n in enumerate(lens):
        kind = (i + variant) % 4
        if n == TMAX:
            first.append(77)
        elif kind == 0:
            first.append((TMAX - n) // 2)
        elif kind == 1:
            first.append(TMAX - n // 2 if n >= 2 else TMAX - 1)
        elif kind == 2:
            first.append(TMAX - 1)
        else:
            first.append(TMAX - n)
    return first


def build_ring(dtype, dh, variant=0, identity=False, lens=LENGTHS):
    """One row per length; row i reads sequence i % SEQS."""
    B = len(lens)
    rows = [(i % SEQS, 0) for i in range(B)]
    first = [0] * B if identity else ring_firsts(lens, variant)
    kc, vc = _empty_cache(B, dh)
    q, log = _rows_of(dtype, dh, rows, lens)
    for b, (_, k, v) in enumerate(log):
        pos = (first[b] + torch.arange(lens[b])) % TMAX
        kc[b][:, pos, :dh], vc[b][:, pos, :dh] = k, v
    return Case(form="ring", dtype=dtype, dh=dh, q=q, kc=kc, vc=vc, row_len=torch.tensor(lens, dtype=torch.int32),
                table=torch.tensor(first, dtype=torch.int32), logical=log, rows=rows, lens=list(lens))


def spec_len(t, j, pitch, cover):
    return max(1, min(t + j, pitch, cover))


def build_spec(dtype, dh, R, ts, pitch, cover, identity=False):
    """len(ts) images of R rows; image i verifies sequence i % SEQS from t = ts[i], row j with query j.  Scattered: key p sits at position
    (37 p + 11) % Tmax of the image's row (p + p // Tmax) % R (one to one for p < 2 Tmax).  identity: key p at position p of row 0.  Entries
    past the longest row name the location beside key 0, which holds NaN."""
    I = len(ts)
    rows = [(i % SEQS, j) for i in range(I) for j in range(R)]
    lens = [spec_len(ts[i], j, pitch, cover) for i in range(I) for j in range(R)]
    assert max(lens) <= (TMAX if identity else min(2 * TMAX, SEQ_LEN)) and R <= 8
    kc, vc = _empty_cache(I * R, dh)
    q, log = _rows_of(dtype, dh, rows, lens)
    _, k, v = logical(dtype, dh)
    tab = torch.empty(I, pitch, dtype=torch.int32)
    for i in range(I):
        n = max(lens[i * R:(i + 1) * R])
        p = torch.arange(n)
        pos, row = (p, torch.zeros(n, dtype=torch.long)) if identity else ((37 * p + 11) % TMAX, (p + p // TMAX) % R)
        tab[i] = 8 * int(pos[0]) + (int(row[0]) + 1) % R
        tab[i, :n] = (8 * pos + row).to(torch.int32)
        s = i % SEQS
        kc[i * R + row, :, pos, :dh], vc[i * R + row, :, pos, :dh] = k[s, :, :n].transpose(0, 1), v[s, :, :n].transpose(0, 1)
    return Case(form="spec", dtype=dtype, dh=dh, q=q, kc=kc, vc=vc, row_len=torch.tensor(ts, dtype=torch.int32), table=tab, pitch=pitch,
                stride=R, cover=cover, logical=log, rows=rows, lens=lens)


def spec_cases(dtype, dh, cover):
    """(id, case): rows on both sides of the length edges; `pitch_cuts`: pitch 128 below t + j; `cover_cuts`: chunk nsplit below t + j and
    below the pitch (rows longer than the cache: the table names positions twice, in different rows)."""
    return [("R3", build_spec(dtype, dh, 3, [7, 31, 63, 127], TMAX, cover)),
            ("R8_t1", build_spec(dtype, dh, 8, [1], TMAX, cover)),
            ("R8_t58", build_spec(dtype, dh, 8, [58], TMAX, cover)),
            ("R8_pitch_cuts", build_spec(dtype, dh, 8, [125], 128, cover)),
            ("R8_cover_cuts", build_spec(dtype, dh, 8, [cover - 4], cover + 8, cover)),
            ("R3_identity", build_spec(dtype, dh, 3, [7, 31, 63, 127], TMAX, cover, identity=True))]


def build_group(dh, group, kind, mems=None):
    """bf16, d_h padded to 64.  One image per memory length, `group` rows each; the images' K/V blocks lie between stretches of NaN.
    kind "mean": q = 0, so every probability is 1 / len exactly; "onehot": K = +-1, row g of an image has q = 32 K[(7 g + 3) % len], which
    puts at least ONE_HOT_NATS nats on that key alone (checked here).  Either way bf16 holds the kernel's probabilities exactly."""
    mems = GROUP_MEMS[group] if mems is None else mems
    dhp, gap = 64, 16 * 64
    g = torch.Generator().manual_seed(7 * dh + group + (0 if kind == "mean" else 1))
    total = gap + sum(H * n * dhp + gap for n in mems)
    kc, vc = torch.zeros(total // dhp, dhp), torch.zeros(total // dhp, dhp)
    kc[:, :dh] = vc[:, :dh] = float("nan")
    offs, qs, log, o = [], [], [], gap
    for n in mems:
        k = rb(torch.randn(H, n, dh, generator=g)) if kind == "mean" else torch.randint(0, 2, (H, n, dh), generator=g).float() * 2 - 1
        v = rb(torch.randn(H, n, dh, generator=g))
        kc[o // dhp:o // dhp + H * n, :dh], vc[o // dhp:o // dhp + H * n, :dh] = k.reshape(H * n, dh), v.reshape(H * n, dh)
        for r in range(group):
            q = torch.zeros(H, dh) if kind == "mean" else 32.0 * k[:, (7 * r + 3) % n]
            if kind == "onehot" and n > 1:
                sc = torch.einsum("hd,hnd->hn", q.double(), k.double()) / math.sqrt(dh)
                top = sc[:, (7 * r + 3) % n].clone()
                sc[:, (7 * r + 3) % n] = float("-inf")
                assert float((top - sc.max(-1).values).min()) >= ONE_HOT_NATS
            qs.append(q.reshape(H * dh))
            log.append((q, k, v))
            offs.append(o)
        o += H * n * dhp + gap
    lens = [n for n in mems for _ in range(group)]
    return Case(form="group", kind=kind, dtype="bf16", dh=dh, q=torch.stack(qs), kc=kc.reshape(-1), vc=vc.reshape(-1), group=group,
                seq_off=torch.tensor(offs, dtype=torch.int64), seq_len=torch.tensor(lens, dtype=torch.int32), logical=log, lens=lens)


def one_hot_targets(case):
    """[B, H * dh]: the V row each rollout row of a "onehot" group case selects."""
    return torch.stack([v[:, (7 * (b % case.group) + 3) % v.shape[1]].reshape(-1) for b, (_, _, v) in enumerate(case.logical)]).double()


def _key_rows(case, b, h, defect):
    """Indices of row b's keys for head h into the cache seen as rows of dhp elements (one past the end: a row of NaN)."""
    f, dh = case.form, case.dh
    if f == "group":
        b0 = b // case.group * case.group
        n, base = int(case.seq_len[b0]), int(case.seq_off[b0]) // 64
        n = n - 1 if defect == "drop_last_key" else n + 1 if defect == "one_key_past_len" else n
        return base + h * int(case.seq_len[b0]) + torch.arange(n)
    if f == "plain":
        n = int(case.step[1]) + 1
    elif f == "ancestor":
        n = int(case.step[1]) + 1
    elif f == "ring":
        n = int(case.row_len[b])
    else:
        R = case.stride
        t = int(case.row_len[b // R])
        n = spec_len(t, 0 if defect == "spec_row_len_not_offset" else b % R, case.pitch, case.cover)
    if defect == "drop_last_key":
        n -= 1
    if defect == "one_key_past_len" and (f in ("plain", "ring") or n < case.pitch):
        n += 1
    p = torch.arange(n)
    if f == "plain":
        row, pos = torch.full((n,), b), p
    elif f == "ancestor":
        par = (int(case.step[0]) & 1) ^ (1 if defect == "other_parity" else 0)
        row, pos = case.table[par, b, :n].long(), p
    elif f == "ring":
        pos = int(case.table[b]) + p
        row, pos = torch.full((n,), b), pos if defect == "ring_no_wrap" else pos % TMAX
    else:
        e = case.table[b // R, :n].long()
        row, pos = b // R * R + torch.clamp(e & 7, max=R - 1), torch.clamp(e >> 3, max=TMAX - 1)
    return (row * H + h) * TMAX + pos


def reference(case, defect=None):
    """softmax(q k^T / sqrt(dh)) v in float64, [B, H * dh], the keys found through the case's operands."""
    assert defect is None or any(defect in d for d in DEFECTS.values()), defect
    dh = case.dh
    dhp = case.kc.shape[-1] if case.form != "group" else 64
    kf, vf = case.kc.reshape(-1, dhp).double(), case.vc.reshape(-1, dhp).double()
    nan = torch.full((1, dhp), float("nan"), dtype=torch.float64)
    kf, vf = torch.cat([kf, nan]), torch.cat([vf, nan])
    q = case.q.double()
    if defect == "group_rows_swapped":
        q = q.clone()
        for b in range(0, q.shape[0]):
            g = b % case.group
            if g % 2 == 0 and g + 1 < case.group:
                q[[b, b + 1]] = q[[b + 1, b]]
    out = torch.empty(q.shape[0], H * dh, dtype=torch.float64)
    for b in range(q.shape[0]):
        for h in range(H):
            idx = torch.clamp(_key_rows(case, b, h, defect), max=kf.shape[0] - 1)
            if idx.numel() == 0:
                out[b, h * dh:(h + 1) * dh] = float("nan")
                continue
            s = kf[idx, :dh] @ q[b, h * dh:(h + 1) * dh] / math.sqrt(dh)
            out[b, h * dh:(h + 1) * dh] = torch.softmax(s, 0) @ vf[idx, :dh]
    return out


def naive(case):
    """The same result from the logical rows alone, one key at a time (no table, no cache, no softmax call)."""
    dh = case.dh
    out = torch.empty(len(case.logical), H * dh, dtype=torch.float64)
    for b, (q, k, v) in enumerate(case.logical):
        q, k, v = q.double(), k.double(), v.double()
        for h in range(H):
            sc = [float(q[h] @ k[h, p]) / math.sqrt(dh) for p in range(k.shape[1])]
            m = max(sc)
            w = [math.exp(s - m) for s in sc]
            acc = torch.zeros(dh, dtype=torch.float64)
            for p, wp in enumerate(w):
                acc += wp * v[h, p]
            out[b, h * dh:(h + 1) * dh] = acc / sum(w)
    return out


def fp32_torch(case):
    """Plain fp32 torch on the logical rows: what a correct fp32 implementation leaves of the bar."""
    dh = case.dh
    out = torch.empty(len(case.logical), H * dh)
    for b, (q, k, v) in enumerate(case.logical):
        s = torch.einsum("hd,hnd->hn", q.float(), k.float()) / math.sqrt(dh)
        out[b] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v.float()).reshape(-1)
    return out


def moved(a, ref):
    """max |a - ref|; infinite when `a` is not finite (a read of NaN: the result is poisoned, which no comparison lets through)."""
    return float((a - ref).abs().max()) if bool(torch.isfinite(a).all()) else float("inf")


def guarded_out(B, cols, dtype=torch.float32, device="cpu"):
    return attn_probe.guarded(torch.empty(B, cols, dtype=dtype, device=device), rows=GUARD_ROWS, kind="out")


def intact(out):
    """Guards untouched, every row written, nothing NaN."""
    return (attn_probe.guards_hold(out, rows=GUARD_ROWS) and attn_probe.all_written(out) and bool(torch.isfinite(out.float()).all()))


def self_cases(dtype, dh, cover):
    """(id, case) of every self-form launch the GPU file compares with float64 at one (chunk, nsplit), chunk nsplit = cover."""
    cs = [(f"plain_L{L}", build_plain(dtype, dh, L)) for L in LENGTHS]
    cs += [(f"ring_v{v}", build_ring(dtype, dh, v)) for v in (0, 1)]
    cs += [(f"ancestor_L{L}_par{par}", build_ancestor(dtype, dh, L, par)) for L in LENGTHS for par in (0, 1)]
    cs += [("spec_" + n, c) for n, c in spec_cases(dtype, dh, cover)]
    return cs


def group_cases():
    return [(f"group{g}_dh{dh}_{kind}", build_group(dh, g, kind)) for g in GROUP_MEMS for dh in (64, 48) for kind in ("mean", "onehot")]
