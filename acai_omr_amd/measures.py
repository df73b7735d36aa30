"""Per-measure results (an extension; no reference counterpart): what the per-token passes know - confidence, cross-attention, edit
alignment - reduced over the spans between delimiter tokens.  LMX opens every measure with a `measure` token, so a span is a measure.

The segmentation and every reduction run on the device (ops.token_segments, ops.segment_reduce, ops.attn_map_segment_sum, ops.attn_map_locate,
ops.attn_map_extent), inside the combined confidence + alignment pass (ViTOMR._confidence_packed), where the flat map buffer exists; one copy
to the host per report: the segment counts, which size the layout of the measure maps.

Whether cross-attention localises measures on trained checkpoints, which layers, heads or weight do it best, and what measure confidence
separates right from wrong have not been measured: no threshold is shipped."""
import torch

from . import engine as EG
from . import ops

MEASURE_WEIGHTS = ("surprisal", "entropy")


class MeasureConfig:
    """How rows are cut and what is reported.  delimiters: the tokens that OPEN a span - token strings resolved through the decoder's
    vocabulary, or ids - 1 to 8 of them; quantile: q of the box, 0 <= q < 0.5 (the box spans the q .. 1 - q mass of the measure map per
    axis); weight: the per-token weight of the measure map - None (uniform), "surprisal" (-log_prob), "entropy", or a (B, T') real tensor of
    which the scored entries are read; max_measures: segment slots per row (a row with more is marked in MeasureReport.overflowed and its
    first max_measures are reported); return_maps: keep the measure maps in the report.  ValueError for anything else."""

    def __init__(self, delimiters=("measure",), quantile=0.05, weight=None, max_measures=256, return_maps=False):
        if isinstance(delimiters, (str, int)) or torch.is_tensor(delimiters):
            delimiters = [delimiters] if not torch.is_tensor(delimiters) else delimiters.reshape(-1).tolist()
        try:
            delimiters = tuple(delimiters)
        except TypeError:
            raise ValueError(f"delimiters must be 1 .. {ops.SEGMENT_MAX_DELIMS} token strings or ids, got {delimiters!r}") from None
        if not 1 <= len(delimiters) <= ops.SEGMENT_MAX_DELIMS or any(isinstance(d, bool) or not isinstance(d, (str, int)) for d in delimiters):
            raise ValueError(f"delimiters must be 1 .. {ops.SEGMENT_MAX_DELIMS} token strings or ids, got {delimiters!r}")
        try:
            quantile = float(quantile)
        except (TypeError, ValueError):
            raise ValueError(f"quantile must be a number with 0 <= quantile < 0.5, got {quantile!r}") from None
        if not 0.0 <= quantile < 0.5:
            raise ValueError(f"quantile must satisfy 0 <= quantile < 0.5, got {quantile}")
        if isinstance(weight, str):
            if weight not in MEASURE_WEIGHTS:
                raise ValueError(f"weight must be None, one of {MEASURE_WEIGHTS} or a (B, T') tensor, got {weight!r}")
        elif weight is not None and (not torch.is_tensor(weight) or weight.dim() != 2 or weight.dtype.is_complex or weight.dtype == torch.bool):
            raise ValueError(f"weight must be None, one of {MEASURE_WEIGHTS} or a real (B, T') tensor, got {type(weight).__name__}")
        if isinstance(max_measures, bool) or not isinstance(max_measures, int) or not 1 <= max_measures <= 65535:
            raise ValueError(f"max_measures must be an int in 1 .. 65535, got {max_measures!r}")
        self.delimiters, self.quantile, self.weight, self.max_measures, self.return_maps = delimiters, quantile, weight, max_measures, bool(return_maps)

    def resolve(self, decoder, shape=None):
        """The delimiters as token ids of `decoder`'s vocabulary (ValueError for an unknown string or an id outside it); with `shape`, a
        weight tensor is held against the sequences' shape."""
        ids = []
        for d in self.delimiters:
            if isinstance(d, str):
                if d not in decoder.tokens_to_idxs:
                    raise ValueError(f"delimiter {d!r} is not in the decoder's vocabulary")
                d = decoder.tokens_to_idxs[d]
            if not 0 <= d < decoder.vocab_size:
                raise ValueError(f"delimiter id {d} lies outside [0, {decoder.vocab_size})")
            ids.append(int(d))
        if shape is not None and torch.is_tensor(self.weight) and tuple(self.weight.shape) != tuple(shape):
            raise ValueError(f"weight is a {tuple(self.weight.shape)} tensor for sequences of shape {tuple(shape)}")
        return ids

    def __repr__(self):
        w = self.weight if not torch.is_tensor(self.weight) else f"tensor{tuple(self.weight.shape)}"
        return (f"MeasureConfig(delimiters={self.delimiters}, quantile={self.quantile}, weight={w!r}, max_measures={self.max_measures}, "
                f"return_maps={self.return_maps})")


class MeasureReport:
    """Per-measure results of B rows, padded to M = the batch's largest reported count.  Entries past a row's count are NaN (floats), -1
    (integers) or False.
      count (B,) int64          the TRUE number of measures; overflowed (B,) bool: it exceeds max_measures, of which the first are reported
      bounds (B, M, 2) int64    token indices [start, end): start is the delimiter, end the next delimiter or the row's <eos> / end
      n_tokens (B, M) int64     end - start
      mean_log_prob, min_log_prob (B, M) fp32; weakest_token (B, M) int64: the index of the lowest log-probability (the first on ties)
      mean_entropy, max_entropy (B, M) fp32 in nats
      forced (B, M) int64       tokens with rank > 0: not the model's arg-max (a grammar or a beam chose them)
      center_px, spread_px (B, M, 2) fp32   centroid (x, y) and standard deviations of the measure map, pixels of the input tensor
      box_px (B, M, 4) fp32     x0, y0, x1, y1: per axis where the map's running mass crosses q and 1 - q (ops.attn_map_extent), in pixels
      maps                      None, or per image the (count_i, h_p * w_p) fp32 measure maps (MeasureConfig.return_maps)
      errors (B, M, 3) int64    with targets: substitutions, insertions, deletions that fall into the measure; correct (B, M) bool: none does;
      outside_errors (B, 3)     the errors before the first delimiter and from the <eos> on.  errors.sum(1) + outside_errors equals the
                                alignment's counts[:, 1:] exactly (for rows that did not overflow).  None without targets.
    A token index that carries no score (index 0) adds 0 to the sums.  grids: the images' patch grids; delimiters: the resolved ids.
    Map rows exist for token indices 1 .. L - 1 only, and the spans are taken to map rows on the device (bounds minus one), where the kernel
    clamps them to the image's block instead of refusing them: a delimiter AT INDEX 0 - only possible when <bos> is a delimiter or a row does
    not start with <bos> - gives a measure whose map leaves that token out, and when the next delimiter follows at index 1 the span has no
    map row at all: its map is all zero, and centre, spread and box are 0, not NaN.  n_tokens and the confidence figures still count it."""

    __slots__ = ("count", "overflowed", "bounds", "n_tokens", "mean_log_prob", "min_log_prob", "weakest_token", "mean_entropy", "max_entropy",
                 "forced", "center_px", "spread_px", "box_px", "maps", "errors", "correct", "outside_errors", "grids", "delimiters")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return (f"MeasureReport(rows={self.count.shape[0]}, M={self.bounds.shape[1]}, delimiters={self.delimiters}, "
                f"errors={'yes' if self.errors is not None else None}, maps={'yes' if self.maps is not None else None})")


def deletion_positions(alignment, width):
    """Per pred position the number of deleted target tokens charged to it (int32 (B, width)): a deleted target token with tgt_slot = s counts
    at index max(s - 1, 0), the last pred token consumed before it.  Integer index_add on the device."""
    B = alignment.pred_op.shape[0]
    out = torch.zeros(B, max(width, 1), dtype=torch.int32, device=alignment.pred_op.device)
    if alignment.tgt_slot.shape[1] and width:
        deleted = (alignment.tgt_to_pred < 0) & (alignment.tgt_slot >= 0)
        pos = (alignment.tgt_slot.long() - 1).clamp(min=0, max=width - 1)
        out.view(-1).index_add_(0, (pos + torch.arange(B, device=pos.device)[:, None] * out.shape[1]).view(-1), deleted.to(torch.int32).view(-1))
    return out[:, :width]


class report_hook:
    """The callable ViTOMR._confidence_packed takes as `measure`: builds the MeasureReport from the pass's state and keeps it in `.report`."""

    def __init__(self, config, alignment=None):
        self.config, self.alignment, self.report = config, alignment, None

    def __call__(self, vitomr, **state):
        self.report = build_report(vitomr, self.config, self.alignment, **state)


def build_report(vitomr, config, alignment, *, seqs, Ls, rows, lens_t, own, conf, grids, patch_size, lens_s, kept):
    """The MeasureReport of one combined pass.  seqs (B, T'), Ls the rows' lengths, rows / lens_t the images that have map rows and how many,
    own = (flat map buffer, offsets, offsets on the device, columns per image) over the memory's own patches (None: no image has a map),
    conf the pass's TokenConfidence, kept / lens_s the packed kept indices and kept counts of a pruned stream (kept None: not pruned)."""
    dec = vitomr.decoder
    dev = dec.pos_embedding.device
    seqs = seqs.to(dev)
    B, Tp = seqs.shape
    cap = config.max_measures
    delims = config.resolve(dec, seqs.shape)
    f32, i64 = torch.float32, torch.int64
    if Tp == 0 or B == 0:
        raise ValueError(f"measure report: sequences of shape {tuple(seqs.shape)}")
    lens = ops.h2d(torch.tensor(Ls, dtype=torch.int32), dev)
    seg, count, bounds = ops.token_segments(seqs, lens, delims, stop=dec.eos_idx, cap=cap)
    planes = [torch.nan_to_num(conf.log_prob, nan=0.0), torch.nan_to_num(conf.entropy, nan=0.0), (conf.rank > 0).to(f32)]
    if alignment is not None:
        if tuple(alignment.pred_op.shape) != (B, Tp):
            raise ValueError(f"measure report: an alignment of width {tuple(alignment.pred_op.shape)} for sequences {tuple(seqs.shape)}")
        planes += [(alignment.pred_op == 1).to(f32), (alignment.pred_op == 2).to(f32), deletion_positions(alignment, Tp).to(f32)]
    stats = ops.segment_reduce(torch.stack(planes).contiguous(), bounds, count)
    counts = [int(c) for c in count.tolist()]                      # the one copy to the host: it sizes everything below
    n = [min(c, cap) for c in counts]
    M = max(n)
    valid = torch.arange(M, device=dev)[None, :] < ops.h2d(torch.tensor(n, dtype=i64), dev)[:, None]
    fl = lambda t: torch.where(valid, t[:, :M], torch.full((), float("nan"), dtype=f32, device=dev))   # noqa: E731
    it = lambda t: torch.where(valid, t[:, :M].long(), torch.full((), -1, dtype=i64, device=dev))   # noqa: E731
    bnd = torch.where(valid[..., None], bounds[:, :M].long(), torch.full((), -1, dtype=i64, device=dev))
    ntok = bnd[..., 1] - bnd[..., 0]
    ntok_f = ntok.clamp(min=1).to(f32)
    rep = MeasureReport(count=count.long(), overflowed=count > cap, bounds=bnd, n_tokens=torch.where(valid, ntok, -torch.ones_like(ntok)),
                        mean_log_prob=fl(stats.sum[0] / _pad(ntok_f, cap)), min_log_prob=fl(stats.min[0]), weakest_token=it(stats.argmin[0]),
                        mean_entropy=fl(stats.sum[1] / _pad(ntok_f, cap)), max_entropy=fl(stats.max[1]), forced=it(stats.sum[2]),
                        grids=list(grids), delimiters=tuple(delims))
    if alignment is not None:
        err = torch.stack([stats.sum[3], stats.sum[4], stats.sum[5]], dim=-1)[:, :M].long()     # 0/1 and small counts: exact in fp32
        rep.errors = torch.where(valid[..., None], err, torch.full((), -1, dtype=i64, device=dev))
        rep.correct = (err.sum(-1) == 0) & valid
        out_of = (seg < 0).to(f32)
        rep.outside_errors = torch.stack([(p * out_of).sum(-1) for p in planes[3:]], dim=-1).long()
    # ---- where each measure looked: the tokens' maps summed over the span, then located and boxed
    P = float(patch_size)
    rep.center_px, rep.spread_px = (torch.full((B, M, 2), float("nan"), dtype=f32, device=dev) for _ in range(2))
    rep.box_px = torch.full((B, M, 4), float("nan"), dtype=f32, device=dev)
    maps = [torch.zeros(0, h * w, dtype=f32, device=dev) for h, w in grids]
    seg_counts = [n[i] for i in rows]
    if own is not None and sum(seg_counts):
        out, offs, map_off, sub_s = own
        pick = ops.h2d(torch.tensor([i * cap + m for i in rows for m in range(n[i])], dtype=i64), dev)
        ranges = (bounds.view(B * cap, 2).index_select(0, pick) - 1).contiguous()     # map row t belongs to token index t + 1
        w = _packed_weight(config.weight, conf, rows, Ls, dev)
        cu_t, cu_s = EG.cu_from_lens(lens_t, dev), EG.cu_from_lens(sub_s, dev)
        mout, moffs, mseg_off, cu_seg = ops.attn_map_segment_sum(out, map_off, cu_t, cu_s, w, ranges, seg_counts, layout=(lens_t, sub_s, offs),
                                                                 check_ranges=False)
        if kept is not None:   # a pruned stream: the measure maps speak of the full grid before anything reads them
            mout, moffs, mseg_off, sub_s = vitomr._expand_maps(mout, moffs, rows, seg_counts, sub_s, lens_s, kept, grids)
            cu_s = EG.cu_from_lens(sub_s, dev)
        gw = [grids[i][1] for i in rows]
        _, loc = ops.attn_map_locate(mout, mseg_off, cu_seg, cu_s, gw, max(seg_counts), sum(seg_counts))
        ext = ops.attn_map_extent(mout, mseg_off, cu_seg, cu_s, gw, config.quantile, layout=(seg_counts, sub_s, moffs))
        put = ops.h2d(torch.tensor([i * M + m for i in rows for m in range(n[i])], dtype=i64), dev)
        rep.center_px.view(B * M, 2)[put] = loc[:, 2:4] * P
        rep.spread_px.view(B * M, 2)[put] = loc[:, 4:6] * P
        rep.box_px.view(B * M, 4)[put] = ext * P
        for i, o, c, s in zip(rows, moffs, seg_counts, sub_s):
            maps[i] = mout[o:o + c * s].view(c, s)
    rep.maps = maps if config.return_maps else None
    return rep


def _pad(t, cap):
    """(B, M) -> (B, cap) with ones: the divisor of the slots that are cut off afterwards."""
    return torch.nn.functional.pad(t, (0, cap - t.shape[1]), value=1.0)


def _packed_weight(weight, conf, rows, Ls, dev):
    """The per-token weight of the measure maps, packed like the map rows (row t of image i is token index t + 1); None: uniform."""
    if weight is None:
        return None
    src = -conf.log_prob if weight == "surprisal" else conf.entropy if weight == "entropy" else weight.to(device=dev, dtype=torch.float32)
    return torch.cat([src[i, 1:Ls[i]] for i in rows]).contiguous()


def measure_accuracy(seqs, seq_mask, target_lmx_seqs, delimiters, pad_idx=None):
    """The share of the TARGET's measures that the decoded rows reproduce without error -> (accuracy as a Python float - the one host sync;
    NaN without a target measure -, reproduced int64 (N,), target measures int64 (N,)).  seqs / seq_mask and the targets as
    utils.symbol_error_rate takes them (both sides as given: <bos> / <eos> count where present); delimiters: 1 .. 8 token ids.  The rule:
    the target rows are cut at the delimiters (a row ends at its length; tokens before the first delimiter belong to no measure), the rows
    are aligned (ops.edit_alignment), and every edit operation is charged to one target measure - a substitution to the measure of the
    target token it is aligned to (pred_to_tgt); a deleted target token to its own measure; an inserted pred token to the measure of the
    target token that the nearest earlier aligned (matched or substituted) pred token is aligned to, and to none when there is no such
    token.  A measure is reproduced when nothing is charged to it.  A missing delimiter is a deletion inside the measure it would have
    opened; an extra one is an insertion inside the measure before it.  No model is needed: ops.token_segments, ops.edit_alignment and
    ops.segment_reduce only."""
    from .utils import _pad_targets
    tgt, tgt_len = _pad_targets(target_lmx_seqs, pad_idx, seqs.device)
    if tgt.shape[0] != seqs.shape[0]:
        raise ValueError(f"measure_accuracy: {seqs.shape[0]} decoded rows against {tgt.shape[0]} targets")
    N, Lt = tgt.shape
    if Lt == 0 or N == 0:   # (a padded target tensor without a column: no target measure)
        none = torch.zeros(N, dtype=torch.int64, device=tgt.device)
        return float("nan"), none, none.clone()
    al = ops.edit_alignment(seqs, seq_mask, tgt, tgt_len)
    _, count, bounds = ops.token_segments(tgt, tgt_len, delimiters, stop=-1, cap=Lt)
    charged = torch.zeros(N, Lt, dtype=torch.int32, device=tgt.device)
    if al.pred_op.shape[1]:
        prev = torch.cummax(al.pred_to_tgt, dim=1).values          # aligned target indices rise along a row: the last one so far
        where = torch.where(al.pred_op == 1, al.pred_to_tgt, torch.where(al.pred_op == 2, prev, torch.full_like(prev, -1)))
        hit = where >= 0
        flat = where.clamp(min=0).long() + torch.arange(N, device=tgt.device)[:, None] * Lt
        charged.view(-1).index_add_(0, flat.view(-1), hit.to(torch.int32).view(-1))
    charged += ((al.tgt_to_pred < 0) & (al.tgt_slot >= 0)).to(torch.int32)
    stats = ops.segment_reduce(charged.to(torch.float32)[None].contiguous(), bounds, count)
    real = torch.arange(Lt, device=tgt.device)[None, :] < count[:, None]
    good = ((stats.sum[0] == 0) & real).sum(-1)
    total = torch.stack([good.sum(), count.sum()]).tolist()
    return (total[0] / total[1] if total[1] else float("nan")), good, count.long()
