"""Host-side helpers the callers on either side of the hot path use: the detokenise edge of inference and
the learning-rate schedules of the two training loops.  Pure Python / stock torch schedulers; they drive `optim.FusedAdamW` exactly as they
drive `torch.optim.AdamW` (only `param_groups[i]["lr"]` changes); and the image-side resize transforms (8f-2), whose arithmetic runs in a HIP
kernel."""
import math
from typing import NamedTuple

import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR

from .config import LMX_EOS_TOKEN


def stringify_lmx_seq(lmx_seq, idxs_to_tokens):
    """(T,) tensor of LMX token indices starting with <bos> -> one LMX string without <bos> / a trailing <eos>
    (acai_omr/utils/utils.py:194-202; consumer acai_omr/ui/routes.py:68-86)."""
    toks = [idxs_to_tokens[idx.item()] for idx in lmx_seq]
    if toks[-1] == LMX_EOS_TOKEN:
        toks.pop(-1)
    return " ".join(toks[1:])


def _pad_targets(target_lmx_seqs, pad_idx, device):
    """(padded int64 (N, L) targets on `device`, int32 (N,) lengths) from a list of 1-D tensors, or from a padded tensor and its pad_idx."""
    if isinstance(target_lmx_seqs, torch.Tensor):
        if pad_idx is None:
            raise ValueError("symbol_error_rate: a padded target tensor needs pad_idx")
        tgt = target_lmx_seqs.to(device=device, dtype=torch.int64)
        return tgt, (tgt != pad_idx).sum(dim=-1, dtype=torch.int32)
    lens = [int(t.shape[0]) for t in target_lmx_seqs]
    tgt = torch.zeros(len(lens), max(lens + [1]), dtype=torch.int64, device=device)
    for i, t in enumerate(target_lmx_seqs):
        tgt[i, :lens[i]] = t.to(device)
    return tgt, torch.tensor(lens, dtype=torch.int32).to(device)


def symbol_error_rate(seqs, seq_mask, target_lmx_seqs, pad_idx=None):
    """Symbol error rate of decoded rows: Levenshtein distance over LMX tokens (ops.edit_distance, on the device) summed over the rows, divided
    by the summed target lengths.  seqs / seq_mask (N, T): what inference(), continuous_inference() and beam search return.  Targets: a list of
    N 1-D tensors, or a right-padded (N, L) tensor with its pad_idx (a row's length is its count of non-pad entries).
    What is compared: seqs[i] at its seq_mask positions against target i, BOTH AS GIVEN - <bos> / <eos> count as symbols where present, so the
    caller strips them from both sides or from neither.  Returns (ser as a Python float - the one host sync, at the end; NaN when every target
    is empty -, distances int32 (N,), target_lens int32 (N,)); a zero-length target row contributes its row's length to the distances."""
    from . import ops
    tgt, target_lens = _pad_targets(target_lmx_seqs, pad_idx, seqs.device)
    if tgt.shape[0] != seqs.shape[0]:
        raise ValueError(f"symbol_error_rate: {seqs.shape[0]} decoded rows against {tgt.shape[0]} targets")
    distances = ops.edit_distance(seqs, seq_mask, tgt, target_lens)
    total = torch.stack([distances.sum(), target_lens.sum()]).tolist()
    return (total[0] / total[1] if total[1] else float("nan")), distances, target_lens


class ErrorBreakdown(NamedTuple):
    """symbol_error_breakdown's result: ser = sub_rate + ins_rate + del_rate as Python floats over the summed target lengths (NaN when every
    target is empty), counts int32 (N, 4) - matches, substitutions, insertions, deletions per row -, target_lens int32 (N,) and the
    ops.EditAlignment the counts come from."""
    ser: float
    sub_rate: float
    ins_rate: float
    del_rate: float
    counts: torch.Tensor
    target_lens: torch.Tensor
    alignment: tuple


def _rates(sums):
    """(ser, sub_rate, ins_rate, del_rate) from the host list [matches, substitutions, insertions, deletions, summed target lengths]."""
    _, s, i, d, total = sums
    if not total:
        return (float("nan"),) * 4
    return (s + i + d) / total, s / total, i / total, d / total


def symbol_error_breakdown(seqs, seq_mask, target_lmx_seqs, pad_idx=None):
    """symbol_error_rate split into its kinds of error -> ErrorBreakdown.  Arguments as symbol_error_rate takes them, and the same rule:
    seqs[i] at its seq_mask positions against target i, both as given, so <bos> / <eos> count where present.  The rows are aligned on the
    device (ops.edit_alignment: the canonical optimal alignment) and a substitution, an insertion (a decoded symbol the target does not have)
    and a deletion (a target symbol the decode dropped) are counted apart; `ser` is symbol_error_rate's value on the same inputs.  One host
    sync, at the end."""
    from . import ops
    tgt, target_lens = _pad_targets(target_lmx_seqs, pad_idx, seqs.device)
    if tgt.shape[0] != seqs.shape[0]:
        raise ValueError(f"symbol_error_breakdown: {seqs.shape[0]} decoded rows against {tgt.shape[0]} targets")
    al = ops.edit_alignment(seqs, seq_mask, tgt, target_lens)
    sums = torch.cat([al.counts.sum(dim=0, dtype=torch.int64), target_lens.sum(dtype=torch.int64).reshape(1)]).tolist()
    return ErrorBreakdown(*_rates(sums), al.counts, target_lens, al)


class TokenConfusions(NamedTuple):
    """token_confusions' result, each list sorted by falling count (then rising id) and cut to `top` entries with a count above zero:
    substitutions [(target id, predicted id, count)], deletions [(target id, count)], insertions [(predicted id, count)]."""
    substitutions: list
    deletions: list
    insertions: list


def token_confusions(alignment, seqs, targets, vocab_size, top=20):
    """Which symbols the errors of an alignment involve -> TokenConfusions.  alignment: the ops.EditAlignment of seqs (N, T) against targets -
    the padded (N, L) tensor the alignment was made with, or the list of 1-D tensors symbol_error_breakdown took (group 1).  The counts are
    formed on the device (torch.bincount over the alignment's indices) and read once.  Ids must lie in [0, vocab_size): ValueError otherwise
    (checked on the rows' aligned positions, with the same read); the substitution table has vocab_size^2 bins."""
    V, top = int(vocab_size), int(top)
    if V < 1 or top < 1:
        raise ValueError(f"token_confusions: vocab_size and top must be positive, got {vocab_size!r} and {top!r}")
    dev = alignment.pred_op.device
    if not isinstance(targets, torch.Tensor):
        targets, _ = _pad_targets(targets, None, dev)
    seqs, targets = seqs.to(dev), targets.to(dev)
    if alignment.pred_op.shape != seqs.shape or alignment.tgt_to_pred.shape != targets.shape:
        raise ValueError(f"token_confusions: alignment of widths {tuple(alignment.pred_op.shape)} / {tuple(alignment.tgt_to_pred.shape)} against "
                         f"seqs {tuple(seqs.shape)} and targets {tuple(targets.shape)}")
    op = alignment.pred_op
    sub, ins = op == 1, op == 2
    dele = (alignment.tgt_to_pred < 0) & (alignment.tgt_slot >= 0)
    if targets.shape[1]:
        partner = targets.gather(1, alignment.pred_to_tgt.clamp(min=0).long())
    else:
        partner = torch.zeros_like(seqs)
    bad = ((sub | ins) & ((seqs < 0) | (seqs >= V))).any() | (sub & ((partner < 0) | (partner >= V))).any() | (dele & ((targets < 0) | (targets >= V))).any()
    p, t, d = seqs.clamp(0, V - 1), partner.clamp(0, V - 1), targets.clamp(0, V - 1)
    # entries that are not of the kind go to one bin past the table
    sub_counts = torch.bincount(torch.where(sub, t * V + p, V * V).flatten(), minlength=V * V + 1)[:V * V]
    ins_counts = torch.bincount(torch.where(ins, p, V).flatten(), minlength=V + 1)[:V]
    del_counts = torch.bincount(torch.where(dele, d, V).flatten(), minlength=V + 1)[:V]
    parts = []
    for counts in (sub_counts, del_counts, ins_counts):
        c, idx = torch.sort(counts, descending=True, stable=True)   # (stable: equal counts keep the smaller id first)
        k = min(top, c.shape[0])
        parts += [c[:k], idx[:k]]
    host = torch.cat(parts + [bad.reshape(1).to(torch.int64)]).tolist()
    if host[-1]:
        raise ValueError(f"token_confusions: a token id outside [0, {V}) takes part in an error")
    out, o = [], 0
    for part in parts[::2]:
        k = part.shape[0]
        out.append([(i, c) for c, i in zip(host[o:o + k], host[o + k:o + 2 * k]) if c > 0])
        o += 2 * k
    return TokenConfusions([(i // V, i % V, c) for i, c in out[0]], out[1], out[2])


def error_token_weights(alignment, pred_lens):
    """The per-token weight of ViTOMR.error_maps from an ops.EditAlignment of decoded rows (B, T') against their targets -> fp32 (B, T'):
    w[i] = [pred_op[i] != 0] + the number of deleted target tokens whose tgt_slot, clamped to [1, L - 1], is i, with L = pred_lens (B,) the
    rows' lengths.  A substituted or inserted token is charged where it stands; a missing one to the output position where it should have
    been emitted - the token it is missing in front of, or the last one (<eos>) when it is missing at the end; never to index 0 (<bos>),
    which no decode step produced.  Device arithmetic only."""
    op = alignment.pred_op
    w = (op > 0).to(torch.float32)
    if op.shape[1] == 0 or alignment.tgt_slot.shape[1] == 0:
        return w
    deleted = (alignment.tgt_to_pred < 0) & (alignment.tgt_slot >= 0)
    last = (pred_lens.to(op.device).long() - 1)[:, None]
    pos = torch.minimum(alignment.tgt_slot.long().clamp(min=1), last).clamp(min=0, max=op.shape[1] - 1)
    return w.scatter_add_(1, pos, deleted.to(torch.float32))


def measure_accuracy(seqs, seq_mask, target_lmx_seqs, delimiters, pad_idx=None):
    """The share of the TARGET's measures that decoded rows reproduce without error -> (accuracy float, reproduced (N,), target measures (N,)).
    measures.measure_accuracy, where the rule is stated: every edit operation of the canonical alignment is charged to one target measure -
    a substitution to the measure of the target token it is aligned to, a deleted target token to its own, an inserted token to the measure
    of the target token the nearest earlier aligned pred token is aligned to - and a measure is reproduced when nothing is charged to it."""
    from .measures import measure_accuracy as impl
    return impl(seqs, seq_mask, target_lmx_seqs, delimiters, pad_idx)


def confidence_error_auroc(score, is_error, mask):
    """How well a per-token score separates the aligned errors from the matches: the area under the ROC curve of `score` (any shape; higher =
    more suspect: 1 - exp(log_prob), entropy, rank, ...) as a detector of is_error (bool, e.g. EditAlignment.pred_op != 0) over the tokens
    that `mask` (bool) selects and whose score is not NaN - the probability that a random error scores above a random match, ties counting
    half.  Rank-based (Mann-Whitney) on the device, tied scores given their average rank, in float64; one host read.  NaN when either class
    is empty.  0.5 is chance; what trained checkpoints reach has not been measured."""
    s = score.reshape(-1).to(torch.float64)
    keep = mask.reshape(-1).to(s.device).bool() & ~torch.isnan(s)
    pos = is_error.reshape(-1).to(s.device).bool() & keep
    big = torch.finfo(torch.float64).max
    s = torch.where(keep, s.clamp(max=big), torch.full_like(s, float("inf")))   # what is left out sorts behind every kept score
    v, _ = torch.sort(s)
    lo = torch.searchsorted(v, s, right=False)
    hi = torch.searchsorted(v, s, right=True)
    rank = (lo + hi + 1).to(torch.float64) * 0.5   # ranks lo + 1 .. hi share their mean
    n_pos, n = pos.sum().to(torch.float64), keep.sum().to(torch.float64)
    u = torch.where(pos, rank, torch.zeros_like(rank)).sum() - n_pos * (n_pos + 1) * 0.5
    return (u / (n_pos * (n - n_pos))).item()


def stepwise_cosine_anneal_with_warmup(optimizer, warmup_steps, total_epochs, final_lr, num_steps_per_epoch):
    """Linear warm-up from 0.5 % of the base LR, then cosine annealing to final_lr, stepped per minibatch (utils.py:204-208)."""
    warmup = LinearLR(optimizer, start_factor=5e-3, end_factor=1.0, total_iters=warmup_steps)
    anneal = CosineAnnealingLR(optimizer, T_max=total_epochs * num_steps_per_epoch - warmup_steps, eta_min=final_lr)
    return SequentialLR(optimizer, schedulers=[warmup, anneal], milestones=[warmup_steps])


def cosine_anneal_with_warmup(optimizer, warmup_epochs, total_epochs, final_lr, num_train_batches=None):
    """The schedule of pre_train.py:107 (per epoch) and omr_teacher_force_train.py:210 (per minibatch when num_train_batches is given)
    (utils.py:212-222)."""
    if not num_train_batches:
        warmup = LinearLR(optimizer, start_factor=5e-3, end_factor=1.0, total_iters=warmup_epochs)
        anneal = CosineAnnealingLR(optimizer, T_max=total_epochs - warmup_epochs, eta_min=final_lr)
        return SequentialLR(optimizer, schedulers=[warmup, anneal], milestones=[warmup_epochs])
    warm = warmup_epochs * num_train_batches
    warmup = LinearLR(optimizer, start_factor=5e-3, end_factor=1.0, total_iters=warm)
    anneal = CosineAnnealingLR(optimizer, T_max=(total_epochs - warmup_epochs) * num_train_batches, eta_min=final_lr)
    return SequentialLR(optimizer, schedulers=[warmup, anneal], milestones=[warm])


def ragged_collate_fn(batch):
    """DataLoader collate for ragged (image, target) examples: the model layer packs them itself (utils.py:225-229)."""
    return list(batch)


# ---- image-side transforms ------------------------------------------------------------------------------------------------
def dynamic_resize_target(height, width, patch_size, max_seq_len):
    """Target (height, width) of `DynamicResize.forward` (acai_omr/utils/utils.py:343-349): integer aspect ratio (floor division), the short
    side = patch_size * floor(sqrt(max_seq_len / aspect)), the long side = short * aspect."""
    if width > height:
        aspect_ratio = width // height
        target_height = patch_size * math.floor(math.sqrt(max_seq_len / aspect_ratio))
        target_width = target_height * aspect_ratio
    else:
        aspect_ratio = height // width
        target_width = patch_size * math.floor(math.sqrt(max_seq_len / aspect_ratio))
        target_height = target_width * aspect_ratio
    return target_height, target_width


def _center_crop(img, out_h, out_w):
    """torchvision `center_crop` for an image at least as large as the crop (the only case DynamicResize reaches, utils.py:360-364):
    top = round((H - out_h) / 2), left = round((W - out_w) / 2) (Python banker's rounding, as torchvision computes them)."""
    h, w = img.shape[-2], img.shape[-1]
    if out_h > h or out_w > w:
        raise ValueError("center crop larger than the image")
    top, left = int(round((h - out_h) / 2.0)), int(round((w - out_w) / 2.0))
    return img[..., top:top + out_h, left:left + out_w]


def _device_image(img, device=None):
    """GPU tensors stay on THEIR device; CPU tensors are uploaded to `device` (default: the current GPU)."""
    if not torch.is_tensor(img) or img.dim() != 3:
        raise TypeError("expected a C x H x W tensor (decode PIL images with ToImage / ToDtype first, as the reference pipelines do)")
    if not torch.cuda.is_available():
        raise RuntimeError("acai_omr_amd transforms run on the GPU (HIP resize kernel); there is no CPU fallback")
    if img.is_cuda:
        return img.to(dtype=torch.float32).contiguous()
    return img.to(device=device if device is not None else torch.device("cuda", torch.cuda.current_device()), dtype=torch.float32).contiguous()


class PackedPatches:
    """A batch of images as the encoder's projection GEMM wants it: the nn.Unfold(P, P) rows of every image in ONE packed [sum N, P*P] tensor
    (fp32, or bf16 for an autocast encoder) plus the patch grid (h_p, w_p) of each image.  `DynamicResize.to_patches` / `resize_batch_to_patches`
    produce it straight from the resize kernel; `Encoder` / `OMREncoder` / `FineTuneOMREncoder` (`forward`, `forward_packed`) and the
    `inference()` entry point accept it wherever they accept a list of image tensors.
    A PRUNED stream (`prune.prune_patches`, an extension) holds only the rows of the patches that were kept: `dims` stay the FULL grids,
    `kept_lens` is the host list of rows per image, `kept` the packed int32 device tensor of their local indices r * w_p + c (ascending within
    an image), and `pe_index` the int32 device tensor of the rows they gather from a positional table of `pe_grid` = (rows, columns) with the
    grids of images beyond it appended in image order (Encoder._pe_packed).  All four are None on a stream that was not pruned."""

    def __init__(self, patches, dims, patch_size, kept=None, kept_lens=None, pe_index=None, pe_grid=None):
        self.patches, self.dims, self.patch_size = patches, [tuple(d) for d in dims], patch_size
        self.kept, self.kept_lens, self.pe_index = kept, None if kept_lens is None else [int(n) for n in kept_lens], pe_index
        self.pe_grid = None if pe_grid is None else (int(pe_grid[0]), int(pe_grid[1]))
        if self.pruned and (kept_lens is None or pe_index is None or pe_grid is None or len(self.kept_lens) != len(self.dims)):
            raise ValueError("a pruned PackedPatches needs kept, kept_lens (one per image), pe_index and pe_grid")

    def __len__(self):
        return len(self.dims)

    @property
    def pruned(self):
        return self.kept is not None

    @property
    def lens(self):
        """Rows per image: the kept counts of a pruned stream, h_p * w_p otherwise."""
        return list(self.kept_lens) if self.pruned else [h * w for h, w in self.dims]

    def _beyond(self, dims):
        """The rows that the images of `dims` whose grid exceeds pe_grid append to the positional table."""
        return sum(h * w for h, w in dims if h > self.pe_grid[0] or w > self.pe_grid[1])

    def slice(self, i0, i1):
        """Images i0 .. i1 - 1 as a `PackedPatches` over a view of the same rows (what a chunked encode takes one chunk at a time)."""
        i0, i1 = max(0, min(int(i0), len(self.dims))), max(0, min(int(i1), len(self.dims)))
        if self.pruned:
            r0, n = sum(self.kept_lens[:i0]), sum(self.kept_lens[i0:i1])
            pe, skipped = self.pe_index[r0:r0 + n], self._beyond(self.dims[:i0])
            if skipped:   # the appended grids of the images in front of the slice are no longer there
                table_rows = self.pe_grid[0] * self.pe_grid[1]
                pe = torch.where(pe >= table_rows, pe - skipped, pe)
            return PackedPatches(self.patches[r0:r0 + n], self.dims[i0:i1], self.patch_size, self.kept[r0:r0 + n], self.kept_lens[i0:i1], pe, self.pe_grid)
        r0 = sum(h * w for h, w in self.dims[:i0])
        return PackedPatches(self.patches[r0:r0 + sum(h * w for h, w in self.dims[i0:i1])], self.dims[i0:i1], self.patch_size)


class PatchDivisibleResize(torch.nn.Module):
    """`PatchDivisibleResize` (acai_omr/utils/utils.py:309-330): resize to the nearest lower patch-divisible size, bicubic + antialias, on the GPU.
    Takes a C x H x W tensor (CPU tensors are uploaded once); returns a GPU tensor."""

    def __init__(self, patch_size, device=None):
        super().__init__()
        self.patch_size = patch_size
        self.device = device   # extension: target GPU for CPU inputs (default: the current device)

    def forward(self, img):
        from . import ops
        img = _device_image(img, self.device)
        _, h, w = img.shape
        new_w = max(w // self.patch_size * self.patch_size, self.patch_size)
        new_h = max(h // self.patch_size * self.patch_size, self.patch_size)
        return ops.resize_bicubic_aa(img, (new_h, new_w))


class DynamicResize(torch.nn.Module):
    """`DynamicResize` (acai_omr/utils/utils.py:334-367): same constructor and the same arithmetic -- target size from the integer aspect ratio and
    the sequence budget, bicubic antialiased resize, optional centre crop to the positional-embedding grid, clamp to [0, 1] -- with the resize and
    the clamp in one HIP launch pair on the GPU.  Takes the float C x H x W tensor the reference's `ToImage -> ToDtype(float32, scale=True)`
    produce (a CPU tensor is uploaded once; this replaces the per-example `.to(device)` of `pre_train.py:56`) and returns a GPU tensor."""

    def __init__(self, patch_size, max_seq_len, pe_max_height, pe_max_width, crop_imgs, device=None):
        super().__init__()
        self.device = device   # extension: target GPU for CPU inputs (default: the current device)
        self.patch_size = patch_size
        self.max_seq_len = max_seq_len
        self.pe_max_height = pe_max_height
        self.pe_max_width = pe_max_width
        self.crop_imgs = crop_imgs

    def forward(self, img):
        from . import ops
        img = _device_image(img, self.device)
        target_height, target_width = dynamic_resize_target(img.shape[-2], img.shape[-1], self.patch_size, self.max_seq_len)
        img = ops.resize_bicubic_aa(img, (target_height, target_width), clamp01=True)
        if self.crop_imgs:
            if target_height / self.patch_size > self.pe_max_height:
                img = _center_crop(img, self.pe_max_height * self.patch_size, img.shape[-1])
            if target_width / self.patch_size > self.pe_max_width:
                img = _center_crop(img, img.shape[-2], self.pe_max_width * self.patch_size)
            img = img.contiguous()
        return img


    # ---- extension (second half): resize straight into the packed patch stream -----------------------------------------------
    def _plan(self, h, w):
        """Target size of `forward` for an h x w input and the centre-crop window (top, left, height, width) inside it."""
        th, tw = dynamic_resize_target(h, w, self.patch_size, self.max_seq_len)
        ch, cw = th, tw
        if self.crop_imgs:
            if th / self.patch_size > self.pe_max_height:
                ch = self.pe_max_height * self.patch_size
            if tw / self.patch_size > self.pe_max_width:
                cw = self.pe_max_width * self.patch_size
        top, left = int(round((th - ch) / 2.0)), int(round((tw - cw) / 2.0))
        return (th, tw), (top, left, ch, cw)

    def to_patches(self, imgs, dtype=torch.float32):
        """`forward` + the encoder's Unfold in one step for a LIST of images: every image - a (1,H,W) / (H,W) float tensor in [0,1] or a uint8
        tensor (what `v2.ToImage` yields; `ToDtype(float32, scale=True)`'s 1/255 is applied on load) - is resized, clamped, cropped and written
        as patch rows of ONE packed tensor by the resize kernel's height pass.  Returns a `PackedPatches` the encoders accept directly;
        patchify(forward(img)) gives the same rows bit for bit."""
        from . import ops
        if torch.is_tensor(imgs):
            imgs = [imgs]
        dev_imgs, plans = [], []
        for img in imgs:
            if not torch.is_tensor(img) or img.dim() not in (2, 3):
                raise TypeError("expected (1,H,W) or (H,W) tensors")
            if not torch.cuda.is_available():
                raise RuntimeError("acai_omr_amd transforms run on the GPU (HIP resize kernel); there is no CPU fallback")
            d = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            t = img if img.is_cuda else img.to(d)
            t = (t if t.dtype == torch.uint8 else t.to(torch.float32)).contiguous()
            dev_imgs.append(t)
            plans.append(self._plan(t.shape[-2], t.shape[-1]))
        P = self.patch_size
        dims = [(crop[2] // P, crop[3] // P) for _, crop in plans]
        out = torch.empty(sum(h * w for h, w in dims), P * P, dtype=dtype, device=dev_imgs[0].device)
        r0 = 0
        for t, (size, crop) in zip(dev_imgs, plans):
            r0 += ops.resize_to_patches(t, size, P, out, r0, crop=crop, clamp01=True)
        return PackedPatches(out, dims, P)
