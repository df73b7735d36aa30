"""numpy restatement of blank-patch pruning (acai_omr_amd/prune.py, csrc/prune.hip), the synthetic systems its tests run on, and the oracle
pipeline over a pruned stream.  A plain module: nothing here touches the GPU or the package's kernels."""
import numpy as np
import torch

PAPER_LO, PAPER_HI, INK_HI = 0.8, 1.0, 0.35     # paper noise in [0.8, 1.0), ink in [0, 0.35): nothing in [0.4, 0.6]


def patch_rows(img, P):
    """nn.Unfold(P, P) rows of one (H, W) image, H and W multiples of P: [h_p * w_p, P * P], row-major over the grid."""
    img = np.asarray(img)
    H, W = img.shape
    return img.reshape(H // P, P, W // P, P).transpose(0, 2, 1, 3).reshape((H // P) * (W // P), P * P)


def ink_counts(rows, ink_level):
    """Per row, the number of elements strictly below ink_level, compared in float32 (a NaN is not ink)."""
    return (np.asarray(rows, dtype=np.float32) < np.float32(ink_level)).sum(axis=1).astype(np.int32)


def keep_mask(ink, h_p, w_p, max_ink=0, halo=1):
    """The keep rule for ONE image: inked = ink > max_ink; keep = an inked patch within Chebyshev distance halo (inside the grid); an image
    without an inked patch keeps everything.  -> bool [h_p, w_p]."""
    inked = (np.asarray(ink).reshape(h_p, w_p) > max_ink)
    if not inked.any():
        return np.ones((h_p, w_p), dtype=bool)
    keep = np.zeros((h_p, w_p), dtype=bool)
    for r in range(h_p):
        for c in range(w_p):
            keep[r, c] = inked[max(r - halo, 0):r + halo + 1, max(c - halo, 0):c + halo + 1].any()
    return keep


def kept_indices(ink, dims, max_ink=0, halo=1):
    """Per image of a stream with grids dims, the ascending local indices r * w_p + c of its kept patches (int32 arrays)."""
    out, o = [], 0
    for h, w in dims:
        out.append(np.flatnonzero(keep_mask(ink[o:o + h * w], h, w, max_ink, halo).reshape(-1)).astype(np.int32))
        o += h * w
    return out


def pe_rows(kept, dims, pe_grid):
    """Per image, the rows its kept patches gather from the positional table of pe_grid = (rows, columns) with the grids of the images beyond
    it appended in image order."""
    pe_h, pe_w = pe_grid
    out, base = [], pe_h * pe_w
    for k, (h, w) in zip(kept, dims):
        r, c = k // w, k % w
        if h > pe_h or w > pe_w:
            out.append((base + r * w + c).astype(np.int32))
            base += h * w
        else:
            out.append((r * pe_w + c).astype(np.int32))
    return out


def compact(rows, kept, dims):
    """The kept rows of the stream, and the packed kept indices."""
    offs = np.cumsum([0] + [h * w for h, w in dims])
    sel = np.concatenate([o + k for o, k in zip(offs, kept)]) if kept else np.zeros(0, dtype=np.int64)
    return np.asarray(rows)[sel], (np.concatenate(kept) if kept else np.zeros(0, dtype=np.int32)), sel


def expand_map(m, kept, full):
    """(T, K) map over kept patches -> (T, full) with zeros at the dropped ones."""
    m = np.asarray(m)
    out = np.zeros((m.shape[0], full), dtype=m.dtype)
    out[:, kept] = m
    return out


def synthetic_system(seed, H, W, P, strokes=None):
    """A (1, H, W) float32 image: paper noise in [PAPER_LO, PAPER_HI) with ink rectangles in [0, INK_HI) - a few long thin horizontal ones
    ("staff lines") across the middle rows of patches and some short vertical ones ("stems")."""
    g = np.random.default_rng(seed)
    img = g.uniform(PAPER_LO, PAPER_HI, size=(H, W)).astype(np.float32)
    img = np.minimum(img, np.float32(0.999))
    h_p, w_p = H // P, W // P
    mid = h_p // 2
    x0, x1 = P + int(g.integers(0, P)), W - P - int(g.integers(0, P))
    if x1 - x0 >= 2:
        for k in range(2):
            y = min(H - 1, mid * P + 1 + k * max(1, P // 2 - 1))
            img[y, x0:x1] = g.uniform(0.0, INK_HI, size=x1 - x0)
    for _ in range(strokes if strokes is not None else max(1, w_p // 4)):
        x = int(g.integers(x0, max(x0 + 1, x1)))
        y = int(g.integers(0, max(1, H - P)))
        img[y:y + P, x] = g.uniform(0.0, INK_HI, size=img[y:y + P, x].shape)
    return torch.from_numpy(img).unsqueeze(0)


def kept_share(imgs, P, max_ink=0, halo=1, ink_level=0.5):
    """(kept, total) patches of a list of (1, H, W) images."""
    kept = total = 0
    for t in imgs:
        a = t[0].numpy()
        h, w = a.shape[0] // P, a.shape[1] // P
        kept += int(keep_mask(ink_counts(patch_rows(a, P), ink_level), h, w, max_ink, halo).sum())
        total += h * w
    return kept, total


# ---- the oracle over a pruned stream ---------------------------------------------------------------------------------------------------
PARITY_FIXTURE = "vitomr_small"
PARITY_SEEDS = (3, 6)
PARITY_SIZES = ((24, 40), (12, 20), (28, 44))     # grids 6 x 10, 3 x 5 and 7 x 11: the last exceeds the fixture's 6 x 10 positional table


MODEL_FIXTURE = "vitomr_dh64b"                    # P = 16, a 4 x 8 positional table: the decode-mode, alignment and identity tests
MODEL_SIZES = ((96, 192), (64, 128), (112, 224))  # grids 6 x 12, 4 x 8 (inside the table) and 7 x 14


def model_images():
    return [synthetic_system(40 + i, H, W, 16) for i, (H, W) in enumerate(MODEL_SIZES)]


def parity_images(seed, P):
    return [synthetic_system(100 * seed + i, H, W, P) for i, (H, W) in enumerate(PARITY_SIZES)]


def oracle_pruned(fx, imgs, ink_level=0.5, max_ink=0, halo=1, return_logits=False):
    """The oracle's fp32 pipeline on the kept patches only: O.encoder_embed rows selected by the restatement's kept set, O.encoder_stack with
    the kept lengths, O.transition_head, O.greedy_generate.  -> dict(latent, memory, lens, kept, seqs, log_probs, seq_mask[, logits])."""
    from oracle import vitomr_oracle as O
    cfg, sd = fx["cfg"], fx["state_dict"]
    P = cfg["P"]
    x, _ = O.encoder_embed(imgs, sd, "encoder.", P, True, "fp32")
    dims = [(t.shape[-2] // P, t.shape[-1] // P) for t in imgs]
    rows = np.concatenate([patch_rows(t[0].numpy(), P) for t in imgs])
    kept = kept_indices(ink_counts(rows, ink_level), dims, max_ink, halo)
    _, _, sel = compact(rows, kept, dims)
    x = x[torch.from_numpy(sel).long()]
    lens = [len(k) for k in kept]
    if "encoder.frozen_blocks.layers.0.norm1.weight" in sd:
        x = O.encoder_stack(x, lens, sd, "encoder.frozen_blocks.", cfg["enc_heads"], "fp32")
    lat = O.encoder_stack(x, lens, sd, "encoder.fine_tune_blocks.", cfg["enc_heads"], "fp32")
    mem = O.transition_head(lat, sd, "fp32")
    out = O.greedy_generate(mem, lens, sd, cfg["dec_heads"], "fp32", cfg["gen_len"], return_logits=return_logits)
    res = dict(latent=lat, memory=mem, lens=lens, kept=kept, seqs=out[0], log_probs=out[1], seq_mask=out[2])
    if return_logits:
        res["logits"] = out[3]
    return res
