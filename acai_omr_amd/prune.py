"""Blank-patch pruning ahead of the encoder (an extension; the reference encodes every patch).

A staff system is mostly paper, and every 16 x 16 patch of it costs an encoder token and a cross-attention key / value row.  This stage
decides on the device which patches of a packed patch stream hold ink and drops the others before the projection GEMM:

    ink[r, c]   = the number of the patch's pixels strictly below `ink_level`              (ops.patch_ink)
    inked[r, c] = ink[r, c] > max_ink
    keep[r, c]  = an inked patch of the same image within Chebyshev distance `halo`;        (ops.patch_keep)
                  an image without an inked patch keeps all of its patches
    the kept rows, their indices in the full grid and their positional rows, packed         (ops.patch_compact)

Three launches for a whole batch and ONE copy to the host, the kept counts, which size the output and plan what follows (cu_seqlens, the
longest memory, the cross-attention chunk).  The result is a `utils.PackedPatches` whose `dims` are still the full grids: everything
downstream that speaks of places on the page - `TokenAlignment.patch`, centroids, heat maps - keeps speaking in full-grid coordinates
(ViTOMR._located / _confidence_packed expand the maps with ops.attn_map_expand).

Opt-in: every entry point takes `prune=None` and is then exactly what it was.  The defaults are chosen on synthetic pages.  Not measured:
the blank share of real systems, and what dropping paper does to the output of a trained checkpoint (the fine-tuned encoder saw every
patch).  Out of scope: training through a pruned stream, the MAE models, `streamed_inference`, pruning fused into the resize kernel,
thresholds tuned on data."""
import math
from dataclasses import dataclass

import torch

from . import ops
from .config import PE_MAX_HEIGHT, PE_MAX_WIDTH
from .utils import PackedPatches


@dataclass(frozen=True)
class PruneConfig:
    """ink_level: a pixel is ink when its value is strictly below it (`page.DetectConfig`'s ink threshold; +inf makes every pixel ink, so
    nothing is dropped).  max_ink: a patch is inked when it holds more ink pixels than that.  halo: the Chebyshev distance, 0 .. 3, within
    which an inked patch keeps its neighbours (stems, slurs and ledger lines thin out towards their ends)."""
    ink_level: float = 0.5
    max_ink: int = 0
    halo: int = 1

    def __post_init__(self):
        if isinstance(self.ink_level, bool) or not isinstance(self.ink_level, (int, float)) or math.isnan(float(self.ink_level)):
            raise ValueError(f"PruneConfig.ink_level must be a number, got {self.ink_level!r}")
        if isinstance(self.max_ink, bool) or not isinstance(self.max_ink, int) or self.max_ink < 0:
            raise ValueError(f"PruneConfig.max_ink must be a non-negative int, got {self.max_ink!r}")
        if isinstance(self.halo, bool) or not isinstance(self.halo, int) or not 0 <= self.halo <= ops.PRUNE_MAX_HALO:
            raise ValueError(f"PruneConfig.halo must be an int in 0 .. {ops.PRUNE_MAX_HALO}, got {self.halo!r}")


def as_config(prune):
    """The `prune` argument of the entry points: None / False -> None (off), True -> the defaults, a PruneConfig -> itself.  TypeError."""
    if prune is None or prune is False:
        return None
    if prune is True:
        return PruneConfig()
    if isinstance(prune, PruneConfig):
        return prune
    raise TypeError(f"prune: expected None, a bool or a prune.PruneConfig, got {type(prune).__name__}")


def prune_patches(packed: PackedPatches, cfg=None, pe_grid=None) -> PackedPatches:
    """The packed patch stream without its paper patches -> a pruned `PackedPatches` (see there): `patches` are the kept rows in the
    stream's own dtype, bit for bit and in ascending order; `dims` are unchanged.  cfg: a PruneConfig (default: its defaults).  pe_grid:
    (pe_max_height, pe_max_width) of the encoder that will read the stream (default: the product's, config.PE_MAX_HEIGHT / PE_MAX_WIDTH);
    `Encoder.prune_packed` passes its own.  An empty stream comes back as an empty pruned stream without a launch."""
    if not isinstance(packed, PackedPatches):
        raise TypeError(f"prune_patches: expected a utils.PackedPatches, got {type(packed).__name__}")
    if packed.pruned:
        raise ValueError("prune_patches: the stream is already pruned")
    cfg = PruneConfig() if cfg is None else cfg
    if not isinstance(cfg, PruneConfig):
        raise TypeError(f"prune_patches: expected a prune.PruneConfig, got {type(cfg).__name__}")
    pe_grid = (PE_MAX_HEIGHT, PE_MAX_WIDTH) if pe_grid is None else (int(pe_grid[0]), int(pe_grid[1]))
    patches = packed.patches
    table, rows, max_grid = ops.prune_table(packed.dims, pe_grid, patches.device)
    if patches.dim() != 2 or patches.shape[0] != rows:
        raise ValueError(f"prune_patches: {tuple(patches.shape)} patch rows for grids that hold {rows} patches")
    if rows == 0:
        empty = torch.empty(0, dtype=torch.int32, device=patches.device)
        return PackedPatches(patches[:0], packed.dims, packed.patch_size, empty, [], empty, pe_grid)
    ink = ops.patch_ink(patches, cfg.ink_level)
    kept_local, count = ops.patch_keep(ink, table, max_grid, cfg.max_ink, cfg.halo)
    kept_lens = count.tolist()   # the stage's one device-to-host copy
    out, kept, pe_index = ops.patch_compact(patches, table, kept_local, kept_lens)
    return PackedPatches(out, packed.dims, packed.patch_size, kept, kept_lens, pe_index, pe_grid)
