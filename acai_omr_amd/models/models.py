"""MI355X backend mirror of `acai_omr.models.models` (reference: acai_omr/models/models.py).

Same class names, constructor arguments and defaults, method names, return contracts, exception types/messages and
state_dict keys as the reference, so it drops in as the model backend (`load_state_dict` of reference checkpoints
works unchanged).  `nn.TransformerEncoder` / `nn.TransformerDecoder` instances are kept as PARAMETER CONTAINERS
(that is what makes the state_dict keys identical); their `forward` is never called.  All arithmetic runs in the HIP
library on a packed token stream (`engine.py`, `ops.py`); padded `(B, L_max, E)` tensors and bool masks only exist at
the API edge.  There is no CPU fallback: inputs are moved to the parameters' GPU device, and a missing HIP library
raises.

Precision: as in the reference, modules compute in fp32 unless called under `torch.autocast("cuda", bfloat16)`
(vitomr_inference.py:81-84 runs the encoder outside and the head + decoder inside autocast); the cached decoder
follows its cache dtype (vitomr_inference.py:94).
"""
import math
import re

import torch
import torch.nn.functional as F
from torch import nn

from .. import engine as EG
from .. import ops
from ..config import LMX_BOS_TOKEN, LMX_EOS_TOKEN, LMX_PAD_TOKEN, InferenceEvent
from .kv_caching import CachedTransformerDecoder, CachedTransformerDecoderLayer, _memory_fp8, _wc

NUM_CHANNELS = 1  # grayscale sheet music


def _autocast_prec():
    return "bf16" if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16 else "fp32"


def _training_path_needed(module):
    return torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


def _as_image_list(x, device):
    """The reference iterates `for t in x`: a list/tuple of (1,H,W) tensors, or a bare (1,H,W) tensor whose single
    channel is then iterated (vitomr_inference.py:81 passes the latter)."""
    out = []
    for t in x:
        if t.dim() == 2:
            t = t.unsqueeze(0)
        out.append(t.to(device=device, dtype=torch.float32).contiguous())
    return out


class Encoder(nn.Module):
    """ViT encoder on ragged images (M:14-96): Unfold(P) -> Linear -> + pos_embedding[:h_p,:w_p] -> post-LN blocks."""

    _allow_pe_interpolation = False

    def __init__(self, patch_size, pe_max_height, pe_max_width, num_layers=12, hidden_dim=768, num_heads=12, mlp_dim=3072, transformer_dropout=0.0):
        super().__init__()
        self.patch_size = patch_size
        self.pe_max_height = pe_max_height
        self.pe_max_width = pe_max_width
        self.hidden_dim = hidden_dim
        self.unfold = nn.Unfold(kernel_size=self.patch_size, stride=self.patch_size)  # kept for attribute parity; patchify runs in HIP
        self.pos_embedding = nn.Parameter(torch.zeros(self.pe_max_height, self.pe_max_width, self.hidden_dim))
        nn.init.trunc_normal_(self.pos_embedding, std=0.1)
        self.projection = nn.Linear(in_features=(NUM_CHANNELS * self.patch_size ** 2), out_features=self.hidden_dim)
        self.encoder_blocks = nn.TransformerEncoder(
            encoder_layer=nn.TransformerEncoderLayer(d_model=self.hidden_dim, nhead=num_heads, dim_feedforward=mlp_dim,
                                                     dropout=transformer_dropout, activation="gelu", batch_first=True),
            num_layers=num_layers, norm=nn.LayerNorm(self.hidden_dim, eps=1e-6))

    # ---- host-side helpers ----------------------------------------------------------------------------------------
    def _stacks(self):
        return [self.encoder_blocks]

    def _num_heads(self):
        return self._stacks()[-1].layers[0].self_attn.num_heads

    def _device(self):
        return self.pos_embedding.device

    def _grid(self, t):
        h_p, w_p = t.shape[-2] // self.patch_size, t.shape[-1] // self.patch_size
        if not self._allow_pe_interpolation and (h_p > self.pe_max_height or w_p > self.pe_max_width):
            raise ValueError(f"{h_p} x {w_p} image is too large for max positional embedding grid of shape {self.pe_max_height} x {self.pe_max_width}")
        return h_p, w_p

    def _pe_packed(self, dims, select=None, index=None):
        """pos_embedding[:h_p,:w_p].reshape(-1,E) of every image, concatenated (M:50); `select[i]` optionally picks rows
        (MAE keeps ids_keep only, M:123).  One row-gather launch; grids beyond the table are interpolated (OMREncoder).
        index (a pruned stream's `pe_index`): the rows to gather, already on the device - no host index lists are built."""
        dev, E = self._device(), self.hidden_dim
        table = self.pos_embedding.detach().reshape(-1, E)
        if index is not None:
            extra = [self.interpolate_pe(h_p, w_p).detach().reshape(-1, E) for h_p, w_p in dims if h_p > self.pe_max_height or w_p > self.pe_max_width]
            if extra:
                table = torch.cat([table] + extra, 0).contiguous()
            return ops.gather_rows(table, index.contiguous())
        idx, extra = [], []
        base = table.shape[0]
        for i, (h_p, w_p) in enumerate(dims):
            if h_p > self.pe_max_height or w_p > self.pe_max_width:
                grid = self.interpolate_pe(h_p, w_p).detach().reshape(-1, E)
                rows = torch.arange(base, base + h_p * w_p, dtype=torch.int32)
                base += h_p * w_p
                extra.append(grid)
            else:
                rows = (torch.arange(h_p, dtype=torch.int32).unsqueeze(1) * self.pos_embedding.shape[1] + torch.arange(w_p, dtype=torch.int32).unsqueeze(0)).reshape(-1)
            if select is not None:
                rows = rows[select[i]]
            idx.append(rows)
        if extra:
            table = torch.cat([table] + extra, 0).contiguous()
        return ops.gather_rows(table, torch.cat(idx).to(dev))

    def create_attention_mask(self, seq_lens, max_len):
        arange = torch.arange(end=max_len).unsqueeze(0)
        return arange >= torch.tensor(seq_lens).unsqueeze(1)

    def _prec(self):
        return _autocast_prec()

    def _check_prune(self, prune, encoding=True):
        """The `prune` argument as a PruneConfig or None; refused (ValueError) where pruning is out of scope: the MAE encoder, and encoding
        in training mode."""
        from ..prune import as_config
        cfg = as_config(prune)
        if cfg is not None:
            if isinstance(self, MAEEncoder):
                raise ValueError("prune: the MAE encoder masks its own patches; pruning it is out of scope")
            if encoding and _training_path_needed(self):
                raise ValueError("prune: training through a pruned patch stream is out of scope (call under torch.no_grad(), or freeze the encoder)")
        return cfg

    def prune_packed(self, packed, cfg=None):
        """`prune.prune_patches` of a `utils.PackedPatches` for THIS encoder's positional table (an extension)."""
        from ..prune import prune_patches
        return prune_patches(packed, self._check_prune(True if cfg is None else cfg, encoding=False), (self.pe_max_height, self.pe_max_width))

    def embed_packed(self, x, prune=None, return_pruned=False):
        """Packed batchify: returns x32 (M,E), xb (bf16 copy or None), lens, dims.  x: images, or a `utils.PackedPatches` (patch rows written by
        the resize kernel: no Unfold / cast here).
        prune (an extension, default None = off: the path above, unchanged, no launch added): True or a `prune.PruneConfig` - the patch rows
        are formed as always and the paper patches dropped (prune.prune_patches) in whatever dtype the rows are in, before any cast; `lens`
        are then the kept counts, `dims` stay the full grids, and the positional rows are gathered through the device index.  A
        `PackedPatches` that is already pruned is taken as it is (and then prune must be None).  return_pruned appends the pruned
        `PackedPatches` (its `kept`, `kept_lens`; None without pruning) to the result.  ValueError in training mode and for the MAE encoder."""
        dev = self._device()
        prec = self._prec()
        bf = prec == "bf16"
        P = self.patch_size
        from ..utils import PackedPatches
        cfg = self._check_prune(prune)
        pruned = None
        if isinstance(x, PackedPatches):
            if x.patch_size != P or x.patches.shape[1] != NUM_CHANNELS * P * P:
                raise ValueError(f"patch rows of size {x.patch_size} for an encoder with patch size {P}")
            dims = list(x.dims)
            for h_p, w_p in dims:
                if not self._allow_pe_interpolation and (h_p > self.pe_max_height or w_p > self.pe_max_width):
                    raise ValueError(f"{h_p} x {w_p} image is too large for max positional embedding grid of shape {self.pe_max_height} x {self.pe_max_width}")
            if x.pruned:
                if cfg is not None:
                    raise ValueError("prune: the patch stream is already pruned")
                self._check_prune(True)
                if x.pe_grid != (self.pe_max_height, self.pe_max_width):
                    raise ValueError(f"the stream was pruned for a positional table of {x.pe_grid}, this encoder's is "
                                     f"{(self.pe_max_height, self.pe_max_width)}: prune it with Encoder.prune_packed")
                pruned = x
            elif cfg is not None:
                if x.patches.device != dev:
                    x = PackedPatches(x.patches.to(device=dev), x.dims, x.patch_size)
                pruned = x = self.prune_packed(x, cfg)
            lens = x.lens
            patches = x.patches.to(device=dev)
            want = torch.bfloat16 if bf else torch.float32
            if patches.dtype != want:
                patches = ops.cast_bf16(patches.float().contiguous()) if bf else patches.float()
            patches = patches.contiguous()
        else:
            imgs = _as_image_list(x, dev)
            dims = [self._grid(t) for t in imgs]
            lens = [h * w for h, w in dims]
            patches = torch.empty(sum(lens), NUM_CHANNELS * P * P, dtype=torch.bfloat16 if bf else torch.float32, device=dev)
            r0 = 0
            for t in imgs:
                r0 += ops.patchify(t, P, patches, r0)
            if cfg is not None:
                pruned = self.prune_packed(PackedPatches(patches, dims, P), cfg)
                lens, patches = pruned.lens, pruned.patches
        pe = self._pe_packed(dims) if pruned is None else self._pe_packed(dims, index=pruned.pe_index)
        more = (pruned,) if return_pruned else ()
        wc = _wc(self)
        if not isinstance(self.projection, nn.Linear):     # a swapped-in module (the reference's tests use nn.Identity, tests/test_mae.py:12)
            x32 = (self.projection(patches.float()) + pe).contiguous()
            return (x32, (ops.cast_bf16(x32) if bf else None), lens, dims) + more
        x32 = ops.gemm_nt(patches, wc.w(self.projection.weight, prec), wc.b(self.projection.bias, prec), residual=pe,
                          out_dtype=torch.float32, round_bf16=bf)
        return (x32, (ops.cast_bf16(x32) if bf else None), lens, dims) + more

    def forward_packed(self, x, prune=None, return_pruned=False):
        """Encoder on the packed token stream: (x32 (M,E), xb, lens).  This is what the inference entry points use.  prune / return_pruned
        (an extension): as in embed_packed - the stacks then run on the short stream, nothing in them changes, and with return_pruned the
        pruned `utils.PackedPatches` (or None) is appended to the result."""
        pruning = self._check_prune(prune) is not None or bool(getattr(x, "pruned", False))
        if _training_path_needed(self):
            if pruning:
                self._check_prune(True)   # raises
            from ..train import autograd_path
            out = autograd_path.encoder_forward_packed(self, x)
            return tuple(out) + (None,) if return_pruned else out
        x32, xb, lens, _, pruned = self.embed_packed(x, prune, True)
        cu = EG.cu_from_lens(lens, x32.device)
        for st in self._stacks():
            x32, xb = EG.encoder_stack(st, x32, xb, cu, max(lens), self._num_heads(), self._prec(), _wc(self))
        return (x32, xb, lens, pruned) if return_pruned else (x32, xb, lens)

    def _pad_fill(self):
        # eval + even head count: torch takes the nested-tensor fast path and padded rows leave the stack as zeros, i.e.
        # as the final LayerNorm's bias (torch transformer.py:529-550); otherwise padded rows are unspecified -> zeros.
        st = self._stacks()[-1]
        if not self.training and self._num_heads() % 2 == 0 and st.norm is not None and not torch.is_grad_enabled():
            return st.norm.bias.detach()
        return None

    # ---- reference API ----------------------------------------------------------------------------------------------
    def batchify(self, x):
        x32, _, lens, _ = self.embed_packed(x)
        # the reference pads the patch rows with zeros and THEN projects (M:55-62): a padded row holds projection(0) = the bias
        bias = getattr(self.projection, "bias", None)
        return EG.pad_rows(x32, lens, None if bias is None else bias.detach())

    def forward(self, x):
        x32, _, lens = self.forward_packed(x)
        if x32.requires_grad:
            from ..train import autograd_path
            return autograd_path.pad_rows(x32, lens, self._pad_fill())
        return EG.pad_rows(x32, lens, self._pad_fill())

    def embed_single_image(self, x):
        return self.embed_packed([x])[0].unsqueeze(0)

    def generate(self, x: torch.Tensor):
        return self.forward_packed([x])[0].unsqueeze(0)


class MAEEncoder(Encoder):
    """Encoder whose batchify shuffles and drops `mask_ratio` of each image's patches (M:100-180)."""

    def __init__(self, mask_ratio, patch_size, pe_max_height, pe_max_width, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072):
        super().__init__(patch_size, pe_max_height, pe_max_width, num_layers, hidden_dim, num_heads, mlp_dim, transformer_dropout=0.0)
        self.mask_ratio = mask_ratio

    def mask_ids(self, n, device, noise=None):
        """mask_sequence's index part (M:108-119): noise -> ids_keep, ids_restore, seq_mask (int32, 1 = masked)."""
        len_keep = int(n * (1 - self.mask_ratio))
        if noise is None:
            noise = torch.rand(n, device=device)
        ids_shuffle = torch.argsort(noise)
        ids_restore = torch.argsort(ids_shuffle)
        seq_mask = torch.ones(n, device=noise.device, dtype=torch.int)
        seq_mask[:len_keep] = 0
        return ids_shuffle[:len_keep], ids_restore, seq_mask.index_select(0, ids_restore), len_keep

    def mask_sequence(self, t: torch.Tensor, h_p: int, w_p: int, noise=None):
        """M:106-125 -> (t_masked, pos_embed_slice, unmasked_seq_len, len_keep, seq_mask, ids_restore) for ONE unfolded image
        t (1, C P^2, L).  `noise` (optional, (L,)) injects the masking noise the reference draws with torch.rand (M:110)."""
        from ..train import autograd_path
        return autograd_path.mae_mask_sequence(self, t, h_p, w_p, noise)

    def batchify(self, x, noises=None):
        """M:128-173 -> (embeddings (B, L_keep_max, E), encoder_attention_mask, decoder_attention_mask, kept_seq_lens, unmasked_seq_lens,
        batch_seq_masks (jagged int32), batch_ids_restore (jagged), patchified_dims)."""
        from ..train import autograd_path
        return autograd_path.mae_encoder_batchify(self, x, noises)

    def forward(self, x, noises=None):
        from ..train import autograd_path
        return autograd_path.mae_encoder_forward(self, x, noises)


class MAEDecoder(nn.Module):
    def __init__(self, num_layers=8, hidden_dim=512, num_heads=16, mlp_dim=3072, transformer_dropout=0.0):
        super().__init__()
        self.decoder_blocks = nn.TransformerEncoder(
            encoder_layer=nn.TransformerEncoderLayer(d_model=hidden_dim, nhead=num_heads, dim_feedforward=mlp_dim, dropout=transformer_dropout,
                                                     activation="gelu", batch_first=True),
            num_layers=num_layers, norm=nn.LayerNorm(hidden_dim, eps=1e-6))

    def forward(self, x: torch.Tensor, attention_mask: torch.Tensor):
        from ..train import autograd_path
        return autograd_path.mae_decoder_forward(self, x, attention_mask)


class MAE(nn.Module):
    """Masked auto-encoder (M:197-269).  forward(batch) -> pred (N,L_m,CP^2), loss_mask (N,L_m) bool, target (N,L_m,CP^2)."""

    def __init__(self, mask_ratio, patch_size, pe_max_height, pe_max_width, encoder_hidden_dim=768, decoder_hidden_dim=512,
                 encoder_kwargs={}, decoder_kwargs={}):
        super().__init__()
        self.patch_size = patch_size
        self.encoder = MAEEncoder(mask_ratio, self.patch_size, pe_max_height, pe_max_width, hidden_dim=encoder_hidden_dim, **encoder_kwargs)
        self.decoder_hidden_dim = decoder_hidden_dim
        self.decoder = MAEDecoder(hidden_dim=self.decoder_hidden_dim, **decoder_kwargs)
        self.decoder_embed = nn.Linear(encoder_hidden_dim, self.decoder_hidden_dim)
        self.decoder_unembed = nn.Linear(self.decoder_hidden_dim, NUM_CHANNELS * patch_size ** 2)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, self.decoder_hidden_dim))
        self.decoder_pos_embedding = nn.Parameter(torch.zeros(pe_max_height, pe_max_width, self.decoder_hidden_dim))
        nn.init.trunc_normal_(self.mask_token, std=0.1)
        nn.init.trunc_normal_(self.decoder_pos_embedding, std=0.1)
        self.unfold = nn.Unfold(kernel_size=self.patch_size, stride=self.patch_size)

    def prepare_for_decoder(self, latent: torch.Tensor, kept_seq_lens, unmasked_seq_lens, batch_ids_restore: torch.Tensor, patchified_dims):
        """M:219-241: per sequence drop the padding, append mask tokens, unshuffle by ids_restore, add the decoder PE slice; returns the
        zero-padded (B, L_max, D) decoder input."""
        from ..train import autograd_path
        return autograd_path.mae_prepare_for_decoder(self, latent, kept_seq_lens, unmasked_seq_lens, batch_ids_restore, patchified_dims)

    def forward(self, batch, noises=None, prune=None):
        """`noises`: optional list of per-image noise vectors (injected masking noise for parity runs; the reference draws
        torch.rand on the model's device, M:110).  prune: refused (ValueError) - blank-patch pruning of the MAE is out of scope."""
        if prune is not None and prune is not False:
            raise ValueError("prune: the MAE masks its own patches; pruning it is out of scope")
        from ..train import autograd_path
        return autograd_path.mae_forward(self, batch, noises)

    def forward_packed(self, batch, noises=None, prune=None):
        if prune is not None and prune is not False:
            raise ValueError("prune: the MAE masks its own patches; pruning it is out of scope")
        from ..train import autograd_path
        return autograd_path.mae_forward(self, batch, noises, packed=True)


class MAELoss(nn.Module):
    """Per-patch normalised-pixel MSE over masked patches (M:271-288); unbiased variance, eps inside the sqrt."""

    def forward(self, pred, loss_mask, target):
        from ..train import autograd_path
        return autograd_path.mae_loss(pred, loss_mask, target)


class OMREncoder(Encoder):
    """Encoder that bilinearly interpolates the PE grid for images beyond it instead of raising (M:290-332)."""

    _allow_pe_interpolation = True

    def interpolate_pe(self, h_p, w_p):
        """(h_p, w_p, E) bilinear resampling of the PE grid, align_corners=False (M:291-302), by the HIP kernel; differentiable w.r.t.
        pos_embedding when it requires grad (the reference interpolates in batchify in every mode, M:315-318)."""
        from ..train import autograd_path
        return autograd_path.PeInterpFn.apply(self.pos_embedding, h_p, w_p).view(h_p, w_p, self.hidden_dim)


class FineTuneOMREncoder(OMREncoder):
    """Encoder split into `frozen_blocks` (no final norm) and `fine_tune_blocks` (with it) (M:334-376)."""

    def __init__(self, patch_size, pe_max_height, pe_max_width, fine_tune_depth, num_layers=12, hidden_dim=768, num_heads=12, mlp_dim=3072,
                 transformer_dropout=0.05):
        super().__init__(patch_size, pe_max_height, pe_max_width, num_layers, hidden_dim, num_heads, mlp_dim)
        assert fine_tune_depth > 0, "If using FineTuneOMREncoder, fine-tune depth should be at least 1"
        del self.encoder_blocks
        self.fine_tune_depth = fine_tune_depth
        self.num_layers = num_layers
        self.num_frozen_layers = self.num_layers - self.fine_tune_depth
        self.superclass_kwargs = {"num_heads": num_heads, "mlp_dim": mlp_dim, "transformer_dropout": transformer_dropout}
        kw = {"d_model": self.hidden_dim, "nhead": num_heads, "dim_feedforward": mlp_dim, "activation": "gelu", "batch_first": True}
        if self.num_frozen_layers == 0:
            self.frozen_blocks = None
        else:
            self.frozen_blocks = nn.TransformerEncoder(encoder_layer=nn.TransformerEncoderLayer(dropout=0.0, **kw), num_layers=self.num_frozen_layers)
        self.fine_tune_blocks = nn.TransformerEncoder(encoder_layer=nn.TransformerEncoderLayer(dropout=transformer_dropout, **kw),
                                                      num_layers=self.fine_tune_depth, norm=nn.LayerNorm(self.hidden_dim, eps=1e-6))

    def _stacks(self):
        return ([self.frozen_blocks] if self.frozen_blocks is not None else []) + [self.fine_tune_blocks]


class OMRDecoder(nn.Module):
    """Autoregressive LMX decoder (M:378-528): embedding + learned positions + post-LN decoder blocks + unembed."""

    def __init__(self, max_lmx_seq_len, lmx_vocab_path, num_layers=10, hidden_dim=1024, num_heads=16, mlp_dim=4096, transformer_dropout=0.1,
                 use_caching=False, max_batch_size=None, cache_dtype=None, memory_cache_dtype=None):
        """memory_cache_dtype (extension, opt-in; cached decoder only): torch.float8_e4m3fn with cache_dtype=torch.bfloat16 keeps the decode
        engine's cross-attention K/V in FP8 (see models/kv_caching.py); None = the cache dtype."""
        super().__init__()
        _memory_fp8(cache_dtype, memory_cache_dtype)   # TypeError for an unsupported combination, cached or not
        self.max_lmx_seq_len = max_lmx_seq_len
        self.lmx_vocab_path = lmx_vocab_path
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.num_heads = num_heads
        self.head_dim = hidden_dim / num_heads
        self.mlp_dim = mlp_dim
        self.transformer_dropout = transformer_dropout
        with open(lmx_vocab_path, "r") as f:
            tokens = [line.strip() for line in f if line.strip()]
        self.tokens_to_idxs = {token: i for i, token in enumerate(tokens)}
        self.idxs_to_tokens = {i: token for i, token in enumerate(tokens)}
        self.pad_idx = self.tokens_to_idxs[LMX_PAD_TOKEN]
        self.bos_idx = self.tokens_to_idxs[LMX_BOS_TOKEN]
        self.eos_idx = self.tokens_to_idxs[LMX_EOS_TOKEN]
        self.vocab_size = len(tokens)
        self.vocab_embedding = nn.Embedding(self.vocab_size, self.hidden_dim, padding_idx=self.pad_idx)
        self.pos_embedding = nn.Parameter(torch.zeros(self.max_lmx_seq_len, self.hidden_dim))
        nn.init.trunc_normal_(self.pos_embedding, std=0.1)
        lkw = dict(d_model=self.hidden_dim, nhead=num_heads, dim_feedforward=mlp_dim, dropout=transformer_dropout, activation="gelu", batch_first=True)
        if use_caching:
            self.decoder_blocks = CachedTransformerDecoder(decoder_layer=CachedTransformerDecoderLayer(**lkw), num_layers=num_layers,
                                                           max_batch_size=max_batch_size, max_decoder_seq_len=max_lmx_seq_len,
                                                           cache_dtype=cache_dtype, norm=nn.LayerNorm(self.hidden_dim, eps=1e-6),
                                                           memory_cache_dtype=memory_cache_dtype)
            self.decoder_blocks.__dict__["_omr"] = self
        else:
            self.decoder_blocks = nn.TransformerDecoder(decoder_layer=nn.TransformerDecoderLayer(**lkw), num_layers=num_layers,
                                                        norm=nn.LayerNorm(self.hidden_dim, eps=1e-6))
        self.unembed = nn.Linear(self.hidden_dim, self.vocab_size)

    def to_cached_version(self, max_batch_size, cache_dtype, memory_cache_dtype=None):
        return OMRDecoder(self.max_lmx_seq_len, self.lmx_vocab_path, self.num_layers, self.hidden_dim, self.num_heads, self.mlp_dim,
                          self.transformer_dropout, use_caching=True, max_batch_size=max_batch_size, cache_dtype=cache_dtype,
                          memory_cache_dtype=memory_cache_dtype)

    # ---- teacher-forced / uncached batch paths -----------------------------------------------------------------------------
    def _embed_packed(self, inputs, lens_t, token_idxs_input, position_offset=0):
        """Token + position embeddings of a packed stream (fp32); positions restart at position_offset in every sequence."""
        dev = self.pos_embedding.device
        pos_idx = torch.cat([torch.arange(t, dtype=torch.int32) for t in lens_t])
        if position_offset:
            pos_idx = pos_idx + int(position_offset)
        x32 = ops.gather_rows(self.pos_embedding.detach(), pos_idx.to(dev))
        if token_idxs_input:
            return ops.gather_rows(self.vocab_embedding.weight.detach(), inputs.to(device=dev, dtype=torch.int32).contiguous(), add=x32)
        return x32 + inputs.to(dev).float()

    def _layers_packed(self, x32, lens_t, mem32, memb, lens_s, prec, maps=None, kv_sink=None):
        """The decoder layers, final norm and unembed on a packed stream: forward_packed's body, shared with cross_attention_maps_packed.
        maps (None = plain forward): {"weights": {layer index: [H] fp32 device tensor}, "out", "map_off", "logits"} - in those layers the
        cross-attention also saves its log-sum-exp and ops.attn_probs_mean adds the layer's weighted head mean to maps["out"]; unless
        maps["logits"], the pass ends after the last such layer's cross-attention and returns None.
        kv_sink (None = off): called as kv_sink(layer index, qkv) with every layer's self-attention in-projection (sum T, 3E) in the compute
        dtype while it is alive - columns E:3E are the layer's self K and V (DecodeEngine._prefill copies them into the decode's caches)."""
        bf = prec == "bf16"
        dev, E, H = self.pos_embedding.device, self.hidden_dim, self.num_heads
        wc = _wc(self)
        xb = ops.cast_bf16(x32) if bf else None
        cu_t, cu_s = EG.cu_from_lens(lens_t, dev), EG.cu_from_lens(lens_s, dev)
        mem = memb if bf else mem32
        if mem is None:
            mem = ops.cast_bf16(mem32)
        mt, dh = max(lens_t), E // H
        picked = maps["weights"] if maps is not None else {}
        lse, first = None, True
        for i, ly in enumerate(self.decoder_blocks.layers):
            sa, ca = ly.self_attn, ly.multihead_attn
            qkv = EG.linear(x32, xb, sa.in_proj_weight, sa.in_proj_bias, prec, wc)
            if kv_sink is not None:
                kv_sink(i, qkv)
            a = ops.attn_varlen(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], cu_t, cu_t, H, dh, mt, causal=True)
            y = ops.gemm_nt(a, wc.w(sa.out_proj.weight, prec), wc.b(sa.out_proj.bias, prec), residual=x32, round_bf16=bf)
            x32, xb = ops.layernorm(y, ly.norm1.weight.detach(), ly.norm1.bias.detach(), ly.norm1.eps, want_bf16=bf)
            cdt = torch.bfloat16 if bf else torch.float32
            q = ops.gemm_nt(xb if bf else x32, wc.w(ca.in_proj_weight, prec)[:E], wc.b(ca.in_proj_bias, prec)[:E], out_dtype=cdt, round_bf16=bf)
            kv = ops.gemm_nt(mem, wc.w(ca.in_proj_weight, prec)[E:], wc.b(ca.in_proj_bias, prec)[E:], out_dtype=cdt, round_bf16=bf)
            if i in picked:
                if lse is None:
                    lse = torch.empty(H * q.shape[0], dtype=torch.float32, device=dev)
                a = ops.attn_varlen(q, kv[:, :E], kv[:, E:], cu_t, cu_s, H, dh, mt, lse=lse)
                ops.attn_probs_mean(q, kv[:, :E], cu_t, cu_s, H, dh, mt, max(lens_s), lse, picked[i], maps["map_off"], maps["out"],
                                    accumulate=not first)
                first = False
                if i == max(picked) and not maps["logits"]:
                    return None
            else:
                a = ops.attn_varlen(q, kv[:, :E], kv[:, E:], cu_t, cu_s, H, dh, mt)
            y = ops.gemm_nt(a, wc.w(ca.out_proj.weight, prec), wc.b(ca.out_proj.bias, prec), residual=x32, round_bf16=bf)
            x32, xb = ops.layernorm(y, ly.norm2.weight.detach(), ly.norm2.bias.detach(), ly.norm2.eps, want_bf16=bf)
            h = EG.linear(x32, xb, ly.linear1.weight, ly.linear1.bias, prec, wc, gelu=True)
            y = ops.gemm_nt(h, wc.w(ly.linear2.weight, prec), wc.b(ly.linear2.bias, prec), residual=x32, round_bf16=bf)
            x32, xb = ops.layernorm(y, ly.norm3.weight.detach(), ly.norm3.bias.detach(), ly.norm3.eps, want_bf16=bf)
        nrm = self.decoder_blocks.norm
        x32, xb = ops.layernorm(x32, nrm.weight.detach(), nrm.bias.detach(), nrm.eps, want_bf16=bf)
        return EG.linear(x32, xb, self.unembed.weight, self.unembed.bias, prec, wc, out_dtype=torch.float32)

    def forward_packed(self, inputs, lens_t, mem32, memb, lens_s, token_idxs_input=True, prec=None):
        """Teacher-forced decoder on packed streams.  inputs: packed token ids (sum T,) int or packed embeddings (sum T, E);
        positions restart at 0 in every sequence (M:465-466).  Returns packed logits (sum T, V) fp32."""
        prec = prec or _autocast_prec()
        return self._layers_packed(self._embed_packed(inputs, lens_t, token_idxs_input), lens_t, mem32, memb, lens_s, prec)

    def _alignment_selection(self, layers, head_weights):
        """cross_attention_maps_packed's `layers` and `head_weights`, checked on the host: (sorted layer indices, float64 CPU weights
        [len(layers), H] in that order, summing to 1 over everything).  ValueError for anything else."""
        L, H = len(self.decoder_blocks.layers), self.num_heads
        if layers is None:
            idx = list(range(L))
        else:
            try:
                raw = [int(i) for i in layers]
            except (TypeError, ValueError):
                raise ValueError(f"layers must be an iterable of layer indices, got {layers!r}") from None
            if not raw:
                raise ValueError("layers is empty: select at least one decoder layer")
            idx = []
            for i in raw:
                if not -L <= i < L:
                    raise ValueError(f"layer index {i} is out of range for a decoder of {L} layers")
                idx.append(i + L if i < 0 else i)
            if len(set(idx)) != len(idx):
                raise ValueError(f"layers holds a layer more than once: {raw}")
        n = len(idx)
        if head_weights is None:
            w = torch.full((n, H), 1.0 / (n * H), dtype=torch.float64)
        else:
            try:
                w = torch.as_tensor(head_weights).detach().to(device="cpu", dtype=torch.float64)
            except (TypeError, ValueError, RuntimeError) as e:
                raise ValueError(f"head_weights must be a [H] or [len(layers), H] tensor or nested list: {e}") from None
            if w.dim() == 1 and w.shape[0] == H:
                w = w.unsqueeze(0).expand(n, H)
            elif w.dim() != 2 or tuple(w.shape) != (n, H):
                raise ValueError(f"head_weights must have shape [{H}] or [{n}, {H}], got {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("head_weights must be finite and non-negative")
            if not float(w.sum()) > 0:
                raise ValueError("head_weights sum to zero")
            w = w / w.sum()
        order = sorted(range(n), key=lambda j: idx[j])
        return [idx[j] for j in order], w[order].contiguous()

    def cross_attention_maps_packed(self, tokens, lens_t, mem32, memb, lens_s, layers=None, head_weights=None, position_offset=0, prec=None,
                                    return_logits=False):
        """Token-to-image alignment (an extension): a teacher-forced pass over packed token ids `tokens` (sum T,) that also writes out, per
        token, the cross-attention distribution over the image's patches - the weighted mean over the selected layers and heads.
        Returns a list of (T_i, S_i) fp32 maps (views of one buffer), and with return_logits (maps, packed logits (sum T, V) fp32).

        position_offset adds to every position index.  The KV-cached decode embeds the token at output index t-1 at position t (quirk Q1),
        so with position_offset=1 row j of a decoded sequence's map is the attention the decode itself ran when it chose index j+1; 0 gives
        the positions of forward_packed.  layers: iterable of layer indices, negative ones counted from the end, default all (ValueError
        when empty, out of range or repeated).  head_weights: a [H] or [len(layers), H] tensor or nested list, in the order `layers` lists
        them, non-negative with a positive sum, normalised so that all weights sum to 1; default uniform (ValueError for a wrong shape,
        negative or non-finite entries, a zero sum).  Each map row sums to 1 up to rounding.  Without return_logits the pass ends after the
        last selected layer's cross-attention.  Which layers and heads align best on trained checkpoints has not been measured: the
        uniform default is a neutral choice, not a tuned one."""
        out, offs, _, logits = self._cross_attention_maps_flat(tokens, lens_t, mem32, memb, lens_s, layers, head_weights, position_offset, prec,
                                                               return_logits)
        views = [out[o:o + int(t) * int(s)].view(int(t), int(s)) for o, t, s in zip(offs, lens_t, lens_s)]
        return (views, logits) if return_logits else views

    def _check_pass_lengths(self, tokens, lens_t, lens_s, position_offset):
        """The lengths and positions of a teacher-forced pass over packed token ids, checked on the host (ValueError) and as ints."""
        lens_t, lens_s = [int(t) for t in lens_t], [int(s) for s in lens_s]
        if len(lens_t) != len(lens_s) or not lens_t or min(lens_t) < 1 or min(lens_s) < 1:
            raise ValueError(f"lens_t {lens_t} and lens_s {lens_s} must be equally many positive lengths")
        position_offset = int(position_offset)
        if position_offset < 0 or max(lens_t) + position_offset > self.max_lmx_seq_len:
            raise ValueError(f"positions {position_offset} .. {max(lens_t) + position_offset - 1} lie outside the {self.max_lmx_seq_len} learned ones")
        if int(tokens.numel()) != sum(lens_t):
            raise ValueError(f"tokens holds {int(tokens.numel())} ids for lens_t summing to {sum(lens_t)}")
        return lens_t, lens_s, position_offset

    def logits_packed(self, tokens, lens_t, mem32, memb, lens_s, position_offset=0, prec=None):
        """forward_packed over packed token ids whose positions start at position_offset: with 1 the KV-cached decode's positions (quirk Q1,
        cross_attention_maps_packed), so row j of a decoded sequence holds the logits the decode chose index j + 1 from.  All layers, no
        maps.  Returns packed logits (sum T, V) fp32."""
        lens_t, lens_s, position_offset = self._check_pass_lengths(tokens, lens_t, lens_s, position_offset)
        prec = prec or _autocast_prec()
        return self._layers_packed(self._embed_packed(tokens.reshape(-1), lens_t, True, position_offset), lens_t, mem32, memb, lens_s, prec)

    def _cross_attention_maps_flat(self, tokens, lens_t, mem32, memb, lens_s, layers, head_weights, position_offset, prec, return_logits):
        """cross_attention_maps_packed's work: (flat fp32 map buffer, the images' element offsets as a list and as an int64 device tensor,
        logits or None)."""
        sel, w = self._alignment_selection(layers, head_weights)
        lens_t, lens_s, position_offset = self._check_pass_lengths(tokens, lens_t, lens_s, position_offset)
        prec = prec or _autocast_prec()
        dev = self.pos_embedding.device
        offs, total = ops.attn_map_layout(lens_t, lens_s)
        out = torch.empty(total, dtype=torch.float32, device=dev)
        wdev = ops.h2d(w.to(torch.float32), dev)
        map_off = ops.h2d(torch.tensor(offs, dtype=torch.int64), dev)
        maps = {"weights": {l: wdev[j] for j, l in enumerate(sel)}, "out": out, "map_off": map_off, "logits": bool(return_logits)}
        logits = self._layers_packed(self._embed_packed(tokens.reshape(-1), lens_t, True, position_offset), lens_t, mem32, memb, lens_s, prec, maps)
        return out, offs, map_off, logits

    def forward(self, input_seqs, img_latent, lmx_attention_mask, latent_attention_mask, token_idxs_input=True, checkpoint_grads=False,
                memory_group_size=None):
        """Teacher-forced logits (B, L_lmxmax, V) (M:445-483).  <pad> positions (lmx_attention_mask True) are not computed
        and come back as zeros (the reference leaves unspecified values there; OMRCELoss ignores them).
        memory_group_size = G (extension, GRPO): img_latent / latent_attention_mask hold one memory per IMAGE and input_seqs G rows per image
        (rows b*G .. b*G+G-1 attend to memory b) - the same logits as over expand_img_latent_for_rollout's copies, without making them."""
        T = input_seqs.shape[1]
        if T > self.max_lmx_seq_len:
            raise ValueError(f"{T} long lmx sequence length is too long for max sequence length of {self.max_lmx_seq_len}")
        if memory_group_size is not None or _training_path_needed(self) or (
                torch.is_grad_enabled() and (img_latent.requires_grad or (not token_idxs_input and input_seqs.requires_grad))):
            from ..train import autograd_path
            return autograd_path.decoder_forward(self, input_seqs, img_latent, lmx_attention_mask, latent_attention_mask, token_idxs_input, checkpoint_grads,
                                                 memory_group_size)
        dev = self.pos_embedding.device
        B = input_seqs.shape[0]
        lens_t = [T] * B if lmx_attention_mask is None else (~lmx_attention_mask).sum(dim=1).tolist()
        mem32, lens_s = EG.unpad_rows(img_latent.to(dev), latent_attention_mask)
        if token_idxs_input:
            packed_in = torch.cat([input_seqs[b, :l] for b, l in enumerate(lens_t)]).to(dev)
        else:
            packed_in = torch.cat([input_seqs[b, :l] for b, l in enumerate(lens_t)], 0)
        logits = self.forward_packed(packed_in, lens_t, mem32, None, lens_s, token_idxs_input)
        out = torch.zeros(B, T, self.vocab_size, dtype=torch.float32, device=dev)
        o = 0
        for b, l in enumerate(lens_t):
            out[b, :l] = logits[o:o + l]
            o += l
        return out.to(torch.bfloat16) if _autocast_prec() == "bf16" else out

    def generate(self, input_seqs, img_latent, latent_attention_mask=None):
        seq_len = input_seqs.shape[1]
        if seq_len > self.max_lmx_seq_len:
            raise ValueError(f"{seq_len} long lmx sequence length is too long for max sequence length of {self.max_lmx_seq_len}")
        return self.forward(input_seqs, img_latent, None, latent_attention_mask)

    # ---- KV-cached path ------------------------------------------------------------------------------------------------
    def _cached_blocks(self):
        """decoder_blocks, which the KV-cached inference pathway needs to be a CachedTransformerDecoder."""
        if not isinstance(self.decoder_blocks, CachedTransformerDecoder):
            raise RuntimeError("Trying to use cached inference pathway with an uncached TransformerDecoder instance")
        return self.decoder_blocks

    def prepare_caches(self, encoder_memory):
        self._cached_blocks().prepare_caches(encoder_memory)

    def cached_generate(self, token_t: torch.Tensor, time_step: int, latent_attention_mask=None):
        """Logits (B,1,V) for the token after `token_t` (B,1); pos_embedding is indexed with `time_step` literally."""
        if time_step >= self.max_lmx_seq_len:
            raise RuntimeError(f"{time_step + 1} decoding steps is too long for max sequence length of {self.max_lmx_seq_len}")
        blocks = self._cached_blocks()
        blocks._materialise(latent_attention_mask)
        eng = blocks.engine(self.pos_embedding.device)
        logits = eng.logits_step(token_t, time_step)
        for c in blocks.self_attn_caches:
            c._pos += 1
        logits = logits.view(-1, 1, self.vocab_size).clone()
        return logits.to(torch.bfloat16) if eng.bf else logits


def batchify_and_split_lmx_seqs(lmx_seqs, pad_idx, device):
    """Pad with <pad>, inputs = seq[:, :-1], targets = seq[:, 1:], mask = inputs == pad (M:531-540).  Integer bookkeeping."""
    B, Lm = len(lmx_seqs), max(int(s.shape[0]) for s in lmx_seqs)
    full = torch.full((B, Lm), pad_idx, dtype=lmx_seqs[0].dtype, device=lmx_seqs[0].device)
    for i, s in enumerate(lmx_seqs):
        full[i, :s.shape[0]] = s
    input_seqs, target_seqs = full[:, :-1], full[:, 1:]
    return input_seqs, target_seqs, (input_seqs == pad_idx).to(device)


class _TransitionHead(nn.Sequential):
    """Linear, GELU, Dropout, Linear (M:655-660) as a parameter container; both GEMMs (bias+GELU fused) run in HIP."""

    def forward_packed(self, x32, xb=None, prec=None):
        prec = prec or _autocast_prec()
        bf = prec == "bf16"
        wc = _wc(self)
        h = EG.linear(x32, xb, self[0].weight, self[0].bias, prec, wc, gelu=True)
        y = EG.linear(None if bf else h, h if bf else None, self[3].weight, self[3].bias, prec, wc)
        return y  # (M, E_dec) in the compute dtype

    def forward(self, x):
        if _training_path_needed(self) or (torch.is_grad_enabled() and x.requires_grad):
            from ..train import autograd_path
            return autograd_path.head_forward(self, x)
        shp = x.shape
        y = self.forward_packed(x.reshape(-1, shp[-1]).float().contiguous())
        return y.view(*shp[:-1], y.shape[-1])


def _continuous_caps(max_len, n):
    """max_len of the continuous-batching entry points: one cap for all n images or n per-image caps."""
    if isinstance(max_len, int) or (torch.is_tensor(max_len) and max_len.dim() == 0):
        return [int(max_len)] * n
    caps = [int(c) for c in max_len]
    if len(caps) != n:
        raise ValueError(f"max_len holds {len(caps)} per-image caps for {n} images")
    return caps


class TokenAlignment:
    """Where on the page each output token came from (ViTOMR.locate_tokens; an extension).  For a batch of B sequences clipped to T' indices:
    patch (B, T') int64 - the arg-max patch of the token's attention map, row-major in the image's patch grid, -1 where there is no map
    (index 0, <bos>, and positions after the row's end); center_px / spread_px (B, T', 2) fp32 - centroid and standard deviation of the map
    as (x, y) in pixels of the input tensor (patch units x patch_size), NaN where there is no map; peak (B, T') fp32 - the map's largest
    probability, NaN where there is none; grids - the images' (h_p, w_p); maps - the list of (L_i - 1, S_i) maps, or None."""

    __slots__ = ("patch", "center_px", "spread_px", "peak", "grids", "maps")

    def __init__(self, patch, center_px, spread_px, peak, grids, maps=None):
        self.patch, self.center_px, self.spread_px, self.peak, self.grids, self.maps = patch, center_px, spread_px, peak, grids, maps

    def __repr__(self):
        return f"TokenAlignment(patch={tuple(self.patch.shape)}, grids={self.grids}, maps={'yes' if self.maps is not None else None})"


class TokenConfidence:
    """How sure the model was about each output token, and what else it could have been (ViTOMR.token_confidence / uncertainty_maps; an
    extension).  For a batch of B sequences clipped to T' indices, from softmax(logits / temperature) of the step that chose each index:
    log_prob (B, T') fp32 - the token's log-probability; entropy (B, T') fp32 - the distribution's entropy in nats; rank (B, T') int64 - how
    many tokens the model ordered before it (raw logit descending, then id ascending; 0 = it was the arg-max); top_tokens (B, T', K) int64
    and top_log_probs (B, T', K) fp32 - the first K tokens of that order and their log-probabilities.  Where no token is scored - index 0,
    <bos>, and every position after the row's end - the floats are NaN and the integers -1.  uncertainty: None, or one (h_p, w_p) fp32 heat
    map per image, the tokens' cross-attention maps summed with a per-token weight; alignment: None or the TokenAlignment of the same
    pass."""

    __slots__ = ("log_prob", "entropy", "rank", "top_tokens", "top_log_probs", "uncertainty", "alignment")

    def __init__(self, log_prob, entropy, rank, top_tokens, top_log_probs, uncertainty=None, alignment=None):
        self.log_prob, self.entropy, self.rank, self.top_tokens, self.top_log_probs = log_prob, entropy, rank, top_tokens, top_log_probs
        self.uncertainty, self.alignment = uncertainty, alignment

    @property
    def margin(self):
        """(B, T') fp32: log-probability of the best token minus the runner-up's; NaN where nothing is scored and when K = 1."""
        if self.top_log_probs.shape[-1] < 2:
            return torch.full_like(self.log_prob, float("nan"))
        return self.top_log_probs[..., 0] - self.top_log_probs[..., 1]

    @property
    def mean_log_prob(self):
        """(B,) fp32: the mean of log_prob over the row's scored tokens (NaN for a row without one).  The reference UI's per-page figure
        (ui/routes.py, avg_log_prob -> avgConfidence) is log_probs.sum() / seq_mask.sum(): the same sum - <bos> carries log-probability 0 -
        divided by one more, because its mask counts <bos>: for a row of L tokens it is (L - 1) / L of this mean."""
        scored = ~torch.isnan(self.log_prob)
        return torch.where(scored, self.log_prob, torch.zeros_like(self.log_prob)).sum(-1) / scored.sum(-1)

    def __repr__(self):
        return (f"TokenConfidence(log_prob={tuple(self.log_prob.shape)}, top_k={self.top_tokens.shape[-1]}, "
                f"uncertainty={'yes' if self.uncertainty is not None else None}, alignment={'yes' if self.alignment is not None else None})")


UNCERTAINTY_WEIGHTS = ("entropy", "surprisal", "error")


class ViTOMR(nn.Module):
    def __init__(self, encoder, transition_head, decoder):
        super().__init__()
        self.encoder = encoder
        self.transition_head = transition_head
        self.decoder = decoder

    def create_inference_mask(self, seqs):
        """True up to and including each row's first <eos> (M:550-559)."""
        eos_mask = seqs == self.decoder.eos_idx
        seen = eos_mask.int().cumsum(dim=-1)
        return (seen == 0) | (eos_mask & (seen == 1))

    def mask_and_clip_seqs(self, seqs, seq_log_probs):
        seq_mask = self.create_inference_mask(seqs)
        seqs = seqs.masked_fill(~seq_mask, self.decoder.pad_idx)
        seq_log_probs = seq_log_probs.masked_fill(~seq_mask, 0.0)
        n = int(seq_mask.sum(dim=-1).max())
        return seqs[:, :n], seq_log_probs[:, :n], seq_mask[:, :n]

    # ---- token-to-image alignment (an extension) --------------------------------------------------------------------------
    def _alignment_lengths(self, seqs, seq_mask):
        """L_i of cross_attention_maps: tokens of row i up to and including its first <eos>, or up to the first masked position."""
        if seqs.dim() != 2 or seqs.dtype.is_floating_point:
            raise ValueError(f"seqs must be a (B, T) integer tensor, got shape {tuple(seqs.shape)} dtype {seqs.dtype}")
        keep = self.create_inference_mask(seqs)
        if seq_mask is not None:
            if seq_mask.shape != seqs.shape:
                raise ValueError(f"seq_mask {tuple(seq_mask.shape)} does not match seqs {tuple(seqs.shape)}")
            keep = keep & (seq_mask.to(seqs.device).bool().int().cumprod(dim=-1) > 0)
        return [int(l) for l in keep.sum(dim=-1).tolist()]

    @staticmethod
    def _check_grids(grids, lens_s):
        """locate_tokens' `grids`: one (h_p, w_p) of positive ints per image with h_p * w_p patches (so S_i % w_p == 0).  ValueError."""
        try:
            out = [(int(h), int(w)) for h, w in grids]
        except (TypeError, ValueError):
            raise ValueError(f"grids must be a list of (h_p, w_p) pairs, one per image, got {grids!r}") from None
        if len(out) != len(lens_s):
            raise ValueError(f"grids holds {len(out)} entries for {len(lens_s)} images")
        for i, ((h, w), s) in enumerate(zip(out, lens_s)):
            if h < 1 or w < 1:
                raise ValueError(f"grids[{i}] = {(h, w)}: both sides must be at least 1")
            if h * w != s:
                raise ValueError(f"grids[{i}] = {(h, w)} does not cover the image's {s} patches")
        return out

    def _scored_rows(self, mem32, memb, lens_s, seqs, seq_mask):
        """The teacher-forced pass's inputs for decoded sequences: (L_i of every row, rows with L_i >= 2, their input lengths L_i - 1, their
        memory lengths, mem32 and memb cut down to those rows, packed input tokens seqs[i, :L_i - 1] - None without such a row, (bi, ti) -
        for every packed token the (row, output index) of a (B, T') tensor that it scores)."""
        Ls = self._alignment_lengths(seqs, seq_mask)
        if len(lens_s) != seqs.shape[0]:
            raise ValueError(f"{seqs.shape[0]} sequences for {len(lens_s)} images")
        dev = self.decoder.pos_embedding.device
        rows = [i for i, L in enumerate(Ls) if L >= 2]
        lens_t = [Ls[i] - 1 for i in rows]
        sub_s = [lens_s[i] for i in rows]
        if not rows:
            return Ls, rows, lens_t, sub_s, mem32, memb, None, None
        if len(rows) < len(Ls):   # rows without a scored token leave the batch: their memory rows are cut out
            starts = [sum(lens_s[:i]) for i in rows]
            cut = lambda m: None if m is None else torch.cat([m[o:o + s] for o, s in zip(starts, sub_s)]).contiguous()   # noqa: E731
            mem32, memb = cut(mem32), cut(memb)
        tokens = torch.cat([seqs[i, :Ls[i] - 1] for i in rows])
        bi = torch.cat([torch.full((t,), i, dtype=torch.int64) for i, t in zip(rows, lens_t)]).to(dev)
        ti = torch.cat([torch.arange(1, t + 1, dtype=torch.int64) for t in lens_t]).to(dev)
        return Ls, rows, lens_t, sub_s, mem32, memb, tokens, (bi, ti)

    def _located(self, shape, lens_s, rows, lens_t, sub_s, at, out, offs, map_off, grids, patch_size, return_maps):
        """The maps list of cross_attention_maps from the flat buffer of a pass over `rows` (out None: no row had a map), and with grids the
        TokenAlignment of those maps."""
        dev = self.decoder.pos_embedding.device
        B, Tp = shape
        maps = [torch.zeros(0, s, dtype=torch.float32, device=dev) for s in lens_s]
        patch = torch.full((B, Tp), -1, dtype=torch.int64, device=dev)
        loc_full = torch.full((B, Tp, 6), float("nan"), dtype=torch.float32, device=dev)
        if out is not None:
            for i, o, t, s in zip(rows, offs, lens_t, sub_s):
                maps[i] = out[o:o + t * s].view(t, s)
            if grids is not None:
                cu_t, cu_s = EG.cu_from_lens(lens_t, dev), EG.cu_from_lens(sub_s, dev)
                p, loc = ops.attn_map_locate(out, map_off, cu_t, cu_s, [grids[i][1] for i in rows], max(lens_t), sum(lens_t))
                patch[at] = p.long()
                loc_full[at] = loc
        if grids is None:
            return maps
        P = float(patch_size)
        return TokenAlignment(patch, loc_full[..., 2:4] * P, loc_full[..., 4:6] * P, loc_full[..., 1].clone(), list(grids), maps if return_maps else None)

    @staticmethod
    def _expand_maps(out, offs, rows, lens_t, sub_s, lens_s, kept, grids):
        """The flat map buffer of a pass over the pruned memories of `rows` (sub_s columns each) taken to the columns of the full grids
        (ops.attn_map_expand): (buffer, offsets list, offsets on the device, the rows' full lengths).  kept: the packed kept indices of ALL
        images (lens_s of them each), as `utils.PackedPatches.kept` holds them."""
        if len(rows) < len(lens_s):
            starts = [sum(lens_s[:i]) for i in rows]
            kept = torch.cat([kept[o:o + k] for o, k in zip(starts, sub_s)])
        full = [grids[i][0] * grids[i][1] for i in rows]
        out, offs, map_off = ops.attn_map_expand(out, lens_t, sub_s, full, kept.contiguous(), offs)
        return out, offs, map_off, full

    def _align_packed(self, mem32, memb, lens_s, seqs, seq_mask, layers, head_weights, as_decoded, grids=None, patch_size=None, return_maps=True,
                      kept=None):
        """The alignment pass on packed memories: the maps list of cross_attention_maps, and with grids a TokenAlignment.  kept (with grids:
        the FULL grids): the memories are those of a pruned patch stream and lens_s its kept counts; the maps are expanded to the full grids
        before anything reads them, so patches, centroids and maps are in full-grid coordinates."""
        dec = self.decoder
        dec._alignment_selection(layers, head_weights)   # argument errors before any work
        _, rows, lens_t, sub_s, mem32, memb, tokens, at = self._scored_rows(mem32, memb, lens_s, seqs, seq_mask)
        out = offs = map_off = None
        if rows:
            out, offs, map_off, _ = dec._cross_attention_maps_flat(tokens, lens_t, mem32, memb, sub_s, layers, head_weights, 1 if as_decoded else 0,
                                                                   None, False)
        if kept is not None:
            if rows:
                out, offs, map_off, sub_s = self._expand_maps(out, offs, rows, lens_t, sub_s, lens_s, kept, grids)
            lens_s = [h * w for h, w in grids]
        return self._located(seqs.shape, lens_s, rows, lens_t, sub_s, at, out, offs, map_off, grids, patch_size, return_maps)

    def cross_attention_maps(self, img_latent, latent_attention_mask, seqs, seq_mask=None, layers=None, head_weights=None, as_decoded=True):
        """Token-to-image alignment (an extension): for decoded (or any) sequences `seqs` (B, T) over the memories img_latent (B, S_max, E) /
        latent_attention_mask, a list of (L_i - 1, S_i) fp32 tensors - row j of image i is the distribution over the image's S_i patches
        (row-major, Encoder) behind output index j + 1: the mean over the selected decoder layers and heads of the cross-attention
        probabilities of a teacher-forced pass over input indices 0 .. L_i - 2.  L_i counts row i's tokens up to and including its first
        <eos>, or up to the first position seq_mask (True = token) masks.  as_decoded (default): positions as the KV-cached decode uses
        them (OMRDecoder.cross_attention_maps_packed, position_offset=1), so a map is the attention that decode itself ran; False: the
        teacher-forced positions of OMRDecoder.forward.  layers / head_weights: see cross_attention_maps_packed - which of them align best
        on trained checkpoints has not been measured.  Runs under the caller's autocast, as forward does, and reads the memory itself, not
        the KV caches: any cache dtype (FP8 memory cache included) gives the same maps and engine state, graphs and caches stay untouched."""
        self.decoder._alignment_selection(layers, head_weights)
        self._alignment_lengths(seqs, seq_mask)
        mem32, lens_s = EG.unpad_rows(img_latent.to(self.decoder.pos_embedding.device), latent_attention_mask)
        with torch.no_grad():
            return self._align_packed(mem32, None, lens_s, seqs, seq_mask, layers, head_weights, as_decoded)

    def locate_tokens(self, img_latent, latent_attention_mask, seqs, seq_mask=None, layers=None, head_weights=None, as_decoded=True, grids=None,
                      return_maps=False, patch_size=None):
        """cross_attention_maps reduced to a location per token (an extension) -> TokenAlignment.  grids (required): the images' patch grids
        [(h_p, w_p), ...] with h_p * w_p = S_i (ValueError otherwise); patch_size: pixels per patch side, default the encoder's.
        return_maps keeps the maps in the result."""
        if grids is None:
            raise ValueError("grids is required: one (h_p, w_p) per image")
        self.decoder._alignment_selection(layers, head_weights)
        B, Lm = img_latent.shape[0], img_latent.shape[1]
        lens_s = [Lm] * B if latent_attention_mask is None else [int(l) for l in (~latent_attention_mask).sum(dim=1).tolist()]
        grids = self._check_grids(grids, lens_s)
        if patch_size is None:
            patch_size = getattr(self.encoder, "patch_size", None)
        if patch_size is None or float(patch_size) <= 0:
            raise ValueError("patch_size is needed (the model has no encoder to take it from) and must be positive")
        self._alignment_lengths(seqs, seq_mask)
        mem32, lens_s = EG.unpad_rows(img_latent.to(self.decoder.pos_embedding.device), latent_attention_mask)
        with torch.no_grad():
            return self._align_packed(mem32, None, lens_s, seqs, seq_mask, layers, head_weights, as_decoded, grids, patch_size, return_maps)

    # ---- per-token confidence (an extension) --------------------------------------------------------------------------------
    def _check_confidence_args(self, top_k, temperature):
        """top_k and temperature of token_confidence / uncertainty_maps, checked on the host: (int, float).  ValueError."""
        V = self.decoder.vocab_size
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(ops.CONFIDENCE_MAX_K, V):
            raise ValueError(f"top_k must be an int with 1 <= top_k <= min({ops.CONFIDENCE_MAX_K}, V={V}), got {top_k!r}")
        try:
            tau = float(temperature)
        except (TypeError, ValueError):
            raise ValueError(f"temperature must be a positive number, got {temperature!r}") from None
        if not (tau > 0 and math.isfinite(tau)):
            raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
        return top_k, tau

    @staticmethod
    def _check_uncertainty_weight(weight, shape):
        """uncertainty_maps' `weight`: one of UNCERTAINTY_WEIGHTS, or a (B, T') real tensor of the caller's.  ValueError."""
        if isinstance(weight, str):
            if weight not in UNCERTAINTY_WEIGHTS:
                raise ValueError(f"weight must be one of {UNCERTAINTY_WEIGHTS} or a (B, T') tensor, got {weight!r}")
        elif not torch.is_tensor(weight) or tuple(weight.shape) != tuple(shape) or weight.dtype.is_complex or weight.dtype == torch.bool:
            what = f"a {tuple(weight.shape)} {weight.dtype} tensor" if torch.is_tensor(weight) else repr(weight)
            raise ValueError(f"weight must be one of {UNCERTAINTY_WEIGHTS} or a real tensor of seqs' shape {tuple(shape)}, got {what}")
        return weight

    def _confidence_packed(self, mem32, memb, lens_s, seqs, seq_mask, top_k, temperature, as_decoded, weight=None, layers=None,
                           head_weights=None, grids=None, patch_size=None, return_alignment=False, kept=None, measure=None, return_maps=False):
        """The confidence pass on packed memories -> TokenConfidence.  weight None: the logits-only pass; otherwise the combined pass (maps and
        logits from one teacher-forced pass), the heat maps over `grids`, and with return_alignment the TokenAlignment of the same maps
        (return_maps keeps the per-token maps in it).  kept: as in _align_packed - the maps of a pruned memory are expanded to the full
        `grids` before the sums and the locations.  measure (default None: nothing is added): a callable that receives the pass's state
        (measures.build_report: the per-measure results are formed here, where the flat map buffer exists); it forces the combined pass,
        without the heat maps when weight is None."""
        dec = self.decoder
        top_k, tau = self._check_confidence_args(top_k, temperature)
        B, Tp = seqs.shape
        dev = dec.pos_embedding.device
        if weight is not None or measure is not None:
            dec._alignment_selection(layers, head_weights)
        if weight is not None:
            weight = self._check_uncertainty_weight(weight, seqs.shape)
        Ls, rows, lens_t, sub_s, mem32, memb, tokens, at = self._scored_rows(mem32, memb, lens_s, seqs, seq_mask)
        nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
        none = lambda *sh: torch.full(sh, -1, dtype=torch.int64, device=dev)   # noqa: E731
        conf = TokenConfidence(nan(B, Tp), nan(B, Tp), none(B, Tp), none(B, Tp, top_k), nan(B, Tp, top_k))
        out = offs = map_off = heat = own = None
        if rows:
            if weight is None and measure is None:
                logits = dec.logits_packed(tokens, lens_t, mem32, memb, sub_s, 1 if as_decoded else 0)
            else:
                out, offs, map_off, logits = dec._cross_attention_maps_flat(tokens, lens_t, mem32, memb, sub_s, layers, head_weights,
                                                                            1 if as_decoded else 0, None, True)
                own = (out, offs, map_off, sub_s)   # the maps over the memory's own patches: what a measure sums before any expansion
                if kept is not None and (weight is not None or return_alignment):
                    out, offs, map_off, sub_s = self._expand_maps(out, offs, rows, lens_t, sub_s, lens_s, kept, grids)
            chosen = torch.cat([seqs[i, 1:Ls[i]] for i in rows]).to(dev)
            lp, ent, rank, ids, top_lp = ops.token_confidence(logits, chosen, top_k, tau)
            conf.log_prob[at], conf.entropy[at], conf.rank[at] = lp, ent, rank.long()
            conf.top_tokens[at], conf.top_log_probs[at] = ids.long(), top_lp
            if weight is not None:
                if isinstance(weight, str):
                    w = ent if weight == "entropy" else -lp if weight == "surprisal" else 1.0 - torch.exp(lp)
                else:
                    w = weight.to(device=dev, dtype=torch.float32)[at]
                cu_t, cu_s = EG.cu_from_lens(lens_t, dev), EG.cu_from_lens(sub_s, dev)
                heat = ops.attn_map_weighted_sum(out, map_off, cu_t, cu_s, w.contiguous(), max(lens_t), layout=(lens_t, sub_s, offs))
        if measure is not None:
            measure(self, seqs=seqs, Ls=Ls, rows=rows, lens_t=lens_t, own=own, conf=conf, grids=grids, patch_size=patch_size, lens_s=lens_s,
                    kept=kept)
        if weight is not None or (measure is not None and return_alignment):
            if kept is not None:
                lens_s = [h * w for h, w in grids]
            if weight is not None:
                conf.uncertainty = [torch.zeros(h, w, dtype=torch.float32, device=dev) for h, w in grids]
                o = 0
                for i, s in zip(rows, sub_s):
                    conf.uncertainty[i] = heat[o:o + s].view(*grids[i])
                    o += s
            if return_alignment:
                conf.alignment = self._located(seqs.shape, lens_s, rows, lens_t, sub_s, at, out, offs, map_off, grids, patch_size, return_maps)
        return conf

    def token_confidence(self, img_latent, latent_attention_mask, seqs, seq_mask=None, top_k=5, temperature=1.0, as_decoded=True):
        """Per-token confidence of decoded (or any) sequences (an extension) -> TokenConfidence.  For seqs (B, T) over the memories
        img_latent (B, S_max, E) / latent_attention_mask: one teacher-forced pass over input indices 0 .. L_i - 2 (L_i as in
        cross_attention_maps; all layers, no maps), with the KV-cached decode's positions when as_decoded (default), so that row j holds the
        logits the decode chose index j + 1 from; then one launch (ops.token_confidence) scores the token actually at each index,
        seqs[i, 1:L_i], under softmax(logits / temperature): its log-probability, the entropy, its rank and the top_k (1 .. 8) best tokens.
        Works after every decode mode - greedy, beam, speculative, prompted, constrained, FP8 memory cache - because it reads the memory
        itself, not the KV caches: engine state, graphs and caches stay untouched, and a decode after it is bitwise the decode before it.
        Runs under the caller's autocast, as forward does.  For a grammar-constrained decode the scores are the UNCONSTRAINED model's (the
        decode's own log_probs are renormalised over the allowed tokens): rank > 0 then marks a token the grammar forced.  ValueError for
        top_k outside 1 .. min(8, V) or a temperature that is not positive and finite."""
        self._check_confidence_args(top_k, temperature)
        self._alignment_lengths(seqs, seq_mask)
        mem32, lens_s = EG.unpad_rows(img_latent.to(self.decoder.pos_embedding.device), latent_attention_mask)
        with torch.no_grad():
            return self._confidence_packed(mem32, None, lens_s, seqs, seq_mask, top_k, temperature, as_decoded)

    def uncertainty_maps(self, img_latent, latent_attention_mask, seqs, seq_mask=None, weight="entropy", layers=None, head_weights=None, grids=None,
                         top_k=5, temperature=1.0, return_alignment=False):
        """token_confidence plus a page uncertainty map (an extension) -> TokenConfidence with `uncertainty` filled: per image an (h_p, w_p)
        fp32 heat map over its patch grid, heat[s] = sum_j weight[j] * map[j, s] - every token's cross-attention map (cross_attention_maps;
        layers / head_weights as there, decode positions) added up with a per-token weight, so that the regions the unsure tokens looked at
        light up.  One teacher-forced pass gives the maps and the logits.  weight: "entropy" (the step's entropy), "surprisal" (-log_prob),
        "error" (1 - exp(log_prob)) or a (B, T') tensor of the caller's, of which only the scored entries (index 1 .. L_i - 1) are read;
        anything else raises ValueError.  grids (required): the images' patch grids [(h_p, w_p), ...] with h_p * w_p = S_i (ValueError
        otherwise).  return_alignment also fills `alignment` with what locate_tokens returns for the same arguments, from the same maps.  As
        in token_confidence, the scores after a grammar-constrained decode are the unconstrained model's.  Which weight marks real errors
        best on trained checkpoints has not been measured, nor which layers and heads to average."""
        if grids is None:
            raise ValueError("grids is required: one (h_p, w_p) per image")
        self._check_confidence_args(top_k, temperature)
        self.decoder._alignment_selection(layers, head_weights)
        B, Lm = img_latent.shape[0], img_latent.shape[1]
        lens_s = [Lm] * B if latent_attention_mask is None else [int(l) for l in (~latent_attention_mask).sum(dim=1).tolist()]
        grids = self._check_grids(grids, lens_s)
        self._alignment_lengths(seqs, seq_mask)
        self._check_uncertainty_weight(weight, seqs.shape)
        patch_size = getattr(self.encoder, "patch_size", None)
        if return_alignment and (patch_size is None or float(patch_size) <= 0):
            raise ValueError("return_alignment needs the encoder's patch_size (the model has no encoder to take it from)")
        mem32, lens_s = EG.unpad_rows(img_latent.to(self.decoder.pos_embedding.device), latent_attention_mask)
        with torch.no_grad():
            return self._confidence_packed(mem32, None, lens_s, seqs, seq_mask, top_k, temperature, True, weight, layers, head_weights, grids,
                                           patch_size, return_alignment)

    # ---- per-measure results (an extension) ---------------------------------------------------------------------------------
    def measure_report(self, img_latent, latent_attention_mask, seqs, seq_mask=None, config=None, target_lmx_seqs=None, layers=None,
                       head_weights=None, grids=None, patch_size=None, as_decoded=True):
        """Per-MEASURE results of decoded (or any) sequences (an extension) -> measures.MeasureReport: the rows cut at the delimiter tokens
        of `config` (a measures.MeasureConfig; default: at every `measure` token), and over each span the tokens' confidence (mean and
        lowest log-probability, the weakest token, mean and highest entropy, tokens that were not the arg-max), where on the page the span
        looked - the tokens' cross-attention maps summed over the span, reduced to a centre, a spread and a quantile box in pixels - and,
        with target_lmx_seqs (as error_maps takes them), the substitutions, insertions and deletions that fall into it.  It runs inside the
        combined confidence + alignment pass of uncertainty_maps, where the flat map buffer exists: the segmentation and the segmented
        reductions are device work (ops.token_segments, segment_reduce, attn_map_segment_sum, attn_map_extent) and the per-token maps are
        never copied out; one copy to the host per call, the segment counts.  grids (required), layers, head_weights and as_decoded as in
        locate_tokens / uncertainty_maps; patch_size defaults to the encoder's.  Whether cross-attention localises measures on trained
        checkpoints, which layers, heads or weight do it best and what confidence marks a wrong measure have not been measured."""
        from ..measures import MeasureConfig, report_hook
        if grids is None:
            raise ValueError("grids is required: one (h_p, w_p) per image")
        config = MeasureConfig() if config is None else config
        if not isinstance(config, MeasureConfig):
            raise TypeError(f"config must be a measures.MeasureConfig, got {type(config).__name__}")
        config.resolve(self.decoder, seqs.shape)   # argument errors before any work
        self.decoder._alignment_selection(layers, head_weights)
        B, Lm = img_latent.shape[0], img_latent.shape[1]
        lens_s = [Lm] * B if latent_attention_mask is None else [int(l) for l in (~latent_attention_mask).sum(dim=1).tolist()]
        grids = self._check_grids(grids, lens_s)
        if patch_size is None:
            patch_size = getattr(self.encoder, "patch_size", None)
        if patch_size is None or float(patch_size) <= 0:
            raise ValueError("patch_size is needed (the model has no encoder to take it from) and must be positive")
        self._alignment_lengths(seqs, seq_mask)
        mem32, lens_s = EG.unpad_rows(img_latent.to(self.decoder.pos_embedding.device), latent_attention_mask)
        with torch.no_grad():
            hook = report_hook(config, None if target_lmx_seqs is None else self._error_weights(seqs, seq_mask, target_lmx_seqs, None)[0])
            self._confidence_packed(mem32, None, lens_s, seqs, seq_mask, 5, 1.0, as_decoded, None, layers, head_weights, grids, patch_size,
                                    measure=hook)
        return hook.report

    # ---- ground-truth error maps (an extension) -----------------------------------------------------------------------------
    def _error_weights(self, seqs, seq_mask, target_lmx_seqs, pad_idx):
        """(ops.EditAlignment of seqs at their seq_mask positions - up to and including the first <eos> when seq_mask is None - against the
        targets, utils.error_token_weights of it): the per-token weight of error_maps.  Device work only."""
        from ..utils import _pad_targets, error_token_weights
        dev = self.decoder.pos_embedding.device
        seqs = seqs.to(dev)
        keep = self.create_inference_mask(seqs) if seq_mask is None else seq_mask.to(dev).bool()
        tgt, target_lens = _pad_targets(target_lmx_seqs, pad_idx, dev)
        if tgt.shape[0] != seqs.shape[0]:
            raise ValueError(f"{seqs.shape[0]} decoded rows against {tgt.shape[0]} targets")
        al = ops.edit_alignment(seqs, keep, tgt, target_lens)
        return al, error_token_weights(al, keep.sum(dim=-1))

    def error_maps(self, img_latent, latent_attention_mask, seqs, seq_mask, target_lmx_seqs, pad_idx=None, grids=None, layers=None,
                   head_weights=None, return_alignment=False):
        """Where on the page the REAL errors of decoded rows are (an extension) -> (TokenConfidence, ops.EditAlignment).  seqs / seq_mask
        (B, T') are aligned to the ground truth on the device (ops.edit_alignment; targets as utils.symbol_error_rate takes them: a list of
        1-D tensors, or a padded tensor with pad_idx; <bos> / <eos> count where present, so give the targets as the decode writes its
        rows) and every output token gets the weight utils.error_token_weights states: 1 when it is substituted or inserted, plus the
        number of target tokens missing in front of it.  That weight goes through uncertainty_maps(weight=<tensor>): the TokenConfidence's
        `uncertainty` is, per image, the (h_p, w_p) heat map of the cross-attention maps of the tokens in error - all zero for a perfect
        row - next to the model's own confidence in the same tokens, which utils.confidence_error_auroc relates to pred_op != 0.  grids,
        layers, head_weights and return_alignment (the TokenAlignment, in `.alignment`) as in uncertainty_maps.  How well the maps point at
        the faulty symbols on trained checkpoints has not been measured."""
        if grids is None:
            raise ValueError("grids is required: one (h_p, w_p) per image")
        self._alignment_lengths(seqs, seq_mask)   # argument errors before any work
        al, w = self._error_weights(seqs, seq_mask, target_lmx_seqs, pad_idx)
        conf = self.uncertainty_maps(img_latent, latent_attention_mask, seqs, seq_mask, weight=w, layers=layers, head_weights=head_weights,
                                     grids=grids, return_alignment=return_alignment)
        return conf, al

    def cached_set_up_inference(self, img_latent, max_len):
        self.decoder.prepare_caches(img_latent)
        B, dev = img_latent.shape[0], img_latent.device
        seqs = torch.full([B, max_len], fill_value=self.decoder.pad_idx, dtype=torch.long, device=dev)
        seqs[:, 0] = self.decoder.bos_idx
        return seqs, torch.zeros_like(seqs, dtype=torch.float), torch.full([B], fill_value=False)

    def cached_get_next_token(self, seqs, t, latent_attention_mask):
        """argmax + log-prob of the next token (M:575-583); passes `t` as the position of token t-1 (quirk Q1)."""
        logits = self.decoder.cached_generate(seqs[:, t - 1].unsqueeze(1), t, latent_attention_mask).squeeze(1)
        idx = torch.argmax(logits, dim=-1)
        lp = F.log_softmax(logits, dim=-1).gather(-1, idx.unsqueeze(1)).squeeze(1)
        return idx, lp

    def _check_prefix(self, prefix, n, max_len):
        """Prompted decoding (an extension): `prefix` as the entry points take it - None, or one entry per image, each a 1-D integer tensor
        or list (possibly empty) holding the image's tokens of output indices 1 .. P_i; a single 1-D tensor stands for one image - checked
        and returned as a list of n 1-D int64 CPU tensors (None stays None).  ValueError for a wrong count, an id outside [0, V), <bos> or
        <pad>, an <eos> before the end of a prompt, or P_i > max_len - 1."""
        if prefix is None:
            return None
        dec = self.decoder
        if torch.is_tensor(prefix) and prefix.dim() == 1:
            prefix = [prefix]
        try:
            rows = [torch.as_tensor(p) for p in prefix]
        except (TypeError, ValueError) as e:
            raise ValueError(f"prefix must be a sequence of 1-D integer tensors or lists, one per image: {e}") from None
        if len(rows) != n:
            raise ValueError(f"prefix holds {len(rows)} entries for {n} images")
        out = []
        for i, r in enumerate(rows):
            if r.numel() == 0:
                out.append(torch.zeros(0, dtype=torch.int64))
                continue
            if r.dim() != 1 or r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool:
                raise ValueError(f"prefix[{i}] must be a 1-D integer tensor or list, got shape {tuple(r.shape)} dtype {r.dtype}")
            r = r.detach().to(device="cpu", dtype=torch.int64)
            if r.numel() > max_len - 1:
                raise ValueError(f"prefix[{i}] holds {r.numel()} tokens: more than max_len - 1 = {max_len - 1}")
            if int(r.min()) < 0 or int(r.max()) >= dec.vocab_size:
                raise ValueError(f"prefix[{i}] holds a token id outside [0, {dec.vocab_size})")
            if bool(((r == dec.bos_idx) | (r == dec.pad_idx)).any()):
                raise ValueError(f"prefix[{i}] holds <bos> or <pad>: a prompt starts after <bos> and has no padding")
            if bool((r[:-1] == dec.eos_idx).any()):
                raise ValueError(f"prefix[{i}] holds <eos> before its end: <eos> may only be a prompt's last token")
            out.append(r)
        return out

    @staticmethod
    def _no_prefix(prefix, what):
        if prefix is not None:
            raise ValueError(f"prefix (prompted decoding) cannot be combined with {what}: out of scope here")

    @staticmethod
    def _check_grammar(grammar, prefix=None):
        """Grammar-constrained decoding (an extension): `grammar` as the entry points take it - None, or a grammar.TokenAutomaton."""
        if grammar is None:
            return
        from ..grammar import TokenAutomaton
        if not isinstance(grammar, TokenAutomaton):
            raise TypeError(f"grammar must be a grammar.TokenAutomaton, got {type(grammar).__name__}")
        if prefix is not None:
            raise ValueError("grammar (constrained decoding) cannot be combined with prefix (prompted decoding): out of scope here")

    @staticmethod
    def _check_prefill(prefill, grammar):
        if prefill and grammar is not None:
            raise ValueError("prefill (prompt prefill) cannot be combined with grammar (constrained decoding): out of scope here")

    @staticmethod
    def _check_loop_guard(loop_guard, **others):
        """Loop detection (an extension): `loop_guard` as the entry points take it - None, or a loops.LoopGuard (TypeError otherwise);
        others: the arguments of the modes it cannot be combined with, by the name the ValueError gives them (None / False = not used)."""
        from ..loops import check_guard, refuse_guard
        if check_guard(loop_guard) is not None:
            for what, arg in others.items():
                if arg is not None and arg is not False:
                    refuse_guard(loop_guard, what)
        return loop_guard

    def _loop_result(self, seqs, lps, caps, stop, period, start, guard):
        """A guarded run's rows -> (seqs, log_probs, mask, LoopReport): a loop stop is a cap found on the device, so the mask is
        _mask_and_clip_capped's at the effective caps - stop + 1, or start + period with trim (one copy of the cycle)."""
        from ..loops import LoopReport
        report = LoopReport(stop.clone(), period.clone(), start.clone())
        return self._mask_and_clip_capped(seqs, lps, report.caps(caps, guard.trim)) + (report,)

    def _greedy_packed(self, mem32, memb, lens, max_len, on_chunk=None, prefix=None, grammar=None, *, prefill=False, loop_guard=None):
        blocks = self.decoder._cached_blocks()
        self._check_grammar(grammar, prefix)
        self._check_prefill(prefill, grammar)
        self._check_loop_guard(loop_guard, **{"prefix (prompted decoding)": prefix, "grammar (constrained decoding)": grammar,
                                              "prefill (prompt prefill)": prefill})
        prompt = self._check_prefix(prefix, len(lens), max_len)
        blocks.prepare_caches_packed(mem32, memb, lens)
        eng = blocks.engine(self.decoder.pos_embedding.device)
        if loop_guard is not None:
            seqs, lps, _ = eng.greedy(max_len, on_chunk=on_chunk, loop_guard=loop_guard)
            return self._loop_result(seqs.clone(), lps.clone(), [max_len] * len(lens), *eng.loop_report(), loop_guard)
        if grammar is not None:
            seqs, lps, _ = eng.greedy(max_len, on_chunk=on_chunk, grammar=grammar)
        else:
            kw = {"prefill": True} if prefill else {}
            seqs, lps, _ = eng.greedy(max_len, on_chunk=on_chunk) if prompt is None else eng.greedy(max_len, on_chunk=on_chunk, prompt=prompt, **kw)
        return self.mask_and_clip_seqs(seqs.clone(), lps.clone())

    def cached_greedy_generate(self, img_latent, latent_attention_mask=None, max_len=1536, prefix=None, *, grammar=None, prefill=False,
                               loop_guard=None):
        """Batched greedy decode with KV caching (M:600-615) -> seqs (B,T') int64, log_probs (B,T') fp32, mask (B,T') bool.
        The whole loop runs as replays of one captured hipGraph; the host only polls an "all finished" counter.
        prefix (an extension, default None = off): prompted decoding - one entry per image (a 1-D integer tensor or list, possibly empty;
        a single 1-D tensor for one image) with the tokens of output indices 1 .. P_i <= max_len - 1 that are already known.  The row takes
        them whatever the model would choose, log_probs holds the model's log-probability of each, and greedy decoding goes on from index
        P_i + 1; a prompt-final <eos> ends the row.  Ids must lie in [0, V), never <bos> or <pad>, <eos> only last (ValueError).  Where
        the prompt is the model's own greedy output the result is bitwise the unprompted one.
        grammar (an extension, default None = off): a grammar.TokenAutomaton - at every index a row takes the best token its automaton state
        allows, log_probs holds the log-softmax over the allowed tokens (the policy actually run), and the state advances on the device
        inside the replayed graph.  An automaton that allows everything gives the unconstrained result bit for bit.  Not combinable with
        prefix (ValueError).
        prefill (an extension, default False = off): prompt prefill - the first C = min_i P_i prompt tokens, which every image has, are
        computed in one teacher-forced pass over the memories instead of C decode steps, and decoding goes on from index C + 1 (images
        with P_i > C keep taking their forced tokens there).  The tokens of a prompt and the mask are what they are without it; the
        log-probs of indices 1 .. C come from the pass and, like everything decoded after them, agree with the stepwise run's within the
        pass-versus-decode bars (1e-4 fp32, 0.07 bf16), so a free token can differ where the model's top two logits are that close.
        Without a prefix, or with an empty prompt in the batch, it changes nothing.  Not with an FP8 memory cache (ValueError).
        loop_guard (an extension, default None = off): a loops.LoopGuard - a row whose tail is periodic by the guard's rule (loops.py) ends at
        that index, `stop`, inside the replayed graph: it counts as finished from there on, so a batch whose remaining rows all loop ends
        early.  Up to `stop` tokens, log-probs and mask are bitwise the unguarded call's; the mask ends at `stop` (with trim: after one copy
        of the cycle) and no <eos> is written.  A fourth value is returned then, the loops.LoopReport (stop, period, start per row; period
        0 = no loop).  Not combinable with prefix, grammar or prefill (ValueError)."""
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        return self._greedy_packed(mem32, None, lens, max_len, prefix=prefix, grammar=grammar, prefill=prefill, loop_guard=loop_guard)

    def _beam_packed(self, mem32, memb, lens, beam_width, max_len, length_penalty):
        blocks = self.decoder._cached_blocks()
        K = int(beam_width)
        if not 1 <= K <= 16:
            raise ValueError(f"beam_width must be in [1, 16], got {beam_width}")
        if len(lens) * K > blocks.max_batch_size:
            raise ValueError(f"{len(lens)} images x beam width {K} = {len(lens) * K} decode rows exceed the cache's max batch size of "
                             f"{blocks.max_batch_size}")
        blocks.prepare_caches_packed(mem32, memb, lens, group_size=K)
        eng = blocks.engine(self.decoder.pos_embedding.device)
        seqs, lps, _ = eng.beam(max_len, K, length_penalty)
        return self.mask_and_clip_seqs(seqs, lps)

    def cached_beam_generate(self, img_latent, latent_attention_mask=None, beam_width=4, max_len=1536, length_penalty=1.0, prefix=None, *,
                             loop_guard=None):
        """Beam-search decode with KV caching (an extension: the reference decodes greedily) -> seqs (B,T') int64, log_probs (B,T') fp32 per
        token, mask (B,T') bool, as cached_greedy_generate.  Each image keeps beam_width hypotheses; a step extends each live one by its
        beam_width best tokens, keeps the beam_width best by cumulative log-probability, and a hypothesis ends at <eos>.  The result per image
        is the hypothesis with the highest cum / len^length_penalty (len: tokens after <bos>, <eos> included).  beam_width = 1 is greedy,
        bit for bit.  The K hypotheses of an image share its cross K/V; a selection moves no self K/V, only an ancestor table.
        prefix (prompted decoding, cached_greedy_generate) is not supported here: anything but None raises ValueError; so does a
        loop_guard (loops.scan_repeats covers the result after the fact)."""
        self._no_prefix(prefix, "beam search")
        self._check_loop_guard(loop_guard, **{"beam search": True})
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        return self._beam_packed(mem32, None, lens, beam_width, max_len, length_penalty)

    def _speculative_packed(self, mem32, memb, lens, max_len, draft_len, ngram=3, drafts=None, poll=16, use_graph=True, prefix=None):
        blocks = self.decoder._cached_blocks()
        prompt = self._check_prefix(prefix, len(lens), max_len)
        D = int(draft_len)
        if not 1 <= D <= 7:
            raise ValueError(f"draft_len must be in [1, 7], got {draft_len}")
        if len(lens) * (D + 1) > blocks.max_batch_size:
            raise ValueError(f"{len(lens)} images x (draft_len {D} + 1) = {len(lens) * (D + 1)} decode rows exceed the cache's max batch size "
                             f"of {blocks.max_batch_size}")
        if blocks.__dict__.get("_memory_fp8", False):
            raise ValueError("speculative decoding does not support an FP8 memory cache; use memory_cache_dtype=None")
        blocks.prepare_caches_packed(mem32, memb, lens, group_size=D + 1, per_row_cross=True)
        eng = blocks.engine(self.decoder.pos_embedding.device)
        kw = {} if prompt is None else {"prompt": prompt}
        seqs, lps, _ = eng.speculative(max_len, D, ngram=ngram, drafts=drafts, poll=poll, use_graph=use_graph, **kw)
        return self.mask_and_clip_seqs(seqs.clone(), lps.clone())

    def cached_speculative_generate(self, img_latent, latent_attention_mask=None, max_len=1536, draft_len=4, ngram=3, drafts=None, prefix=None, *,
                                    loop_guard=None):
        """Speculative greedy decode with KV caching (an extension: the reference emits one token per step) -> seqs (B,T') int64, log_probs
        (B,T') fp32, mask (B,T') bool: bitwise what cached_greedy_generate returns for the same arguments, in fewer decode steps when drafts
        are accepted.  Each image owns draft_len + 1 decode rows (so B * (draft_len + 1) <= max batch size, 1 <= draft_len <= 7): one step
        verifies up to draft_len draft tokens and emits the accepted ones plus one.  Drafts are looked up in the sequence's own earlier
        n-grams (suffixes of up to `ngram` tokens, 1..8) or taken from `drafts` (B, max_len) - the token proposed for each index, negative =
        none.  An image that ends early idles until the batch does.  Beam search, sampling, continuous batching (slot mode) and an FP8
        memory cache cannot be combined with it (ValueError): out of scope here.
        prefix: prompted decoding as in cached_greedy_generate, bitwise its result; the prompt is consumed draft_len + 1 tokens per step.
        loop_guard: not supported here (ValueError); loops.scan_repeats covers the result after the fact."""
        self._check_loop_guard(loop_guard, **{"speculative decoding": True})
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        return self._speculative_packed(mem32, None, lens, max_len, draft_len, ngram, drafts, prefix=prefix)

    def _continuous_run(self, mem32, memb, lens, max_len, slots, poll, use_graph, **sampling):
        """(engine, caps, generator of finished image indices) of a continuous-batching run; argument errors are raised here, at the call.
        sampling: DecodeEngine.continuous's sample / uniforms / group."""
        blocks = self.decoder._cached_blocks()
        caps = _continuous_caps(max_len, len(lens) * sampling.get("group", 1))
        eng = blocks.engine((mem32 if mem32 is not None else memb).device)
        S = blocks.max_batch_size if slots is None else slots
        return eng, caps, eng.continuous(mem32, memb, lens, caps, S, poll=poll, use_graph=use_graph, **sampling)

    def _continuous_packed_iter(self, mem32, memb, lens, max_len, slots=None, poll=16, use_graph=True, grammar=None, loop_guard=None):
        """Continuous-batching greedy decode of packed memories: yields (index, seqs (1,T'), log_probs (1,T'), mask (1,T')) per image in
        completion order, each what _greedy_packed of that image alone at its cap returns (with a loop_guard: and its LoopReport)."""
        self._check_grammar(grammar)
        self._check_loop_guard(loop_guard, **{"grammar (constrained decoding)": grammar})
        kw = {} if loop_guard is None else {"loop_guard": loop_guard}
        eng, caps, run = self._continuous_run(mem32, memb, lens, max_len, slots, poll, use_graph, grammar=grammar, **kw)

        def images():
            for i in run:
                if loop_guard is not None:
                    yield (i,) + self._loop_result(eng.cont_seqs[i:i + 1, :caps[i]], eng.cont_lps[i:i + 1, :caps[i]], [caps[i]],
                                                   *eng.cont_loops[:, i:i + 1], loop_guard)
                    continue
                yield (i,) + self._mask_and_clip_capped(eng.cont_seqs[i:i + 1, :caps[i]], eng.cont_lps[i:i + 1, :caps[i]], [caps[i]])
        return images()

    def _mask_and_clip_capped(self, seqs, lps, caps):
        """mask_and_clip_seqs with per-row caps: positions at or past a row's cap are never part of it."""
        seq_mask = self.create_inference_mask(seqs)
        if min(caps) < seqs.shape[1]:
            seq_mask &= torch.arange(seqs.shape[1], device=seqs.device) < torch.tensor(caps, device=seqs.device).unsqueeze(1)
        seqs = seqs.masked_fill(~seq_mask, self.decoder.pad_idx)
        lps = lps.masked_fill(~seq_mask, 0.0)
        n = int(seq_mask.sum(dim=-1).max())
        return seqs[:, :n], lps[:, :n], seq_mask[:, :n]

    def _continuous_packed(self, mem32, memb, lens, max_len, slots=None, poll=16, use_graph=True, **sampling):
        self._check_grammar(sampling.get("grammar"))
        guard = self._check_loop_guard(sampling.get("loop_guard"), **{"sample (sampled rollouts)": sampling.get("sample"),
                                                                     "grammar (constrained decoding)": sampling.get("grammar")})
        eng, caps, run = self._continuous_run(mem32, memb, lens, max_len, slots, poll, use_graph, **sampling)
        for _ in run:
            pass
        if guard is not None:
            return self._loop_result(eng.cont_seqs, eng.cont_lps, caps, *eng.cont_loops, guard)
        return self._mask_and_clip_capped(eng.cont_seqs, eng.cont_lps, caps)

    def cached_continuous_generate(self, img_latent, latent_attention_mask=None, max_len=1536, slots=None, prefix=None, *, grammar=None,
                                   loop_guard=None):
        """Continuous-batching greedy decode (an extension: the reference decodes one static batch) -> seqs (N,T') int64, log_probs (N,T')
        fp32, mask (N,T') bool, as cached_greedy_generate on the same batch.  `slots` decode rows (default: the cache's max batch size)
        work through the N images in input order; a row that finishes (<eos> or its cap) is refilled with the next image while the others
        go on, so N may exceed the max batch size.  max_len: one cap for every image, or a sequence of N per-image caps (positions at or
        past an image's cap are masked).  prefix (prompted decoding, cached_greedy_generate) is not supported here: anything but None
        raises ValueError.  grammar: constrained decoding as in cached_greedy_generate; every image gets what it gets there alone.
        loop_guard: loop detection as in cached_greedy_generate - an image that loops frees its row at `stop` for the next image in the
        queue, and a fourth value, the loops.LoopReport over the N images, is returned.  Not combinable with grammar (ValueError)."""
        self._no_prefix(prefix, "continuous batching")
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        kw = {} if loop_guard is None else {"loop_guard": loop_guard}
        return self._continuous_packed(mem32, None, lens, max_len, slots, grammar=grammar, **kw)

    def _check_flush_interval(self, flush_interval):
        """flush_interval of the streamed continuous-batching entry points: an int in [1, the cache's maximum sequence length]."""
        top = self.decoder._cached_blocks().max_decoder_seq_len
        if isinstance(flush_interval, bool) or not isinstance(flush_interval, int) or not 1 <= flush_interval <= top:
            raise ValueError(f"flush_interval must be an int in [1, {top}] (the cache's max sequence length), got {flush_interval!r}")
        return flush_interval

    def _streamed_continuous_packed_iter(self, mem32, memb, lens, max_len, slots=None, flush_interval=25, use_graph=True, grammar=None,
                                         tags=None):
        """Streamed continuous-batching greedy decode of packed memories (DecodeEngine.continuous(flush=)): a generator of STEP and
        INFERENCE_FINISH events, as streamed_continuous_generate describes them.  tags: None, or per image a dictionary that is merged
        into the payload of its events (the page entry point names the row's page and system with it).  Argument errors are raised here,
        at the call.  The generator's return value (`yield from`) is _continuous_packed's triple of all rows."""
        self._check_grammar(grammar)
        self._check_flush_interval(flush_interval)
        eng, caps, run = self._continuous_run(mem32, memb, lens, max_len, slots, 16, use_graph, grammar=grammar, flush=flush_interval)
        if tags is not None and len(tags) != len(caps):
            raise ValueError(f"{len(tags)} tags for {len(caps)} images")

        def events():
            for ev in run:
                i = ev[1]
                tag = {} if tags is None else tags[i]
                if ev[0] == "step":
                    yield {"type": InferenceEvent.STEP.value, "payload": {"image": i, "start": ev[2], "tokens": ev[3], "log_probs": ev[4], **tag}}
                else:
                    seqs, lps, mask = self._mask_and_clip_capped(eng.cont_seqs[i:i + 1, :caps[i]], eng.cont_lps[i:i + 1, :caps[i]], [caps[i]])
                    yield {"type": InferenceEvent.INFERENCE_FINISH.value,
                           "payload": {"image": i, "sequence": seqs, "log_probs": lps, "mask": mask, **tag}}
            return self._mask_and_clip_capped(eng.cont_seqs, eng.cont_lps, caps)   # (the generator's value: all rows, as _continuous_packed)
        return events()

    def streamed_continuous_generate(self, img_latent, latent_attention_mask=None, max_len=1536, slots=None, flush_interval=25, *, grammar=None,
                                     loop_guard=None):
        """cached_continuous_generate as a generator of {"type", "payload"} events (an extension: the reference streams one image at a
        time), so that a caller sees every image's tokens while `slots` rows decode the batch.  Every flush_interval decode steps - sooner
        where a row reaches its cap - each image that is being decoded and has new tokens gives one STEP {"image": i, "start": t0,
        "tokens": int32 (1, n), "log_probs": fp32 (1, n)}, both on the CPU: the row's indices t0 .. t0 + n - 1.  An image's STEP events tile
        its row from index 1 (<bos> is never sent) through its last token - its <eos>, or the token at its cap - and all precede its
        INFERENCE_FINISH {"image": i, "sequence", "log_probs", "mask"}, the three exactly what cached_continuous_generate's row i is when
        decoded alone (iter_continuous_inference's tuple).  Within a poll the STEP events come in slot order, then the INFERENCE_FINISH of
        the rows that ended.  An image with a cap below 2 has no STEP and finishes first.  The event list is a function of the inputs,
        `slots` and flush_interval alone.  max_len, slots, grammar: as in cached_continuous_generate; a prefix is not offered.
        flush_interval: an int in [1, the cache's max sequence length] (ValueError, at the call).  loop_guard: not supported in a streamed
        run (ValueError)."""
        self._check_loop_guard(loop_guard, **{"streamed continuous batching": True})
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        return self._streamed_continuous_packed_iter(mem32, None, lens, max_len, slots, flush_interval, grammar=grammar)

    def streamed_cached_greedy_generate(self, img_latent, latent_attention_mask=None, max_len=1536, flush_interval=25, prefix=None, *,
                                        grammar=None, prefill=False, loop_guard=None):
        """Generator of {"type", "payload"} events (M:625-647); single image only.
        prefix: prompted decoding as in cached_greedy_generate; STEP events carry the forced tokens like any others.
        grammar: constrained decoding as in cached_greedy_generate (not with prefix).
        prefill: prompt prefill as in cached_greedy_generate; the STEP events of the prefilled tokens follow each other at once.
        loop_guard: not supported in a streamed run (ValueError)."""
        self._check_loop_guard(loop_guard, **{"streamed greedy decoding": True})
        if img_latent.shape[0] != 1:
            raise ValueError("Streamed generation only supports single image batches")
        self._check_grammar(grammar, prefix)
        self._check_prefill(prefill, grammar)
        prompt = self._check_prefix(prefix, 1, max_len)
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        blocks = self.decoder._cached_blocks()
        blocks.prepare_caches_packed(mem32, None, lens)
        eng = blocks.engine(self.decoder.pos_embedding.device)
        # replay the decode graph flush_interval tokens at a time; after each chunk hand out the freshly written tokens
        # (the reference yields STEP at every t % flush_interval == 0 that did not finish the sequence - also at t == max_len - 1, M:641-645)
        kw = {} if grammar is None else {"grammar": grammar}
        for t_done, finished in (eng.greedy_chunks(max_len, flush_interval, **kw) if prompt is None else
                                 eng.greedy_chunks(max_len, flush_interval, prompt=prompt, **({"prefill": True} if prefill else {}))):
            if finished:
                break
            if t_done % flush_interval == 0:
                buf = eng.seqs[:1, t_done - flush_interval + 1:t_done + 1].to(torch.int)
                yield {"type": InferenceEvent.STEP.value, "payload": {"tokens": buf}}
        seqs, lps, mask = self.mask_and_clip_seqs(eng.seqs[:1, :max_len].clone(), eng.logprobs[:1, :max_len].clone())
        yield {"type": InferenceEvent.INFERENCE_FINISH.value, "payload": {"sequence": seqs, "log_probs": lps, "mask": mask}}


class GRPOViTOMR(ViTOMR):
    """ViTOMR prepared for GRPO (M:840-1049): the rollout policy - sampling decode with KV caching - and the helpers around it.  The reward
    functions and the GRPO training loop itself stay outside the hot path; the rollout decode is SURVEY 8f-1."""

    def __init__(self, encoder, transition_head, decoder, teacher_forced_state_dict):
        super().__init__(encoder, transition_head, decoder)
        if isinstance(self.encoder, FineTuneOMREncoder):
            teacher_forced_state_dict = self.convert_teacher_forced_state_dict(teacher_forced_state_dict, encoder.num_frozen_layers)
            self.encoder = OMREncoder(self.encoder.patch_size, self.encoder.pe_max_height, self.encoder.pe_max_width, self.encoder.num_layers,
                                      self.encoder.hidden_dim, **encoder.superclass_kwargs)
        self.load_state_dict(teacher_forced_state_dict)
        self.freeze_component(self.encoder)
        self.freeze_component(self.transition_head)

    def freeze_component(self, component):
        for param in component.parameters():
            param.requires_grad = False
        for child in component.modules():
            if isinstance(child, nn.Dropout):
                child.p = 0.0

    def convert_teacher_forced_state_dict(self, teacher_forced_state_dict, num_frozen_layers):
        """frozen_blocks / fine_tune_blocks keys -> one encoder_blocks stack, fine-tune layer numbers shifted by num_frozen_layers (M:860-880)."""
        converted = {}
        pat = re.compile(r"(?:\w|\.)+?(\d+)(?:\w|\.)+")
        for name in teacher_forced_state_dict.keys():
            if "frozen_blocks" in name:
                new = name.replace("frozen_blocks", "encoder_blocks")
            elif "fine_tune_blocks" in name:
                new = name.replace("fine_tune_blocks", "encoder_blocks")
                m = pat.match(name)
                if m:
                    n = int(m.group(1))
                    new = new.replace(f"layers.{n}", f"layers.{n + num_frozen_layers}")
            else:
                new = name
            converted[new] = teacher_forced_state_dict[name]
        return converted

    def create_rollout_mask(self, rollouts):
        """Name the reference's own tests use (tests/test_vitomr.py:438-442) for the mask `cached_forward_rollout_policy` returns: True up to
        and including each row's first <eos> - the same rule as `create_inference_mask`."""
        return self.create_inference_mask(rollouts)

    def expand_img_latent_for_rollout(self, img_latent, latent_attention_mask, group_size):
        img_latent = img_latent.unsqueeze(1).expand(-1, group_size, -1, -1).flatten(start_dim=0, end_dim=1)
        latent_attention_mask = latent_attention_mask.unsqueeze(1).expand(-1, group_size, -1).flatten(start_dim=0, end_dim=1)
        return img_latent, latent_attention_mask

    def uncached_forward_rollout_policy(self, img_latent, latent_attention_mask, max_actions=768, top_k=50, temperature=1.2):
        """The reference's deprecated rollout policy without KV caching (M:897-945; "absurdly slow ... treated as deprecated"): every step
        re-runs `decoder.generate` (the uncached HIP forward) on the whole prefix.  Its arithmetic differs from the cached policy's and is kept:
        log-probs are log_softmax over the FULL vocabulary of the top-k-masked logits divided by the temperature, the outputs are not clipped
        to the longest rollout.  Only the small per-step glue (top-k of 227 logits, the multinomial draw) runs as torch ops."""
        device = img_latent.device
        R = img_latent.shape[0]
        rollouts = torch.full([R, max_actions], fill_value=self.decoder.pad_idx, dtype=torch.long, device=device)
        rollouts[:, 0] = self.decoder.bos_idx
        rollout_log_probs = torch.zeros_like(rollouts, dtype=torch.float, device=device)
        for t in range(1, max_actions):
            logits = self.decoder.generate(rollouts[:, :t], img_latent, latent_attention_mask=latent_attention_mask)[:, -1, :].float()
            top_k_logits, top_k_indices = torch.topk(logits, top_k, dim=-1)
            softmax_logits = torch.full_like(logits, float("-inf")).scatter(-1, top_k_indices, top_k_logits) / temperature
            next_token_idxs = torch.multinomial(F.softmax(softmax_logits, dim=-1), num_samples=1)
            rollouts[:, t] = next_token_idxs.squeeze(1)
            rollout_log_probs[:, t] = F.log_softmax(softmax_logits, dim=-1).gather(-1, index=next_token_idxs).squeeze(1)
            if torch.all(torch.any(rollouts == self.decoder.eos_idx, dim=-1)):
                break
        rollout_mask = self.create_inference_mask(rollouts)
        return rollouts.masked_fill(~rollout_mask, self.decoder.pad_idx), rollout_log_probs.masked_fill(~rollout_mask, 0.0), rollout_mask

    def prepare_rollouts_for_policy_theta(self, rollouts, rollout_mask):
        rollout_lens = rollout_mask.sum(dim=-1, keepdim=True)
        right_shifted_rollout_lens = rollout_lens - 1
        rollout_attention_mask = torch.arange(int(torch.max(right_shifted_rollout_lens)), device=rollouts.device).repeat([rollouts.shape[0], 1])
        rollout_attention_mask = rollout_attention_mask >= right_shifted_rollout_lens
        return rollouts[:, :-1], rollout_attention_mask

    def forward_teacher_forced(self, img_latent, latent_attention_mask, lmx_seqs, checkpoint_grads):
        input_seqs, target_seqs, lmx_attention_mask = batchify_and_split_lmx_seqs(lmx_seqs, self.decoder.pad_idx, img_latent.device)
        pred = self.decoder(input_seqs, img_latent, lmx_attention_mask, latent_attention_mask, checkpoint_grads=checkpoint_grads)
        return pred, target_seqs

    def batch_policy_inference(self, imgs, max_actions, top_k, temperature):
        img_latent, latent_attention_mask = self.encoder(imgs)
        # the reference calls self.forward_rollout_policy here, a method it does not define (M:977); the cached policy is what it means
        return self.cached_forward_rollout_policy(img_latent, latent_attention_mask, max_actions, top_k, temperature)

    def cached_forward_rollout_policy(self, img_latent, latent_attention_mask, max_actions=768, top_k=50, temperature=1.2, group_size=None,
                                      uniforms=None, prefix=None, *, grammar=None, loop_guard=None):
        """Sampling rollouts with KV caching (M:988-1049): per step keep the top_k logits, draw from softmax(kept / temperature), record
        log_softmax(kept)[drawn]; rows stop mattering after their first <eos>.  Returns rollouts (R, T') int64, rollout_log_probs (R, T') fp32,
        rollout_mask (R, T') bool with padding / zero log-probs outside the mask.

        The whole loop is replayed hipGraphs of `acai_decode_sample_step`.  torch.multinomial's random stream cannot be reproduced: the draws
        are inverse-CDF samples from `uniforms` (R, max_actions) in [0, 1), taken from torch's generator when None (so torch.manual_seed makes
        a rollout reproducible).  group_size (extension): img_latent rows r*group_size .. are the copies expand_img_latent_for_rollout made of
        one image; their cross K/V is then projected and stored once per image instead of once per rollout.  prefix (prompted decoding,
        cached_greedy_generate) is not supported here: anything but None raises ValueError.  grammar (an extension, default None = off): a
        grammar.TokenAutomaton - the top-k filter, the draw and the recorded log_softmax(kept) run over the tokens the rollout's automaton
        state allows, so a rollout cannot hold a transition the automaton forbids; rollout_log_probs is then the log-probability under the
        constrained policy, which is the old policy of the GRPO ratio.  loop_guard: not supported in sampled decoding (ValueError);
        loops.scan_repeats covers the rollouts after the fact (train/grpo.py logs their loop_rate with it)."""
        self._no_prefix(prefix, "sampling")
        self._check_grammar(grammar)
        self._check_loop_guard(loop_guard, **{"sampling": True})
        blocks = self.decoder._cached_blocks()
        G = 1 if group_size is None else int(group_size)
        if img_latent.shape[0] % G:
            raise ValueError(f"{img_latent.shape[0]} rollout rows are not a multiple of group_size {G}")
        lat = img_latent[::G] if G > 1 else img_latent
        msk = latent_attention_mask[::G] if (G > 1 and latent_attention_mask is not None) else latent_attention_mask
        mem32, lens = EG.unpad_rows(lat, msk)
        blocks.prepare_caches_packed(mem32, None, lens, group_size=G)
        eng = blocks.engine(self.decoder.pos_embedding.device)
        seqs, lps, _ = eng.sample(max_actions, top_k, temperature, uniforms=uniforms, grammar=grammar)
        return self.mask_and_clip_seqs(seqs.clone(), lps.clone())

    def cached_continuous_rollout_policy(self, img_latent, latent_attention_mask, max_actions=768, top_k=50, temperature=1.2, slots=None,
                                         group_size=1, uniforms=None):
        """Sampling rollouts through continuous batching (an extension: the reference samples one static batch) -> the triple of
        cached_forward_rollout_policy, in input order, same dtypes and clipping.  `slots` decode rows (default: the cache's max batch size)
        work through the rollouts; a row that draws <eos> or reaches its cap is refilled with the next queued rollout while the others go
        on, so the number of rollouts may exceed the max batch size and a long rollout does not hold the finished ones' rows.  Rollout r draws
        token index t from uniforms[r, t] (`uniforms` (R, max cap) in [0, 1); torch's generator when None) exactly as it would alone in
        cached_forward_rollout_policy, whichever row and step it runs in.  max_actions: one cap, or a sequence of R per-rollout caps.

        group_size = G > 1: img_latent holds the UNEXPANDED images and each is queued G times (rollouts i*G .. i*G+G-1 of the result, uniforms
        rows likewise).  Every admission prefills its own row's region, so an image's cross K/V projection is repeated G times - unlike
        cached_forward_rollout_policy(group_size=G), which stores it once per image.  The grammar-constrained form is
        cached_constrained_continuous_rollout_policy."""
        return self._continuous_rollouts(img_latent, latent_attention_mask, max_actions, top_k, temperature, slots, group_size, uniforms, None)

    def cached_constrained_continuous_rollout_policy(self, img_latent, latent_attention_mask, grammar, max_actions=768, top_k=50, temperature=1.2,
                                                     slots=None, group_size=1, uniforms=None):
        """cached_continuous_rollout_policy under a grammar.TokenAutomaton (an extension; a method of its own because that one's parameter
        list is pinned): every rollout is constrained as in cached_forward_rollout_policy(grammar=) and draws what it draws there alone."""
        self._check_grammar(grammar)
        if grammar is None:
            raise TypeError("grammar must be a grammar.TokenAutomaton, got None")
        return self._continuous_rollouts(img_latent, latent_attention_mask, max_actions, top_k, temperature, slots, group_size, uniforms, grammar)

    def _continuous_rollouts(self, img_latent, latent_attention_mask, max_actions, top_k, temperature, slots, group_size, uniforms, grammar):
        G = int(group_size)
        if G < 1:
            raise ValueError(f"group_size must be >= 1, got {group_size}")
        mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
        kw = {} if grammar is None else {"grammar": grammar}
        return self._continuous_packed(mem32, None, lens, max_actions, slots, sample=(top_k, temperature), uniforms=uniforms, group=G, **kw)


class TeacherForcedViTOMR(ViTOMR):
    """ViTOMR assembled from a (pre-trained MAE) encoder, a transition head and an OMRDecoder (M:649-781)."""

    def __init__(self, omr_encoder, pretrained_mae_state_dict, omr_decoder, transition_head_dim=4096, transition_head_dropout=0.05):
        encoder, decoder = omr_encoder, omr_decoder
        transition_head = _TransitionHead(nn.Linear(encoder.hidden_dim, transition_head_dim), nn.GELU(), nn.Dropout(transition_head_dropout),
                                          nn.Linear(transition_head_dim, decoder.hidden_dim))
        super().__init__(encoder, transition_head, decoder)
        if pretrained_mae_state_dict:
            encoder.load_state_dict(self.create_omr_encoder_state_dict_from_mae(pretrained_mae_state_dict))
        # freezing rules (M:667-677)
        if isinstance(self.encoder, FineTuneOMREncoder) and self.encoder.frozen_blocks:
            for p in self.encoder.frozen_blocks.parameters():
                p.requires_grad = False
            for p in self.encoder.projection.parameters():
                p.requires_grad = False
            self.encoder.pos_embedding.requires_grad = False
        elif isinstance(self.encoder, OMREncoder) and not isinstance(self.encoder, FineTuneOMREncoder):
            for p in self.encoder.parameters():
                p.requires_grad = False

    def create_omr_encoder_state_dict_from_mae(self, pretrained_mae_state_dict):
        """MAE 'encoder.*' keys -> this encoder's keys; for a FineTuneOMREncoder the first num_layers - fine_tune_depth
        layers go to frozen_blocks and the rest, renumbered from 0, to fine_tune_blocks (M:679-713)."""
        sd = {k[len("encoder."):]: v for k, v in pretrained_mae_state_dict.items() if k.startswith("encoder.")}
        if not isinstance(self.encoder, FineTuneOMREncoder):
            return sd
        thr = self.encoder.num_layers - self.encoder.fine_tune_depth
        out = {}
        for k, v in sd.items():
            m = re.match(r"encoder_blocks\.layers\.(\d+)\.(.*)", k)
            if m:
                n = int(m.group(1))
                if n < thr:
                    out[f"frozen_blocks.layers.{n}.{m.group(2)}"] = v
                else:
                    out[f"fine_tune_blocks.layers.{n - thr}.{m.group(2)}"] = v
            elif k in ("encoder_blocks.norm.weight", "encoder_blocks.norm.bias"):
                out[k.replace("encoder_blocks", "fine_tune_blocks")] = v
            else:
                out[k] = v
        return out

    def forward(self, x):
        """x: list of (image, lmx_sequence) -> pred (B, L_lmxmax, V), target_seqs (B, L_lmxmax) (M:722-736)."""
        imgs, lmx_seqs = zip(*x)
        img_latent, latent_attention_mask = self.encoder(imgs)
        img_latent = self.transition_head(img_latent)
        input_seqs, target_seqs, lmx_attention_mask = batchify_and_split_lmx_seqs(lmx_seqs, self.decoder.pad_idx, img_latent.device)
        pred = self.decoder(input_seqs, img_latent, lmx_attention_mask, latent_attention_mask)
        return pred, target_seqs

    def generate(self, img_latent: torch.Tensor, seqs: torch.Tensor):
        img_latent = img_latent.expand(seqs.shape[0], -1, -1)
        logits = self.decoder.generate(seqs, img_latent)
        return F.log_softmax(logits[:, -1, :].float(), dim=-1)

    def create_fine_tune_param_groups(self, base_lr: float, fine_tune_base_lr: float, fine_tune_decay_factor: float):
        """AdamW parameter groups with layer-wise LR decay over the fine-tuned encoder blocks, last block first (M:761-781)."""
        groups = [{"params": self.decoder.parameters(), "lr": base_lr}, {"params": self.transition_head.parameters(), "lr": base_lr}]
        layer_lrs = []
        for i, layer in enumerate(reversed(self.encoder.fine_tune_blocks.layers)):
            lr = fine_tune_base_lr * (fine_tune_decay_factor ** i)
            groups.append({"params": layer.parameters(), "lr": lr})
            layer_lrs.append(lr)
        groups.append({"params": self.encoder.fine_tune_blocks.norm.parameters(), "lr": fine_tune_base_lr})
        groups.append({"params": (p for p in [self.encoder.pos_embedding]), "lr": layer_lrs[-1]})
        groups.append({"params": self.encoder.projection.parameters(), "lr": layer_lrs[-1]})
        return groups, layer_lrs


class OMRCELoss(nn.Module):
    """Cross entropy over the LMX vocabulary, <pad> targets ignored, mean over the rest (M:784-796)."""

    def __init__(self, pad_idx, label_smoothing=0.0):
        super().__init__()
        self.pad_idx = pad_idx
        self.label_smoothing = label_smoothing

    def forward(self, pred, target_seqs):
        from ..train import autograd_path
        return autograd_path.ce_loss(pred, target_seqs, self.pad_idx, self.label_smoothing)


def _gumbel_softmax(logits, tau, hard, exponential=None):
    """F.gumbel_softmax (torch/nn/functional.py) restated with its exponential draw injectable, in the logits' dtype: -log of the draw, the
    shifted logits and the softmax output are rounded to that dtype as CPU autocast rounds them (bf16 logits), the softmax itself runs in
    fp32.  hard: the straight-through form y_hard - y_soft.detach() + y_soft."""
    dt = logits.dtype
    with torch.autocast(logits.device.type, enabled=False):
        e = torch.empty_like(logits).exponential_() if exponential is None else exponential.to(device=logits.device, dtype=dt)
        g = (-e.float().log()).to(dt) if dt != torch.float32 else -e.log()
        z = (logits + g) / tau
        y = z.float().softmax(-1).to(dt)
        if hard:
            y_hard = torch.zeros_like(y).scatter_(-1, y.argmax(-1, keepdim=True), 1.0)
            y = y_hard - y.detach() + y
    return y


class ScheduledSamplingViTOMR(TeacherForcedViTOMR):
    def sample_and_mix_seqs(self, teacher_forcing_prob, tf_input_seqs, tf_pred_logits, sample_tau, use_hard_sampling, device, noise=None):
        """Mix gold embeddings with expected embeddings of a Gumbel-softmax sample of the first pass (M:801-817).
        Tiny (B,T,227)x(227,E) work; stays in PyTorch-ROCm as SURVEY section 2.2 allows.

        noise (extension, like MAE.forward(noises=)): the two raw draws {"uniform": (B, T) fp32, "exponential": (B, T, V)} in place of
        torch.rand (M:803) and the exponential_ inside F.gumbel_softmax; None draws them from torch's generator.  The sample mask and the
        Gumbel noise are derived from them here, as the reference derives them.  Under autocast the Gumbel-softmax keeps the reference's
        rounding points (CPU autocast, the oracle's "bf16" convention): the draw, the Gumbel sum and the softmax output in the logits' dtype
        (bf16), softmax arithmetic in fp32 - CUDA autocast would run log and softmax in fp32 and return fp32."""
        from ..train import autograd_path as AP
        u = noise["uniform"].to(device) if noise is not None else torch.rand(tf_input_seqs.shape, device=device)
        sample_mask = u < (1 - teacher_forcing_prob)
        dec = self.decoder
        W = dec.vocab_embedding.weight
        B, T = tf_input_seqs.shape
        # nn.Embedding (M:805) as a row gather of the HIP path; the <pad> row is read through a detached copy (padding_idx: it gets no gradient)
        tok = tf_input_seqs.to(device).reshape(-1)
        table = torch.cat([W, W[dec.pad_idx:dec.pad_idx + 1].detach()], 0)
        idx = torch.where(tok == dec.pad_idx, torch.full_like(tok, W.shape[0]), tok).to(torch.int32).contiguous()
        gold = AP.GatherRowsFn.apply(table, idx, None).view(B, T, -1)
        distr = _gumbel_softmax(tf_pred_logits, sample_tau, use_hard_sampling, None if noise is None else noise["exponential"])
        # (B, T, V) x (V, E) (M:809) on the path's own GEMM kernels, forward and both gradients (round 2 left it to ATen / hipBLASLt)
        expected = AP.MatmulKNFn.apply(distr.reshape(B * T, -1), W, AP._prec(), _wc(dec)).view(B, T, -1).to(gold.dtype)
        expected = torch.cat([gold[:, 0:1, :], expected], dim=1)[:, :-1]
        return torch.where(sample_mask.unsqueeze(-1), expected, gold)

    def forward_train(self, x, teacher_forcing_prob: float, sample_tau: float, use_hard_sampling: bool, noise=None):
        """noise: the draws of sample_and_mix_seqs (extension; None = torch's generator)."""
        imgs, lmx_seqs = zip(*x)
        img_latent, latent_attention_mask = self.encoder(imgs)
        img_latent = self.transition_head(img_latent)
        device = img_latent.device
        tf_input_seqs, target_seqs, lmx_attention_mask = batchify_and_split_lmx_seqs(lmx_seqs, self.decoder.pad_idx, device)
        from ..train.autograd_path import shared_cross_kv
        with shared_cross_kv():   # both passes attend to the same latent: its packed form and cross K/V projections are computed once
            tf_pred_logits = self.decoder(tf_input_seqs, img_latent, lmx_attention_mask, latent_attention_mask)
            mixed = self.sample_and_mix_seqs(teacher_forcing_prob, tf_input_seqs, tf_pred_logits, sample_tau, use_hard_sampling, device,
                                             noise=noise)
            pred = self.decoder(mixed, img_latent, lmx_attention_mask, latent_attention_mask, token_idxs_input=False)
        return pred, target_seqs

    def forward_eval(self, x):
        return super().forward(x)
