"""Entry points of acai_omr/inference/vitomr_inference.py:51-86 on the MI355X backend.

Same signatures and return contracts.  The plumbing is the reference's: eval(), no_grad(), encoder OUTSIDE autocast
(fp32), transition head + greedy decode INSIDE autocast(bfloat16) with a bf16 KV cache.  Internally the image latent
stays a packed token stream from the encoder to the decode loop (no pad / unpad round trip)."""
import logging

import torch
from torch.amp import autocast

from ..config import (ENCODER_FINE_TUNE_DEPTH, LMX_VOCAB_PATH, MAX_LMX_SEQ_LEN, NUM_DECODER_LAYERS, PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH,
                      InferenceEvent)
from ..models.models import FineTuneOMREncoder, OMRDecoder, ScheduledSamplingViTOMR, ViTOMR
from .. import page as pg
from ..utils import PackedPatches

logger = logging.getLogger(__name__)


def set_up_omr_inference(lmx_vocab_path=LMX_VOCAB_PATH, max_batch_size=32, cache_dtype=torch.bfloat16, device="cuda", memory_cache_dtype=None):
    """Model construction of omr_teacher_force_train.set_up_omr_inference (:265-284) + the cached-decoder swap of
    vitomr_inference.__main__ (:98).  The torchvision image transform is host preprocessing and out of scope.  memory_cache_dtype
    (extension): torch.float8_e4m3fn keeps the decoder's cross-attention K/V in FP8 (OMRDecoder.to_cached_version)."""
    encoder = FineTuneOMREncoder(PATCH_SIZE, PE_MAX_HEIGHT, PE_MAX_WIDTH, ENCODER_FINE_TUNE_DEPTH)
    decoder = OMRDecoder(MAX_LMX_SEQ_LEN, lmx_vocab_path, num_layers=NUM_DECODER_LAYERS)
    vitomr = ScheduledSamplingViTOMR(encoder, None, decoder)
    vitomr.decoder = vitomr.decoder.to_cached_version(max_batch_size, cache_dtype, memory_cache_dtype)
    return vitomr.to(device), device


def _encode(vitomr, img, prune=None, return_pruned=False):
    # encoder outside autocast, as the reference (its eval fast path is not autocastable, vitomr_inference.py:63)
    with autocast(device_type="cuda", enabled=False):
        if prune is None and not return_pruned:
            return vitomr.encoder.forward_packed(img)
        return vitomr.encoder.forward_packed(img, prune=prune, return_pruned=return_pruned)


def _full_grid(dims, lens, pruned):
    """(the lengths `_check_grids` compares the grids with, the packed kept indices or None): with a pruned memory the grids are the FULL
    grids, not the kept counts, and the maps are expanded to them (ViTOMR._align_packed)."""
    if pruned is None:
        return lens, None
    return [h * w for h, w in dims], pruned.kept


def inference(vitomr: ViTOMR, img, device, max_inference_len=1536, beam_width=1, length_penalty=1.0, speculative=0, ngram=3, prefix=None, *,
              grammar=None, prune=None, prefill=False, loop_guard=None):
    """img: one (1,H,W) tensor or a list of them -> (seqs int64 (B,T'), log_probs fp32 (B,T'), seq_mask bool (B,T')).
    beam_width > 1 (extension): beam search with that many hypotheses per image, scored by cum / len^length_penalty
    (ViTOMR.cached_beam_generate); beam_width = 1 is the reference's greedy decode.
    speculative = D in 1..7 (extension, default 0 = off): greedy decoding that verifies up to D n-gram draft tokens per step
    (ViTOMR.cached_speculative_generate) - the same result in fewer steps where the output repeats itself; needs images * (D + 1) <= the
    cache's max batch size, and cannot be combined with beam_width > 1 or an FP8 memory cache (ValueError).
    prefix (extension, default None = off): prompted decoding - one entry per image with the already known tokens of output indices
    1 .. P_i (ViTOMR.cached_greedy_generate); works with greedy and speculative decoding, not with beam search (ValueError: out of scope
    here).
    grammar (extension, default None = off): a grammar.TokenAutomaton - greedy decoding in which every token is one the automaton allows
    after the tokens before it (ViTOMR.cached_greedy_generate); with beam_width > 1, speculative or prefix it raises ValueError (out of
    scope here).  What a learned automaton does to the output of a trained checkpoint has not been measured.
    prune (an extension, default None = off: the path above, bit for bit, no launch added): True or a `prune.PruneConfig` - the patches that
    are blank paper are dropped from the packed stream before the encoder's projection (prune.prune_patches: three launches and one copy
    of the kept counts to the host per batch), so the encoder, the cross K/V prefill and every decode step see a shorter memory; img may
    also be an already pruned `utils.PackedPatches`.  It combines with every decode mode above and with the FP8 memory cache.  The
    thresholds are chosen on synthetic pages; the blank share of real systems and what dropping paper does to the output of a trained
    checkpoint have not been measured.
    prefill (an extension, default False = off: the paths above, bit for bit, no launch added): prompt prefill of greedy prompted decoding
    (ViTOMR.cached_greedy_generate) - the prompt tokens all images have in one teacher-forced pass instead of one decode step each.  With
    speculative, beam_width > 1, grammar or an FP8 memory cache it raises ValueError (out of scope here).
    loop_guard (an extension, default None = off: the paths above, bit for bit, no launch added): a `loops.LoopGuard` - greedy decoding in
    which a row that fell into a repeat cycle ends at the index where the guard's rule fires (ViTOMR.cached_greedy_generate), found on
    the device inside the replayed graph; the `loops.LoopReport` is appended to the result.  With beam_width > 1, speculative, prefix,
    prefill or grammar it raises ValueError (out of scope here; `loops.scan_repeats` covers their output after the fact).  How often
    trained checkpoints loop, and which thresholds separate a runaway row from a genuine ostinato, has not been measured."""
    _check_loop_guard(loop_guard, beam_width, speculative, prefix, grammar, prefill)
    if grammar is not None:
        for other, on in (("beam search (beam_width > 1)", beam_width != 1), ("speculative decoding (speculative)", bool(speculative)),
                          ("prompted decoding (prefix)", prefix is not None)):
            if on:
                raise ValueError(f"grammar (constrained decoding) cannot be combined with {other}: out of scope here")
    if speculative and beam_width != 1:
        raise ValueError("speculative decoding cannot be combined with beam search (beam_width > 1)")
    if prefix is not None and beam_width != 1:
        raise ValueError("prefix (prompted decoding) cannot be combined with beam search (beam_width > 1): out of scope here")
    _check_prefill(prefill, beam_width, speculative, grammar)
    vitomr.eval()
    with torch.no_grad():
        lat32, _, lens = _encode(vitomr, img, prune)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
            bf = mem.dtype == torch.bfloat16
            if speculative:
                return vitomr._speculative_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, speculative, ngram,
                                                  prefix=prefix)
            if beam_width != 1:
                return vitomr._beam_packed(None if bf else mem, mem if bf else None, lens, beam_width, max_inference_len, length_penalty)
            return vitomr._greedy_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, prefix=prefix, grammar=grammar,
                                         prefill=prefill, loop_guard=loop_guard)


def _check_loop_guard(loop_guard, beam_width=1, speculative=0, prefix=None, grammar=None, prefill=False):
    """loop_guard of the entry points: None or a loops.LoopGuard (TypeError), and none of the modes it cannot be combined with (ValueError
    naming the mode)."""
    from ..loops import check_guard, refuse_guard
    if check_guard(loop_guard) is None:
        return
    for other, on in (("beam search (beam_width > 1)", beam_width != 1), ("speculative decoding (speculative)", bool(speculative)),
                      ("prompted decoding (prefix)", prefix is not None), ("prompt prefill (prefill)", bool(prefill)),
                      ("grammar (constrained decoding)", grammar is not None)):
        if on:
            refuse_guard(loop_guard, other)


def _check_prefill(prefill, beam_width, speculative, grammar):
    """prefill (prompt prefill) belongs to greedy prompted decoding alone: the modes it cannot be combined with, refused by name."""
    if not prefill:
        return
    for other, on in (("speculative decoding (speculative)", bool(speculative)), ("beam search (beam_width > 1)", beam_width != 1),
                      ("grammar (constrained decoding)", grammar is not None)):
        if on:
            raise ValueError(f"prefill (prompt prefill) cannot be combined with {other}: out of scope here")


def _check_decode_kwargs(who, decode_kwargs):
    """The decode arguments that aligned_inference / confident_inference pass on to inference()'s decode, refused as inference() refuses them."""
    unknown = set(decode_kwargs) - {"beam_width", "length_penalty", "speculative", "ngram", "prefix", "grammar", "prefill"}
    if unknown:
        raise TypeError(f"{who}() got unexpected decode arguments {sorted(unknown)}")
    beam_width, speculative = decode_kwargs.get("beam_width", 1), decode_kwargs.get("speculative", 0)
    prefix, grammar = decode_kwargs.get("prefix"), decode_kwargs.get("grammar")
    if grammar is not None:
        for other, on in (("beam search (beam_width > 1)", beam_width != 1), ("speculative decoding (speculative)", bool(speculative)),
                          ("prompted decoding (prefix)", prefix is not None)):
            if on:
                raise ValueError(f"grammar (constrained decoding) cannot be combined with {other}: out of scope here")
    if speculative and beam_width != 1:
        raise ValueError("speculative decoding cannot be combined with beam search (beam_width > 1)")
    if prefix is not None and beam_width != 1:
        raise ValueError("prefix (prompted decoding) cannot be combined with beam search (beam_width > 1): out of scope here")
    _check_prefill(decode_kwargs.get("prefill", False), beam_width, speculative, grammar)


def _decode_packed(vitomr, mem32, memb, lens, max_inference_len, decode_kwargs):
    """inference()'s decode of packed memories with checked decode_kwargs -> (seqs, log_probs, seq_mask)."""
    beam_width, speculative = decode_kwargs.get("beam_width", 1), decode_kwargs.get("speculative", 0)
    prefix, grammar = decode_kwargs.get("prefix"), decode_kwargs.get("grammar")
    if speculative:
        return vitomr._speculative_packed(mem32, memb, lens, max_inference_len, speculative, decode_kwargs.get("ngram", 3), prefix=prefix)
    if beam_width != 1:
        return vitomr._beam_packed(mem32, memb, lens, beam_width, max_inference_len, decode_kwargs.get("length_penalty", 1.0))
    return vitomr._greedy_packed(mem32, memb, lens, max_inference_len, prefix=prefix, grammar=grammar, prefill=decode_kwargs.get("prefill", False))


def aligned_inference(vitomr: ViTOMR, img, device, max_inference_len=1536, layers=None, head_weights=None, return_maps=False, *, prune=None,
                      **decode_kwargs):
    """inference() plus token-to-image alignment (an extension) -> (seqs, log_probs, seq_mask, TokenAlignment).  The images are encoded once;
    the decode is inference()'s own (decode_kwargs - beam_width, length_penalty, speculative, ngram, prefix, grammar, prefill - are passed on, and
    its errors stay its errors); then one teacher-forced pass over the produced tokens on the same packed memory, with the decode's
    positions, writes each token's cross-attention map over the image's patches and reduces it to a location
    (ViTOMR.locate_tokens; the grids come from the image sizes).  layers / head_weights select and weight the decoder layers and heads
    that are averaged (OMRDecoder.cross_attention_maps_packed; default all, uniform): which of them align best on trained checkpoints has
    not been measured.  return_maps keeps the per-token maps in the result.  prune: as in inference(); the alignment still speaks of the
    FULL patch grid - `patch` indexes it, centroids and spreads are pixels of the input, `maps[i]` is (L_i - 1, h_p * w_p) with zeros at the
    dropped patches (ops.attn_map_expand)."""
    _check_decode_kwargs("aligned_inference", decode_kwargs)
    vitomr.decoder._alignment_selection(layers, head_weights)
    vitomr.eval()
    with torch.no_grad():
        dims = list(img.dims) if hasattr(img, "dims") else [vitomr.encoder._grid(t) for t in img]
        lat32, _, lens, pruned = _encode(vitomr, img, prune, True)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
            bf = mem.dtype == torch.bfloat16
            mem32, memb = (None, mem) if bf else (mem, None)
            seqs, lps, mask = _decode_packed(vitomr, mem32, memb, lens, max_inference_len, decode_kwargs)
            full, kept = _full_grid(dims, lens, pruned)
            grids = vitomr._check_grids(dims, full)
            align = vitomr._align_packed(mem32, memb, lens, seqs, mask, layers, head_weights, True, grids, vitomr.encoder.patch_size, return_maps,
                                         kept=kept)
    return seqs, lps, mask, align


def confident_inference(vitomr: ViTOMR, img, device, max_inference_len=1536, top_k=5, temperature=1.0, uncertainty=None, layers=None,
                        head_weights=None, *, prune=None, **decode_kwargs):
    """inference() plus per-token confidence (an extension) -> (seqs, log_probs, seq_mask, TokenConfidence).  The images are encoded once
    and the decode is inference()'s own (decode_kwargs as in aligned_inference; its errors stay its errors); then one teacher-forced pass
    over the produced tokens on the same packed memory, with the decode's positions, scores every token under softmax(logits / temperature):
    log-probability, entropy, rank and the top_k best tokens (ViTOMR.token_confidence).  uncertainty=None runs the logits-only pass;
    "entropy", "surprisal" or "error" runs the combined pass instead, which also writes the tokens' cross-attention maps (layers /
    head_weights as in aligned_inference), and fills TokenConfidence.uncertainty - a heat map per image over its patch grid, the maps summed
    with that per-token weight (ViTOMR.uncertainty_maps) - and TokenConfidence.alignment, what aligned_inference returns.  After a
    grammar-constrained decode the scores are the unconstrained model's: rank > 0 marks a token the grammar forced.  How well the scores
    mark real errors on trained checkpoints has not been measured.  prune: as in inference(); heat maps and alignment cover the FULL patch
    grid, as in aligned_inference."""
    _check_decode_kwargs("confident_inference", decode_kwargs)
    vitomr._check_confidence_args(top_k, temperature)
    if uncertainty is not None:
        if not isinstance(uncertainty, str):
            raise ValueError(f"uncertainty must be None or a weight name, got {type(uncertainty).__name__}")
        vitomr._check_uncertainty_weight(uncertainty, None)
        vitomr.decoder._alignment_selection(layers, head_weights)
    vitomr.eval()
    with torch.no_grad():
        dims = list(img.dims) if hasattr(img, "dims") else [vitomr.encoder._grid(t) for t in img]
        lat32, _, lens, pruned = _encode(vitomr, img, prune, True)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
            bf = mem.dtype == torch.bfloat16
            mem32, memb = (None, mem) if bf else (mem, None)
            seqs, lps, mask = _decode_packed(vitomr, mem32, memb, lens, max_inference_len, decode_kwargs)
            full, kept = _full_grid(dims, lens, pruned)
            grids = vitomr._check_grids(dims, full) if uncertainty is not None else None
            conf = vitomr._confidence_packed(mem32, memb, lens, seqs, mask, top_k, temperature, True, uncertainty, layers, head_weights, grids,
                                             vitomr.encoder.patch_size, uncertainty is not None, kept=kept)
    return seqs, lps, mask, conf


def diagnosed_inference(vitomr: ViTOMR, img, target_lmx_seqs, device, max_inference_len=1536, *, prune=None, **decode_kwargs):
    """inference() scored against the ground truth (an extension) -> (seqs, log_probs, seq_mask, TokenConfidence, EditAlignment).  The
    images are encoded once and the decode is inference()'s own (decode_kwargs as in aligned_inference; its errors stay its errors); the
    decoded rows are then aligned to target_lmx_seqs - a list of 1-D token tensors, one per image, written as the decode writes its rows
    (<bos> first, <eos> last) - on the device (ops.edit_alignment), and one teacher-forced pass on the same packed memory gives the
    per-token confidence and, in TokenConfidence.uncertainty, the page heat map of the tokens that are wrong (ViTOMR.error_maps): a
    substituted or inserted token weighs 1 where it stands, a missing one 1 at the output position where it should have been emitted.
    TokenConfidence.alignment locates every token.  EditAlignment.pred_op != 0 are the error labels utils.confidence_error_auroc takes.
    prune: as in inference(); the error map and the alignment cover the FULL patch grid, as in aligned_inference."""
    _check_decode_kwargs("diagnosed_inference", decode_kwargs)
    vitomr.eval()
    with torch.no_grad():
        dims = list(img.dims) if hasattr(img, "dims") else [vitomr.encoder._grid(t) for t in img]
        lat32, _, lens, pruned = _encode(vitomr, img, prune, True)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
            bf = mem.dtype == torch.bfloat16
            mem32, memb = (None, mem) if bf else (mem, None)
            seqs, lps, mask = _decode_packed(vitomr, mem32, memb, lens, max_inference_len, decode_kwargs)
            full, kept = _full_grid(dims, lens, pruned)
            grids = vitomr._check_grids(dims, full)
            al, w = vitomr._error_weights(seqs, mask, target_lmx_seqs, None)
            conf = vitomr._confidence_packed(mem32, memb, lens, seqs, mask, 5, 1.0, True, w, None, None, grids, vitomr.encoder.patch_size, True,
                                             kept=kept)
    return seqs, lps, mask, conf, al


def measured_inference(vitomr: ViTOMR, img, device, max_inference_len=1536, measures=None, target_lmx_seqs=None, *, prune=None, **decode_kwargs):
    """inference() plus per-MEASURE results (an extension) -> (seqs, log_probs, seq_mask, TokenConfidence, measures.MeasureReport).  The first
    four are bit for bit what confident_inference(uncertainty="entropy") returns for the same arguments: the images are encoded once, the
    decode is inference()'s own (decode_kwargs as in aligned_inference; its errors stay its errors), and the combined pass on the same packed
    memory scores every token and writes the cross-attention maps.  Inside that pass the rows are cut at the delimiter tokens of `measures`
    (a measures.MeasureConfig; None: the default, every `measure` token) and confidence, location, box and - with target_lmx_seqs, written
    as diagnosed_inference takes them - the edit errors are reduced per measure on the device (ViTOMR.measure_report).  MeasureConfig.return_maps
    also keeps the per-token maps in TokenConfidence.alignment.maps (views of the pass's buffer, no copy).  prune: as in inference(); boxes
    and maps cover the FULL patch grid.  Whether cross-attention localises measures on trained checkpoints has not been measured."""
    from ..measures import MeasureConfig, report_hook
    _check_decode_kwargs("measured_inference", decode_kwargs)
    config = MeasureConfig() if measures is None else measures
    if not isinstance(config, MeasureConfig):
        raise TypeError(f"measures must be a measures.MeasureConfig or None, got {type(config).__name__}")
    config.resolve(vitomr.decoder)
    vitomr.eval()
    with torch.no_grad():
        dims = list(img.dims) if hasattr(img, "dims") else [vitomr.encoder._grid(t) for t in img]
        lat32, _, lens, pruned = _encode(vitomr, img, prune, True)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mem = vitomr.transition_head.forward_packed(lat32)
            bf = mem.dtype == torch.bfloat16
            mem32, memb = (None, mem) if bf else (mem, None)
            seqs, lps, mask = _decode_packed(vitomr, mem32, memb, lens, max_inference_len, decode_kwargs)
            full, kept = _full_grid(dims, lens, pruned)
            grids = vitomr._check_grids(dims, full)
            config.resolve(vitomr.decoder, seqs.shape)
            hook = report_hook(config, None if target_lmx_seqs is None else vitomr._error_weights(seqs, mask, target_lmx_seqs, None)[0])
            conf = vitomr._confidence_packed(mem32, memb, lens, seqs, mask, 5, 1.0, True, "entropy", None, None, grids, vitomr.encoder.patch_size,
                                             True, kept=kept, measure=hook, return_maps=config.return_maps)
    return seqs, lps, mask, conf, hook.report


def _encode_chunks(vitomr, imgs, device, prune=None):
    """Encoder (fp32, outside autocast) and transition head (inside autocast) over chunks of at most max_batch_size images; the packed
    memories of all chunks, concatenated, and their lengths.  imgs: a list of image tensors, or a `utils.PackedPatches`.  prune: as in
    inference() - a `PackedPatches` is pruned whole, once (three launches for all chunks), image lists chunk by chunk."""
    chunk = vitomr.decoder.decoder_blocks.max_batch_size if hasattr(vitomr.decoder.decoder_blocks, "max_batch_size") else len(imgs)
    if prune is not None and prune is not False and isinstance(imgs, PackedPatches) and not imgs.pruned:
        imgs, prune = vitomr.encoder.prune_packed(imgs, None if prune is True else prune), None
    mems, lens = [], []
    for c0 in range(0, len(imgs), chunk):
        lat32, _, ln = _encode(vitomr, imgs.slice(c0, c0 + chunk) if isinstance(imgs, PackedPatches) else imgs[c0:c0 + chunk], prune)
        with autocast(device_type=device, dtype=torch.bfloat16):
            mems.append(vitomr.transition_head.forward_packed(lat32))
        lens += ln
    return (mems[0] if len(mems) == 1 else torch.cat(mems)), lens


def iter_continuous_inference(vitomr: ViTOMR, imgs, device, max_inference_len=1536, slots=None, prefix=None, *, grammar=None, prune=None,
                              loop_guard=None):
    """Continuous-batching greedy inference (an extension) as a generator: yields (index, seqs (1,T'), log_probs (1,T'), mask (1,T')) for
    each image as soon as it finishes, in completion order; each is what inference(vitomr, [imgs[index]]) returns.  max_inference_len: one
    cap or a list of per-image caps; slots: decode rows (default: the cache's max batch size).  prefix (prompted decoding, inference())
    is not supported here: anything but None raises ValueError.  grammar: constrained decoding as in inference().  prune: blank-patch
    pruning as in inference(); imgs may then also be a `utils.PackedPatches`, pruned or not.  loop_guard: loop detection as in inference()
    (not with grammar) - an image that loops frees its row where the rule fires, and each tuple ends with the image's `loops.LoopReport`."""
    vitomr._no_prefix(prefix, "continuous batching")
    _check_loop_guard(loop_guard, grammar=grammar)
    vitomr.eval()
    imgs = imgs if isinstance(imgs, PackedPatches) else list(imgs)
    with torch.no_grad():
        mem, lens = _encode_chunks(vitomr, imgs, device, prune)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            run = vitomr._continuous_packed_iter(None if bf else mem, mem if bf else None, lens, max_inference_len, slots, grammar=grammar,
                                                 loop_guard=loop_guard)

    def images():
        with torch.no_grad():
            yield from run
    return images()


def continuous_inference(vitomr: ViTOMR, imgs, device, max_inference_len=1536, slots=None, prefix=None, *, grammar=None, prune=None,
                         loop_guard=None):
    """inference() over a list of any length through continuous batching (an extension): `slots` decode rows work through the images in
    input order and a finished row is refilled with the next image at once.  Returns exactly what inference(vitomr, imgs, ...) returns
    (seqs (N,T'), log_probs (N,T'), mask (N,T'), clipped to the longest row); max_inference_len may be a list of per-image caps.  prefix
    (prompted decoding, inference()) is not supported here: anything but None raises ValueError.  grammar: constrained decoding as in
    inference().  prune: blank-patch pruning as in inference(); imgs may then also be a `utils.PackedPatches`, pruned or not.
    loop_guard: loop detection as in inference() (not with grammar) - a looping image frees its row where the rule fires instead of
    holding it to its cap, and the `loops.LoopReport` over the N images is appended to the result."""
    vitomr._no_prefix(prefix, "continuous batching")
    _check_loop_guard(loop_guard, grammar=grammar)
    vitomr.eval()
    imgs = imgs if isinstance(imgs, PackedPatches) else list(imgs)
    kw = {} if loop_guard is None else {"loop_guard": loop_guard}
    with torch.no_grad():
        mem, lens = _encode_chunks(vitomr, imgs, device, prune)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            return vitomr._continuous_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, slots, grammar=grammar, **kw)


def page_inference(vitomr: ViTOMR, pages, device, resize, boxes=None, max_inference_len=1536, slots=None, detect=None, *, assess=None, prune=None, grammar=None, loop_guard=None, orient=None, deskew=None, flatten=None, rectify=None):
    """Whole pages in, their systems decoded as one batch (an extension; the reference's service crops hand-drawn boxes with PIL and decodes
    them one by one, acai_omr/ui/routes.py:93-129) -> a `page.PageResult`.
    pages: one (H,W) / (1,H,W) tensor or a list of them, uint8 or float in [0, 1]; a decoded colour photo, uint8 (H, W, 3), (H, W, 4) or
    (3, H, W), is made grey first (page.ingest_pages; float colour input is a TypeError).  boxes: None - the systems are found on the device (page.detect_systems with the
    `page.DetectConfig` detect, which assumes roughly level staff lines) - or, per page, a list of pixel boxes (x0, y0, x1, y1) or of the
    UI's fraction boxes (page.pixel_boxes); for one page the list may be given bare.  Boxes and quads a caller supplies refer to the page
    as the stages before detection leave it: UPRIGHT, rectified, levelled.  resize: the `utils.DynamicResize` every box goes through.
    All systems of all pages are cut out and resized into one packed patch stream by one launch pair (page.split_pages), encoded in chunks
    of the cache's batch size and decoded by continuous batching: the rows are what continuous_inference returns for the resized crops, in
    page order and top to bottom.  max_inference_len, slots, grammar, loop_guard: as in continuous_inference; with a loop guard the
    result's `loops` is the `loops.LoopReport` over the systems.  A page without systems contributes no
    rows; with no system at all nothing is encoded or decoded and the result is empty.

    The stages, every one an extension that is off at None or False (the path above, unchanged: no launch added, no copy made), in the
    order they run.  True: the stage estimates what it needs on the device with its default config; a config: with that one.  Every
    keyword is checked before anything is uploaded (page.resolve_stage): anything not listed is a TypeError, a code outside 1 .. 8 a
    ValueError.  The function named last says what the stage does, what it costs and what it does not handle.

      order  keyword  besides None / False / True             adds to the result                               documented at
      1      orient   page.OrientConfig; one EXIF code        orientations, source_sizes; the maps back reach  page.ingest_pages,
                      1 .. 8, or a list with one per page     the photo's own pixels                           page.estimate_orientation
      2      rectify  page.RectifyConfig; one quad [TL, TR,   quads, source_sizes, inset; page_sizes is the    page.rectify_pages,
                      BR, BL], or a list of quads or None     size of the rectified pages                      page.find_page_quad
      3      flatten  page.FlattenConfig                      flattened (geometry does not change)             page.flatten_pages
      4      deskew   page.SkewConfig; one angle in degrees,  angles; boxes are in the levelled pages          page.deskew_pages,
                      or a list with one per page                                                              page.estimate_skew
      5      assess   page.AssessConfig                       quality, system_staff_space; with boxes=None     page.assess_pages,
                                                              detection is sized from the staff scale          page.DetectConfig.resolved
      6      prune    prune.PruneConfig                       patches_kept below patches_total                 prune.prune_patches

    Stages 1 - 4 are page.prepare_pages, so the order is ingest -> rectify -> flatten -> deskew -> detect; 5 measures the pages detection sees and never drops a row; 6 acts on the packed patches of all
    systems at once.  `PageResult.to_page_xy` / `from_page_xy` / `box_corners` go back through 4, 2 and 1 to the pages as they were passed
    in.  orient=True gives, bit for bit, what orient=<the estimated codes> gives.  The defaults of every config were chosen on synthetic
    pages and not measured on real photographs (there are none in this repository)."""
    _check_loop_guard(loop_guard, grammar=grammar)
    pages, per_page, plans, specials, extra, prune = _page_front(vitomr, pages, resize, boxes, detect, assess, prune, orient, deskew, flatten, rectify)
    system_page, sizes, windows = [p for p, *_ in plans], [s for _, _, s, _ in plans], [c for *_, c in plans]
    if not plans:
        return pg.PageResult(per_page, None, None, None, [], [], [], specials, **extra)
    vitomr.eval()
    kw = {} if loop_guard is None else {"loop_guard": loop_guard}
    with torch.no_grad():
        packed, total, mem, lens = _page_encode(vitomr, pages, per_page, resize, prune, device)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            seqs, lps, mask, *loops = vitomr._continuous_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, slots,
                                                                grammar=grammar, **kw)
    extra = dict(extra, loops=loops[0]) if loops else extra
    return pg.PageResult(per_page, seqs, lps, mask, system_page, sizes, windows, specials, patches_kept=packed.lens, patches_total=total, **extra)


def _page_front(vitomr, pages, resize, boxes, detect, assess, prune, orient, deskew, flatten, rectify):
    """page_inference up to the split, shared with streamed_page_inference: the keyword checks, the page stages, assessment, detection (or
    the caller's boxes) and the crop plans -> (pages as detection saw them, per-page boxes, plans, the special token ids, PageResult's
    stage keywords, the resolved prune config)."""
    from ..prune import as_config
    prune, (assess, _) = as_config(prune), pg.resolve_stage("assess", assess)
    pages, boxes = pg.page_lists(pages, boxes)
    pages, prepared = pg.prepare_pages(pages, resize.device, orient=orient, rectify=rectify, flatten=flatten, deskew=deskew)
    extra, scales = dict(vars(prepared)), None
    if assess is not None and pages:
        measured = pg.assess_counts(pages, assess)          # the launches and the one copy; the gate waits for the systems' sizes
        scales = [pg.choose_staff_scale(hists, assess) for hists, _, _ in measured]
    if boxes is None:
        per_page = [pg.detect_systems(p, detect) if scales is None or scales[i] is None else pg.detect_systems(p, detect, scales[i].pitch_bin)
                    for i, p in enumerate(pages)]
    else:
        per_page = [pg.pixel_boxes(b, *p.shape) for p, b in zip(pages, boxes)]
    plans = pg.plan_systems([tuple(p.shape) for p in pages], per_page, resize)
    specials = [getattr(vitomr.decoder, n) for n in ("bos_idx", "eos_idx", "pad_idx") if hasattr(vitomr.decoder, n)]
    if scales is not None:
        spaces = pg.system_staff_spaces(scales, plans)
        smallest = [min((v for v, (p, *_) in zip(spaces, plans) if p == i and v is not None), default=None) for i in range(len(pages))]
        extra.update(quality=[pg.page_quality(*m, assess, small) for m, small in zip(measured, smallest)], system_staff_space=spaces)
    return pages, per_page, plans, specials, extra, prune


def _page_encode(vitomr, pages, per_page, resize, prune, device):
    """All systems of all pages cut out and resized into one packed patch stream, pruned when asked, and encoded in chunks -> (the packed
    patches, the patch counts before pruning, the packed memories, their lengths).  The caller holds no_grad."""
    packed = pg.split_pages(pages, per_page, resize)
    total = packed.lens
    if prune is not None:
        packed = vitomr.encoder.prune_packed(packed, prune)
    mem, lens = _encode_chunks(vitomr, packed, device)
    return packed, total, mem, lens


def streamed_continuous_inference(vitomr: ViTOMR, imgs, device, max_inference_len=1536, slots=None, flush_interval=25, *, grammar=None, prune=None):
    """continuous_inference as a generator of {"type", "payload"} events (an extension: the reference's service streams one image at a time,
    acai_omr/ui/routes.py) - every image's tokens while they are decoded, with continuous batching kept.  imgs: a list of image tensors or
    a `utils.PackedPatches`; max_inference_len, slots, grammar, prune: as in continuous_inference.  The events, in order:
      ENCODING_START        None
      ENCODING_FINISH       {"images": N}, after the chunked encode
      STEP                  {"image": i, "start": t0, "tokens": int32 (1, n), "log_probs": fp32 (1, n)}, CPU tensors: the row's indices
                            t0 .. t0 + n - 1; per poll (every flush_interval decode steps, sooner at a cap) one for each image being decoded
      INFERENCE_FINISH      {"image": i, "sequence", "log_probs", "mask"}: what iter_continuous_inference yields for i; after its last STEP
      ALL_INFERENCE_FINISH  None
    An image's STEP events tile its row from index 1 through its last token (ViTOMR.streamed_continuous_generate).  The GPU decodes the
    next flush_interval steps while the caller consumes a poll's events.  A prefix is not offered, as in continuous batching.
    flush_interval: an int in [1, the cache's max sequence length] - anything else is a ValueError, raised at the call like grammar's
    TypeError; what the decode itself refuses (slots, caps) is raised when the decode starts."""
    vitomr._check_grammar(grammar)
    vitomr._check_flush_interval(flush_interval)
    imgs = imgs if isinstance(imgs, PackedPatches) else list(imgs)

    def events():
        vitomr.eval()
        yield {"type": InferenceEvent.ENCODING_START.value, "payload": None}
        with torch.no_grad():
            mem, lens = _encode_chunks(vitomr, imgs, device, prune)
            bf = mem.dtype == torch.bfloat16
            yield {"type": InferenceEvent.ENCODING_FINISH.value, "payload": {"images": len(lens)}}
            with autocast(device_type=device, dtype=torch.bfloat16):
                run = vitomr._streamed_continuous_packed_iter(None if bf else mem, mem if bf else None, lens, max_inference_len, slots,
                                                              flush_interval, grammar=grammar)
            yield from run
        yield {"type": InferenceEvent.ALL_INFERENCE_FINISH.value, "payload": None}
    return events()


def streamed_page_inference(vitomr: ViTOMR, pages, device, resize, boxes=None, max_inference_len=1536, slots=None, detect=None, flush_interval=25, *, assess=None, prune=None, grammar=None, orient=None, deskew=None, flatten=None, rectify=None):
    """page_inference as a generator of {"type", "payload"} events (an extension): the systems of whole pages, decoded by continuous batching,
    token by token as they come.  Every argument but flush_interval is page_inference's and is checked as there, at the call: the keyword
    checks and flush_interval (an int in [1, the cache's max sequence length], else ValueError) before anything is uploaded, then the page
    stages and detection run at the call as well, so that what they refuse is raised there.  The events, in order:
      ENCODING_START        None: the stages and detection are done, the split is about to start
      SYSTEMS_FOUND         {"layout": PageResult} with the geometry and the stage reports but no rows yet (seqs None): boxes, angles, quads,
                            orientations, quality, sizes, windows, to_page_xy, box_corners ... all work - for a UI to draw the boxes while the
                            encoder runs
      ENCODING_FINISH       {"images": N}, N the systems of all pages
      STEP                  streamed_continuous_inference's payload plus "page" and "system": the row's page and its index within that page
      INFERENCE_FINISH      likewise, {"image", "sequence", "log_probs", "mask", "page", "system"}
      ALL_INFERENCE_FINISH  {"result": PageResult}, equal to page_inference's on the same arguments
    A page set without systems yields ENCODING_START, SYSTEMS_FOUND and ALL_INFERENCE_FINISH with the empty result; nothing is encoded."""
    vitomr._check_grammar(grammar)
    vitomr._check_flush_interval(flush_interval)
    pages, per_page, plans, specials, extra, prune = _page_front(vitomr, pages, resize, boxes, detect, assess, prune, orient, deskew, flatten, rectify)
    system_page, sizes, windows = [p for p, *_ in plans], [s for _, _, s, _ in plans], [c for *_, c in plans]
    tags = [{"page": p, "system": system_page[:i].count(p)} for i, p in enumerate(system_page)]

    def events():
        yield {"type": InferenceEvent.ENCODING_START.value, "payload": None}
        layout = pg.PageResult(per_page, None, None, None, system_page, sizes, windows, specials, **extra)
        yield {"type": InferenceEvent.SYSTEMS_FOUND.value, "payload": {"layout": layout}}
        if not plans:
            yield {"type": InferenceEvent.ALL_INFERENCE_FINISH.value, "payload": {"result": pg.PageResult(per_page, None, None, None, [], [], [], specials, **extra)}}
            return
        vitomr.eval()
        with torch.no_grad():
            packed, total, mem, lens = _page_encode(vitomr, pages, per_page, resize, prune, device)
            bf = mem.dtype == torch.bfloat16
            yield {"type": InferenceEvent.ENCODING_FINISH.value, "payload": {"images": len(lens)}}
            with autocast(device_type=device, dtype=torch.bfloat16):
                run = vitomr._streamed_continuous_packed_iter(None if bf else mem, mem if bf else None, lens, max_inference_len, slots,
                                                              flush_interval, grammar=grammar, tags=tags)
            seqs, lps, mask = yield from run
        result = pg.PageResult(per_page, seqs, lps, mask, system_page, sizes, windows, specials, patches_kept=packed.lens, patches_total=total, **extra)
        yield {"type": InferenceEvent.ALL_INFERENCE_FINISH.value, "payload": {"result": result}}
    return events()


def streamed_inference(img, vitomr: ViTOMR, device, max_inference_len=1536, flush_interval=25, prefix=None, *, grammar=None, prefill=False):
    """prefix (extension, default None = off): prompted decoding of the one image, as in inference(); the forced tokens arrive in the
    STEP events like any others.  grammar (extension, default None = off): constrained decoding as in inference(), not with prefix.
    prefill (extension, default False = off): prompt prefill as in inference(); not with grammar."""
    vitomr.eval()
    with torch.no_grad():
        yield {"type": InferenceEvent.ENCODING_START.value, "payload": None}
        img_latent, latent_attention_mask = vitomr.encoder(img)
        with autocast(device_type=device, dtype=torch.bfloat16):
            img_latent = vitomr.transition_head(img_latent)
            yield {"type": InferenceEvent.ENCODING_FINISH.value, "payload": None}
            for event in vitomr.streamed_cached_greedy_generate(img_latent, latent_attention_mask, max_len=max_inference_len,
                                                                flush_interval=flush_interval, prefix=prefix, grammar=grammar,
                                                                prefill=prefill):
                yield event
