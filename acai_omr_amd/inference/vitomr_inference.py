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
              grammar=None, prune=None, prefill=False):
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
    speculative, beam_width > 1, grammar or an FP8 memory cache it raises ValueError (out of scope here)."""
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
                                         prefill=prefill)


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


def iter_continuous_inference(vitomr: ViTOMR, imgs, device, max_inference_len=1536, slots=None, prefix=None, *, grammar=None, prune=None):
    """Continuous-batching greedy inference (an extension) as a generator: yields (index, seqs (1,T'), log_probs (1,T'), mask (1,T')) for
    each image as soon as it finishes, in completion order; each is what inference(vitomr, [imgs[index]]) returns.  max_inference_len: one
    cap or a list of per-image caps; slots: decode rows (default: the cache's max batch size).  prefix (prompted decoding, inference())
    is not supported here: anything but None raises ValueError.  grammar: constrained decoding as in inference().  prune: blank-patch
    pruning as in inference(); imgs may then also be a `utils.PackedPatches`, pruned or not."""
    vitomr._no_prefix(prefix, "continuous batching")
    vitomr.eval()
    imgs = imgs if isinstance(imgs, PackedPatches) else list(imgs)
    with torch.no_grad():
        mem, lens = _encode_chunks(vitomr, imgs, device, prune)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            run = vitomr._continuous_packed_iter(None if bf else mem, mem if bf else None, lens, max_inference_len, slots, grammar=grammar)

    def images():
        with torch.no_grad():
            yield from run
    return images()


def continuous_inference(vitomr: ViTOMR, imgs, device, max_inference_len=1536, slots=None, prefix=None, *, grammar=None, prune=None):
    """inference() over a list of any length through continuous batching (an extension): `slots` decode rows work through the images in
    input order and a finished row is refilled with the next image at once.  Returns exactly what inference(vitomr, imgs, ...) returns
    (seqs (N,T'), log_probs (N,T'), mask (N,T'), clipped to the longest row); max_inference_len may be a list of per-image caps.  prefix
    (prompted decoding, inference()) is not supported here: anything but None raises ValueError.  grammar: constrained decoding as in
    inference().  prune: blank-patch pruning as in inference(); imgs may then also be a `utils.PackedPatches`, pruned or not."""
    vitomr._no_prefix(prefix, "continuous batching")
    vitomr.eval()
    imgs = imgs if isinstance(imgs, PackedPatches) else list(imgs)
    with torch.no_grad():
        mem, lens = _encode_chunks(vitomr, imgs, device, prune)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            return vitomr._continuous_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, slots, grammar=grammar)


def page_inference(vitomr: ViTOMR, pages, device, resize, boxes=None, max_inference_len=1536, slots=None, detect=None, *, assess=None, prune=None, grammar=None, orient=None, deskew=None, flatten=None, rectify=None):
    """Whole pages in, their systems decoded as one batch (an extension; the reference's service crops hand-drawn boxes with PIL and decodes
    them one by one, acai_omr/ui/routes.py:93-129) -> a `page.PageResult`.
    pages: one (H,W) / (1,H,W) tensor or a list of them, uint8 or float in [0, 1].  boxes: None - the systems are found on the device
    (page.detect_systems with the `page.DetectConfig` detect; it assumes roughly level staff lines, and how well it does on real scans has
    not been measured) - or, per page, a list of pixel boxes (x0, y0, x1, y1) or of the UI's fraction boxes (dicts, or tuples holding
    floats: page.boxes_from_fractions); for one page the list may be given bare.  resize: the `utils.DynamicResize` every box goes through.
    All systems of all pages are cut out and resized into one packed patch stream by one launch pair (page.split_pages), encoded in chunks
    of the cache's batch size and decoded by continuous batching: the rows are what continuous_inference returns for the resized crops, in
    page order and top to bottom.  max_inference_len, slots, grammar: as in continuous_inference.  A page without systems contributes no
    rows; with no system at all nothing is launched and the result is empty.
    deskew (an extension, default None = off: the path above, unchanged): True or a `page.SkewConfig` - every page's skew is estimated on
    the device (page.estimate_skew) - or one angle in degrees, or a list with one per page.  The pages are turned level before the
    detection (page.deskew_pages); detection then runs on the levelled pages, and boxes the caller supplies refer to the LEVELLED pages too
    (pixels of, or fractions of, the page after the turn, which has the size of the page before it).  The result's boxes are in the levelled
    pages, its `angles` says by how much each was turned, and `to_page_xy` / `box_corners` lead back to the pages as they were passed in.
    flatten (an extension, default None = off, as is False: the path above, unchanged, no launch added): True or a `page.FlattenConfig` -
    the uneven illumination of every page is divided out before deskew (page.flatten_pages, two launches per page, no copy to the host);
    deskew (if asked for), detection and the crops the model reads all see the flattened pages.  Geometry does not change: boxes, angles and
    the maps back to the page are what they are without it.  The result's `flattened` says which pages were.  Chosen on synthetic shading;
    not measured on real photographs.
    rectify (an extension, default None = off, as is False: the path above, unchanged, no launch added, no copy made): True or a
    `page.RectifyConfig` - the outline of the sheet is found in every page (page.find_page_quad: two launches and one copy to the host per
    page) - or the corners themselves, one quad [TL, TR, BR, BL] of (x, y) for all pages or a list with one quad or None per page (a UI
    lets its user tap them).  The sheet is warped flat FIRST (page.rectify_pages, one launch per page): the order is rectify -> flatten
    -> deskew -> detect, so that flatten and deskew see the sheet and not the table around it.  A page in which no sheet is found, or
    which the sheet fills, is left as it is.  Boxes the caller supplies refer to the RECTIFIED page, and then the levelled one.  The
    result's `quads` and `source_sizes` say what was cut from what, `page_sizes` is the size of the rectified pages, and `to_page_xy` /
    `from_page_xy` / `box_corners` go the whole way back to the pages as they were passed in.  Not handled: page curl, a sheet lighter
    than its surroundings or cut off by the frame on more than one side.  Chosen on synthetic quadrilaterals over a noise table; not
    measured on real photographs.
    orient (an extension, default None = off, as is False: with single-channel pages the path above, unchanged, no launch added): colour
    input and EXIF / quarter-turn orientation.  A page may then also be a decoded colour photo, uint8 (H, W, 3), (H, W, 4) or (3, H, W)
    (page.ingest_pages says how shapes are read) - also with orient=None, where it is only made grey - and orient is the photo's EXIF
    orientation code 1 .. 8, one for all pages or a list with one per page (anything PIL's `ImageOps.exif_transpose` would apply), or
    True or a `page.OrientConfig`: the tag is missing, and one of the codes 1, 3, 6, 8 is estimated per photo on the device
    (page.estimate_orientation: sideways from row against column profiles, upside down from the ink at the two ends of the systems - a
    heuristic chosen on synthetic pages, not measured on real photographs; the EXIF code remains the primary path).  The photo is uploaded
    as it is and ONE launch per photo makes the grey, upright page (page.ingest_pages) before everything else: the order is ingest ->
    rectify -> flatten -> deskew -> detect.  The estimate is a function of the photo alone: it is made on a temporary that went through
    rectify (when the outline is to be found) and flatten if those were asked for, the photo is then ingested with that code and the path
    above runs, so orient=True gives, bit for bit, what orient=<the estimated codes> gives.  Boxes and quads the caller supplies refer
    to the UPRIGHT page.  The result's `orientations` says which code every page was turned by, `source_sizes` is the size of the photos
    as passed in, and `to_page_xy` / `from_page_xy` / `box_corners` go back through the turn to the photo's own pixels.  Anything else for
    orient is a TypeError, a code outside 1 .. 8 a ValueError.  Not handled: float colour input, mirrored photos without a tag, reading
    the tag out of a file (PIL or any decoder gives the number), JPEG decoding, folding the quarter turn into the rectification warp.
    prune (an extension, default None = off, as is False: the path above, unchanged, no launch added): True or a `prune.PruneConfig` - the
    blank patches of all systems are dropped from the packed stream at once (prune.prune_patches: three launches and one copy of the kept
    counts to the host for the whole call) before it is encoded; the rows are then what continuous_inference returns for the pruned stream.
    The result's `patches_kept` / `patches_total` say per system how many patches the model read.  Chosen on synthetic pages; the blank
    share of real systems and the effect on a trained checkpoint's output have not been measured.
    assess (an extension, default None = off, as is False: the path above, unchanged, no launch added, no copy made): True or a
    `page.AssessConfig` - every page is assessed (page.assess_pages: three launches per page and ONE copy to the host for all pages) on
    the page detection sees, that is after ingest, rectify, flatten and deskew where those are on; flatten comes first so that one ink
    threshold holds for the whole page.  The result's `quality` holds per page its `page.PageQuality`: the staff scale (line thickness and
    the distance from staff line to staff line, from vertical run lengths), sharpness, contrast, focus.  Where the scale was found and
    boxes is None, detection is sized from it - `detect.resolved(H, W, staff_space=scale.pitch_bin)`: the fields of `detect` left at None
    come from 180 staff spaces in place of the page height, the fields the caller set win as before - so a dense page of small staves,
    a half-empty page or a sheet that fills half the frame keeps its systems; a page in engraved A4 proportion resolves to what it
    resolved to anyway.  `system_staff_space` gives per system the staff space in MODEL pixels.  A page that fails a bound the caller set
    in the `AssessConfig` (all default to None) has `quality[i].ok` False and the reasons in words, and is decoded all the same: this call
    reports and never drops rows - refusing the photo is the caller's to do, with the reasons in hand.  Rectify and deskew resample
    bilinearly, which lowers `sharpness` a little, and flatten stretches the levels: values compare only under the same stage settings,
    and `page.assess_pages` on the raw page judges the photo itself.  Not handled: sizing flatten, deskew or rectify from the scale
    (they run before it can be measured), horizontal runs, a scale per system, any default threshold; nothing has been measured on real
    photographs."""
    from .. import page as pg
    from ..prune import as_config
    prune = as_config(prune)
    if assess is not None and assess is not False and assess is not True and not isinstance(assess, pg.AssessConfig):
        raise TypeError("assess: expected None, a bool or a page.AssessConfig")
    assess = None if assess is None or assess is False else (pg.AssessConfig() if assess is True else assess)
    pages, boxes = pg._page_lists(pages, boxes)
    if boxes is not None and len(boxes) != len(pages):
        raise ValueError(f"{len(pages)} pages but boxes for {len(boxes)}")
    oriented = {}
    if orient is None or orient is False:
        pages = pg.ingest_pages(pages, None, device=resize.device)      # (single-channel pages: `pg._device_page` of each, nothing else)
    else:
        estimate = orient is True or isinstance(orient, pg.OrientConfig)
        if not estimate and (isinstance(orient, bool) or not isinstance(orient, (int, list, tuple))):
            raise TypeError("orient: expected None, a bool, a page.OrientConfig, one EXIF orientation code 1 .. 8 or a list with one per page")
        codes = None if estimate else pg.orientation_codes(orient, len(pages))
        photos = [pg._device_photo(p, resize.device) for p in pages]
        if estimate:
            codes = []
            for tmp in pg.ingest_pages(photos):
                if rectify is True or isinstance(rectify, pg.RectifyConfig):
                    tmp = pg.rectify_pages(tmp, None, rectify if isinstance(rectify, pg.RectifyConfig) else None)[0][0]
                if flatten is True or isinstance(flatten, pg.FlattenConfig):
                    tmp = pg.flatten_pages(tmp, None if flatten is True else flatten)[0]
                codes.append(pg.estimate_orientation(tmp, orient if isinstance(orient, pg.OrientConfig) else None)[0])
        oriented = dict(orientations=codes, source_sizes=[pg.photo_size(p) for p in photos])
        pages = pg.ingest_pages(photos, codes)
    angles, flattened, rectified = None, None, {}
    if rectify is not None and rectify is not False:
        find = rectify is True or isinstance(rectify, pg.RectifyConfig)
        if not find and not (pg._is_quad(rectify) or (isinstance(rectify, (list, tuple)) and all(q is None or pg._is_quad(q) for q in rectify))):
            raise TypeError("rectify: expected None, a bool, a page.RectifyConfig, one quad [TL, TR, BR, BL] or a list of quads (or None) per page")
        cfg = rectify if isinstance(rectify, pg.RectifyConfig) else pg.RectifyConfig()
        source_sizes = [tuple(p.shape) for p in pages]
        pages, quads = pg.rectify_pages(pages, None if find else rectify, cfg)
        rectified = dict(quads=quads, source_sizes=source_sizes, inset=cfg.inset)
    if flatten is not None and flatten is not False:
        if flatten is not True and not isinstance(flatten, pg.FlattenConfig):
            raise TypeError("flatten: expected None, a bool or a page.FlattenConfig")
        pages = pg.flatten_pages(pages, None if flatten is True else flatten)
        flattened = [True] * len(pages)
    if deskew is not None and deskew is not False:
        estimate = deskew is True or isinstance(deskew, pg.SkewConfig)
        pages, angles = pg.deskew_pages(pages, None if estimate else deskew, deskew if isinstance(deskew, pg.SkewConfig) else None)
    turned = dict(angles=angles, page_sizes=[tuple(p.shape) for p in pages], flattened=flattened, **{**rectified, **oriented})
    scales = None
    if assess is not None and pages:
        measured = pg.assess_counts(pages, assess)          # the launches and the one copy; the gate waits for the systems' sizes
        scales = [pg.choose_staff_scale(hists, assess) for hists, _, _ in measured]
    if boxes is None:
        per_page = [pg.detect_systems(p, detect) if scales is None or scales[i] is None else pg.detect_systems(p, detect, scales[i].pitch_bin)
                    for i, p in enumerate(pages)]
    else:
        per_page = [pg.boxes_from_fractions(b, *p.shape) if b and pg._is_fraction_box(b[0]) else [pg._pixel_box(x, *p.shape) for x in b]
                    for p, b in zip(pages, boxes)]
    plans = pg.plan_systems([tuple(p.shape) for p in pages], per_page, resize)
    system_page, sizes, windows = [p for p, *_ in plans], [s for _, _, s, _ in plans], [c for *_, c in plans]
    dec = vitomr.decoder
    specials = [getattr(dec, n) for n in ("bos_idx", "eos_idx", "pad_idx") if hasattr(dec, n)]
    if scales is not None:
        spaces = pg.system_staff_spaces(scales, plans)
        smallest = [min((v for v, (p, *_) in zip(spaces, plans) if p == i and v is not None), default=None) for i in range(len(pages))]
        turned.update(quality=[pg.page_quality(*m, assess, small) for m, small in zip(measured, smallest)], system_staff_space=spaces)
    if not plans:
        return pg.PageResult(per_page, None, None, None, [], [], [], specials, **turned)
    vitomr.eval()
    with torch.no_grad():
        packed = pg.split_pages(pages, per_page, resize)
        total = packed.lens
        if prune is not None:
            packed = vitomr.encoder.prune_packed(packed, prune)
        mem, lens = _encode_chunks(vitomr, packed, device)
        bf = mem.dtype == torch.bfloat16
        with autocast(device_type=device, dtype=torch.bfloat16):
            seqs, lps, mask = vitomr._continuous_packed(None if bf else mem, mem if bf else None, lens, max_inference_len, slots, grammar=grammar)
    return pg.PageResult(per_page, seqs, lps, mask, system_page, sizes, windows, specials, patches_kept=packed.lens, patches_total=total, **turned)


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
