"""ctypes binding of the C-ABI shared library (include/acai_omr_hip.h).

The product path has NO CPU fallback: if `libacai_omr_hip.so` is missing or a symbol is absent, importing
the ops raises, loudly.  `build()` compiles the library in-tree for gfx950 with hipcc (cross-compiles
without a GPU); the built .so is git-ignored but travels to the GPU box with the source tree.
"""
import ctypes
import os
import subprocess
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p, c_size_t

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("ACAI_OMR_LIB") or os.path.join(CSRC, "libacai_omr_hip.so")   # (override: A/B builds of the same sources, tools/ab_*.sh)
SOURCES = ["gemm.hip", "gemm_tile.hip", "gemm_ring.hip", "gemm_pp.hip", "elementwise.hip", "attn.hip", "attn_varlen.hip", "attn_probs.hip", "confidence.hip", "measures.hip", "attn_fwd64.hip", "attn_fwd64w.hip", "attn_bwd.hip", "attn_bwd64w.hip", "attn_bwd1p.hip", "train.hip", "grpo.hip", "seqdist.hip", "seqalign.hip", "grammar.hip", "loops.hip", "decode.hip", "decode_gemv.hip", "decode_attn.hip", "decode_select.hip", "decode_prefill.hip", "resize.hip", "augment.hip", "page.hip", "deskew.hip", "flatten.hip", "rectify.hip", "ingest.hip", "prune.hip", "assess.hip"]

ACAI_F32, ACAI_BF16, ACAI_FP8_E4M3 = 0, 1, 2
GEMM_GELU, GEMM_ROUND_BF16 = 1, 2
# AcaiGemmLaunch.kernel (ACAI_GEMM_K_*) and .pp_mode (ACAI_PP_*): what acai_gemm_plan / acai_gemm_last_plan report
(GEMM_K_REG, GEMM_K_GLDS, GEMM_K_GLDS3, GEMM_K_PERS, GEMM_K_256, GEMM_K_PERS256, GEMM_K_PP, GEMM_K_TN_GLDS, GEMM_K_TN_RING,
 GEMM_K_TN_PP) = range(10)
GEMM_KERNEL_NAMES = ("gemm_nt_kernel", "gemm_nt_glds_kernel", "gemm_nt_glds3_kernel", "gemm_nt_pers_kernel", "gemm_nt_256_kernel",
                     "gemm_nt_pers256_kernel", "gemm_nt_pp_kernel", "gemm_tn_glds_kernel", "gemm_tn_ring_kernel", "gemm_tn_pp_kernel")
GEMM_PP_OBF, GEMM_PP_GELU, GEMM_PP_AUX1, GEMM_PP_AUX2, GEMM_PP_RES, GEMM_PP_SCALE, GEMM_PP_DEFER, GEMM_PP_AUX3, GEMM_PP_AUX4 = 1, 2, 4, 8, 16, 32, 64, 128, 256
DEC_CROSS_FP8 = 256   # AcaiDecoder.flags: e4m3fn cross K/V with per-row scales (AcaiDecLayer.k_cross_scale / v_cross_scale)


class AcaiDecLayer(Structure):
    _fields_ = [(n, c_void_p) for n in (
        "self_in_w", "self_in_b", "self_out_w", "self_out_b", "cross_q_w", "cross_q_b", "cross_out_w", "cross_out_b",
        "lin1_w", "lin1_b", "lin2_w", "lin2_b", "n1_w", "n1_b", "n2_w", "n2_b", "n3_w", "n3_b",
        "k_self", "v_self", "k_cross", "v_cross", "k_cross_scale", "v_cross_scale")]


class AcaiGemmQuery(Structure):
    _fields_ = [(n, c_int) for n in (
        "elem_size", "epi", "trans_a", "trans_w", "M", "N", "K", "lda", "ldw", "ldc", "ldr", "ldaux",
        "a_aligned", "w_aligned", "c_aligned", "r_aligned", "aux_aligned", "out_dtype", "flags", "aux_mode",
        "has_residual", "scale_cols", "want_colsum", "variant", "n_cu")]


class AcaiGemmLaunch(Structure):
    _fields_ = [(n, c_int) for n in ("kernel", "wm", "fast", "pp_mode", "grid", "block", "ksplit", "vec_epi", "row0", "rows", "k0", "k", "colsum")]


def gemm_last_plan():
    """The launches of the calling thread's most recent GEMM entry call (acai_gemm_last_plan), as a list of AcaiGemmLaunch."""
    out, n = (AcaiGemmLaunch * 2)(), c_int(0)
    check(lib().acai_gemm_last_plan(out, ctypes.byref(n)), "acai_gemm_last_plan")
    return [out[i] for i in range(n.value)]


def gemm_last_kernels():
    """gemm_last_plan() as kernel names with the template form that was chosen: "gemm_nt_glds_kernel<wm=2>", "gemm_nt_kernel<fast=0>",
    "gemm_nt_pp_kernel<mode=33>" (GEMM_PP_* bits); the other kernels by name alone.  What the GPU tests assert after a call."""
    form = {GEMM_K_GLDS: lambda l: f"<wm={l.wm}>", GEMM_K_REG: lambda l: f"<fast={l.fast}>", GEMM_K_PP: lambda l: f"<mode={l.pp_mode}>"}
    return [GEMM_KERNEL_NAMES[l.kernel] + form.get(l.kernel, lambda l: "")(l) for l in gemm_last_plan()]


# AcaiAttnLaunch.kernel (ACAI_ATTN_K_*), the overrides of acai_attn_set_override (ACAI_ATTN_OV_*: default, lowest, highest value) and the
# values of ATTN_OV_FWD64 (ACAI_ATTN_FWD64_*)
(ATTN_K_FWD, ATTN_K_FWD64, ATTN_K_FWD64W, ATTN_K_FWD64_TAIL, ATTN_K_BWD_DQ, ATTN_K_BWD_DKV, ATTN_K_BWD_DQ2, ATTN_K_BWD_DKV2, ATTN_K_BWD64W_DQ,
 ATTN_K_BWD64W_DKV, ATTN_K_BWD1P) = range(11)
ATTN_KERNEL_NAMES = ("attn_fwd_kernel", "attn_fwd64_kernel", "attn_fwd64w_kernel", "attn_fwd64_tail_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel",
                     "attn_bwd_dq2_kernel", "attn_bwd_dkv2_kernel", "attn_bwd64w_dq_kernel", "attn_bwd64w_dkv_kernel", "attn_bwd1p_kernel")
ATTN_OV_TWO_BLOCK, ATTN_OV_FWD64, ATTN_OV_BWD64_WIDE, ATTN_OV_BWD_1P, ATTN_OV_XCD_ORDER, ATTN_OV_COUNT = range(6)
ATTN_OV_RANGE = ((1, 0, 1), (0, 0, 3), (-1, -1, 3), (1, 0, 1), (-1, -1, 1))
ATTN_FWD64_AUTO, ATTN_FWD64_NW4, ATTN_FWD64_NW8, ATTN_FWD64_GENERIC = range(4)
ATTN_REFUSE_PRESCALED, ATTN_REFUSE_ACCUM = 1, 2


class AcaiAttnQuery(Structure):
    _fields_ = [(n, c_int) for n in (
        "backward", "elem_size", "B", "H", "dh", "max_q", "max_k", "total_q", "total_k", "causal", "accum_dkv", "dropout", "q_prescaled",
        "ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv", "aligned", "cu_k_is_cu_q")] + [("ov", c_int * ATTN_OV_COUNT), ("workspace_bytes", c_int64)]


class AcaiAttnLaunch(Structure):
    _fields_ = [(n, c_int) for n in ("kernel", "elem_size", "dhp", "fast", "drop", "pre", "nq", "waves", "grid_x", "grid_y", "grid_z", "block", "lds_bytes",
                                     "tail", "tail256", "nblk", "partial_blocks", "equal_len", "rows")]


def attn_last_plan():
    """The launches of the calling thread's most recent acai_attn_varlen_fwd / _bwd[_ws] call (acai_attn_last_plan), as a list of AcaiAttnLaunch."""
    out, n = (AcaiAttnLaunch * 4)(), c_int(0)
    check(lib().acai_attn_last_plan(out, ctypes.byref(n)), "acai_attn_last_plan")
    return [out[i] for i in range(n.value)]


def attn_kernel_name(l):
    """An AcaiAttnLaunch as its kernel's name with the template form that was chosen: "attn_fwd_kernel<bf16,32,fast=1,drop=0,pre=1,nq=2>",
    "attn_bwd_dq_kernel<fp32,64,fast=0,drop=0,pre=0>", "attn_fwd64_kernel<8>"; the other kernels by name alone.  What the GPU tests assert."""
    name = ATTN_KERNEL_NAMES[l.kernel]
    if l.kernel in (ATTN_K_FWD, ATTN_K_BWD_DQ, ATTN_K_BWD_DKV):
        name += f"<{'bf16' if l.elem_size == 2 else 'fp32'},{l.dhp},fast={l.fast},drop={l.drop},pre={l.pre}" + (f",nq={l.nq}>" if l.kernel == ATTN_K_FWD else ">")
    elif l.kernel == ATTN_K_FWD64:
        name += f"<{l.waves}>"
    return name


def attn_last_kernels():
    return [attn_kernel_name(l) for l in attn_last_plan()]


class AcaiAdamWTensor(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n", c_int64), ("group", c_int32), ("pad_", c_int32),
                ("bias_c1", c_float), ("bias_c2_sqrt", c_float)]


GRAD_NORM_TOTAL, GRAD_NORM_COEF, GRAD_NORM_FINITE, GRAD_NORM_WORDS = 0, 1, 2, 4   # the result block of acai_grad_norm (ACAI_GRAD_NORM_*)


class AcaiCastEntry(Structure):
    _fields_ = [("src", c_void_p), ("dst16", c_void_p), ("dst16t", c_void_p), ("dst32r", c_void_p), ("rows", c_int32), ("cols", c_int32),
                ("tile0", c_int32), ("pad_", c_int32)]


class AcaiAdamWGroup(Structure):
    _fields_ = [(n, c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "pad0_", "pad1_", "pad2_")]


class AcaiDecoder(Structure):
    _fields_ = [(n, c_int32) for n in (
        "B", "E", "H", "dh", "dhp", "F", "V", "L", "Tmax", "dtype", "flags", "max_len",
        "self_chunk", "cross_chunk", "self_nsplit", "cross_nsplit", "bos", "pad", "eos", "cross_group")] + [
        ("layers", POINTER(AcaiDecLayer))] + [(n, c_void_p) for n in (
            "emb", "pos", "fn_w", "fn_b", "unembed_w", "unembed_b", "cross_off", "cross_len", "seqs", "logprobs",
            "step", "finished", "x", "xn", "qkv", "attn", "proj", "hid", "logits", "partial", "tickets", "stats")]


class AcaiBeam(Structure):
    _fields_ = [("K", c_int32), ("pitch", c_int32), ("rows", c_int32), ("pad_", c_int32)] + [
        (n, c_void_p) for n in ("anc", "tok", "lp", "cum", "len")]


class AcaiSlots(Structure):
    _fields_ = [(n, c_void_p) for n in ("t", "first", "cap")] + [("rows", c_int32), ("pad_", c_int32)]


class AcaiSpec(Structure):
    _fields_ = [(n, c_int32) for n in ("D", "ngram", "pitch", "rows")] + [(n, c_void_p) for n in ("t", "cap", "steps", "tab", "next", "drafts")]


class AcaiPrompt(Structure):
    _fields_ = [("tok", c_void_p), ("len", c_void_p), ("pitch", c_int32), ("rows", c_int32)]


class AcaiGrammar(Structure):
    _fields_ = [("next", c_void_p), ("resync", c_void_p), ("state", c_void_p)] + [(n, c_int32) for n in ("states", "start", "rows", "pad_")]


class AcaiLoop(Structure):
    _fields_ = [(n, c_void_p) for n in ("run", "stop", "period", "start")] + [(n, c_int32) for n in ("rows", "max_period", "min_repeats", "min_tokens")]


AUG_MAX_TAPS, AUG_MEAN_PARTS = 32, 128
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_BRIGHTNESS_FIRST = 1, 2, 4   # AcaiAugImage.jitter


class AcaiAugImage(Structure):
    _fields_ = [("src", c_void_p), ("buf", c_void_p * 2), ("noise", c_void_p), ("out", c_void_p), ("partials", c_void_p),
                ("rot_cos", c_double), ("rot_sin", c_double), ("persp", c_double * 8)] + [
        (n, c_int32) for n in ("H", "W", "apply", "jitter", "ktaps", "row0")] + [
        (n, c_float) for n in ("noise_sigma", "fb", "fc", "pad_")] + [("w", c_float * AUG_MAX_TAPS)]


PAGE_LANE_PIXELS, PAGE_WAVES, PAGE_MAX_W, PAGE_MAX_H = 4, 4, 16384, 65535   # acai_page_profile's layout (ACAI_PAGE_*): 4 pixels per lane, 4 waves per row


# csrc/deskew.hip (ACAI_STRIP_* / ACAI_SKEW_*): the strip kernel's tile (rows, 16-byte units), the row differences per workgroup of the score
# kernel, the size of a slope table and the largest slope, round(tan(15 deg) * 65536).  The strip profile is uint8 [nS][H].
STRIP_TILE_ROWS, STRIP_TILE_UNITS, SKEW_CHUNK, SKEW_MAX_SLOPES, SKEW_MAX_SLOPE = 64, 32, 1023, 1024, 17560
STRIP_WIDTHS = (8, 16, 32, 64)
FLATTEN_TILES = (16, 32, 64, 128)   # csrc/flatten.hip: the tile sizes of acai_page_tile_levels / acai_page_flatten
EXTENTS_MAX_RUN = 256               # csrc/rectify.hip (ACAI_EXTENTS_MAX_RUN): the longest run acai_page_extents can be asked for
COL_CHUNK_ROWS, COL_MAX_CHUNKS = 64, 64   # csrc/ingest.hip (ACAI_COL_*): acai_page_col_profile walks chunks of max(64, ceil(H / 64)) rows
# csrc/assess.hip (ACAI_RUNS_CHUNK_ROWS, ACAI_SHARP_CHUNK_ROWS): the rows a wave of acai_page_runs / acai_page_sharpness walks; the words of their outputs
RUNS_CHUNK_ROWS, SHARP_CHUNK_ROWS, RUNS_WORDS, SHARP_WORDS = 32, 32, 3 * 256, 3 + 256


# csrc/prune.hip (ACAI_PRUNE_*): the columns of the device table, the largest halo, grid (patches of one image) and number of images
PRUNE_TABLE_COLS, PRUNE_MAX_HALO, PRUNE_MAX_GRID, PRUNE_MAX_IMAGES = 8, 3, 1 << 20, 65535


def col_chunks(H):
    """(rows per chunk, chunks) of acai_page_col_profile for a page of H rows: its `work` holds 4 * chunks * W int32."""
    rows = max(COL_CHUNK_ROWS, -(-int(H) // COL_MAX_CHUNKS))
    return rows, -(-int(H) // rows)


class AcaiCropResize(Structure):
    _fields_ = [("page", c_void_p), ("tmp_off", c_int64)] + [
        (n, c_int32) for n in ("page_h", "page_w", "pitch", "in_u8", "x0", "y0", "w", "h", "OH", "OW", "top", "left", "ch", "cw", "row0", "pad_")]


_SIGNATURES = {
    "acai_version": (c_int, []),
    "acai_last_error": (c_char_p, []),
    "acai_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "acai_gemm_nt": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_int, c_void_p]),
    "acai_gemm_nt_ex": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "acai_gemm_set_variant": (c_int, [c_int]),
    "acai_gemm_plan": (c_int, [POINTER(AcaiGemmQuery), POINTER(AcaiGemmLaunch), POINTER(c_int)]),
    "acai_gemm_last_plan": (c_int, [POINTER(AcaiGemmLaunch), POINTER(c_int)]),
    "acai_gemm": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                          c_int, c_int, c_int, c_void_p]),
    "acai_cross_kv_prefill": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "acai_patchify": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_resize_bicubic_aa": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_resize_to_patches": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_void_p]),
    "acai_augment_blur_noise": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "acai_augment_warp": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "acai_augment_jitter_out": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_page_profile": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "acai_page_systems": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p]),
    "acai_crop_resize_to_patches": (c_int, [c_void_p, POINTER(AcaiCropResize), c_int, c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int,
                                            c_void_p]),
    "acai_page_strips": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    "acai_page_skew_scores": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, POINTER(c_int32), c_int, c_void_p, c_void_p]),
    "acai_page_rotate": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p]),
    "acai_page_tile_levels": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "acai_page_flatten": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "acai_page_extents": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    "acai_page_warp": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int64), c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_page_ingest": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_int, c_void_p]),
    "acai_page_col_profile": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acai_page_box_ink": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "acai_page_runs": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "acai_page_sharpness": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "acai_patch_ink": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_float, c_void_p, c_void_p]),
    "acai_patch_keep": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "acai_patch_compact": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_attn_map_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_gather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "acai_attn_varlen_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_float, c_uint32, c_int, c_void_p]),
    "acai_attn_probs_mean": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                     c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "acai_attn_map_locate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "acai_token_confidence": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_attn_map_weighted_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p,
                                           c_void_p]),
    "acai_token_segments": (c_int, [c_void_p, c_int, c_void_p, c_int, POINTER(c_int64), c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "acai_segment_reduce": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "acai_attn_map_segment_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p]),
    "acai_attn_map_extent": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_float, c_void_p, c_void_p]),
    "acai_attn_varlen_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_int, c_float, c_uint32, c_int, c_void_p]),
    "acai_attn_varlen_bwd_ws": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                        c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_int, c_int, c_int, c_float, c_uint32, c_int, c_void_p, c_size_t, c_void_p]),
    "acai_attn_varlen_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int]),
    "acai_attn_plan": (c_int, [POINTER(AcaiAttnQuery), POINTER(AcaiAttnLaunch), POINTER(c_int), POINTER(c_int)]),
    "acai_attn_last_plan": (c_int, [POINTER(AcaiAttnLaunch), POINTER(c_int)]),
    "acai_attn_set_override": (c_int, [c_int, c_int]),
    "acai_attn_get_override": (c_int, [c_int, POINTER(c_int)]),
    "acai_dropout_add": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_uint32, c_int, c_int, c_void_p]),
    "acai_layernorm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "acai_gelu_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "acai_gelu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "acai_adamw_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "acai_grad_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_adamw_step_clipped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "acai_cast_weights": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "acai_gemm_dw": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "acai_colsum": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_scatter_add_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "acai_mae_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "acai_ce_loss": (c_int, [c_void_p, c_int, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "acai_grpo_objective_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float,
                                        c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_grpo_objective_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                        c_void_p, c_void_p]),
    "acai_edit_distance": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "acai_edit_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "acai_edit_align": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "acai_debug_stamps": (c_int, [c_void_p, c_int]),
    "acai_debug_lds_dma_oob": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "acai_debug_lane_xor": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "acai_pe_interp_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "acai_pe_interp_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "acai_cast_f32_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "acai_skinny_gemm": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                 c_int, c_int, c_void_p]),
    "acai_skinny_gemm_ex": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_decode_attn": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "acai_decode_attn_fp8": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "acai_debug_decode_self_attn": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p,
                                            c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p]),
    "acai_debug_decode_attn_group": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                             c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "acai_debug_decode_select": (c_int, [c_int, POINTER(AcaiDecoder), POINTER(AcaiSlots), POINTER(AcaiGrammar), POINTER(AcaiPrompt), POINTER(AcaiBeam),
                                         c_void_p, c_int, c_void_p, c_int, c_float, c_int, c_void_p]),
    "acai_debug_decode_spec_accept": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSpec), POINTER(AcaiPrompt), c_int, c_void_p]),
    "acai_cross_kv_quantize_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "acai_decode_embed": (c_int, [POINTER(AcaiDecoder), c_void_p]),
    "acai_decode_step": (c_int, [POINTER(AcaiDecoder), c_void_p]),
    "acai_decode_sample_step": (c_int, [POINTER(AcaiDecoder), c_void_p, c_int, c_float, c_void_p]),
    "acai_decode_beam_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiBeam), c_void_p]),
    "acai_decode_slot_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), c_void_p]),
    "acai_decode_slot_sample_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), c_void_p, c_int, c_void_p, c_int, c_float,
                                             c_void_p]),
    "acai_decode_slot_arm": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), c_void_p, c_int, c_void_p]),
    "acai_decode_slot_flush": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "acai_decode_spec_arm": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSpec), c_void_p]),
    "acai_decode_spec_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSpec), c_void_p]),
    "acai_decode_prompt_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiPrompt), c_void_p]),
    "acai_decode_spec_prompt_arm": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSpec), POINTER(AcaiPrompt), c_void_p]),
    "acai_decode_spec_prompt_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSpec), POINTER(AcaiPrompt), c_void_p]),
    "acai_decode_prefill_self_kv": (c_int, [POINTER(AcaiDecoder), c_int, c_void_p, c_int, c_int, c_void_p]),
    "acai_decode_prefill_arm": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiPrompt), c_void_p, c_int, c_void_p]),
    "acai_decode_grammar_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiGrammar), c_void_p]),
    "acai_decode_grammar_sample_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiGrammar), c_void_p, c_int, c_float, c_void_p]),
    "acai_decode_slot_grammar_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), POINTER(AcaiGrammar), c_void_p]),
    "acai_decode_slot_grammar_sample_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), POINTER(AcaiGrammar), c_void_p, c_int, c_void_p,
                                                     c_int, c_float, c_void_p]),
    "acai_grammar_scan": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "acai_decode_loop_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiLoop), c_void_p]),
    "acai_decode_slot_loop_step": (c_int, [POINTER(AcaiDecoder), POINTER(AcaiSlots), POINTER(AcaiLoop), c_void_p]),
    "acai_debug_decode_loop_select": (c_int, [c_int, POINTER(AcaiDecoder), POINTER(AcaiSlots), POINTER(AcaiLoop), c_int, c_void_p]),
    "acai_repeat_scan": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acai_decode_logits": (c_int, [POINTER(AcaiDecoder), c_void_p, c_int, c_void_p]),
    "acai_decode_hidden": (c_int, [POINTER(AcaiDecoder), c_void_p, c_void_p]),
    "acai_decode_merge_in_launch": (c_int, [c_int, c_int]),
    "acai_graph_begin": (c_int, [c_void_p]),
    "acai_graph_end": (c_int, [c_void_p, POINTER(c_void_p)]),
    "acai_graph_launch": (c_int, [c_void_p, c_void_p]),
    "acai_graph_destroy": (c_int, [c_void_p]),
}

_lib = None


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 over csrc/*.hip -> csrc/libacai_omr_hip.so (in-tree).  One object per source (rebuilt only when the
    source or a shared header is newer), compiled in parallel, then one link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(os.path.dirname(CSRC), "..", "include", "acai_omr_hip.h")]
    hipcc = "hipcc" if subprocess.run(["which", "hipcc"], capture_output=True).returncode == 0 else "/opt/rocm/bin/hipcc"
    flags = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-value"]
    # The attention kernels are bound by VALU issue, and the SLP vectoriser pairs their per-score multiplies into v_pk_mul_f32, which costs
    # more issue time than the two v_mul_f32 it replaces (PMC: +24 % VALU instructions without it, -9 % wave cycles).
    per_file = {"attn_varlen.hip": ["-fno-slp-vectorize"], "attn_fwd64.hip": ["-fno-slp-vectorize"],
                # (one wave per SIMD: the score MFMAs must write VGPRs, the output accumulators are asm-owned AGPRs - see the file header)
                "attn_fwd64w.hip": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"], "attn_bwd.hip": ["-fno-slp-vectorize"],
                "attn_bwd64w.hip": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"],
                "attn_bwd1p.hip": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]}
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)

    def stale(out, deps):
        return force or not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps)

    # Sources whose correctness rests on something the compiler does not model (asm loads it cannot see, a counted LDS wait): their generated
    # assembly is checked on every rebuild and a hit FAILS the build (acai_omr_amd/_asmcheck.py; ADVICE r3: the check used to be a manual tool).
    asm_checks = {"gemm_pp.hip": ["check_untracked_loads"], "attn_fwd64w.hip": ["check_fwd64w_barrier", "check_asm_mfma_operands"],
                  "attn_bwd64w.hip": ["check_asm_mfma_operands"], "attn_bwd1p.hip": ["check_asm_mfma_operands"]}
    jobs, to_check = [], []
    for src in srcs:
        base = os.path.basename(src)
        obj = os.path.join(objdir, base + ".o")
        asm = os.path.join(objdir, base + ".s")
        rebuilt = stale(obj, [src] + hdrs)
        if rebuilt:
            jobs.append([hipcc] + flags + per_file.get(base, []) + ["-c", src, "-o", obj])
        if base in asm_checks and (rebuilt or stale(asm, [src] + hdrs)):
            jobs.append([hipcc] + flags + per_file.get(base, []) + ["--cuda-device-only", "-S", src, "-o", asm])
            to_check.append((base, asm))
    if verbose:
        for j in jobs:
            print(" ".join(j))
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), 16, max(1, (os.cpu_count() or 2) // 2))) as ex:
            for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
                if r.returncode != 0:
                    raise RuntimeError(f"hipcc failed: {' '.join(r.args)}\n{r.stdout}\n{r.stderr}")
    from . import _asmcheck
    for base, asm in to_check:
        problems = []
        for chk in asm_checks[base]:
            pr, n = getattr(_asmcheck, chk)(open(asm).read())
            problems += pr
            if verbose:
                print(f"asm check {base} ({chk}): {n} sites, {len(pr)} problems")
        if problems:
            os.remove(asm)   # (so that the next build checks again instead of trusting a stale pass)
            raise RuntimeError(f"generated code of {base} violates an assumption the kernel relies on:\n" + "\n".join(problems))
    objs = [os.path.join(objdir, os.path.basename(src) + ".o") for src in srcs]
    if jobs or stale(LIB_PATH, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return LIB_PATH


def lib():
    """Load (once) and type the C-ABI library.  Raises if it is missing: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"acai_omr_amd: HIP extension {LIB_PATH} is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                           "there is no CPU fallback for the product path")
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7, the same soname
    # /opt/rocm's carries).  Load torch's copy first so that our NEEDED entry resolves to it; loading ours first would
    # pull in /opt/rocm's runtime and torch would later add a second one (streams / events are not shared between them).
    import torch
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if L.acai_version() != 1:
        raise RuntimeError("acai_omr_amd: ABI version mismatch")
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {lib().acai_last_error().decode()}")


def exported_symbols():
    return list(_SIGNATURES)
