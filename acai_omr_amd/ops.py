"""Thin tensor-level wrappers over the C ABI (include/acai_omr_hip.h).

PyTorch is plumbing here: it owns device memory and the current stream; every FLOP of the path runs in
the HIP library.  Every wrapper checks device / dtype / contiguity on the host before the launch (a
faulting kernel can take the whole node down) and raises RuntimeError on a non-zero return code.
"""
import contextlib
import ctypes
import functools
import itertools

import math
from typing import NamedTuple

import torch

from . import _lib
from ._lib import ACAI_BF16, ACAI_F32, GEMM_GELU, GEMM_ROUND_BF16  # noqa: F401


def _st(t=None):
    """Raw handle of torch's current stream on `t`'s device (the current device when t is None).  Every public wrapper below runs under
    `_on_operand_device`, which makes the operands' device current first, so both forms name the same stream."""
    return torch.cuda.current_stream(t.device if t is not None else None).cuda_stream


def _on_operand_device(fn):
    """Launch on the OPERANDS' device: a model on cuda:N while another device is current (set_up_omr_inference(device="cuda:1"), a DP rank
    that never called set_device) would otherwise get device 0's stream against device-N pointers - a memory fault without peer access.
    Mixed-device operands are refused."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        idx = -1
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if idx < 0:
                    idx = a.device.index
                elif a.device.index != idx:
                    raise RuntimeError(f"{fn.__name__}: operands on different GPUs (cuda:{idx} and {a.device})")
        if idx >= 0 and idx != torch.cuda.current_device():
            with torch.cuda.device(idx):
                return fn(*args, **kw)
        return fn(*args, **kw)
    return wrapped


def _dt(t):
    if t.dtype == torch.bfloat16:
        return ACAI_BF16
    if t.dtype == torch.float32:
        return ACAI_F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _chk(t, name, dtype=None, rows_contig=True):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the product path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if rows_contig and t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: last dim must be contiguous")
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    """Row stride of a 2-D tensor whose last dim is contiguous; a single-row tensor reports an arbitrary stride(0)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def layernorm(x, w, b, eps, want_f32=True, want_bf16=False, out_f32=None):
    _chk(x, "x", torch.float32)
    assert x.is_contiguous() and x.dim() == 2
    rows, dim = x.shape
    y32 = (out_f32 if out_f32 is not None else torch.empty_like(x)) if want_f32 else None
    y16 = torch.empty(rows, dim, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    assert w.numel() == dim and b.numel() == dim and w.dtype == torch.float32 and b.dtype == torch.float32
    if rows == 0:       # an empty tensor's data_ptr() is null, which the C entry point refuses before it looks at rows
        return y32, y16
    _lib.check(_lib.lib().acai_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), float(eps), _p(y32), _p(y16), rows, dim, _st()),
               "acai_layernorm_fwd")
    return y32, y16


def gemm_nt(a, w, bias=None, residual=None, out_dtype=torch.float32, gelu=False, round_bf16=False, out=None, pre_act=None, gelu_grad_of=None,
            col_scale=None, gelu_grad_out=None, times=None):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias) (+ residual).  a, w share a dtype (fp32 or bf16); 2-D, row stride free.
    pre_act (with gelu): [M,N] tensor of out's dtype that receives the pre-activation; gelu_grad_of: [M,N] saved pre-activation whose GELU
    derivative multiplies the (rounded) product; gelu_grad_out (with gelu): [M,N] tensor that receives gelu'(pre-activation) instead (the
    forward epilogue holds Phi(-|a|) anyway) and times: [M,N] saved tensor that multiplies the (rounded) product - together the MLP's backward
    epilogue is one multiply per element; col_scale = (n, s): columns [0, n) of (a @ w^T + bias) are multiplied by s before rounding
    (the in-projection hands q to the attention kernels as q * log2(e) / sqrt(dh), see attn_varlen(q_prescaled=True))."""
    _chk(a, "a"), _chk(w, "w")
    assert a.dim() == 2 and w.dim() == 2 and a.dtype == w.dtype and a.shape[1] == w.shape[1], (a.shape, w.shape, a.dtype, w.dtype)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == (M, N) and residual.stride(1) == 1
    flags = (GEMM_GELU if gelu else 0) | (GEMM_ROUND_BF16 if round_bf16 else 0)
    given = [(m, t) for m, t in ((1, pre_act), (2, gelu_grad_of), (3, gelu_grad_out), (4, times)) if t is not None]
    assert len(given) <= 1, "one auxiliary operand per launch"
    aux = given[0][1] if given else None
    if aux is not None or col_scale is not None:
        mode = 0
        if aux is not None:
            mode = given[0][0]
            assert aux.shape == (M, N) and aux.dtype == out.dtype and aux.stride(1) == 1
            assert gelu == (mode in (1, 3))
        ncol, cs = col_scale if col_scale is not None else (0, 1.0)
        _lib.check(_lib.lib().acai_gemm_nt_ex(a.data_ptr(), _ld(a), w.data_ptr(), _ld(w), _p(bias), _p(residual),
                                              _ld(residual) if residual is not None else 0, out.data_ptr(), _ld(out),
                                              aux.data_ptr() if aux is not None else None, _ld(aux) if aux is not None else 0,
                                              mode, M, N, K, _dt(a), _dt(out), flags, int(ncol), float(cs), _st()), "acai_gemm_nt_ex")
        return out
    _lib.check(_lib.lib().acai_gemm_nt(a.data_ptr(), _ld(a), w.data_ptr(), _ld(w), _p(bias), _p(residual),
                                       _ld(residual) if residual is not None else 0, out.data_ptr(), _ld(out),
                                       M, N, K, _dt(a), _dt(out), flags, _st()), "acai_gemm_nt")
    return out


def h2d(t, device, dtype=None):
    """Host tensor -> device WITHOUT stalling the host: staged in pinned memory (torch's caching host allocator) and copied asynchronously on
    the current stream.  `t.to(device)` from pageable memory synchronises the stream - inside a training step every such copy (cu_seqlens,
    index lists, optimizer tables) drained the GPU queue and left it idle until the host had enqueued the next kernels (MAE step: 6-9 ms of
    idle GPU per 120 ms step, tools/gpu_idle_from_trace.py).  Device tensors pass through."""
    if t.device.type == "cpu" and torch.device(device).type == "cuda":
        t = t.pin_memory().to(device, non_blocking=True)
    else:
        t = t.to(device)
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


class _ZeroArena:
    """Zeroed fp32 scratch for the split-K weight-gradient GEMMs (they accumulate with float atomics into a zeroed output): slices of a few
    large chunks, each zeroed by ONE fill, instead of one `torch.zeros` launch per weight gradient (the MAE step issued ~380 five-microsecond
    fills, the teacher-forced step ~700).  A slice becomes `param.grad` (autograd keeps the tensor it is handed), so a chunk lives exactly as
    long as the gradients cut from it; a fresh chunk is taken from torch's caching allocator when the current one is used up."""
    CHUNK = 64 << 20   # elements (256 MB)
    SMALL_CHUNK, SMALL_MAX = 1 << 20, 1 << 16   # 4 MB chunks for slices of up to 256 KB: bias / LayerNorm / column-sum accumulators

    def __init__(self):
        self._buf, self._off = {}, {}

    def take(self, rows, cols, device):
        n = rows * cols
        if n >= self.CHUNK // 4:
            return torch.zeros(rows, cols, dtype=torch.float32, device=device)
        # one arena per (device, stream): a chunk is zero-filled on the stream that is current when it is created, and every slice of it is
        # consumed by a GEMM launched on that same stream (ops launch on torch's current stream), so fill and use are ordered.
        # Small slices (the 1-D accumulators that become bias / LayerNorm gradients) come from their own 4 MB chunks: a caller that keeps one
        # such gradient after training must not pin a 256 MB weight-gradient chunk with it.
        small = n <= self.SMALL_MAX
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream, small)
        buf, off = self._buf.get(key), self._off.get(key, 0)
        if buf is None or off + n > buf.numel():
            buf, off = torch.zeros(self.SMALL_CHUNK if small else self.CHUNK, dtype=torch.float32, device=device), 0
            self._buf[key] = buf
        self._off[key] = off + ((n + 63) & ~63)   # 256-byte aligned slices
        return buf[off:off + n].view(rows, cols)


    def release(self):
        """Drop the cached chunks (gradients already cut from them keep their chunk alive until they are freed themselves)."""
        self._buf.clear()
        self._off.clear()


_ZEROS = _ZeroArena()


def release_scratch():
    """Free the zeroed weight-gradient arena's current chunks (up to 256 MB per device and stream stay cached after training ends).  Note for
    callers that serialise gradients: a weight gradient produced by `gemm(trans_a=True, trans_w=True)` is a VIEW of a 256 MB chunk -
    `torch.save(p.grad)` writes the whole storage; save `p.grad.clone()` instead (optimizer / model state dicts hold no gradients)."""
    _ZEROS.release()


def gemm(a, w, trans_a=False, trans_w=False, bias=None, residual=None, out_dtype=torch.float32, out=None):
    """out[M,N] = op(a) @ op(w)^T: logical a [M,K] (stored [K,M] if trans_a), logical w [N,K] (stored [K,N] if trans_w)."""
    _chk(a, "a"), _chk(w, "w")
    assert a.dim() == 2 and w.dim() == 2 and a.dtype == w.dtype
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    N, K2 = (w.shape[1], w.shape[0]) if trans_w else w.shape
    assert K == K2, (a.shape, w.shape, trans_a, trans_w)
    if out is None:
        # the weight-gradient form accumulates (split-K atomics) into an fp32 output
        out = _ZEROS.take(M, N, a.device) if (trans_a and trans_w) else torch.empty(M, N, dtype=out_dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == (M, N) and residual.stride(1) == 1
    _lib.check(_lib.lib().acai_gemm(a.data_ptr(), _ld(a), 1 if trans_a else 0, w.data_ptr(), _ld(w), 1 if trans_w else 0, _p(bias),
                                    _p(residual), _ld(residual) if residual is not None else 0, out.data_ptr(), _ld(out), M, N, K,
                                    _dt(a), _dt(out), 0, _st()), "acai_gemm")
    return out


def cast_bf16(x):
    _chk(x, "x", torch.float32)
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if x.numel() == 0:
        return y
    _lib.check(_lib.lib().acai_cast_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _st()), "acai_cast_f32_bf16")
    return y


def patchify(img, P, out, row0):
    """img (1,H,W) fp32 -> rows row0.. of out [M, P*P]."""
    _chk(img, "img", torch.float32)
    assert img.dim() == 3 and img.shape[0] == 1 and img.is_contiguous()
    H, W = img.shape[1], img.shape[2]
    n = (H // P) * (W // P)
    assert out.dim() == 2 and out.shape[1] == P * P and row0 + n <= out.shape[0] and out.stride(1) == 1
    _lib.check(_lib.lib().acai_patchify(img.data_ptr(), H, W, P, out.data_ptr(), out.stride(0), row0, _dt(out), _st()), "acai_patchify")
    return n


def resize_bicubic_aa(img, size, clamp01=False):
    """img (C,H,W) fp32 on the GPU -> (C,OH,OW): bicubic, antialiased, align_corners=False (the float path of torchvision's resize that
    DynamicResize / PatchDivisibleResize call, acai_omr/utils/utils.py:325-330,351-356); clamp01 fuses DynamicResize's clamp (:367)."""
    _chk(img, "img", torch.float32)
    assert img.dim() == 3 and img.is_contiguous()
    C, H, W = img.shape
    OH, OW = int(size[0]), int(size[1])
    tmp = torch.empty(C, H, OW, dtype=torch.float32, device=img.device)
    out = torch.empty(C, OH, OW, dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().acai_resize_bicubic_aa(img.data_ptr(), C, H, W, tmp.data_ptr(), out.data_ptr(), OH, OW, int(bool(clamp01)), _st()),
               "acai_resize_bicubic_aa")
    return out


def resize_to_patches(img, size, P, out, row0, crop=None, clamp01=False):
    """One (1,H,W) or (H,W) image on the GPU - fp32 in [0,1], or uint8 (scaled by 1/255 on load) - resized to `size` = (OH, OW) (bicubic,
    antialiased, optional clamp) and written as the nn.Unfold(P, P) rows row0 .. of the packed patch stream `out` [rows, P*P] (fp32 or bf16):
    the resize's height pass stores patch rows directly - no resized image tensor, no patchify launch, no bf16 cast.
    crop = (top, left, h, w): the window of the resized image that is kept (DynamicResize's centre crop).  Returns the number of rows written."""
    assert img.is_cuda and img.dtype in (torch.float32, torch.uint8) and img.is_contiguous()
    if img.dim() == 3:
        assert img.shape[0] == 1, "one channel (NUM_CHANNELS = 1)"
        img = img[0]
    H, W = img.shape
    OH, OW = int(size[0]), int(size[1])
    top, left, ch, cw = (0, 0, OH, OW) if crop is None else [int(v) for v in crop]
    assert out.is_cuda and out.dim() == 2 and out.shape[1] == P * P and out.stride(1) == 1 and out.dtype in (torch.float32, torch.bfloat16)
    n = (ch // P) * (cw // P)
    assert row0 + n <= out.shape[0]
    tmp = torch.empty(H, OW, dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().acai_resize_to_patches(img.data_ptr(), 1 if img.dtype == torch.uint8 else 0, H, W, tmp.data_ptr(), out.data_ptr(), out.stride(0),
                                                 int(row0), OH, OW, top, left, ch, cw, int(P), _dt(out), int(bool(clamp01)), _st(img)), "acai_resize_to_patches")
    return n


# ---- whole pages (csrc/page.hip) --------------------------------------------------------------------------------------------------------
def _page(page):
    """A page operand: one channel, uint8 or fp32, (H, W) or (1, H, W) on the GPU, rows `pitch` elements apart (a column slice of a wider
    tensor is taken as it is).  Returns (2-D view, H, W, pitch, in_u8)."""
    if not torch.is_tensor(page):
        raise TypeError("page: expected a tensor")
    _chk(page, "page")
    if page.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"page: expected uint8 or float32, got {page.dtype}")
    if page.dim() == 3 and page.shape[0] == 1:
        page = page[0]
    if page.dim() != 2 or page.shape[0] < 1 or page.shape[1] < 1:
        raise ValueError("page: expected one channel, (H, W) or (1, H, W), not empty")
    H, W = page.shape
    pitch = page.stride(0) if H > 1 else W
    if pitch < W:
        raise ValueError("page: rows overlap (row stride below the width)")
    return page, H, W, pitch, 1 if page.dtype == torch.uint8 else 0


@_on_operand_device
def page_profile(page, ink_threshold=0.5):
    """Row profiles of a page -> (ink, run), int32 [H] each: the number of pixels below ink_threshold in each row and the longest run of
    consecutive such pixels (uint8 pages are read as p / 255).  W <= 16384, H <= 65535."""
    page, H, W, pitch, u8 = _page(page)
    out = torch.empty(2, H, dtype=torch.int32, device=page.device)
    _lib.check(_lib.lib().acai_page_profile(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), out[0].data_ptr(), out[1].data_ptr(), _st(page)),
               "acai_page_profile")
    return out[0], out[1]


@_on_operand_device
def page_systems(page, ink, run, ink_threshold, min_ink, merge_gap, min_height, line_len, min_line_rows, margin, max_systems, out=None):
    """The profiles of `page_profile` -> (count int32 [1], boxes int32 [max_systems, 4]) on the device: bands of inked rows
    (ink >= min_ink, gaps of at most merge_gap rows bridged) that are at least min_height tall and hold at least min_line_rows rows with
    run >= line_len, as boxes (x0, y0, x1, y1) around their ink grown by margin and clipped to the page, top to bottom.  count may exceed
    max_systems; box rows from min(count, max_systems) on are left as they are.  Both are views of one int32 buffer (`out`, 4 + 4
    max_systems elements, allocated when None), so one copy brings both to the host."""
    page, H, W, pitch, u8 = _page(page)
    _chk(ink, "ink", torch.int32), _chk(run, "run", torch.int32)
    if tuple(ink.shape) != (H,) or tuple(run.shape) != (H,) or ink.device != page.device or run.device != page.device:
        raise ValueError(f"ink / run: expected int32 [{H}] on the page's device")
    n = int(max_systems)
    if out is None:
        out = torch.empty(4 + 4 * max(n, 0), dtype=torch.int32, device=page.device)
    _chk(out, "out", torch.int32)
    if out.dim() != 1 or out.numel() < 4 + 4 * n or out.device != page.device:
        raise ValueError(f"out: expected at least {4 + 4 * n} int32 on the page's device")
    count, boxes = out[:1], out[4:4 + 4 * n].view(n, 4)
    _lib.check(_lib.lib().acai_page_systems(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), ink.data_ptr(), run.data_ptr(), int(min_ink),
                                            int(merge_gap), int(min_height), int(line_len), int(min_line_rows), int(margin), n, count.data_ptr(),
                                            boxes.data_ptr(), _st(page)), "acai_page_systems")
    return count, boxes


def crop_resize_entry(page, box, size, crop, row0, tmp_off):
    """One `_lib.AcaiCropResize`: `box` = (x0, y0, w, h) of `page` (a GPU tensor as `page_profile` takes it) resized to `size` = (OH, OW), of
    which the window `crop` = (top, left, ch, cw) goes to the patch rows from row0; tmp_off: its offset into the width-pass scratch."""
    page, H, W, pitch, u8 = _page(page)
    x0, y0, w, h = (int(v) for v in box)
    top, left, ch, cw = (int(v) for v in crop)
    return _lib.AcaiCropResize(page.data_ptr(), int(tmp_off), H, W, pitch, u8, x0, y0, w, h, int(size[0]), int(size[1]), top, left, ch, cw, int(row0), 0)


@_on_operand_device
def crop_resize_to_patches(entries, out, P, clamp01=False):
    """A list of `crop_resize_entry` -> their nn.Unfold(P, P) rows in the packed patch stream `out` [rows, P*P] (fp32 or bf16) in two
    launches, whatever the number of entries: every box is cut from its page, resized (bicubic, antialiased, taps clamped to the box) and
    cropped to its window exactly as `resize_to_patches` does it for a contiguous copy of the box - the same bits.  The pages must stay alive
    until the call returns (the entries hold raw pointers) and lie on `out`'s device.  One table upload, one scratch allocation."""
    _chk(out, "out")
    if out.dim() != 2 or out.shape[1] != P * P or out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out: expected [rows, {P * P}] fp32 or bf16, got {tuple(out.shape)} {out.dtype}")
    if not entries:
        raise ValueError("crop_resize_to_patches: no entries")
    host = (_lib.AcaiCropResize * len(entries))(*entries)
    tmp_elems = max(e.tmp_off + e.h * e.OW for e in entries)
    table = h2d(torch.frombuffer(memoryview(host).cast("B"), dtype=torch.uint8), out.device)
    tmp = torch.empty(max(int(tmp_elems), 1), dtype=torch.float32, device=out.device)
    _lib.check(_lib.lib().acai_crop_resize_to_patches(table.data_ptr(), host, len(entries), tmp.data_ptr(), int(tmp_elems), out.data_ptr(), _ld(out),
                                                      out.shape[0], int(P), _dt(out), int(bool(clamp01)), _st(out)), "acai_crop_resize_to_patches")


# ---- page deskew (csrc/deskew.hip) ------------------------------------------------------------------------------------------------------
def _strip(S):
    if S not in _lib.STRIP_WIDTHS:
        raise ValueError(f"strip width {S}: expected one of {_lib.STRIP_WIDTHS}")
    return int(S)


@_on_operand_device
def page_strips(page, S=16, ink_threshold=0.5):
    """Strip profile of a page (as `page_profile` takes it) -> uint8 [nS, H], nS = ceil(W / S): the number of pixels below ink_threshold of
    row y in columns [s S, min((s + 1) S, W)), strip-major so that the rows of a strip are contiguous.  S in {8, 16, 32, 64}."""
    S = _strip(S)
    page, H, W, pitch, u8 = _page(page)
    out = torch.empty(-(-W // S), H, dtype=torch.uint8, device=page.device)
    _lib.check(_lib.lib().acai_page_strips(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), S, out.data_ptr(), _st(page)), "acai_page_strips")
    return out


def skew_slope_table(slopes, device):
    """Q16 slopes (Python ints, round(tan(angle) * 65536)) -> (device int32 [K], the ctypes host copy the C ABI checks): the one upload a
    batch of `page_skew_scores` calls shares."""
    slopes = [int(m) for m in slopes]
    if not 1 <= len(slopes) <= _lib.SKEW_MAX_SLOPES or any(abs(m) > _lib.SKEW_MAX_SLOPE for m in slopes):
        raise ValueError(f"skew slopes: expected 1 .. {_lib.SKEW_MAX_SLOPES} values within +-{_lib.SKEW_MAX_SLOPE} (tan 15 deg in Q16)")
    return h2d(torch.tensor(slopes, dtype=torch.int32), device), (ctypes.c_int32 * len(slopes))(*slopes)


@_on_operand_device
def page_skew_scores(strips, W, S, slopes, out=None):
    """`page_strips` of a page of width W at strip width S, and K Q16 slopes (a list of ints, or a `skew_slope_table`) -> int64 [K]: for
    every slope the strip profile sheared along it, summed over the strips and scored by the sum of its squared row differences
    (include/acai_omr_hip.h has the integer definition).  `out`: an int64 [K] to write into (a row of a larger tensor)."""
    _chk(strips, "strips", torch.uint8)
    S = _strip(S)
    if strips.dim() != 2 or not strips.is_contiguous() or strips.shape[0] != -(-int(W) // S) or strips.shape[1] < 1:
        raise ValueError(f"strips: expected a contiguous uint8 [ceil({W} / {S}), H], got {tuple(strips.shape)}")
    table, host = slopes if isinstance(slopes, tuple) else skew_slope_table(slopes, strips.device)
    _chk(table, "slopes", torch.int32)
    K = len(host)
    if table.dim() != 1 or table.numel() != K or table.device != strips.device:
        raise ValueError(f"slopes: expected int32 [{K}] on the strips' device")
    if out is None:
        out = torch.empty(K, dtype=torch.int64, device=strips.device)
    _chk(out, "out", torch.int64)
    if tuple(out.shape) != (K,) or out.device != strips.device:
        raise ValueError(f"out: expected int64 [{K}] on the strips' device")
    _lib.check(_lib.lib().acai_page_skew_scores(strips.data_ptr(), strips.shape[1], int(W), S, table.data_ptr(), host, K, out.data_ptr(), _st(strips)),
               "acai_page_skew_scores")
    return out


def rotation_q16(angle_deg):
    """(cos_q, sin_q) = (round(cos * 65536), round(sin * 65536)) of an angle in degrees: what `page_rotate` turns by."""
    a = math.radians(float(angle_deg))
    return int(round(math.cos(a) * 65536.0)), int(round(math.sin(a) * 65536.0))


@_on_operand_device
def page_rotate(page, angle=None, fill=None, cos_sin_q=None):
    """The page turned about its centre by `angle` degrees (positive: what is displayed turns counter-clockwise), or by the Q16 pair
    cos_sin_q = (cos_q, sin_q) -> a new contiguous page of the same size and dtype.  Bilinear with Q16 source coordinates and 8-bit weights
    (include/acai_omr_hip.h); taps outside the page read `fill` (default: the paper, 255 / 1.0).  uint8 results are exact integers."""
    page, H, W, pitch, u8 = _page(page)
    if (angle is None) == (cos_sin_q is None):
        raise ValueError("page_rotate: give the angle in degrees or cos_sin_q")
    cos_q, sin_q = rotation_q16(angle) if cos_sin_q is None else (int(v) for v in cos_sin_q)
    if fill is None:
        fill = 255 if u8 else 1.0
    out = torch.empty(H, W, dtype=page.dtype, device=page.device)
    _lib.check(_lib.lib().acai_page_rotate(page.data_ptr(), u8, H, W, pitch, cos_q, sin_q, float(fill), out.data_ptr(), W, _st(page)), "acai_page_rotate")
    return out


# ---- page illumination flattening (csrc/flatten.hip) ------------------------------------------------------------------------------------
def _tile(tile):
    if tile not in _lib.FLATTEN_TILES:
        raise ValueError(f"tile {tile}: expected one of {_lib.FLATTEN_TILES}")
    return int(tile)


@_on_operand_device
def page_tile_levels(page, tile, percent=50):
    """Tile levels of a page (as `page_profile` takes it) -> uint8 [GH, GW], GH = ceil(H / tile), GW = ceil(W / tile): per tile of tile x
    tile pixels (cut off at the page's edges) the rank-th smallest level of its n pixels, rank = max(1, (n percent + 99) // 100) - at the
    default 50 the median, the paper of a tile that is not mostly ink.  A uint8 pixel is its own level, an fp32 pixel v is
    floor(v * 255 + 0.5) clipped to 0 .. 255.  tile in {16, 32, 64, 128}, percent an integer in 1 .. 100 (ValueError otherwise)."""
    tile = _tile(tile)
    if int(percent) != percent or not 1 <= int(percent) <= 100:
        raise ValueError(f"percent = {percent}: expected an integer in 1 .. 100")
    page, H, W, pitch, u8 = _page(page)
    out = torch.empty(-(-H // tile), -(-W // tile), dtype=torch.uint8, device=page.device)
    _lib.check(_lib.lib().acai_page_tile_levels(page.data_ptr(), u8, H, W, pitch, tile, int(percent), out.data_ptr(), _st(page)), "acai_page_tile_levels")
    return out


@_on_operand_device
def page_flatten(page, grid, tile, rq=85, floor=32, out=None):
    """The page divided by its paper level -> a page of the same size and dtype (`out`: a (H, W) view to write into, its padding is left
    alone; allocated contiguous when None).  grid: `page_tile_levels` of the page at `tile`.  A tile whose level is below rq / 256 of the
    brightest level among its 3 x 3 neighbours takes that level (it is mostly ink; rq = 0: never), every level is raised to `floor`, the
    grid is interpolated bilinearly between the tile centres, and a pixel p becomes min(255, p * 255 / background) rounded to nearest -
    include/acai_omr_hip.h has the integer definition, which the fp32 output follows with one multiply.  One launch.  A grid of another
    shape, dtype or device, a tile other than 16, 32, 64, 128, rq outside 0 .. 256 or floor outside 1 .. 255: ValueError."""
    tile = _tile(tile)
    page, H, W, pitch, u8 = _page(page)
    want = (-(-H // tile), -(-W // tile))
    if not torch.is_tensor(grid) or not grid.is_cuda or grid.device != page.device or grid.dtype != torch.uint8 or tuple(grid.shape) != want or not grid.is_contiguous():
        raise ValueError(f"grid: expected a contiguous uint8 {list(want)} on the page's device (page_tile_levels at tile {tile})")
    if int(rq) != rq or not 0 <= int(rq) <= 256 or int(floor) != floor or not 1 <= int(floor) <= 255:
        raise ValueError(f"rq = {rq}, floor = {floor}: expected integers in 0 .. 256 and 1 .. 255")
    if out is None:
        out = torch.empty(H, W, dtype=page.dtype, device=page.device)
    if (not torch.is_tensor(out) or not out.is_cuda or out.device != page.device or out.dtype != page.dtype or tuple(out.shape) != (H, W)
            or out.stride(1) != 1 or (H > 1 and out.stride(0) < W) or out.data_ptr() == page.data_ptr()):
        raise ValueError(f"out: expected a {page.dtype} ({H}, {W}) view on the page's device with contiguous, non-overlapping rows, not the page itself")
    _lib.check(_lib.lib().acai_page_flatten(page.data_ptr(), u8, H, W, pitch, grid.data_ptr(), tile, int(rq), int(floor), out.data_ptr(),
                                            out.stride(0) if H > 1 else W, _st(page)), "acai_page_flatten")
    return out


# ---- page rectification (csrc/rectify.hip) ----------------------------------------------------------------------------------------------
def default_min_run(H, W):
    """The run of paper pixels that counts as the sheet in `page_extents`: max(4, min(H, W) // 100), capped at what the kernel takes."""
    return min(max(4, min(int(H), int(W)) // 100), _lib.EXTENTS_MAX_RUN)


@_on_operand_device
def page_extents(page, paper_threshold=0.5, min_run=None):
    """Paper extents of a page (as `page_profile` takes it) -> int32 [2 H + 2 W] = row_lo [H], row_hi [H], col_lo [W], col_hi [W].  A pixel
    is paper when it is not ink at paper_threshold; with R = min_run (default `default_min_run`; 1 .. 256), row_lo[y] is the smallest x
    with pixels x .. x + R - 1 of row y all paper (W: none), row_hi[y] the largest x with x - R + 1 .. x all paper (-1: none), col_lo /
    col_hi the same down the columns (H / -1: none).  Two launches."""
    page, H, W, pitch, u8 = _page(page)
    R = default_min_run(H, W) if min_run is None else min_run
    if isinstance(R, bool) or int(R) != R or not 1 <= int(R) <= _lib.EXTENTS_MAX_RUN:
        raise ValueError(f"min_run = {min_run!r}: expected an integer in 1 .. {_lib.EXTENTS_MAX_RUN}")
    out = torch.empty(2 * H + 2 * W, dtype=torch.int32, device=page.device)
    _lib.check(_lib.lib().acai_page_extents(page.data_ptr(), u8, H, W, pitch, float(paper_threshold), int(R), out.data_ptr(), _st(page)), "acai_page_extents")
    return out


def _solve_square_to_quad(quad):
    """The unit square's (0, 0), (1, 0), (1, 1), (0, 1) -> the quad's TL, TR, BR, BL: (a, b, c, d, e, f, g, h) of x = (a u + b v + c) / (g u +
    h v + 1), y = (d u + e v + f) / (g u + h v + 1) in closed form (Heckbert 1989), every operation in float64 and in this order."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = ((float(x), float(y)) for x, y in quad)
    dx1, dx2, sx = x1 - x2, x3 - x2, (x0 - x1) + (x2 - x3)
    dy1, dy2, sy = y1 - y2, y3 - y2, (y0 - y1) + (y2 - y3)
    det = dx1 * dy2 - dx2 * dy1
    if det == 0.0:
        raise ValueError(f"quad {quad}: three corners on a line")
    g, h = (sx * dy2 - dx2 * sy) / det, (dx1 * sy - sx * dy1) / det
    return (x1 - x0) + g * x1, (x3 - x0) + h * x3, x0, (y1 - y0) + g * y1, (y3 - y0) + h * y3, y0, g, h


def homography_q30(quad, out_size, inset=0):
    """The nine integers A .. I `page_warp` takes: the homography (float64 on the host, no trigonometry) that takes the corners of the
    output rectangle grown by `inset` pixels - (-inset, -inset), (OW - 1 + inset, -inset), (OW - 1 + inset, OH - 1 + inset), (-inset,
    OH - 1 + inset) - to quad = [TL, TR, BR, BL] (x, y) of the page, scaled so that the largest of its denominators at the output pixels
    (0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1) is 1, every entry int(round(v * 2**30)).  out_size = (OH, OW).  A quad whose
    denominator is not positive at all four: ValueError."""
    OH, OW = (int(v) for v in out_size)
    inset = float(inset)
    lx, ly = OW - 1 + 2.0 * inset, OH - 1 + 2.0 * inset
    if OH < 1 or OW < 1 or not (lx > 0 and ly > 0):
        raise ValueError(f"homography_q30: out_size {out_size} with inset {inset} spans no rectangle")
    a, b, c, d, e, f, g, h = _solve_square_to_quad(quad)
    # u = (x + inset) / lx, v = (y + inset) / ly
    m = [a / lx, b / ly, c + (a * inset) / lx + (b * inset) / ly,
         d / lx, e / ly, f + (d * inset) / lx + (e * inset) / ly,
         g / lx, h / ly, 1.0 + (g * inset) / lx + (h * inset) / ly]
    dens = [m[6] * x + m[7] * y + m[8] for x, y in ((0, 0), (OW - 1, 0), (OW - 1, OH - 1), (0, OH - 1))]
    if not min(dens) > 0.0:
        raise ValueError(f"quad {quad}: the output rectangle crosses the horizon of its homography (not a convex quad in TL, TR, BR, BL order?)")
    top = max(dens)
    return [int(round(v / top * 2.0 ** 30)) for v in m]


@_on_operand_device
def page_warp(page, coef, out_size, fill=None, out=None):
    """The page seen through the homography coef = nine integers A .. I (`homography_q30`) -> a new contiguous (OH, OW) page of the same
    dtype, out_size = (OH, OW) (or written into `out`, a view of that shape with contiguous rows).  Output pixel (x, y) is sampled at
    floor((A x + B y + C) * 256 / (G x + H y + I)) / 256, floor((D x + E y + F) * 256 / (G x + H y + I)) / 256, bilinear with 8-bit weights
    as `page_rotate` (include/acai_omr_hip.h); taps outside the page read `fill` (default: the paper, 255 / 1.0).  uint8 results are exact
    integers.  A denominator that is not positive over the output, or forms beyond 2^62: RuntimeError from the library."""
    page, H, W, pitch, u8 = _page(page)
    coef = [int(v) for v in coef]
    if len(coef) != 9 or any(not -2 ** 63 <= v < 2 ** 63 for v in coef):
        raise ValueError("page_warp: coef is nine integers A .. I that fit 64 bits")
    OH, OW = (int(v) for v in out_size)
    if fill is None:
        fill = 255 if u8 else 1.0
    if out is None:
        if OH < 1 or OW < 1:
            raise ValueError(f"page_warp: out_size {out_size}")
        out = torch.empty(OH, OW, dtype=page.dtype, device=page.device)
    if (not torch.is_tensor(out) or not out.is_cuda or out.device != page.device or out.dtype != page.dtype or tuple(out.shape) != (OH, OW)
            or out.stride(1) != 1 or (OH > 1 and out.stride(0) < OW)):
        raise ValueError(f"out: expected a {page.dtype} ({OH}, {OW}) view on the page's device with contiguous, non-overlapping rows")
    _lib.check(_lib.lib().acai_page_warp(page.data_ptr(), u8, H, W, pitch, (ctypes.c_int64 * 9)(*coef), float(fill), out.data_ptr(), OH, OW,
                                         out.stride(0) if OH > 1 else OW, _st(page)), "acai_page_warp")
    return out


# ---- camera augmentation (csrc/augment.hip) ---------------------------------------------------------------------------------------------
# ---- page ingest: colour photos and EXIF / quarter-turn orientation (csrc/ingest.hip) ------------------------------------------------------
EXIF_TRANSPOSED = (5, 6, 7, 8)        # the orientation codes that swap height and width
EXIF_INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}   # the code that undoes a code: a quarter turn is undone by the opposite one


def exif_code(code):
    """An EXIF orientation code as an int in 1 .. 8: anything that is not an integer is a TypeError, an integer outside 1 .. 8 a ValueError."""
    if isinstance(code, bool) or not isinstance(code, int):
        raise TypeError(f"orientation: expected an EXIF code, an integer in 1 .. 8, got {code!r}")
    if not 1 <= code <= 8:
        raise ValueError(f"orientation: {code} is not an EXIF code (1 .. 8)")
    return code


def oriented_size(H, W, code):
    """(H', W') of an H x W photo once orientation `code` is applied."""
    return (W, H) if code in EXIF_TRANSPOSED else (H, W)


def _photo(image, layout=None):
    """A decoded photo on the GPU -> (H, W, C, pixel stride, row stride, channel stride), strides in elements.  (H, W); or three
    dimensions with layout "hwc" (interleaved, C = 1, 3 or 4) or "chw" (planar, C = 1 or 3).  layout None decides by the shape: a leading
    1 is planar, then a trailing 3 or 4 interleaved, then a leading 3 planar, then a trailing 1 interleaved - so a planar photo 3 or 4
    pixels wide needs layout="chw" said.  uint8, or single-channel float32.  Any strides (a slice of a larger tensor), none of them 0."""
    if not torch.is_tensor(image):
        raise TypeError("image: expected a tensor")
    _chk(image, "image", rows_contig=False)
    if image.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"image: expected uint8 or float32, got {image.dtype}")
    if layout not in (None, "hwc", "chw"):
        raise ValueError(f"layout: expected None, 'hwc' or 'chw', got {layout!r}")
    if image.dim() == 2:
        shape, stride = (*image.shape, 1), (*image.stride(), 1)                                    # (H, W, C), (row, pixel, channel)
    elif image.dim() == 3:
        if layout is None:
            layout = ("chw" if image.shape[0] == 1 else "hwc" if image.shape[2] in (3, 4) else "chw" if image.shape[0] == 3
                      else "hwc" if image.shape[2] == 1 else None)
        if layout == "hwc":
            shape, stride = tuple(image.shape), tuple(image.stride())
        elif layout == "chw":
            shape, stride = (image.shape[1], image.shape[2], image.shape[0]), (image.stride(1), image.stride(2), image.stride(0))
        else:
            raise TypeError(f"image: a {tuple(image.shape)} tensor is neither (H, W, C) with C in 1, 3, 4 nor (C, H, W) with C in 1, 3")
    else:
        raise TypeError("image: expected (H, W), (H, W, C) or (C, H, W)")
    (H, W, C), (rs, ps, cs) = shape, stride
    if C not in ((1, 3, 4) if layout != "chw" else (1, 3)):
        raise TypeError(f"image: {C} channels ({'planar' if layout == 'chw' else 'interleaved'})")
    if C != 1 and image.dtype != torch.uint8:
        raise TypeError("image: float colour input is not taken (single-channel float32, or uint8)")
    if H < 1 or W < 1:
        raise ValueError("image: empty")
    if (H > 1 and rs < 1) or (W > 1 and ps < 1) or (C > 1 and cs < 1):
        raise ValueError("image: a stride of 0 (an expanded tensor)")
    return H, W, C, max(int(ps), 1), max(int(rs), 1), max(int(cs), 1)


@_on_operand_device
def page_ingest(image, orientation=1, layout=None, out=None):
    """A decoded photo (`_photo`: uint8 (H, W), (H, W, C), (C, H, W), or single-channel float32, any strides) -> the grey, upright page, a new
    contiguous (H', W') tensor of the photo's dtype (or `out`, a view of that shape with contiguous rows), in ONE launch.  The grey value
    is PIL's convert("L"): (19595 R + 38470 G + 7471 B + 32768) >> 16, a fourth channel ignored; a single channel is moved as it is, float32
    bit for bit.  orientation is an EXIF code 1 .. 8, applied as PIL's ImageOps.exif_transpose applies it (include/acai_omr_hip.h has the
    eight index maps); 5 .. 8 give a (W, H) page."""
    code = exif_code(orientation)
    H, W, C, ps, rs, cs = _photo(image, layout)
    OH, OW = oriented_size(H, W, code)
    if out is None:
        out = torch.empty(OH, OW, dtype=image.dtype, device=image.device)
    if (not torch.is_tensor(out) or not out.is_cuda or out.device != image.device or out.dtype != image.dtype or tuple(out.shape) != (OH, OW)
            or out.stride(1) != 1 or (OH > 1 and out.stride(0) < OW)):
        raise ValueError(f"out: expected a {image.dtype} ({OH}, {OW}) view on the image's device with contiguous, non-overlapping rows")
    _lib.check(_lib.lib().acai_page_ingest(image.data_ptr(), 1 if image.dtype == torch.uint8 else 0, H, W, C, ps, rs, cs, code, out.data_ptr(),
                                           out.stride(0) if OH > 1 else OW, _st(image)), "acai_page_ingest")
    return out


@_on_operand_device
def page_col_profile(page, ink_threshold=0.5):
    """Column profiles of a page (as `page_profile` takes it) -> (ink, run), int32 [W] each: the number of pixels below ink_threshold in
    each column and the longest run of consecutive such pixels down it - `page_profile` of the transposed page.  Two launches."""
    page, H, W, pitch, u8 = _page(page)
    out = torch.empty(2, W, dtype=torch.int32, device=page.device)
    work = torch.empty(4 * _lib.col_chunks(H)[1] * W, dtype=torch.int32, device=page.device)
    _lib.check(_lib.lib().acai_page_col_profile(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), out[0].data_ptr(), out[1].data_ptr(), work.data_ptr(),
                                                work.numel(), _st(page)), "acai_page_col_profile")
    return out[0], out[1]


@_on_operand_device
def page_box_ink(page, boxes, ink_threshold=0.5):
    """The ink count of every rectangle of a device table -> int32 [n]: boxes is a contiguous int32 [n, 4] of (x0, y0, x1, y1) on the page's
    device (clipped to the page; an empty rectangle counts 0).  One launch for the whole table, none for an empty one."""
    page, H, W, pitch, u8 = _page(page)
    if not torch.is_tensor(boxes):
        raise TypeError("boxes: expected a tensor")
    _chk(boxes, "boxes", torch.int32)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous() or boxes.device != page.device or boxes.shape[0] > 65535:
        raise ValueError("boxes: expected a contiguous int32 [n, 4] on the page's device, n <= 65535")
    n = boxes.shape[0]
    out = torch.empty(n, dtype=torch.int32, device=page.device)
    _lib.check(_lib.lib().acai_page_box_ink(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), boxes.data_ptr() if n else None, n,
                                            out.data_ptr() if n else None, _st(page)), "acai_page_box_ink")
    return out


# ---- page assessment (csrc/assess.hip) --------------------------------------------------------------------------------------------------
def _assess_out(out, words, page, name):
    """The int64 words a page assessment kernel adds into: fresh zeros, or the caller's (a contiguous view on the page's device that it has
    zeroed - one fill then serves every page of a call)."""
    if out is None:
        return torch.zeros(words, dtype=torch.int64, device=page.device)
    if not torch.is_tensor(out):
        raise TypeError(f"{name}: out: expected a tensor")
    _chk(out, "out", torch.int64)
    if out.numel() != words or not out.is_contiguous() or out.device != page.device:
        raise ValueError(f"{name}: out: expected {words} contiguous int64 on the page's device")
    return out


@_on_operand_device
def page_runs(page, ink_threshold=0.5, out=None):
    """Vertical run-length histograms of a page (as `page_profile` takes it) -> int64 [3, 256]: in every column, the closed runs of ink
    (row 0) and of paper (row 1) by their length, and every closed ink run together with the closed paper run directly under it by the
    sum of the two (row 2), lengths clamped to 255; a run that touches the first or the last row of the page is open and not counted.
    Two launches.  out: 768 zeroed int64 that the counts are ADDED to (default: fresh zeros)."""
    page, H, W, pitch, u8 = _page(page)
    hist = _assess_out(out, _lib.RUNS_WORDS, page, "page_runs")
    work = torch.empty(-(-H // _lib.RUNS_CHUNK_ROWS) * W, dtype=torch.int32, device=page.device)
    _lib.check(_lib.lib().acai_page_runs(page.data_ptr(), u8, H, W, pitch, float(ink_threshold), hist.data_ptr(), work.data_ptr(), work.numel(), _st(page)),
               "acai_page_runs")
    return hist.view(3, 256)


@_on_operand_device
def page_sharpness(page, out=None):
    """One read of a page (as `page_profile` takes it) -> (stats int64 [3], levels int64 [256]), two views of one buffer: the sum and the
    sum of squares of the Laplacian L = 4 p - up - down - left - right of the levels over the interior pixels with their number, and the
    histogram of the levels of all pixels (a uint8 value as it is, a float one as floor(v * 255 + 0.5), clamped).  One launch.  out: 259
    zeroed int64 that everything is ADDED to (default: fresh zeros)."""
    page, H, W, pitch, u8 = _page(page)
    buf = _assess_out(out, _lib.SHARP_WORDS, page, "page_sharpness")
    _lib.check(_lib.lib().acai_page_sharpness(page.data_ptr(), u8, H, W, pitch, buf.data_ptr(), _st(page)), "acai_page_sharpness")
    return buf[:3], buf[3:]


def augment_table(entries, device):
    """A list of `_lib.AcaiAugImage` -> the read-only descriptor table in device memory (a uint8 tensor): the one upload of a call."""
    import ctypes
    if not entries:
        raise ValueError("augment_table: no images")
    arr = (_lib.AcaiAugImage * len(entries))(*entries)
    host = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8)
    assert host.numel() == len(entries) * ctypes.sizeof(_lib.AcaiAugImage)
    return host.to(device)


def _aug_chk(table, n_images, max_h, max_w, slots):
    import ctypes
    _chk(table, "table", torch.uint8)
    if table.dim() != 1 or not table.is_contiguous() or table.numel() != int(n_images) * ctypes.sizeof(_lib.AcaiAugImage):
        raise ValueError(f"table: expected {n_images} AcaiAugImage descriptors ({ctypes.sizeof(_lib.AcaiAugImage)} bytes each) in one contiguous uint8 tensor")
    if not (0 < int(n_images) <= 65535 and 0 < int(max_h) <= 65535 and int(max_w) > 0):
        raise ValueError(f"augment: {n_images} images of at most {max_h} x {max_w}: images and rows are grid dimensions (1 .. 65535)")
    if len(set(slots)) != len(slots) or any(s not in (-1, 0, 1) for s in slots) or any(s < 0 for s in slots[1:]):
        raise ValueError(f"augment: slots {slots}: the input is -1 (the source), 0 or 1, every other slot 0 or 1, all different")


def augment_blur_noise(table, n_images, max_h, max_w, in_slot, tmp_slot, out_slot, do_blur=True, do_noise=True):
    """GaussianBlur (separable, reflect padding) and GaussianNoise + clamp over every applied image of the descriptor table:
    in_slot -> tmp_slot -> out_slot; without blur the noise pass alone, in_slot -> out_slot."""
    _aug_chk(table, n_images, max_h, max_w, (in_slot, tmp_slot, out_slot) if do_blur else (in_slot, out_slot))
    _lib.check(_lib.lib().acai_augment_blur_noise(table.data_ptr(), int(n_images), int(max_h), int(max_w), int(in_slot), int(tmp_slot), int(out_slot),
                                                  int(bool(do_blur)), int(bool(do_noise)), _st(table)), "acai_augment_blur_noise")


def augment_warp(table, n_images, max_h, max_w, in_slot, out_slot, perspective):
    """RandomRotation (perspective=False) or RandomPerspective (True) of every applied image: bilinear, zero fill, in_slot -> out_slot."""
    _aug_chk(table, n_images, max_h, max_w, (in_slot, out_slot))
    _lib.check(_lib.lib().acai_augment_warp(table.data_ptr(), int(n_images), int(max_h), int(max_w), int(in_slot), int(out_slot), int(bool(perspective)),
                                            _st(table)), "acai_augment_warp")


def augment_jitter_out(table, n_images, max_h, max_w, in_slot, do_jitter=True, patches=None, patch_size=0):
    """ColorJitter (brightness / contrast with the order-fixed image mean) and the output stage: every image goes to its descriptor's `out`,
    or, with `patches` [rows, P*P] (fp32 / bf16), to its nn.Unfold(P, P) rows from its descriptor's row0.  Images that are not applied are
    copied from their source."""
    _aug_chk(table, n_images, max_h, max_w, (in_slot,))
    ld = P = dt = 0
    if patches is not None:
        _chk(patches, "patches")
        P = int(patch_size)
        if P <= 0 or patches.dim() != 2 or patches.shape[1] != P * P:
            raise ValueError(f"patches: expected [rows, {P * P}] for patch size {P}, got {tuple(patches.shape)}")
        ld, dt = _ld(patches), _dt(patches)
    _lib.check(_lib.lib().acai_augment_jitter_out(table.data_ptr(), int(n_images), int(max_h), int(max_w), int(in_slot), int(bool(do_jitter)), _p(patches),
                                                  ld, P, dt, _st(table)), "acai_augment_jitter_out")


def gather_rows(table, idx, add=None, out=None):
    _chk(table, "table", torch.float32), _chk(idx, "idx", torch.int32)
    assert table.dim() == 2 and table.is_contiguous() and idx.dim() == 1 and idx.is_contiguous()
    rows, dim = idx.numel(), table.shape[1]
    if out is None:
        out = torch.empty(rows, dim, dtype=torch.float32, device=table.device)
    assert out.is_contiguous() and out.shape == (rows, dim)
    if add is not None:
        assert add.shape == (rows, dim) and add.is_contiguous() and add.dtype == torch.float32
    if rows == 0:
        return out
    _lib.check(_lib.lib().acai_gather_rows(table.data_ptr(), idx.data_ptr(), _p(add), out.data_ptr(), rows, dim, _st()), "acai_gather_rows")
    return out


def QSCALE(dh):
    """The factor a prescaled q carries: the softmax scale in the log2 domain."""
    return 1.4426950408889634 / math.sqrt(dh)


@contextlib.contextmanager
def attn_override(which, value):
    """Sets one process-wide override of the attention selection rule (_lib.ATTN_OV_*, acai_attn_set_override) and puts the previous value
    back on exit: tests and A/B runs."""
    L, old = _lib.lib(), ctypes.c_int(0)
    _lib.check(L.acai_attn_get_override(int(which), ctypes.byref(old)), "acai_attn_get_override")
    _lib.check(L.acai_attn_set_override(int(which), int(value)), "acai_attn_set_override")
    try:
        yield
    finally:
        _lib.check(L.acai_attn_set_override(int(which), old.value), "acai_attn_set_override")


def attn_varlen(q, k, v, cu_q, cu_k, H, dh, max_q, causal=False, out=None, lse=None, dropout_p=0.0, seed=0, q_prescaled=False):
    """q [Mq, >=H*dh], k/v [Mk, >=H*dh] (2-D views with any row stride), cu_* int32 [B+1] on the GPU.
    q_prescaled: q already carries log2(e) / sqrt(dh) (QSCALE(dh); gemm_nt(col_scale=...) on the in-projection)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, n)
        assert t.dim() == 2 and t.dtype == q.dtype
    _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32)
    B = cu_q.numel() - 1
    assert cu_k.numel() == B + 1
    if out is None:
        out = torch.empty(q.shape[0], H * dh, dtype=q.dtype, device=q.device)
    assert out.shape[0] == q.shape[0] and out.stride(1) == 1 and out.dtype == q.dtype
    _lib.check(_lib.lib().acai_attn_varlen_fwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                               out.data_ptr(), out.stride(0), cu_q.data_ptr(), cu_k.data_ptr(), B, H, dh, int(max_q),
                                               1 if causal else 0, _dt(q), _p(lse), q.shape[0], float(dropout_p), int(seed) & 0xFFFFFFFF,
                                               1 if q_prescaled else 0, _st()),
               "acai_attn_varlen_fwd")
    return out


def attn_map_layout(lens_q, lens_k, guard=0):
    """Element offsets of the dense [T_b][S_b] blocks of an attention map buffer laid out back to back (`guard` spare elements before,
    between and after them) and the buffer's total length: (offsets list, total)."""
    offs, o = [], int(guard)
    for t, s in zip(lens_q, lens_k):
        offs.append(o)
        o += int(t) * int(s) + int(guard)
    return offs, o


def attn_probs_mean(q, k, cu_q, cu_k, H, dh, max_q, max_k, lse, head_w, map_off, out, accumulate=False):
    """Weighted mean over heads of the attention probabilities (acai_attn_probs_mean): q [Mq, >=H*dh], k [Mk, >=H*dh] as attn_varlen takes
    them, lse [H * Mq] fp32 as attn_varlen(lse=) wrote it for the same q and k, head_w [H] fp32, map_off [B] int64 element offsets into the
    flat fp32 `out` (attn_map_layout), all on the GPU.  Image b's [T_b][S_b] block is overwritten, or added to with accumulate."""
    for t, n in ((q, "q"), (k, "k")):
        _chk(t, n)
        assert t.dim() == 2 and t.dtype == q.dtype
    _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32), _chk(map_off, "map_off", torch.int64)
    _chk(lse, "lse", torch.float32), _chk(head_w, "head_w", torch.float32), _chk(out, "out", torch.float32)
    B = cu_q.numel() - 1
    assert cu_k.numel() == B + 1 and map_off.numel() == B and map_off.is_contiguous()
    assert lse.is_contiguous() and lse.numel() == H * q.shape[0], "lse must be the [H][total_q] buffer of the same q"
    assert head_w.is_contiguous() and head_w.numel() == H and out.is_contiguous() and out.dim() == 1
    assert q.shape[1] >= H * dh and k.shape[1] >= H * dh
    _lib.check(_lib.lib().acai_attn_probs_mean(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), cu_q.data_ptr(), cu_k.data_ptr(), B, H, dh,
                                               int(max_q), int(max_k), _dt(q), lse.data_ptr(), q.shape[0], head_w.data_ptr(), map_off.data_ptr(),
                                               out.data_ptr(), 1 if accumulate else 0, _st()), "acai_attn_probs_mean")
    return out


def attn_map_locate(maps, map_off, cu_q, cu_k, grid_w, max_q, total_q):
    """Every row of the maps of attn_probs_mean -> (patch [total_q] int32, loc [total_q, 6] fp32: row sum, peak, centroid x, y, spread x, y
    in patch units) in one launch (acai_attn_map_locate).  grid_w: the images' patches per row, a host list of ints."""
    _chk(maps, "maps", torch.float32), _chk(map_off, "map_off", torch.int64), _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32)
    B = cu_q.numel() - 1
    assert maps.is_contiguous() and maps.dim() == 1 and map_off.numel() == B and cu_k.numel() == B + 1 and len(grid_w) == B
    gw = (ctypes.c_int32 * B)(*[int(w) for w in grid_w])
    patch = torch.empty(total_q, dtype=torch.int32, device=maps.device)
    loc = torch.empty(total_q, 6, dtype=torch.float32, device=maps.device)
    _lib.check(_lib.lib().acai_attn_map_locate(maps.data_ptr(), map_off.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), gw, B, int(max_q),
                                               patch.data_ptr(), loc.data_ptr(), _st()), "acai_attn_map_locate")
    return patch, loc


CONFIDENCE_MAX_K = 8
_WSUM_ROWS = 32   # tokens per split of acai_attn_map_weighted_sum (confidence.hip, WS_ROWS)


def token_confidence(logits, chosen, top_k=5, temperature=1.0):
    """Per-row confidence statistics in one launch (acai_token_confidence).  logits (N, V) fp32 contiguous and chosen (N,) integer ids on the
    GPU, 1 <= top_k <= min(8, V), temperature > 0 -> (log_prob (N,) fp32, entropy (N,) fp32 in nats, rank (N,) int32, top_ids (N, top_k) int32,
    top_log_probs (N, top_k) fp32) of softmax(logits / temperature): the chosen token's log-probability, the row's entropy, how many tokens
    come before the chosen one in the row's order (raw logit descending, then index ascending; 0 = the arg-max) and the first top_k tokens of
    that order.  -inf logits are allowed (log-probability -inf, ordered last by index); a row without a finite maximum or with a NaN is
    outside the contract.  Everything is checked on the host before the launch - ValueError (RuntimeError for CPU tensors, as every op); a
    chosen id outside [0, V) costs one device-to-host read.  N = 0 returns empty tensors without a launch."""
    _chk(logits, "logits"), _chk(chosen, "chosen")
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError(f"logits must be a contiguous (N, V) float32 tensor, got {tuple(logits.shape)} {logits.dtype} strides {logits.stride()}")
    N, V = logits.shape
    if chosen.dim() != 1 or chosen.shape[0] != N or chosen.dtype.is_floating_point or chosen.dtype.is_complex or chosen.dtype == torch.bool:
        raise ValueError(f"chosen must be {N} integer token ids, got {tuple(chosen.shape)} {chosen.dtype}")
    if chosen.device != logits.device:
        raise ValueError(f"chosen is on {chosen.device}, logits on {logits.device}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(CONFIDENCE_MAX_K, max(V, 1)) or V < 1:
        raise ValueError(f"top_k must be an int with 1 <= top_k <= min({CONFIDENCE_MAX_K}, V={V}), got {top_k!r}")
    try:
        tau = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a positive number, got {temperature!r}") from None
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
    dev = logits.device
    log_prob, entropy = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    rank = torch.empty(N, dtype=torch.int32, device=dev)
    top_ids, top_lp = torch.empty(N, top_k, dtype=torch.int32, device=dev), torch.empty(N, top_k, dtype=torch.float32, device=dev)
    if N == 0:
        return log_prob, entropy, rank, top_ids, top_lp
    chosen = chosen.to(torch.int64).contiguous()
    lo, hi = (int(x) for x in torch.stack([chosen.min(), chosen.max()]).tolist())   # the kernel reads logits[r, chosen[r]]
    if lo < 0 or hi >= V:
        raise ValueError(f"chosen holds a token id outside [0, {V}) (smallest {lo}, largest {hi})")
    _lib.check(_lib.lib().acai_token_confidence(logits.data_ptr(), chosen.data_ptr(), N, V, top_k, tau, log_prob.data_ptr(), entropy.data_ptr(),
                                                rank.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(), _st()), "acai_token_confidence")
    return log_prob, entropy, rank, top_ids, top_lp


def attn_map_weighted_sum(maps, map_off, cu_q, cu_k, weights, max_q, layout=None):
    """The maps of attn_probs_mean summed over the token axis, one weight per token (acai_attn_map_weighted_sum): maps (flat fp32 buffer),
    map_off [B] int64, cu_q / cu_k [B + 1] int32 as attn_probs_mean takes them, weights (sum T,) fp32 packed like the tokens, max_q >= every
    T_b -> (sum S,) fp32 packed like the patches, heat_b[s] = sum_t weights_b[t] * map_b[t, s].  The same bits on every run.  The layout
    is checked on the host (ValueError): every block lies inside `maps`, weights has sum T entries.  layout: the host lists (lens_q, lens_k,
    offsets) that cu_q, cu_k and map_off were built from, when the caller still has them; without it they are read back from the device once."""
    _chk(maps, "maps", torch.float32), _chk(map_off, "map_off", torch.int64), _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32)
    _chk(weights, "weights", torch.float32)
    B = cu_q.numel() - 1
    if B < 1 or cu_k.numel() != B + 1 or map_off.numel() != B or maps.dim() != 1 or weights.dim() != 1:
        raise ValueError(f"attn_map_weighted_sum: {B} images need cu_q / cu_k of {B + 1} entries, map_off of {B}, flat maps and weights")
    if not (maps.is_contiguous() and weights.is_contiguous() and map_off.is_contiguous() and cu_q.is_contiguous() and cu_k.is_contiguous()):
        raise ValueError("attn_map_weighted_sum: operands must be contiguous")
    if layout is None:
        host = torch.cat([cu_q.long(), cu_k.long(), map_off]).tolist()
        hq, hk, ho = host[:B + 1], host[B + 1:2 * B + 2], host[2 * B + 2:]
        lens_q, lens_k = [b - a for a, b in zip(hq, hq[1:])], [b - a for a, b in zip(hk, hk[1:])]
    else:
        lens_q, lens_k, ho = ([int(v) for v in x] for x in layout)
        if not len(lens_q) == len(lens_k) == len(ho) == B:
            raise ValueError(f"attn_map_weighted_sum: layout must hold {B} query lengths, key lengths and offsets")
        hq, hk = [0], [0]
        for t, k in zip(lens_q, lens_k):
            hq.append(hq[-1] + t), hk.append(hk[-1] + k)
    if hq[0] != 0 or hk[0] != 0 or min(lens_q) < 0 or min(lens_k) < 1:
        raise ValueError(f"attn_map_weighted_sum: bad cumulative lengths cu_q={hq} cu_k={hk}")
    if weights.numel() != hq[-1]:
        raise ValueError(f"attn_map_weighted_sum: weights holds {weights.numel()} entries for {hq[-1]} tokens")
    if int(max_q) < max(max(lens_q), 1):
        raise ValueError(f"attn_map_weighted_sum: max_q={max_q} is smaller than the longest sequence ({max(lens_q)})")
    for b, (o, t, s) in enumerate(zip(ho, lens_q, lens_k)):
        if o < 0 or o + t * s > maps.numel():
            raise ValueError(f"attn_map_weighted_sum: image {b}'s [{t}][{s}] block at offset {o} lies outside the {maps.numel()} map elements")
    total_k, nsplit = hk[-1], -(-int(max_q) // _WSUM_ROWS)
    out = torch.empty(total_k, dtype=torch.float32, device=maps.device)
    partial = torch.empty(nsplit * total_k, dtype=torch.float32, device=maps.device) if nsplit > 1 else None
    _lib.check(_lib.lib().acai_attn_map_weighted_sum(maps.data_ptr(), map_off.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), weights.data_ptr(), B,
                                                     int(max_q), max(lens_k), total_k, _p(partial), out.data_ptr(), _st()),
               "acai_attn_map_weighted_sum")
    return out


SEGMENT_MAX_DELIMS, SEGMENT_MAX_PLANES = 8, 8     # measures.hip: SEG_MAX_DELIMS, RED_MAX_K
EXTENT_MAX_IMAGES, EXTENT_MAX_SIDE = 512, 4096    # measures.hip: EXT_MAX_B, EXT_MAX_SIDE


class SegmentStats(NamedTuple):
    """What segment_reduce returns for K planes, R rows and `cap` segment slots, each (K, R, cap): sum, min, max fp32 and argmin, argmax int32
    (token indices within the row, the lowest on ties); 0 and -1 in the slots past a row's count."""
    sum: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    argmin: torch.Tensor
    argmax: torch.Tensor


def _seg_outputs(who, out, shapes, dev):
    """The output tensors of a segment op: allocated, or the caller's `out` checked against (shape, dtype) one by one."""
    if out is None:
        return tuple(torch.empty(s, dtype=d, device=dev) for s, d in shapes)
    out = tuple(out)
    if len(out) != len(shapes):
        raise ValueError(f"{who}: out must hold {len(shapes)} tensors, got {len(out)}")
    for i, (t, (s, d)) in enumerate(zip(out, shapes)):
        _chk(t, f"{who}: out[{i}]", d)
        if tuple(t.shape) != tuple(s) or not t.is_contiguous():
            raise ValueError(f"{who}: out[{i}] must be a contiguous {tuple(s)} tensor, got {tuple(t.shape)}")
        if t.device != dev:
            raise RuntimeError(f"{who}: operands on different devices ({dev} and {t.device})")
    return out


@_on_operand_device
def token_segments(tokens, lens, delims, stop=-1, cap=256, out=None):
    """Token rows cut at delimiter tokens (acai_token_segments; one launch) -> (seg (R, ld) int32, count (R,) int32, bounds (R, cap, 2) int32).
    tokens (R, ld) int64 on the GPU, ld >= 1; lens: int32 lengths (R,) or a bool prefix mask of tokens' shape, read on the device and clamped
    to [0, ld] (no host sync); delims: 1 .. 8 token ids; stop: the <eos> id, or -1 for none; cap >= 1 segment slots per row.  A row ends at E,
    its first `stop` (or its length); seg[r, p] is the number of delimiters at indices <= p minus one for p < E - so -1 before the first
    delimiter - and -1 from E on; count[r] is the TRUE number of segments, also beyond cap; bounds[r, m] = (index of the m-th delimiter,
    index of the next one or E) for m < min(count, cap), (-1, -1) beyond.  ValueError for bad shapes or arguments, RuntimeError for CPU
    tensors.  With int32 lengths and `out` (the three tensors) given, the call is one kernel launch and nothing else."""
    _chk(tokens, "tokens", torch.int64), _chk(lens, "lens")
    if tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError(f"token_segments: tokens must be (rows, ld >= 1), got {tuple(tokens.shape)}")
    R, ld = tokens.shape
    if lens.dtype == torch.bool:
        if lens.shape != tokens.shape:
            raise ValueError(f"token_segments: a mask must have tokens' shape {tuple(tokens.shape)}, got {tuple(lens.shape)}")
        lens = lens.sum(dim=-1, dtype=torch.int32)
    elif lens.dtype != torch.int32:
        raise TypeError(f"token_segments: expected int32 lengths or a bool mask, got {lens.dtype}")
    if lens.shape != (R,):
        raise ValueError(f"token_segments: expected {R} lengths, got {tuple(lens.shape)}")
    try:
        ids = [int(d) for d in delims]
    except (TypeError, ValueError):
        raise ValueError(f"token_segments: delims must be 1 .. {SEGMENT_MAX_DELIMS} token ids, got {delims!r}") from None
    if not 1 <= len(ids) <= SEGMENT_MAX_DELIMS or min(ids) < 0:
        raise ValueError(f"token_segments: delims must be 1 .. {SEGMENT_MAX_DELIMS} non-negative token ids, got {ids}")
    stop, cap = int(stop), int(cap)
    if stop < -1 or cap < 1:
        raise ValueError(f"token_segments: stop={stop} (an id, or -1 for none) and cap={cap} (at least 1)")
    if lens.device != tokens.device:
        raise RuntimeError(f"token_segments: operands on different devices ({tokens.device} and {lens.device})")
    seg, count, bounds = _seg_outputs("token_segments", out, (((R, ld), torch.int32), ((R,), torch.int32), ((R, cap, 2), torch.int32)),
                                      tokens.device)
    if R == 0:
        return seg, count, bounds
    tokens, lens = tokens.contiguous(), lens.contiguous()
    _lib.check(_lib.lib().acai_token_segments(tokens.data_ptr(), ld, lens.data_ptr(), R, (ctypes.c_int64 * len(ids))(*ids), len(ids), stop, cap,
                                              seg.data_ptr(), count.data_ptr(), bounds.data_ptr(), _st(tokens)), "acai_token_segments")
    return seg, count, bounds


@_on_operand_device
def segment_reduce(values, bounds, count, out=None):
    """Per-token values reduced over the spans of token_segments (acai_segment_reduce; one launch) -> SegmentStats.  values (K, R, ld) fp32 with
    1 <= K <= 8 planes, bounds (R, cap, 2) and count (R,) int32 as token_segments returns them, all on the GPU.  Every output is (K, R, cap):
    sum, min, max, and argmin / argmax as token indices within the row (the lowest on ties); slots past min(count, cap) hold 0 and -1.  Lane
    j of a wave adds the span's elements j, j + 64, ... in order, then a fixed butterfly: the same bits on every run, and exact for values
    whose partial sums fp32 holds (0/1 planes).  A NaN inside a span is outside the contract.  ValueError for bad shapes, RuntimeError for
    CPU tensors.  With `out` (five tensors) given, the call is one kernel launch and nothing else."""
    _chk(values, "values", torch.float32), _chk(bounds, "bounds", torch.int32), _chk(count, "count", torch.int32)
    if values.dim() != 3 or not 1 <= values.shape[0] <= SEGMENT_MAX_PLANES or values.shape[2] < 1:
        raise ValueError(f"segment_reduce: values must be (1 .. {SEGMENT_MAX_PLANES} planes, rows, ld >= 1), got {tuple(values.shape)}")
    K, R, ld = values.shape
    if bounds.dim() != 3 or bounds.shape[0] != R or bounds.shape[1] < 1 or bounds.shape[2] != 2 or count.shape != (R,):
        raise ValueError(f"segment_reduce: {R} rows need bounds ({R}, cap >= 1, 2) and count ({R},), got {tuple(bounds.shape)} and "
                         f"{tuple(count.shape)}")
    cap = bounds.shape[1]
    if K * R * cap >= 2 ** 31:
        raise ValueError(f"segment_reduce: {K} x {R} x {cap} spans are too many")
    for t in (bounds, count):
        if t.device != values.device:
            raise RuntimeError(f"segment_reduce: operands on different devices ({values.device} and {t.device})")
    f32, i32 = torch.float32, torch.int32
    out = SegmentStats(*_seg_outputs("segment_reduce", out, [((K, R, cap), d) for d in (f32, f32, f32, i32, i32)], values.device))
    if R == 0:
        return out
    values, bounds, count = values.contiguous(), bounds.contiguous(), count.contiguous()
    _lib.check(_lib.lib().acai_segment_reduce(values.data_ptr(), K, R, ld, bounds.data_ptr(), count.data_ptr(), cap, *(t.data_ptr() for t in out),
                                              _st(values)), "acai_segment_reduce")
    return out


def _map_layout_host(who, maps, map_off, cu_q, cu_k, layout):
    """(lens_q, lens_k, offsets) of a flat map buffer as host lists, checked: from `layout`, or read back from the device once."""
    B = cu_q.numel() - 1
    if B < 1 or cu_k.numel() != B + 1 or map_off.numel() != B or maps.dim() != 1:
        raise ValueError(f"{who}: {B} images need cu_q / cu_k of {B + 1} entries, map_off of {B} and flat maps")
    if not (maps.is_contiguous() and map_off.is_contiguous() and cu_q.is_contiguous() and cu_k.is_contiguous()):
        raise ValueError(f"{who}: operands must be contiguous")
    if layout is None:
        host = torch.cat([cu_q.long(), cu_k.long(), map_off]).tolist()
        hq, hk, ho = host[:B + 1], host[B + 1:2 * B + 2], host[2 * B + 2:]
        if hq[0] != 0 or hk[0] != 0:
            raise ValueError(f"{who}: bad cumulative lengths cu_q={hq} cu_k={hk}")
        lens_q, lens_k = [b - a for a, b in zip(hq, hq[1:])], [b - a for a, b in zip(hk, hk[1:])]
    else:
        lens_q, lens_k, ho = ([int(v) for v in x] for x in layout)
        if not len(lens_q) == len(lens_k) == len(ho) == B:
            raise ValueError(f"{who}: layout must hold {B} query lengths, key lengths and offsets")
    if min(lens_q) < 0 or min(lens_k) < 1:
        raise ValueError(f"{who}: bad lengths lens_q={lens_q} lens_k={lens_k}")
    for b, (o, t, s) in enumerate(zip(ho, lens_q, lens_k)):
        if o < 0 or o + t * s > maps.numel():
            raise ValueError(f"{who}: image {b}'s [{t}][{s}] block at offset {o} lies outside the {maps.numel()} map elements")
    return lens_q, lens_k, ho


@_on_operand_device
def attn_map_segment_sum(maps, map_off, cu_q, cu_k, weights, ranges, seg_counts, layout=None, check_ranges=True):
    """The maps of attn_probs_mean summed over ranges of map rows, one map per range (acai_attn_map_segment_sum; one launch): the segmented
    form of attn_map_weighted_sum.  maps / map_off / cu_q / cu_k / layout as there; weights (sum T,) fp32 packed like the tokens, or None for
    all ones (the same bits as a tensor of ones); ranges (sum n, 2) int32 on the GPU: per segment the half-open range [t0, t1) of map rows
    within its image's block, image after image (map row t belongs to token index t + 1: token_segments' bounds minus one); seg_counts: the
    images' segment counts n_b, a host list.  -> (out, offsets list, offsets as an int64 device tensor, cu_seg int32 device tensor): image b
    owns the dense [n_b][S_b] block at offsets[b] of the flat fp32 `out` - attn_map_layout(seg_counts, lens_k) - with out_b[m, s] = sum over
    the range's rows t, ascending, of weights_b[t] * map_b[t, s]; attn_map_locate, attn_map_expand and attn_map_extent take it with cu_seg in
    the place of cu_q.  The same bits on every run.  check_ranges reads the ranges back once and refuses (ValueError) an empty one or one
    outside [0, T_b]; without it the kernel clamps them to the block (callers that built them on the device from token_segments)."""
    who = "attn_map_segment_sum"
    _chk(maps, "maps", torch.float32), _chk(map_off, "map_off", torch.int64), _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32)
    _chk(ranges, "ranges", torch.int32)
    if weights is not None:
        _chk(weights, "weights", torch.float32)
    lens_q, lens_k, _ = _map_layout_host(who, maps, map_off, cu_q, cu_k, layout)
    B = len(lens_q)
    try:
        counts = [int(n) for n in seg_counts]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: seg_counts must be a list of {B} segment counts, got {seg_counts!r}") from None
    if len(counts) != B or min(counts) < 0 or max(counts) > 65535 or B > 65535:
        raise ValueError(f"{who}: seg_counts must hold {B} counts in [0, 65535], got {counts}")
    if ranges.dim() != 2 or tuple(ranges.shape) != (sum(counts), 2) or not ranges.is_contiguous():
        raise ValueError(f"{who}: ranges must be a contiguous ({sum(counts)}, 2) tensor for segment counts {counts}, got {tuple(ranges.shape)}")
    if weights is not None and (weights.dim() != 1 or weights.numel() != sum(lens_q) or not weights.is_contiguous()):
        raise ValueError(f"{who}: weights holds {weights.numel()} entries for {sum(lens_q)} tokens")
    for t in (map_off, cu_q, cu_k, ranges, weights):
        if t is not None and t.device != maps.device:
            raise RuntimeError(f"{who}: operands on different devices ({maps.device} and {t.device})")
    if check_ranges and sum(counts):
        host, g = ranges.tolist(), 0
        for b, (n, T) in enumerate(zip(counts, lens_q)):
            for t0, t1 in host[g:g + n]:
                if not 0 <= t0 < t1 <= T:
                    raise ValueError(f"{who}: image {b} has the range [{t0}, {t1}) - empty or outside its {T} map rows")
            g += n
    dev = maps.device
    offs, total = attn_map_layout(counts, lens_k)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    # (both tables go up as one tensor: the int64 offsets first, viewed as int32 pairs, then the cumulative counts)
    both = h2d(torch.cat([torch.tensor(offs, dtype=torch.int64).view(torch.int32), torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32)]),
               dev)
    seg_off, tab = both[:2 * B].view(torch.int64), both[2 * B:]
    if total:
        _lib.check(_lib.lib().acai_attn_map_segment_sum(maps.data_ptr(), map_off.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), _p(weights),
                                                        ranges.data_ptr(), tab.data_ptr(), seg_off.data_ptr(), B, max(lens_k), max(counts),
                                                        out.data_ptr(), _st(maps)), "acai_attn_map_segment_sum")
    return out, offs, seg_off, tab


@_on_operand_device
def attn_map_extent(maps, map_off, cu_q, cu_k, grid_w, q, layout=None):
    """A quantile box for every row of the maps of attn_probs_mean or attn_map_segment_sum (acai_attn_map_extent; one launch) -> (sum T, 4)
    fp32 (x0, y0, x1, y1) in patch units.  maps / map_off / cu_q / cu_k / layout as attn_map_weighted_sum takes them (for segment maps: cu_seg
    in the place of cu_q); grid_w: the images' patches per row, a host list of ints in 1 .. 4096; 0 <= q < 0.5.  With the row's column
    marginal a[x], its running sums C and its mass m, x0 is where C crosses q * m and x1 where it crosses (1 - q) * m, interpolated inside
    the cell (include/acai_omr_hip.h states the rule); y0, y1 the same over the grid rows, of which the last may be partial.  A row without
    mass gives zeros.  ValueError for a grid side above 4096, more than 512 images, grid_w < 1 or q outside [0, 0.5)."""
    who = "attn_map_extent"
    _chk(maps, "maps", torch.float32), _chk(map_off, "map_off", torch.int64), _chk(cu_q, "cu_q", torch.int32), _chk(cu_k, "cu_k", torch.int32)
    lens_q, lens_k, _ = _map_layout_host(who, maps, map_off, cu_q, cu_k, layout)
    B = len(lens_q)
    try:
        gw, q = [int(w) for w in grid_w], float(q)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: grid_w must be a list of ints and q a number, got {grid_w!r} and {q!r}") from None
    if len(gw) != B or B > EXTENT_MAX_IMAGES:
        raise ValueError(f"{who}: {len(gw)} grid widths for {B} images (at most {EXTENT_MAX_IMAGES})")
    if not 0.0 <= q < 0.5:
        raise ValueError(f"{who}: q must satisfy 0 <= q < 0.5, got {q}")
    for b, (w, s) in enumerate(zip(gw, lens_k)):
        if not 1 <= w <= EXTENT_MAX_SIDE or -(-s // w) > EXTENT_MAX_SIDE:
            raise ValueError(f"{who}: image {b} has {s} patches in rows of {w}: both grid sides must lie in 1 .. {EXTENT_MAX_SIDE}")
    for t in (map_off, cu_q, cu_k):
        if t.device != maps.device:
            raise RuntimeError(f"{who}: operands on different devices ({maps.device} and {t.device})")
    ext = torch.empty(sum(lens_q), 4, dtype=torch.float32, device=maps.device)
    if sum(lens_q):
        _lib.check(_lib.lib().acai_attn_map_extent(maps.data_ptr(), map_off.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(),
                                                   (ctypes.c_int32 * B)(*gw), B, max(lens_q), q, ext.data_ptr(), _st(maps)), "acai_attn_map_extent")
    return ext


PRUNE_MAX_HALO, PRUNE_MAX_GRID, PRUNE_MAX_IMAGES = _lib.PRUNE_MAX_HALO, _lib.PRUNE_MAX_GRID, _lib.PRUNE_MAX_IMAGES


def _patch_stream(patches, name):
    """A packed patch stream [M, L]: fp32 or bf16 on the GPU, rows contiguous, any row pitch and any base (a view of a larger stream)."""
    _chk(patches, name)
    if patches.dim() != 2 or patches.shape[1] < 1 or patches.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{name}: expected a [M, L] float32 or bfloat16 tensor with L >= 1, got {tuple(patches.shape)} {patches.dtype}")
    return patches


def prune_table(dims, pe_grid, device):
    """The device table of patch_keep / patch_compact for images of patch grids dims = [(h_p, w_p), ...] that lie back to back in a patch
    stream, with the positional table of pe_grid = (pe_max_height, pe_max_width) rows by columns: int32 [B, 8] (include/acai_omr_hip.h).
    An image whose grid exceeds the table gathers from its own (h_p, w_p) grid appended behind the table, in image order, as
    Encoder._pe_packed appends the interpolated grids.  -> (table, rows of the stream, the largest grid).  ValueError beyond the limits."""
    dims = [(int(h), int(w)) for h, w in dims]
    pe_h, pe_w = (int(v) for v in pe_grid)
    if len(dims) > PRUNE_MAX_IMAGES:
        raise ValueError(f"{len(dims)} images in one pruning call (at most {PRUNE_MAX_IMAGES})")
    rows, off, base = [], 0, pe_h * pe_w
    for h, w in dims:
        if h < 1 or w < 1 or h * w > PRUNE_MAX_GRID:
            raise ValueError(f"a grid of {h} x {w} patches: both sides must be at least 1 and the grid at most {PRUNE_MAX_GRID} patches")
        if h > pe_h or w > pe_w:
            rows.append((h, w, off, base, w, 0, 0, 0))
            base += h * w
        else:
            rows.append((h, w, off, 0, pe_w, 0, 0, 0))
        off += h * w
    if off >= 2 ** 31 or base >= 2 ** 31:
        raise ValueError(f"{off} patch rows do not fit 32-bit row indices")
    table = h2d(torch.tensor(rows, dtype=torch.int32).reshape(len(dims), _lib.PRUNE_TABLE_COLS), device)
    return table, off, max((h * w for h, w in dims), default=0)


@_on_operand_device
def patch_ink(patches, ink_level=0.5, out=None):
    """ink [M] int32: per row of the packed patch stream, the number of elements strictly below ink_level, compared on the stored value
    widened to fp32 (acai_patch_ink; one launch, none for M = 0)."""
    _patch_stream(patches, "patches")
    level = float(ink_level)
    if level != level:
        raise ValueError("ink_level is NaN")
    M, L = patches.shape
    if out is None:
        out = torch.empty(M, dtype=torch.int32, device=patches.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == M and out.device == patches.device
    _lib.check(_lib.lib().acai_patch_ink(patches.data_ptr(), _dt(patches), M, L, _ld(patches), level, out.data_ptr(), _st()), "acai_patch_ink")
    return out


@_on_operand_device
def patch_keep(ink, table, max_grid, max_ink=0, halo=1):
    """The keep rule on the ink counts of a stream of images (acai_patch_keep; one launch, one workgroup per image): a patch is inked when
    its count exceeds max_ink, and kept when an inked patch of its own image lies within Chebyshev distance halo; an image without an
    inked patch keeps all.  table: prune_table's.  -> (kept_local [M] int32 - image i's kept local indices r * w_p + c, ascending, from its
    first row on; the rest of its slot is not written -, count [B] int32), both on the device."""
    _chk(ink, "ink", torch.int32), _chk(table, "table", torch.int32)
    if isinstance(halo, bool) or not isinstance(halo, int) or not 0 <= halo <= PRUNE_MAX_HALO:
        raise ValueError(f"halo must be an int in 0 .. {PRUNE_MAX_HALO}, got {halo!r}")
    if isinstance(max_ink, bool) or not isinstance(max_ink, int) or max_ink < 0:
        raise ValueError(f"max_ink must be a non-negative int, got {max_ink!r}")
    if table.dim() != 2 or table.shape[1] != _lib.PRUNE_TABLE_COLS or not table.is_contiguous() or ink.dim() != 1 or not ink.is_contiguous():
        raise ValueError(f"patch_keep: ink must be a contiguous [M] tensor and table a contiguous [B, {_lib.PRUNE_TABLE_COLS}] one")
    B = table.shape[0]
    if B > PRUNE_MAX_IMAGES or not 0 <= int(max_grid) <= PRUNE_MAX_GRID:
        raise ValueError(f"patch_keep: {B} images (at most {PRUNE_MAX_IMAGES}), largest grid {max_grid} (at most {PRUNE_MAX_GRID})")
    kept_local = torch.empty(ink.numel(), dtype=torch.int32, device=ink.device)
    count = torch.empty(B, dtype=torch.int32, device=ink.device)
    _lib.check(_lib.lib().acai_patch_keep(ink.data_ptr(), table.data_ptr(), B, int(max_grid), max_ink, halo, kept_local.data_ptr(), count.data_ptr(),
                                          _st()), "acai_patch_keep")
    return kept_local, count


@_on_operand_device
def patch_compact(patches, table, kept_local, counts):
    """The kept rows as a stream of their own (acai_patch_compact; one launch, none when nothing is kept).  counts: patch_keep's count as a
    HOST list - reading it is the one device-to-host copy of the stage.  -> (out [sum counts, L] in the input's dtype, the kept rows bit
    for bit; kept [sum counts] int32, the packed local indices; pe_idx [sum counts] int32, the rows of the positional table)."""
    _patch_stream(patches, "patches"), _chk(table, "table", torch.int32), _chk(kept_local, "kept_local", torch.int32)
    counts = [int(c) for c in counts]
    B, (M, L) = table.shape[0], patches.shape
    if len(counts) != B or kept_local.numel() != M or not kept_local.is_contiguous() or not table.is_contiguous() or min(counts, default=0) < 0:
        raise ValueError(f"patch_compact: {len(counts)} counts for {B} images, {kept_local.numel()} kept slots for {M} rows")
    total = sum(counts)
    if total > M:
        raise ValueError(f"patch_compact: {total} kept rows of a stream of {M}")
    dev = patches.device
    out = torch.empty(total, L, dtype=patches.dtype, device=dev)
    kept, pe_idx = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    if total == 0:
        return out, kept, pe_idx
    cu = [0]
    for c in counts:
        cu.append(cu[-1] + c)
    cu_out = h2d(torch.tensor(cu, dtype=torch.int32), dev)
    _lib.check(_lib.lib().acai_patch_compact(patches.data_ptr(), _dt(patches), L, _ld(patches), table.data_ptr(), kept_local.data_ptr(),
                                             cu_out.data_ptr(), B, total, out.data_ptr(), kept.data_ptr(), pe_idx.data_ptr(), _st()),
               "acai_patch_compact")
    return out, kept, pe_idx


@_on_operand_device
def attn_map_expand(maps, lens_q, kept_lens, full_lens, kept, offs=None):
    """Per-token maps over kept patches -> over the full grids (acai_attn_map_expand; one launch plus the zero fill).  maps: the flat fp32
    buffer of attn_probs_mean with image b's [T_b][K_b] block at offs[b] (default: attn_map_layout(lens_q, kept_lens)); kept: the packed
    int32 local indices of the kept patches, K_b per image, each below S_b = full_lens[b].  -> (out, offsets list, offsets as an int64 device
    tensor) with image b's [T_b][S_b] block at the offsets of attn_map_layout(lens_q, full_lens): out_b[t, kept_b[j]] = maps_b[t, j], every
    other element 0."""
    _chk(maps, "maps", torch.float32), _chk(kept, "kept", torch.int32)
    lens_q, kept_lens, full_lens = ([int(v) for v in x] for x in (lens_q, kept_lens, full_lens))
    B = len(lens_q)
    if not (len(kept_lens) == len(full_lens) == B) or B > PRUNE_MAX_IMAGES or maps.dim() != 1 or kept.dim() != 1:
        raise ValueError(f"attn_map_expand: {B} token lengths, {len(kept_lens)} kept and {len(full_lens)} full lengths; flat maps and kept")
    if not (maps.is_contiguous() and kept.is_contiguous()) or kept.numel() != sum(kept_lens):
        raise ValueError(f"attn_map_expand: kept holds {kept.numel()} indices for kept lengths summing to {sum(kept_lens)}")
    if any(t < 0 or k < 0 or k > s for t, k, s in zip(lens_q, kept_lens, full_lens)) or max(lens_q, default=0) > 65535:
        raise ValueError(f"attn_map_expand: bad lengths lens_q={lens_q} kept_lens={kept_lens} full_lens={full_lens}")
    in_offs = attn_map_layout(lens_q, kept_lens)[0] if offs is None else [int(o) for o in offs]
    for o, t, k in zip(in_offs, lens_q, kept_lens):
        if o < 0 or o + t * k > maps.numel():
            raise ValueError(f"attn_map_expand: a [{t}][{k}] block at offset {o} lies outside the {maps.numel()} map elements")
    out_offs, total = attn_map_layout(lens_q, full_lens)
    dev = maps.device
    out = torch.zeros(total, dtype=torch.float32, device=dev)
    out_off = h2d(torch.tensor(out_offs, dtype=torch.int64), dev)
    if B and max(lens_q) and max(kept_lens):
        # (the three cumulative length tables, [B + 1] each, go up as one tensor)
        cus = [[0] + list(itertools.accumulate(lens)) for lens in (lens_q, kept_lens, full_lens)]
        cu = h2d(torch.tensor(cus, dtype=torch.int32), dev)
        in_off = h2d(torch.tensor(in_offs, dtype=torch.int64), dev)
        _lib.check(_lib.lib().acai_attn_map_expand(maps.data_ptr(), in_off.data_ptr(), out.data_ptr(), out_off.data_ptr(), cu[0].data_ptr(),
                                                   cu[1].data_ptr(), cu[2].data_ptr(), kept.data_ptr(), B, max(lens_q), max(kept_lens), _st()),
                   "acai_attn_map_expand")
    return out, out_offs, out_off


def cross_kv_prefill(mem, w_kv, b_kv, row_seq, row_pos, seq_off, seq_len, k_out, v_out, H, dh, dhp, round_bf16=False):
    _chk(mem, "mem"), _chk(w_kv, "w_kv")
    M, E = mem.shape
    assert w_kv.shape == (2 * E, E) and mem.dtype == w_kv.dtype == k_out.dtype == v_out.dtype
    assert row_seq.dtype == torch.int32 and row_pos.dtype == torch.int32 and seq_off.dtype == torch.int64 and seq_len.dtype == torch.int32
    assert row_seq.numel() == M and row_pos.numel() == M
    _lib.check(_lib.lib().acai_cross_kv_prefill(mem.data_ptr(), mem.stride(0), w_kv.data_ptr(), w_kv.stride(0), _p(b_kv), row_seq.data_ptr(),
                                                row_pos.data_ptr(), seq_off.data_ptr(), seq_len.data_ptr(), k_out.data_ptr(), v_out.data_ptr(),
                                                M, E, H, dh, dhp, _dt(mem), GEMM_ROUND_BF16 if round_bf16 else 0, _st()), "acai_cross_kv_prefill")


def cross_kv_quantize_fp8(k_in, v_in, k_out, v_out, k_scale, v_scale, row0, nrows, dhp):
    """FP8 memory cache prefill: rows row0 .. row0+nrows-1 (dhp elements each) of the bf16 cross K/V k_in / v_in -> e4m3fn rows of k_out /
    v_out and their fp32 power-of-two scales k_scale[row] / v_scale[row] (the format of acai_omr_amd.fp8.quantize_rows)."""
    for t, n in ((k_in, "k_in"), (v_in, "v_in")):
        _chk(t, n, torch.bfloat16)
    for t, n in ((k_out, "k_out"), (v_out, "v_out")):
        _chk(t, n, torch.float8_e4m3fn)
    for t, n in ((k_scale, "k_scale"), (v_scale, "v_scale")):
        _chk(t, n, torch.float32)
    end = (int(row0) + int(nrows)) * dhp
    assert all(t.is_contiguous() and t.numel() >= end for t in (k_in, v_in, k_out, v_out)), "row range beyond a K/V buffer"
    assert k_scale.numel() >= end // dhp and v_scale.numel() >= end // dhp, "row range beyond a scale buffer"
    _lib.check(_lib.lib().acai_cross_kv_quantize_fp8(k_in.data_ptr(), v_in.data_ptr(), k_out.data_ptr(), v_out.data_ptr(), k_scale.data_ptr(),
                                                     v_scale.data_ptr(), int(row0), int(nrows), int(dhp), _st()), "acai_cross_kv_quantize_fp8")


def slot_flush_views(buf, B, ld):
    """(hdr int32 (B, 4), out_tok int32 (B, ld), out_lp fp32 (B, ld)) as views of the first B * (4 + 2 ld) entries of the flat int32 `buf`,
    device or host: the layout `slot_flush` writes and the engine copies in one piece.  The header leads, so every part starts on a
    16-byte boundary of the allocation whenever B * ld is a multiple of 4, and on a 4-byte one always (the kernel stores dwords)."""
    B, ld = int(B), int(ld)
    if buf.dtype != torch.int32 or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() < B * (4 + 2 * ld):
        raise ValueError(f"slot_flush: the buffer must be flat contiguous int32 of at least B * (4 + 2 ld) = {B * (4 + 2 * ld)} entries")
    return (buf[:4 * B].view(B, 4), buf[4 * B:4 * B + B * ld].view(B, ld), buf[4 * B + B * ld:4 * B + 2 * B * ld].view(torch.float32).view(B, ld))


@_on_operand_device
def slot_flush(seqs, logprobs, slot_t, finished, mark, B, ld, buf=None):
    """What slots 0 .. B-1 of a slot-mode run wrote since `mark` (acai_decode_slot_flush; the numpy statement is
    tests/stream_reference.flush_reference): per slot, end = t + 1 if finished else t, n = clamp(end - mark, 0, ld), the n tokens (as
    int32) and log-probs from index mark, the header (n, mark before, finished, 0), then mark += n.  seqs int64 / logprobs fp32
    (rows, pitch), slot_t / finished / mark int32 (>= B entries; the fewest rows any of the five has is the `rows` the call is checked
    against).  buf: flat int32 of B * (4 + 2 ld) entries that receives everything (allocated when None; entries past a slot's n keep what
    they held).  Returns
    (hdr, out_tok, out_lp), `slot_flush_views` of buf.  The C ABI refuses a null operand (None here), ld < 1, ld > pitch and fewer than B
    rows (RuntimeError); nothing is launched then."""
    B, ld = int(B), int(ld)
    for t, n, dt in ((seqs, "seqs", torch.int64), (logprobs, "logprobs", torch.float32), (slot_t, "slot_t", torch.int32),
                     (finished, "finished", torch.int32), (mark, "mark", torch.int32)):
        if t is not None:
            _chk(t, n, dt)
            if not t.is_contiguous():
                raise ValueError(f"{n}: must be contiguous")
    pitch = 0 if seqs is None else seqs.shape[-1]
    if seqs is not None and logprobs is not None and (seqs.dim() != 2 or seqs.shape != logprobs.shape):
        raise ValueError(f"seqs / logprobs: expected two (rows, pitch) tensors of one shape, got {tuple(seqs.shape)} and {tuple(logprobs.shape)}")
    rows = min((t.shape[0] for t in (seqs, logprobs, slot_t, finished, mark) if t is not None), default=0)
    if buf is None:
        buf = torch.zeros(max(B, 1) * (4 + 2 * max(ld, 1)), dtype=torch.int32, device=mark.device if mark is not None else seqs.device)
    _chk(buf, "buf", torch.int32)
    hdr, out_tok, out_lp = slot_flush_views(buf, max(B, 1), max(ld, 1))
    _lib.check(_lib.lib().acai_decode_slot_flush(_p(seqs), _p(logprobs), pitch, _p(slot_t), _p(finished), _p(mark), rows, B, ld,
                                                 out_tok.data_ptr(), out_lp.data_ptr(), hdr.data_ptr(), _st()), "acai_decode_slot_flush")
    return hdr, out_tok, out_lp


def skinny_gemm(x, w, bias=None, residual=None, gelu=False, round_bf16=False, out=None):
    """x [B,K] fp32, w [N,K] fp32 or bf16 -> y [B,N] fp32."""
    _chk(x, "x", torch.float32), _chk(w, "w")
    B, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    flags = (GEMM_GELU if gelu else 0) | (GEMM_ROUND_BF16 if round_bf16 else 0)
    _lib.check(_lib.lib().acai_skinny_gemm(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), _p(bias), _p(residual),
                                           residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, N, K,
                                           _dt(w), flags, _st()), "acai_skinny_gemm")
    return out


def skinny_gemm_ex(x, w, bias=None, residual=None, gelu=False, round_bf16=False, out_dtype=torch.float32, ln=None, stats_out=None,
                   rln=None, rstats=None, ln_eps=1e-5):
    """Decode GEMV with its fusions: x [B,K] fp32 or bf16, w [N,K]; ln = (weight, bias) applied to x on load;
    rln = (weight, bias) + rstats [B,2] applied to the residual."""
    _chk(x, "x"), _chk(w, "w")
    B, K = x.shape
    N = w.shape[0]
    out = torch.empty(B, N, dtype=out_dtype, device=x.device)
    flags = (GEMM_GELU if gelu else 0) | (GEMM_ROUND_BF16 if round_bf16 else 0)
    _lib.check(_lib.lib().acai_skinny_gemm_ex(x.data_ptr(), x.stride(0), _dt(x), w.data_ptr(), w.stride(0), _p(bias), _p(residual),
                                              residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), _dt(out), B, N, K,
                                              _dt(w), flags, _p(ln[0]) if ln else None, _p(ln[1]) if ln else None, float(ln_eps), _p(stats_out),
                                              _p(rln[0]) if rln else None, _p(rln[1]) if rln else None, _p(rstats), _st()), "acai_skinny_gemm_ex")
    return out


def decode_attn(q, kc, vc, seq_off, seq_len, H, dh, dhp, max_len, round_out=False, chunk=256, fused_merge=False, k_scale=None, v_scale=None):
    """q [B, H*dh] fp32 (row stride free); kc/vc flat caches addressed by seq_off / seq_len (see header).  kc / vc in torch.float8_e4m3fn:
    the FP8 cache form (acai_decode_attn_fp8), with k_scale / v_scale the fp32 per-row scales (row = element offset / dhp)."""
    _chk(q, "q", torch.float32)
    B = q.shape[0]
    nsplit = max(1, -(-int(max_len) // chunk))
    partial = torch.empty(B * H * nsplit * (dhp + 2), dtype=torch.float32, device=q.device)
    out = torch.empty(B, H * dh, dtype=torch.float32, device=q.device)
    tickets = torch.zeros(B * H, dtype=torch.int32, device=q.device) if fused_merge else None
    tk = tickets.data_ptr() if tickets is not None else None
    if kc.dtype == torch.float8_e4m3fn:
        assert vc.dtype == kc.dtype and k_scale is not None and v_scale is not None
        _chk(k_scale, "k_scale", torch.float32), _chk(v_scale, "v_scale", torch.float32)
        _lib.check(_lib.lib().acai_decode_attn_fp8(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
                                                   seq_off.data_ptr(), seq_len.data_ptr(), partial.data_ptr(), out.data_ptr(), out.stride(0), B, H,
                                                   dh, dhp, chunk, nsplit, 1 if round_out else 0, tk, _st()), "acai_decode_attn_fp8")
    else:
        assert k_scale is None and v_scale is None, "per-row scales belong to an FP8 cache"
        _lib.check(_lib.lib().acai_decode_attn(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), seq_off.data_ptr(), seq_len.data_ptr(),
                                               partial.data_ptr(), out.data_ptr(), out.stride(0), B, H, dh, dhp, chunk, nsplit, _dt(kc),
                                               1 if round_out else 0, tk, _st()), "acai_decode_attn")
    if tickets is not None:
        assert int(tickets.abs().sum().item()) == 0, "arrival counters must re-arm to zero"
    return out


DATTN_PLAIN, DATTN_ANCESTOR, DATTN_RING, DATTN_SPEC = 0, 1, 2, 3   # acai_debug_decode_self_attn's `form`


def debug_decode_self_attn(form, q, k_cache, v_cache, H, dh, chunk, nsplit, step=None, row_len=None, table=None, table_pitch=0, table_stride=0,
                           out=None, round_out=False, tickets=None):
    """Test entry (acai_debug_decode_self_attn, see the header): the step's self-attention kernels on given operands.  q [B, >= H*dh] fp32
    (any row stride and alignment); k_cache / v_cache [rows, H, Tmax, dhp] fp32 or bf16; step / row_len / table int32 as the form needs.
    out: [B, >= H*dh] fp32, or bf16 for the bf16 output form (allocated fp32 when None); tickets: B*H zeroed int32 counters for the merge
    inside the launch, None for the separate combine launch.  Returns out."""
    _chk(q, "q", torch.float32), _chk(k_cache, "k_cache"), _chk(v_cache, "v_cache", k_cache.dtype)
    assert k_cache.dim() == 4 and k_cache.is_contiguous() and v_cache.is_contiguous() and v_cache.shape == k_cache.shape and k_cache.shape[1] == H
    B, Tmax, dhp = q.shape[0], k_cache.shape[2], k_cache.shape[3]
    for t, name in ((step, "step"), (row_len, "row_len"), (table, "table"), (tickets, "tickets")):
        if t is not None:
            assert _chk(t, name, torch.int32).is_contiguous(), name
    if out is None:
        out = torch.empty(B, H * dh, dtype=torch.float32, device=q.device)
    assert out.dtype in (torch.float32, torch.bfloat16) and out.shape[0] == B and out.shape[1] >= H * dh and out.stride(1) == 1
    assert tickets is None or tickets.numel() >= B * H
    partial = torch.empty(B * H * nsplit * (dhp + 2), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().acai_debug_decode_self_attn(int(form), q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), _p(step),
                                                      _p(row_len), _p(table), int(table_pitch), int(table_stride), partial.data_ptr(),
                                                      out.data_ptr(), out.stride(0), B, H, dh, dhp, Tmax, chunk, nsplit, _dt(k_cache),
                                                      1 if round_out else 0, 1 if out.dtype == torch.bfloat16 else 0, _p(tickets), _st()),
               "acai_debug_decode_self_attn")
    return out


def debug_decode_attn_group(q, kc, vc, seq_off, seq_len, H, dh, dhp, group, chunk, nsplit, out=None, round_out=False, tickets=None):
    """Test entry (acai_debug_decode_attn_group): decode_attn's operands through the matrix-core rollout-group kernel; rows i*group ..
    i*group + group - 1 share one image's K/V (seq_off / seq_len keep one entry per row).  bf16, dhp 64; nsplit > 1 needs tickets."""
    _chk(q, "q", torch.float32), _chk(kc, "kc", torch.bfloat16), _chk(vc, "vc", torch.bfloat16)
    _chk(seq_off, "seq_off", torch.int64), _chk(seq_len, "seq_len", torch.int32)
    B = q.shape[0]
    assert seq_off.numel() == B and seq_len.numel() == B
    if out is None:
        out = torch.empty(B, H * dh, dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.shape[0] == B and out.shape[1] >= H * dh and out.stride(1) == 1
    assert tickets is None or (tickets.dtype == torch.int32 and tickets.numel() >= B * H)
    partial = torch.empty(B * H * nsplit * (dhp + 2), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().acai_debug_decode_attn_group(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), seq_off.data_ptr(),
                                                       seq_len.data_ptr(), partial.data_ptr(), out.data_ptr(), out.stride(0), B, H, dh, dhp,
                                                       chunk, nsplit, _dt(kc), 1 if round_out else 0, _p(tickets), int(group), _st()),
               "acai_debug_decode_attn_group")
    return out


(SELECT_ARGMAX, SELECT_PROMPT, SELECT_GRAMMAR_ARGMAX, SELECT_SLOT_ARGMAX, SELECT_SLOT_GRAMMAR_ARGMAX, SELECT_SAMPLE, SELECT_GRAMMAR_SAMPLE,
 SELECT_SLOT_SAMPLE, SELECT_SLOT_GRAMMAR_SAMPLE, SELECT_BEAM) = range(10)   # acai_debug_decode_select's `form`


def debug_decode_select(form, logits, seqs, logprobs, step, finished, *, max_len, Tmax, eos, bos=0, pad=0, emb=None, pos=None, x=None,
                        tickets=None, round_lp=False, chained=True, slots=None, grammar=None, prompt=None, beam=None, uniforms=None,
                        ld_uniforms=0, urow=None, top_k=1, temperature=1.0, B=None, V=None, E=None):
    """Test entry (acai_debug_decode_select, see the header): one token-selection launch on the logits the caller wrote.  logits [B, V] fp32,
    seqs [B, max_len] int64, logprobs [B, max_len] fp32, step [2] int32, finished [B + 1] int32, emb [V, E] / pos [Tmax, E] / x [B, E] fp32,
    tickets int32 (one zeroed counter) or None.  slots = dict(t, cap) int32 [B]; grammar = dict(next int16 [S, V], resync int16 [V], state
    int32 [B], start); prompt = dict(tok int32 [B, pitch], len int32 [B]); beam = dict(K, anc int32 / tok int64 / lp fp32 [2, B, pitch],
    cum fp32 [B], len int32 [B]).  Any tensor may be None and B / V / E may be overridden: the entry refuses what its form needs and lacks.
    Everything is written in place."""
    d = _lib.AcaiDecoder()
    d.B = int(B if B is not None else logits.shape[0])
    d.V = int(V if V is not None else logits.shape[1])
    d.E = int(E if E is not None else (emb.shape[1] if emb is not None else 4))
    d.max_len, d.Tmax, d.eos, d.bos, d.pad = int(max_len), int(Tmax), int(eos), int(bos), int(pad)
    d.flags = GEMM_ROUND_BF16 if round_lp else 0
    for name, t, dt in (("logits", logits, torch.float32), ("seqs", seqs, torch.int64), ("logprobs", logprobs, torch.float32),
                        ("step", step, torch.int32), ("finished", finished, torch.int32), ("emb", emb, torch.float32),
                        ("pos", pos, torch.float32), ("x", x, torch.float32), ("tickets", tickets, torch.int32)):
        if t is not None:
            assert _chk(t, name, dt).is_contiguous(), name
            setattr(d, name, t.data_ptr())

    def ptrs(desc, src, fields):
        for name, dt in fields:
            t = src.get(name)
            if t is not None:
                assert _chk(t, name, dt).is_contiguous(), name
                setattr(desc, name, t.data_ptr())
        return desc

    sl = gr = pr = bs = None
    if slots is not None:
        sl = ptrs(_lib.AcaiSlots(), slots, (("t", torch.int32), ("cap", torch.int32)))
        sl.rows = int(slots.get("rows", d.B))
    if grammar is not None:
        gr = ptrs(_lib.AcaiGrammar(), grammar, (("next", torch.int16), ("resync", torch.int16), ("state", torch.int32)))
        nxt = grammar.get("next")
        gr.states = int(grammar.get("states", nxt.shape[0] if nxt is not None else 0))
        gr.start, gr.rows = int(grammar.get("start", 0)), int(grammar.get("rows", d.B))
    if prompt is not None:
        pr = ptrs(_lib.AcaiPrompt(), prompt, (("tok", torch.int32), ("len", torch.int32)))
        tk = prompt.get("tok")
        pr.pitch, pr.rows = int(prompt.get("pitch", tk.shape[1] if tk is not None else 0)), int(prompt.get("rows", d.B))
    if beam is not None:
        bs = ptrs(_lib.AcaiBeam(), beam, (("anc", torch.int32), ("tok", torch.int64), ("lp", torch.float32), ("cum", torch.float32),
                                          ("len", torch.int32)))
        an = beam.get("anc")
        bs.K, bs.rows = int(beam["K"]), int(beam.get("rows", an.shape[1] if an is not None else d.B))
        bs.pitch = int(beam.get("pitch", an.shape[2] if an is not None else 0))
    if uniforms is not None:
        assert _chk(uniforms, "uniforms", torch.float32).is_contiguous()
        if not ld_uniforms:
            ld_uniforms = uniforms.shape[1]
    if urow is not None:
        assert _chk(urow, "urow", torch.int32).is_contiguous()

    def ref(desc):
        return None if desc is None else ctypes.byref(desc)

    _lib.check(_lib.lib().acai_debug_decode_select(int(form), ref(d), ref(sl), ref(gr), ref(pr), ref(bs), _p(uniforms), int(ld_uniforms),
                                                   _p(urow), int(top_k), float(temperature), 1 if chained else 0, _st()),
               "acai_debug_decode_select")


def debug_decode_loop_select(slot, logits, seqs, logprobs, step, finished, *, loop, max_len, Tmax, eos, bos=0, pad=0, emb=None, pos=None, x=None,
                             round_lp=False, chained=True, slots=None, B=None, V=None, E=None):
    """Test entry (acai_debug_decode_loop_select, see the header): one selection launch of the guarded greedy step (slot: of the guarded slot
    step) on the logits the caller wrote.  Tensors as debug_decode_select takes them; slots = dict(t, cap) int32 [B]; loop = dict(run int32
    [rows, 64], stop / period / start int32 [rows], max_period, min_repeats, min_tokens).  Everything is written in place."""
    d = _lib.AcaiDecoder()
    d.B = int(B if B is not None else logits.shape[0])
    d.V = int(V if V is not None else logits.shape[1])
    d.E = int(E if E is not None else (emb.shape[1] if emb is not None else 4))
    d.max_len, d.Tmax, d.eos, d.bos, d.pad = int(max_len), int(Tmax), int(eos), int(bos), int(pad)
    d.flags = GEMM_ROUND_BF16 if round_lp else 0
    for name, t, dt in (("logits", logits, torch.float32), ("seqs", seqs, torch.int64), ("logprobs", logprobs, torch.float32),
                        ("step", step, torch.int32), ("finished", finished, torch.int32), ("emb", emb, torch.float32),
                        ("pos", pos, torch.float32), ("x", x, torch.float32)):
        if t is not None:
            assert _chk(t, name, dt).is_contiguous(), name
            setattr(d, name, t.data_ptr())
    sl = lp = None
    if slots is not None:
        sl = _lib.AcaiSlots()
        for name in ("t", "cap"):
            if slots.get(name) is not None:
                assert _chk(slots[name], name, torch.int32).is_contiguous(), name
                setattr(sl, name, slots[name].data_ptr())
        sl.rows = int(slots.get("rows", d.B))
    if loop is not None:
        lp = _lib.AcaiLoop()
        for name in ("run", "stop", "period", "start"):
            if loop.get(name) is not None:
                assert _chk(loop[name], name, torch.int32).is_contiguous(), name
                setattr(lp, name, loop[name].data_ptr())
        run = loop.get("run")
        lp.rows = int(loop.get("rows", run.shape[0] if run is not None else d.B))
        lp.max_period, lp.min_repeats, lp.min_tokens = int(loop["max_period"]), int(loop["min_repeats"]), int(loop["min_tokens"])
    _lib.check(_lib.lib().acai_debug_decode_loop_select(1 if slot else 0, ctypes.byref(d), None if sl is None else ctypes.byref(sl),
                                                        None if lp is None else ctypes.byref(lp), 1 if chained else 0, _st()),
               "acai_debug_decode_loop_select")


def debug_decode_spec_accept(logits, seqs, logprobs, step, finished, *, spec, max_len, Tmax, eos, pad=0, emb=None, pos=None, x=None,
                             round_lp=False, arm=False, prompt=None, B=None, V=None, E=None):
    """Test entry (acai_debug_decode_spec_accept, see the header): the one launch that closes a speculative step (arm: that opens the run) on
    the state the caller wrote.  logits [B, V] fp32 (None with arm: give B and V), seqs [rows, max_len] int64, logprobs [rows, max_len] fp32,
    step [2] int32, finished [B + 1] int32, emb [V, E] / pos [Tmax, E] / x [B, E] fp32.  spec = dict(D, ngram, t / cap / steps int32 [rows],
    tab int32 [rows, pitch], next int32 [rows, 8], drafts int32 [rows, pitch] or None; pitch and rows default to tab's shape);
    prompt = dict(tok int32 [rows, pitch], len int32 [rows]) for the prompted launch.  Any tensor may be None and B / V / E may be
    overridden: the entry refuses what it needs and lacks.  Everything is written in place."""
    d = _lib.AcaiDecoder()
    d.B = int(B if B is not None else logits.shape[0])
    d.V = int(V if V is not None else logits.shape[1])
    d.E = int(E if E is not None else (emb.shape[1] if emb is not None else 4))
    d.max_len, d.Tmax, d.eos, d.pad = int(max_len), int(Tmax), int(eos), int(pad)
    d.flags = GEMM_ROUND_BF16 if round_lp else 0
    for name, t, dt in (("logits", logits, torch.float32), ("seqs", seqs, torch.int64), ("logprobs", logprobs, torch.float32),
                        ("step", step, torch.int32), ("finished", finished, torch.int32), ("emb", emb, torch.float32),
                        ("pos", pos, torch.float32), ("x", x, torch.float32)):
        if t is not None:
            assert _chk(t, name, dt).is_contiguous(), name
            setattr(d, name, t.data_ptr())

    def ptrs(desc, src, names):
        for name in names:
            t = src.get(name)
            if t is not None:
                assert _chk(t, name, torch.int32).is_contiguous(), name
                setattr(desc, name, t.data_ptr())
        return desc

    sp = pr = None
    if spec is not None:
        sp = ptrs(_lib.AcaiSpec(), spec, ("t", "cap", "steps", "tab", "next", "drafts"))
        tab = spec.get("tab")
        sp.D, sp.ngram = int(spec["D"]), int(spec.get("ngram", 0))
        sp.pitch = int(spec.get("pitch", tab.shape[1] if tab is not None else 0))
        sp.rows = int(spec.get("rows", tab.shape[0] if tab is not None else 0))
    if prompt is not None:
        pr = ptrs(_lib.AcaiPrompt(), prompt, ("tok", "len"))
        tk = prompt.get("tok")
        pr.pitch = int(prompt.get("pitch", tk.shape[1] if tk is not None else 0))
        pr.rows = int(prompt.get("rows", tk.shape[0] if tk is not None else 0))
    _lib.check(_lib.lib().acai_debug_decode_spec_accept(ctypes.byref(d), None if sp is None else ctypes.byref(sp),
                                                        None if pr is None else ctypes.byref(pr), 1 if arm else 0, _st()),
               "acai_debug_decode_spec_accept")


_BWD_WS = {}   # (device, stream) -> the one-pass attention backward's fp32 query-gradient workspace (used only inside a call, in stream order)


def _bwd_workspace(device, nbytes):
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _BWD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _BWD_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def attn_varlen_bwd(q, k, v, o, dout, lse, cu_q, cu_k, H, dh, max_q, max_k, causal, dq, dk, dv, dropout_p=0.0, seed=0, q_prescaled=False, accumulate_dkv=False,
                    lend_workspace=True):
    """Gradients of attn_varlen w.r.t. q, k, v, written into the (strided) views dq, dk, dv.  q_prescaled: q is the forward's prescaled
    q; dq is still the gradient w.r.t. the unscaled in-projection output.  accumulate_dkv: dk, dv += (bf16, aligned operands only).
    lend_workspace=False: no workspace is offered, i.e. the two-kernel form whose dq is bit-reproducible (acai_attn_varlen_bwd_ws)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o"), (dout, "dout"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk(t, n)
        assert t.dim() == 2 and t.dtype == q.dtype, n
    _chk(lse, "lse", torch.float32)
    B = cu_q.numel() - 1
    total_q = q.shape[0]
    assert lse.numel() == H * total_q and dout.shape == o.shape
    delta = torch.empty(H * total_q, dtype=torch.float32, device=q.device)
    flags = (1 if causal else 0) | (2 if accumulate_dkv else 0)
    total_k = k.shape[0]
    need = _lib.lib().acai_attn_varlen_bwd_workspace_bytes(B, H, dh, int(max_q), int(max_k), total_q, total_k, flags, _dt(q), float(dropout_p), 1 if q_prescaled else 0)
    ws = _bwd_workspace(q.device, need) if need and lend_workspace else None
    _lib.check(_lib.lib().acai_attn_varlen_bwd_ws(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o.data_ptr(), o.stride(0),
                                                  dout.data_ptr(), dout.stride(0), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(),
                                                  dv.stride(0), lse.data_ptr(), delta.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), B, H, dh, int(max_q),
                                                  int(max_k), total_q, total_k, flags, _dt(q), float(dropout_p), int(seed) & 0xFFFFFFFF,
                                                  1 if q_prescaled else 0, _p(ws), need if ws is not None else 0, _st()),
               "acai_attn_varlen_bwd_ws")


def dropout_add(x, residual, p, seed, out_dtype=None):
    """out = residual + keep * x / (1 - p) (residual fp32 or None); the mask depends only on (seed, row, col)."""
    _chk(x, "x")
    assert x.dim() == 2 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=out_dtype or (torch.float32 if residual is not None else x.dtype), device=x.device)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == x.shape and residual.is_contiguous()
    _lib.check(_lib.lib().acai_dropout_add(x.data_ptr(), _p(residual), out.data_ptr(), x.shape[0], x.shape[1], float(p), int(seed) & 0xFFFFFFFF,
                                           _dt(x), _dt(out), _st()), "acai_dropout_add")
    return out


def layernorm_bwd(x, w, dy, eps, want_param_grads=True, want_bf16=False, want_colsum=False, accum_into=None):
    """Returns (dx, dw, db) or, with want_bf16 (dim % 256 == 0, dim <= 1024), (dx, dw, db, dx_bf16); want_colsum appends the column sums of
    dx (of its bf16 copy when one is written): the bias gradient of the nn.Linear whose output this LayerNorm normalised.
    accum_into = (dw, db): existing fp32 vectors the parameter gradients are ADDED to (returned dw / db are then None)."""
    _chk(x, "x", torch.float32), _chk(dy, "dy", torch.float32)
    assert x.is_contiguous() and dy.is_contiguous() and x.shape == dy.shape
    rows, dim = x.shape
    dx = torch.empty_like(x)
    dxb = torch.empty(rows, dim, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    n_acc = (2 if want_param_grads else 0) + (1 if want_colsum else 0)
    acc = _ZEROS.take(max(n_acc, 1), dim, x.device)   # zeroed accumulators: slices of the arena's chunk (one fill per 256 MB, not one per call)
    dw = acc[0] if want_param_grads else None
    db = acc[1] if want_param_grads else None
    dcs = acc[n_acc - 1] if want_colsum else None
    if accum_into is not None:
        assert want_param_grads
        dw, db = accum_into
        _chk(dw, "dw", torch.float32), _chk(db, "db", torch.float32)
        assert dw.is_contiguous() and db.is_contiguous() and dw.numel() == dim and db.numel() == dim
    _lib.check(_lib.lib().acai_layernorm_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), float(eps), dx.data_ptr(), _p(dxb), _p(dw), _p(db), _p(dcs),
                                             stats.data_ptr(), rows, dim, _st()), "acai_layernorm_bwd")
    if accum_into is not None:
        dw = db = None
    out = (dx, dw, db, dxb) if want_bf16 else (dx, dw, db)
    return out + (dcs,) if want_colsum else out


def gemm_dw(dy, x, out=None, bias_out=None, want_bias=False):
    """Both parameter gradients of an nn.Linear from one pass over dy: dW[M, N] (+)= dy[K, M]^T x[K, N] and, with want_bias or bias_out,
    db[M] (+)= column sums of dy.  out / bias_out: existing fp32 gradients to ACCUMULATE into (else zeroed arena slices).  Returns (dW, db)."""
    _chk(dy, "dy"), _chk(x, "x")
    assert dy.dim() == 2 and x.dim() == 2 and dy.dtype == x.dtype and dy.shape[0] == x.shape[0] and dy.stride(1) == 1 and x.stride(1) == 1
    K, M = dy.shape
    N = x.shape[1]
    if out is None:
        out = _ZEROS.take(M, N, dy.device)
    if bias_out is None and want_bias:
        bias_out = _ZEROS.take(1, M, dy.device).view(-1)
    assert out.shape == (M, N) and out.dtype == torch.float32 and out.stride(1) == 1
    if bias_out is not None:
        _chk(bias_out, "bias_out", torch.float32)
        assert bias_out.is_contiguous() and bias_out.numel() == M
    _lib.check(_lib.lib().acai_gemm_dw(dy.data_ptr(), _ld(dy), x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), _p(bias_out), M, N, K, _dt(dy), _st()),
               "acai_gemm_dw")
    return out, bias_out


def cast_weights(items):
    """One launch for the operand copies of many fp32 parameters (engine.WeightCache after an optimizer step).  items: (src, want16, want16t,
    want32r) with src a contiguous fp32 CUDA tensor of one or two dimensions; returns per item (bf16 copy | None, transposed bf16 copy
    [cols, rows] | None, bf16-rounded fp32 copy | None).  Replaces `t.to(bfloat16)`, `out.copy_(t.t())` and `t.to(bfloat16).to(float32)`."""
    if not items:
        return []
    dev = items[0][0].device
    arr = (_lib.AcaiCastEntry * len(items))()
    outs, tiles = [], 0
    for i, (src, w16, w16t, w32r) in enumerate(items):
        _chk(src, "src", torch.float32)
        assert src.is_contiguous() and src.dim() in (1, 2) and src.device == dev
        rows, cols = (1, src.shape[0]) if src.dim() == 1 else src.shape
        d16 = torch.empty(src.shape, dtype=torch.bfloat16, device=dev) if w16 else None
        d16t = torch.empty((cols, rows), dtype=torch.bfloat16, device=dev) if w16t else None
        d32 = torch.empty(src.shape, dtype=torch.float32, device=dev) if w32r else None
        arr[i].src, arr[i].dst16, arr[i].dst16t, arr[i].dst32r = src.data_ptr(), _p(d16), _p(d16t), _p(d32)
        arr[i].rows, arr[i].cols, arr[i].tile0 = rows, cols, tiles
        tiles += ((rows + 63) // 64) * ((cols + 63) // 64)
        outs.append((d16, d16t, d32))
    table = h2d(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().acai_cast_weights(table.data_ptr(), len(items), tiles, _st()), "acai_cast_weights")
    return outs


GRAD_CHUNK = 16384   # elements per workgroup of the gradient-norm sums (optim.CHUNK: the AdamW step shares its chunk table with them)


def chunk_tables(sizes, chunk=GRAD_CHUNK):
    """The chunk tables of the multi-tensor launches (acai_adamw_step, acai_grad_norm) for tensors of `sizes` elements: per workgroup its tensor
    and first element, and per tensor its first chunk (n + 1 entries, the last one the chunk count).  Host lists."""
    ct, co, c0 = [], [], []
    for i, n in enumerate(sizes):
        c0.append(len(ct))
        for off in range(0, n, chunk):
            ct.append(i)
            co.append(off)
    c0.append(len(ct))
    return ct, co, c0


def grad_norm_launch(tensors, chunk_tensor, chunk_off, tensor_chunk0, n_tensors, n_chunks, chunk, grad_scale, max_norm, workspace, want_per_tensor=True):
    """acai_grad_norm over device tables the caller owns (optim.FusedAdamW: the tables of its step).  workspace: float64 [n_chunks].  Returns
    (result block fp32 [GRAD_NORM_WORDS], per-tensor norms fp32 [n_tensors] or None), both fresh."""
    dev = tensors.device
    assert tensors.dtype == torch.uint8 and tensors.numel() == n_tensors * ctypes.sizeof(_lib.AcaiAdamWTensor)
    assert chunk_tensor.dtype == torch.int32 and chunk_tensor.numel() == n_chunks and chunk_off.dtype == torch.int64 and chunk_off.numel() == n_chunks
    assert tensor_chunk0.dtype == torch.int32 and tensor_chunk0.numel() == n_tensors + 1
    assert workspace.dtype == torch.float64 and workspace.is_contiguous() and workspace.numel() >= n_chunks
    assert all(t.device == dev for t in (chunk_tensor, chunk_off, tensor_chunk0, workspace))
    result = torch.empty(_lib.GRAD_NORM_WORDS, dtype=torch.float32, device=dev)
    norms = torch.empty(n_tensors, dtype=torch.float32, device=dev) if want_per_tensor else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().acai_grad_norm(tensors.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), tensor_chunk0.data_ptr(), n_tensors,
                                             n_chunks, chunk, float(grad_scale), float(max_norm), workspace.data_ptr(), _p(norms), result.data_ptr(),
                                             _st()), "acai_grad_norm")
    return result, norms


def grad_norm(tensors, *, grad_scale=1.0, per_tensor=False):
    """The 2-norm of `grad_scale * t` over all of `tensors` (contiguous fp32 CUDA tensors on one device) as a 0-dim fp32 device tensor, and
    with per_tensor=True also the fp32 vector of each tensor's own norm.  Two launches, sums in fp64 in a fixed order (bitwise repeatable), no
    host synchronisation: what `torch.nn.utils.get_total_norm` computes through a foreach norm, a stack and a second norm."""
    tensors = list(tensors)
    if not tensors:
        raise RuntimeError("grad_norm: no tensors")
    dev = tensors[0].device
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and not t.is_sparse and t.is_contiguous() and t.device == dev):
            raise RuntimeError("grad_norm: dense contiguous fp32 tensors on one GPU only (the product path has no CPU fallback)")
    arr = (_lib.AcaiAdamWTensor * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i].g, arr[i].n = t.data_ptr(), t.numel()
    ct, co, c0 = chunk_tables([t.numel() for t in tensors])
    table = h2d(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8), dev)
    ctd, cod = h2d(torch.tensor(ct, dtype=torch.int32), dev), h2d(torch.tensor(co, dtype=torch.int64), dev)
    result, norms = grad_norm_launch(table, ctd, cod, h2d(torch.tensor(c0, dtype=torch.int32), dev), len(tensors), len(ct), GRAD_CHUNK, grad_scale, 0.0,
                                     torch.empty(len(ct), dtype=torch.float64, device=dev), want_per_tensor=per_tensor)
    total = result[_lib.GRAD_NORM_TOTAL]
    return (total, norms) if per_tensor else total


def gelu_fwd(a):
    _chk(a, "a")
    assert a.is_contiguous()
    h = torch.empty_like(a)
    _lib.check(_lib.lib().acai_gelu_fwd(a.data_ptr(), h.data_ptr(), a.numel(), _dt(a), _st()), "acai_gelu_fwd")
    return h


def gelu_bwd(a, dh):
    _chk(a, "a"), _chk(dh, "dh")
    assert a.is_contiguous() and dh.is_contiguous() and a.dtype == dh.dtype and a.shape == dh.shape
    da = torch.empty_like(a)
    _lib.check(_lib.lib().acai_gelu_bwd(a.data_ptr(), dh.data_ptr(), da.data_ptr(), a.numel(), _dt(a), _st()), "acai_gelu_bwd")
    return da


def colsum(x, out=None):
    """Column sums of x (fp32).  out: an existing fp32 vector to ADD them to (the kernel accumulates with float atomics)."""
    _chk(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1     # the kernel takes a row stride only
    if out is None:
        out = _ZEROS.take(1, x.shape[1], x.device).view(-1)
    else:
        _chk(out, "out", torch.float32)
        assert out.is_contiguous() and out.numel() == x.shape[1]
    _lib.check(_lib.lib().acai_colsum(x.data_ptr(), x.stride(0), out.data_ptr(), x.shape[0], x.shape[1], _dt(x), _st()), "acai_colsum")
    return out


def scatter_add_rows(src, idx, dst, shared_row=-1):
    """dst[idx[r]] += src[r].  shared_row >= 0: the only index that may repeat (everything else is updated without atomics)."""
    _chk(src, "src", torch.float32), _chk(idx, "idx", torch.int32), _chk(dst, "dst", torch.float32)
    assert src.is_contiguous() and dst.is_contiguous() and src.shape[1] == dst.shape[1] and idx.numel() == src.shape[0]
    _lib.check(_lib.lib().acai_scatter_add_rows(src.data_ptr(), idx.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], int(shared_row), _st()),
               "acai_scatter_add_rows")
    return dst


def mae_loss(pred, target, mask, count, want_grad):
    """pred/target [R,D] fp32, mask [R] uint8; returns (loss scalar tensor, dpred or None) for loss = masked mean."""
    _chk(pred, "pred", torch.float32), _chk(target, "target", torch.float32), _chk(mask, "mask", torch.uint8)
    assert pred.is_contiguous() and target.is_contiguous() and pred.shape == target.shape and mask.numel() == pred.shape[0]
    loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    _lib.check(_lib.lib().acai_mae_loss(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), 1.0 / float(count), loss.data_ptr(), _p(dpred),
                                        pred.shape[0], pred.shape[1], _st()), "acai_mae_loss")
    return loss[0], dpred


def pe_interp(table, h_out, w_out):
    """table (Hin, Win, E) fp32 -> (h_out * w_out, E): bilinear, align_corners=False (OMREncoder.interpolate_pe, models.py:291-302)."""
    _chk(table, "table", torch.float32)
    assert table.dim() == 3 and table.is_contiguous()
    Hin, Win, E = table.shape
    out = torch.empty(int(h_out) * int(w_out), E, dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().acai_pe_interp_fwd(table.data_ptr(), Hin, Win, E, out.data_ptr(), int(h_out), int(w_out), _st(table)), "acai_pe_interp_fwd")
    return out


def pe_interp_bwd(dout, h_out, w_out, table_shape):
    """Gradient of pe_interp w.r.t. the table: (Hin, Win, E) fp32."""
    _chk(dout, "dout", torch.float32)
    Hin, Win, E = table_shape
    assert dout.is_contiguous() and dout.shape == (int(h_out) * int(w_out), E)
    dt = torch.zeros(Hin, Win, E, dtype=torch.float32, device=dout.device)
    _lib.check(_lib.lib().acai_pe_interp_bwd(dout.data_ptr(), int(h_out), int(w_out), E, dt.data_ptr(), Hin, Win, _st(dout)), "acai_pe_interp_bwd")
    return dt


def ce_loss(logits, target, ignore_index, count, want_grad, label_smoothing=0.0):
    _chk(logits, "logits", torch.float32), _chk(target, "target", torch.int64)
    assert logits.dim() == 2 and logits.stride(1) == 1 and target.numel() == logits.shape[0] and target.is_contiguous()
    loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty(logits.shape, dtype=torch.float32, device=logits.device) if want_grad else None
    _lib.check(_lib.lib().acai_ce_loss(logits.data_ptr(), logits.stride(0), target.data_ptr(), int(ignore_index), 1.0 / float(count), float(label_smoothing),
                                       loss.data_ptr(), _p(dl), logits.shape[0], logits.shape[1], _st(logits)), "acai_ce_loss")
    return loss[0], dl



def grpo_objective_fwd(logits, rollouts, mask, old_lp, adv, clip_lo, clip_hi, num_groups, logv):
    """GRPO objective and entropy bonus in one pass (acai_grpo_objective_fwd).  logits [R, T, V] fp32 / bf16, rollouts [R, >T] int64, mask [R, T]
    (True = masked), old_lp [R, >T] fp32, adv [R] fp32.  Returns (out [2] = (objective, bonus), stats, rowstat): the workspaces the backward reads."""
    R, T, V = logits.shape
    _chk(logits, "logits"), _chk(rollouts, "rollouts", torch.int64), _chk(old_lp, "old_lp", torch.float32), _chk(adv, "adv", torch.float32)
    assert logits.is_contiguous() and logits.data_ptr() % 16 == 0, "logits: contiguous and 16-byte aligned"
    assert rollouts.shape[0] == R and rollouts.shape[1] > T and old_lp.shape[0] == R and old_lp.shape[1] > T and adv.numel() == R and adv.is_contiguous()
    assert mask.shape == (R, T) and mask.is_contiguous() and mask.dtype in (torch.bool, torch.uint8)
    stats = torch.empty(R * T, 4, dtype=torch.float32, device=logits.device)
    rowstat = torch.empty(R, 4, dtype=torch.float32, device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    _lib.check(_lib.lib().acai_grpo_objective_fwd(logits.data_ptr(), _dt(logits), rollouts.data_ptr(), _ld(rollouts), old_lp.data_ptr(), _ld(old_lp),
                                                  mask.data_ptr(), adv.data_ptr(), R, T, V, float(clip_lo), float(clip_hi), int(num_groups), float(logv),
                                                  stats.data_ptr(), rowstat.data_ptr(), out.data_ptr(), _st(logits)), "acai_grpo_objective_fwd")
    return out, stats, rowstat


def grpo_objective_bwd(logits, rollouts, mask, stats, rowstat, grad_out, num_groups, logv):
    """dlogits (logits' dtype) of grad_out[0] * objective + grad_out[1] * bonus; grad_out is a [2] fp32 device tensor (read on the device)."""
    R, T, V = logits.shape
    _chk(grad_out, "grad_out", torch.float32)
    assert grad_out.numel() == 2 and grad_out.is_contiguous()
    dl = torch.empty_like(logits, memory_format=torch.contiguous_format)
    _lib.check(_lib.lib().acai_grpo_objective_bwd(logits.data_ptr(), _dt(logits), rollouts.data_ptr(), _ld(rollouts), mask.data_ptr(), stats.data_ptr(),
                                                  rowstat.data_ptr(), grad_out.data_ptr(), R, T, V, int(num_groups), float(logv), dl.data_ptr(),
                                                  _st(logits)), "acai_grpo_objective_bwd")
    return dl


EDIT_DISTANCE_MAX_LEN = 4096


def _seq_rows(t, lens, name):
    """(rows with stride == width, int32 lengths) of one side of edit_distance; lens may be a bool prefix mask of t's shape (summed on the device,
    not validated: no host sync)."""
    _chk(t, name, torch.int64)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected (rows, tokens), got {tuple(t.shape)}")
    if t.shape[1] > EDIT_DISTANCE_MAX_LEN:
        raise ValueError(f"{name}: rows of {t.shape[1]} tokens; edit_distance takes at most {EDIT_DISTANCE_MAX_LEN}")
    _chk(lens, name + "_len")
    if lens.dtype == torch.bool:
        if lens.shape != t.shape:
            raise ValueError(f"{name}_len: a mask must have {name}'s shape {tuple(t.shape)}, got {tuple(lens.shape)}")
        lens = lens.sum(dim=-1, dtype=torch.int32)
    elif lens.dtype != torch.int32:
        raise TypeError(f"{name}_len: expected int32 lengths or a bool mask, got {lens.dtype}")
    if lens.shape != (t.shape[0],):
        raise ValueError(f"{name}_len: expected {t.shape[0]} lengths, got {tuple(lens.shape)}")
    return (t if t.is_contiguous() else t.contiguous()), lens.contiguous()


def edit_distance(pred, pred_len, tgt, tgt_len, group=1, out=None):
    """Unit-cost Levenshtein distance of each pred[r, :pred_len[r]] to tgt[r // group, :tgt_len[r // group]] (acai_edit_distance): int32 (R,).
    pred (R, Lp) and tgt (R // group, Lt) int64, Lp, Lt <= 4096 (ValueError beyond); the lengths are int32 vectors or bool prefix masks of the
    padded shapes, read on the device (no host sync; positions past a length are never read).  With int32 lengths and `out` given, the call is one
    kernel launch and nothing else, so it can be captured in a Graph."""
    pred, pred_len = _seq_rows(pred, pred_len, "pred")
    tgt, tgt_len = _seq_rows(tgt, tgt_len, "tgt")
    R, group = pred.shape[0], int(group)
    if group < 1 or tgt.shape[0] * group != R:
        raise ValueError(f"edit_distance: {R} pred rows against {tgt.shape[0]} tgt rows with group {group}")
    if out is None:
        out = torch.empty(R, dtype=torch.int32, device=pred.device)
    else:
        _chk(out, "out", torch.int32)
        if out.shape != (R,):
            raise ValueError(f"out: expected ({R},), got {tuple(out.shape)}")
    for t in (pred_len, tgt, tgt_len, out):
        if t.device != pred.device:
            raise RuntimeError(f"edit_distance: operands on different devices ({pred.device} and {t.device})")
    if R == 0:
        return out
    _lib.check(_lib.lib().acai_edit_distance(pred.data_ptr(), pred.shape[1], pred_len.data_ptr(), tgt.data_ptr(), tgt.shape[1], tgt_len.data_ptr(),
                                             R, group, out.data_ptr(), _st(pred)), "acai_edit_distance")
    return out


class EditAlignment(NamedTuple):
    """What edit_alignment returns for R pairs of widths (Lp, Lt).  counts (R, 4) int32: matches, substitutions, insertions, deletions;
    pred_op (R, Lp) int8: 0 match, 1 substitution, 2 insertion; pred_to_tgt (R, Lp) int32: the aligned target index, -1 for an insertion;
    tgt_to_pred (R, Lt) int32: the aligned pred index, -1 for a deleted target token; tgt_slot (R, Lt) int32: pred tokens consumed before
    the target token on the path (for a deleted token: the pred index it is missing in front of, in [0, len]).  -1 past a row's length."""
    counts: torch.Tensor
    pred_op: torch.Tensor
    pred_to_tgt: torch.Tensor
    tgt_to_pred: torch.Tensor
    tgt_slot: torch.Tensor


EDIT_ALIGNMENT_WORKSPACE_LIMIT = 256 << 20   # bytes of direction words beyond which edit_alignment runs its rows in chunks


def edit_alignment_workspace_bytes(ld_pred, ld_tgt, rows=1):
    """Bytes of workspace that one launch over `rows` pairs of widths (ld_pred, ld_tgt) needs (acai_edit_align_workspace_bytes)."""
    return int(_lib.lib().acai_edit_align_workspace_bytes(int(ld_pred), int(ld_tgt), int(rows)))


def edit_alignment(pred, pred_len, tgt, tgt_len, group=1, out=None, workspace=None):
    """The canonical optimal edit alignment of each pred[r, :pred_len[r]] to tgt[r // group, :tgt_len[r // group]] (acai_edit_align) ->
    EditAlignment.  Arguments as edit_distance takes them: pred (R, Lp) and tgt (R // group, Lt) int64, Lp, Lt <= 4096 (ValueError beyond), the
    lengths int32 vectors or bool prefix masks read on the device (no host sync).  Among the optimal paths the one is returned that, walking
    back from the ends, prefers the diagonal (match / substitution), then an insertion, then a deletion; counts[:, 1:].sum(1) is
    edit_distance's result.  out: an EditAlignment (or five tensors) to write into; workspace: a GPU buffer for the direction words
    (edit_alignment_workspace_bytes; default: allocated here).  When the workspace of all R rows would exceed 256 MiB - or the given one is
    smaller than that - the rows run in chunks of whole groups, one launch per chunk, with the same results; a workspace too small for one group
    raises ValueError.  With int32 lengths, out and workspace given and a single chunk, the call is one kernel launch and nothing else."""
    pred, pred_len = _seq_rows(pred, pred_len, "pred")
    tgt, tgt_len = _seq_rows(tgt, tgt_len, "tgt")
    R, group = pred.shape[0], int(group)
    Lp, Lt = pred.shape[1], tgt.shape[1]
    if group < 1 or tgt.shape[0] * group != R:
        raise ValueError(f"edit_alignment: {R} pred rows against {tgt.shape[0]} tgt rows with group {group}")
    shapes = (((R, 4), torch.int32), ((R, Lp), torch.int8), ((R, Lp), torch.int32), ((R, Lt), torch.int32), ((R, Lt), torch.int32))
    if out is None:
        out = EditAlignment(*(torch.empty(s, dtype=d, device=pred.device) for s, d in shapes))
    else:
        out = EditAlignment(*out)
        for t, name, (s, d) in zip(out, EditAlignment._fields, shapes):
            _chk(t, "out." + name, d)
            if tuple(t.shape) != s or not t.is_contiguous():
                raise ValueError(f"out.{name}: expected a contiguous {s} tensor, got {tuple(t.shape)}")
    if workspace is not None:
        _chk(workspace, "workspace")
        if not workspace.is_contiguous():
            raise ValueError("workspace: expected a contiguous buffer")
    for t in (pred_len, tgt, tgt_len, workspace) + tuple(out):
        if t is not None and t.device != pred.device:
            raise RuntimeError(f"edit_alignment: operands on different devices ({pred.device} and {t.device})")
    if R == 0:
        return out
    per_pair = edit_alignment_workspace_bytes(Lp, Lt, 1)
    limit = EDIT_ALIGNMENT_WORKSPACE_LIMIT if workspace is None else workspace.numel() * workspace.element_size()
    if workspace is not None and limit < per_pair * group:
        raise ValueError(f"workspace: {limit} bytes, one group of {group} pairs needs {per_pair * group}")
    chunk = R if R * per_pair <= limit else max(limit // (per_pair * group), 1) * group
    if workspace is None:
        workspace = torch.empty(min(chunk, R) * per_pair, dtype=torch.uint8, device=pred.device)
        limit = workspace.numel()
    L = _lib.lib()
    for r0 in range(0, R, chunk):
        r1 = min(r0 + chunk, R)
        g0, g1 = r0 // group, r1 // group
        _lib.check(L.acai_edit_align(pred[r0:r1].data_ptr(), Lp, pred_len[r0:r1].data_ptr(), tgt[g0:g1].data_ptr(), Lt, tgt_len[g0:g1].data_ptr(),
                                     r1 - r0, group, out.counts[r0:r1].data_ptr(), out.pred_op[r0:r1].data_ptr(), out.pred_to_tgt[r0:r1].data_ptr(),
                                     out.tgt_to_pred[r0:r1].data_ptr(), out.tgt_slot[r0:r1].data_ptr(), workspace.data_ptr(), limit, _st(pred)),
                   "acai_edit_align")
    return out


def grammar_scan(rollouts, rollout_mask, automaton):
    """(violations int32 (R,), complete bool (R,)) of the rows rollouts[r, :len_r] under a grammar.TokenAutomaton (acai_grammar_scan; the CPU
    statement is automaton.violations).  rollouts (R, T) int64; rollout_mask: a bool prefix mask of that shape or int32 lengths (R,), read on
    the device as edit_distance reads them (no host sync).  The automaton's tables are used where they lie when they are on rollouts'
    device (automaton.to(device) once, outside the loop) and copied there otherwise.  CPU rollouts take automaton.violations itself."""
    if not rollouts.is_cuda:
        return automaton.violations(rollouts, rollout_mask)
    _chk(rollouts, "rollouts", torch.int64)
    if rollouts.dim() != 2:
        raise ValueError(f"rollouts: expected (rows, tokens), got {tuple(rollouts.shape)}")
    _chk(rollout_mask, "rollout_mask")
    lens = rollout_mask
    if lens.dtype == torch.bool:
        if lens.shape != rollouts.shape:
            raise ValueError(f"rollout_mask: a mask must have rollouts' shape {tuple(rollouts.shape)}, got {tuple(lens.shape)}")
        lens = lens.sum(dim=-1, dtype=torch.int32)
    elif lens.dtype != torch.int32:
        raise TypeError(f"rollout_mask: expected a bool mask or int32 lengths, got {lens.dtype}")
    if lens.shape != (rollouts.shape[0],) or lens.device != rollouts.device:
        raise ValueError(f"rollout_mask: expected {rollouts.shape[0]} lengths on {rollouts.device}, got {tuple(lens.shape)} on {lens.device}")
    rollouts, lens = rollouts.contiguous(), lens.contiguous()
    nxt, rs = automaton.next.to(rollouts.device).contiguous(), automaton.resync.to(rollouts.device).contiguous()
    if nxt.dtype != torch.int16 or rs.dtype != torch.int16 or nxt.dim() != 2 or rs.shape != (nxt.shape[1],):
        raise TypeError("grammar_scan: the automaton's tables must be int16 [states][V] and [V]")
    R = rollouts.shape[0]
    viol = torch.empty(R, dtype=torch.int32, device=rollouts.device)
    comp = torch.empty(R, dtype=torch.int32, device=rollouts.device)
    if R:
        _lib.check(_lib.lib().acai_grammar_scan(rollouts.data_ptr(), rollouts.shape[1], lens.data_ptr(), R, nxt.data_ptr(), rs.data_ptr(),
                                                nxt.shape[0], automaton.start, nxt.shape[1], automaton.eos_idx, viol.data_ptr(), comp.data_ptr(),
                                                _st(rollouts)), "acai_grammar_scan")
    return viol, comp != 0


def repeat_scan(tokens, max_period, min_repeats, min_tokens, lens=None):
    """(stop, period, start, end) int32 (N,) of the loop guard's rule over the rows tokens[n, :len_n] (acai_repeat_scan, see the header; the
    rule is stated in loops.py).  tokens (N, T) int64, a row-strided view included; lens: None (every row holds T tokens), int32 lengths
    (N,), read on the device (no host sync), or a bool prefix mask of tokens' shape.  period == 0: the row did not fire and the other three
    are 0; end is the last index up to which the reported period keeps holding."""
    _chk(tokens, "tokens", torch.int64, rows_contig=False)
    if tokens.dim() != 2:
        raise ValueError(f"tokens: expected (rows, tokens), got {tuple(tokens.shape)}")
    if not 1 <= int(max_period) <= 64 or int(min_repeats) < 2 or int(min_tokens) < 1:
        raise ValueError(f"repeat_scan: needs 1 <= max_period <= 64, min_repeats >= 2, min_tokens >= 1 (got {max_period}, {min_repeats}, "
                         f"{min_tokens})")
    N, T = tokens.shape
    if T and tokens.stride(1) != 1:
        tokens = tokens.contiguous()
    ld = _ld(tokens) if N and T else T
    if lens is not None:
        _chk(lens, "lens")
        if lens.dtype == torch.bool:
            if lens.shape != tokens.shape:
                raise ValueError(f"lens: a mask must have tokens' shape {tuple(tokens.shape)}, got {tuple(lens.shape)}")
            lens = lens.sum(dim=-1, dtype=torch.int32)
        elif lens.dtype != torch.int32:
            raise TypeError(f"lens: expected a bool mask or int32 lengths, got {lens.dtype}")
        if lens.shape != (N,) or lens.device != tokens.device:
            raise ValueError(f"lens: expected {N} lengths on {tokens.device}, got {tuple(lens.shape)} on {lens.device}")
        lens = lens.clamp(max=T).contiguous()
    elif ld != T:   # a view of wider rows: the kernel's bound without lengths is the row stride
        lens = torch.full((N,), T, dtype=torch.int32, device=tokens.device)
    out = torch.zeros(4, N, dtype=torch.int32, device=tokens.device)
    if N and T:
        _lib.check(_lib.lib().acai_repeat_scan(tokens.data_ptr(), _p(lens), N, ld, int(max_period), min(int(min_repeats), 1 << 24),
                                               min(int(min_tokens), 1 << 24), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                               out[3].data_ptr(), _st(tokens)), "acai_repeat_scan")
    return out[0], out[1], out[2], out[3]


for _name, _fn in list(globals().items()):
    if callable(_fn) and not _name.startswith("_") and getattr(_fn, "__module__", None) == __name__ and not isinstance(_fn, type):
        globals()[_name] = _on_operand_device(_fn)
del _name, _fn


class Graph:
    """hipGraph capture/replay of whatever is enqueued on the current stream between begin() and end()."""

    def __init__(self):
        self.exec = None

    def begin(self):
        _lib.check(_lib.lib().acai_graph_begin(_st()), "acai_graph_begin")

    def end(self):
        import ctypes
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().acai_graph_end(_st(), ctypes.byref(h)), "acai_graph_end")
        self.exec = h

    def launch(self):
        _lib.check(_lib.lib().acai_graph_launch(self.exec, _st()), "acai_graph_launch")

    def __del__(self):
        if self.exec is not None and _lib._lib is not None:
            _lib._lib.acai_graph_destroy(self.exec)
            self.exec = None
