"""The "camera" augmentation of the reference's training entry points, on the GPU (csrc/augment.hip): Gaussian blur, Gaussian noise, a small
rotation, a random perspective warp and a brightness / contrast jitter, all applied together with one probability per image
(`v2.RandomApply`), or any subset in that order (the GrandStaff pair: perspective + jitter) - acai_omr/train/pre_train.py:178-190,
omr_teacher_force_train.py:320-331, omr_grpo_train.py:530-541.  It runs between `utils.DynamicResize` and the model, on one-channel float32
images in [0, 1].

torchvision is not a dependency of this package, so its v2 tensor path cannot be imported or diffed here: the contract is the arithmetic
written down in include/acai_omr_hip.h and restated on the CPU by tests/augment_reference.py (DESIGN.md section 5 says what that rests on).

Every random quantity is drawn on the host (`sample_params`, a `torch.Generator`; ranges and distributions are torchvision's, the random
stream is not) into `ImageParams` objects that can be built by hand and passed back in; the noise field comes from `torch.randn` on the
device unless the parameters carry one.  There is no CPU fallback (`RuntimeError` without a GPU); sampling and this import work anywhere.
A call costs a fixed number of launches whatever the number of images, and one host-to-device copy (the descriptor table)."""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .utils import PackedPatches

STAGE_ORDER = ("blur", "noise", "rotation", "perspective", "jitter")


def _rand(generator):
    return float(torch.rand(1, dtype=torch.float64, generator=generator))


def _uniform(lo, hi, generator):
    return lo + (hi - lo) * _rand(generator)


def _range(value, name, center=0.0, lowest=None):
    """torchvision's (min, max) forms: a number v means [center - v, center + v] (clipped at `lowest`), a pair is taken as it is."""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"{name}: a single number must be non-negative")
        lo, hi = center - float(value), center + float(value)
        if lowest is not None:
            lo = max(lo, lowest)
    else:
        lo, hi = (float(v) for v in value)
    if lo > hi or (lowest is not None and lo < lowest):
        raise ValueError(f"{name}: bad range ({lo}, {hi})")
    return lo, hi


@dataclass
class ImageParams:
    """What the augmentation does to ONE image.  A stage whose field is None is left out for this image."""
    apply: bool = True
    sigma: Optional[float] = None                       # Gaussian blur
    noise_sigma: Optional[float] = None                 # Gaussian noise: clamp(img + noise_sigma * noise, 0, 1)
    noise: Optional[torch.Tensor] = None                # (H, W) standard-normal draws; None: torch.randn on the device
    angle: Optional[float] = None                       # rotation, degrees
    endpoints: Optional[List[Tuple[int, int]]] = None   # perspective: where (0,0), (W-1,0), (W-1,H-1), (0,H-1) go, as (x, y)
    brightness: Optional[float] = None                  # factor fb
    contrast: Optional[float] = None                    # factor fc
    brightness_first: bool = True


class GaussianBlur:
    """`v2.GaussianBlur(kernel_size, sigma)`: odd kernel size, sigma fixed (a number) or uniform in (min, max); one sigma for both axes."""
    stage = "blur"

    def __init__(self, kernel_size, sigma=(0.1, 2.0)):
        if isinstance(kernel_size, (tuple, list)):
            if len(set(kernel_size)) != 1:
                raise ValueError("GaussianBlur: one kernel size for both axes")
            kernel_size = kernel_size[0]
        from ._lib import AUG_MAX_TAPS
        if kernel_size <= 0 or kernel_size % 2 == 0 or kernel_size > AUG_MAX_TAPS:
            raise ValueError(f"GaussianBlur: kernel size must be odd, positive and at most {AUG_MAX_TAPS - 1}")
        self.kernel_size = int(kernel_size)
        self.sigma = (float(sigma), float(sigma)) if isinstance(sigma, (int, float)) else tuple(float(s) for s in sigma)
        if not 0.0 < self.sigma[0] <= self.sigma[1]:
            raise ValueError("GaussianBlur: sigma must be positive (and min <= max)")

    def sample(self, p, h, w, generator):
        p.sigma = _uniform(self.sigma[0], self.sigma[1], generator)


class GaussianNoise:
    """`v2.GaussianNoise(mean=0, sigma, clip=True)`."""
    stage = "noise"

    def __init__(self, mean=0.0, sigma=0.1, clip=True):
        if mean != 0.0 or not clip:
            raise ValueError("GaussianNoise: only mean = 0 with clip = True is built (what every recipe uses)")
        if sigma < 0:
            raise ValueError("GaussianNoise: sigma must be non-negative")
        self.mean, self.sigma, self.clip = 0.0, float(sigma), True

    def sample(self, p, h, w, generator):
        p.noise_sigma = self.sigma


class RandomRotation:
    """`v2.RandomRotation(degrees, interpolation=BILINEAR)`: about the image centre, same size out, fill 0."""
    stage = "rotation"

    def __init__(self, degrees, interpolation="bilinear"):
        if str(getattr(interpolation, "value", interpolation)).lower() != "bilinear":
            raise ValueError("RandomRotation: only bilinear interpolation is built (what every recipe uses)")
        self.degrees = _range(degrees, "degrees")

    def sample(self, p, h, w, generator):
        p.angle = _uniform(self.degrees[0], self.degrees[1], generator)


class RandomPerspective:
    """`v2.RandomPerspective(distortion_scale, p)`: bilinear, fill 0; with probability 1 - p the image keeps its geometry."""
    stage = "perspective"

    def __init__(self, distortion_scale=0.5, p=0.5):
        if not 0.0 <= distortion_scale <= 1.0 or not 0.0 <= p <= 1.0:
            raise ValueError("RandomPerspective: distortion_scale and p lie in [0, 1]")
        self.distortion_scale, self.p = float(distortion_scale), float(p)

    def sample(self, p, h, w, generator):
        if _rand(generator) >= self.p:
            return
        bh, bw = int(self.distortion_scale * (h // 2)) + 1, int(self.distortion_scale * (w // 2)) + 1

        def ri(lo, hi):
            return int(torch.randint(lo, hi, (1,), generator=generator))
        p.endpoints = [(ri(0, bw), ri(0, bh)), (ri(w - bw, w), ri(0, bh)), (ri(w - bw, w), ri(h - bh, h)), (ri(0, bw), ri(h - bh, h))]


class ColorJitter:
    """`v2.ColorJitter(brightness, contrast, saturation, hue)` on one channel: saturation does nothing there and is only accepted; hue must be
    0.  Of the random order of the four, whether brightness comes before contrast is all that can be observed."""
    stage = "jitter"

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
        if hue not in (0, 0.0, None, (0, 0), (0.0, 0.0)):
            raise ValueError("ColorJitter: hue is not built (0 in every recipe; nothing to shift on one channel)")
        self.brightness = _range(brightness, "brightness", 1.0, 0.0) if brightness else None
        self.contrast = _range(contrast, "contrast", 1.0, 0.0) if contrast else None
        self.saturation = _range(saturation, "saturation", 1.0, 0.0) if saturation else None

    def sample(self, p, h, w, generator):
        order = torch.randperm(4, generator=generator).tolist()   # 0 brightness, 1 contrast, 2 saturation, 3 hue
        p.brightness_first = order.index(0) < order.index(1)
        if self.brightness is not None:
            p.brightness = _uniform(self.brightness[0], self.brightness[1], generator)
        if self.contrast is not None:
            p.contrast = _uniform(self.contrast[0], self.contrast[1], generator)


def blur_weights(kernel_size, sigma):
    """softmax(-(x / sigma)^2) over x = linspace(-lim, lim, k), lim = (k - 1) / (2 sqrt 2), in float64."""
    lim = (kernel_size - 1) / (2.0 * math.sqrt(2.0))
    x = torch.linspace(-lim, lim, kernel_size, dtype=torch.float64)
    return torch.softmax(-(x / sigma) ** 2, dim=0)


def perspective_coeffs_batch(endpoints, sizes):
    """For every (four end points, (h, w)): c0 .. c7 that map each end point onto its start point (0,0), (w-1,0), (w-1,h-1), (0,h-1).  Float64
    least squares on the host, one batched LAPACK call (each system is solved on its own: a batch gives what single calls give)."""
    rows, rhs = [], []
    for ends, (h, w) in zip(endpoints, sizes):
        start = [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]
        a = []
        for (px, py), (sx, sy) in zip(ends, start):
            a.append([px, py, 1, 0, 0, 0, -sx * px, -sx * py])
            a.append([0, 0, 0, px, py, 1, -sy * px, -sy * py])
        rows.append(a)
        rhs.append([v for s in start for v in s])
    a, b = torch.tensor(rows, dtype=torch.float64), torch.tensor(rhs, dtype=torch.float64)
    return torch.linalg.lstsq(a, b[..., None], driver="gelsd").solution[..., 0].tolist()


def perspective_coeffs(endpoints, h, w):
    return perspective_coeffs_batch([endpoints], [(h, w)])[0]


def _as_image(img, device):
    """(tensor (H, W) fp32 contiguous on the GPU, the input's shape); errors as `utils._device_image` raises them."""
    if not torch.is_tensor(img) or img.dim() not in (2, 3):
        raise TypeError("expected a (1, H, W) or (H, W) tensor (decode PIL images with ToImage / ToDtype first, as the reference pipelines do)")
    if not torch.cuda.is_available():
        raise RuntimeError("acai_omr_amd transforms run on the GPU (HIP augmentation kernels); there is no CPU fallback")
    if img.dim() == 3 and img.shape[0] != 1:
        raise ValueError("expected one channel (NUM_CHANNELS = 1)")
    if img.is_floating_point() is False:
        raise TypeError("expected a float image in [0, 1] (ToDtype(float32, scale=True) first)")
    dev = img.device if img.is_cuda else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    t = img.to(device=dev, dtype=torch.float32).contiguous()
    return t.reshape(t.shape[-2], t.shape[-1]), tuple(img.shape)


class CameraAugment(torch.nn.Module):
    """`v2.RandomApply(transforms, p)` over the camera stages: every stage of `transforms` (a subset of blur, noise, rotation, perspective,
    jitter, in that order) is applied to an image with probability p, or none is.

    sample_params(sizes) draws the per-image parameters on the host; forward(imgs, params) returns the augmented image(s) as GPU tensors
    of the input shapes; to_patches(imgs, patch_size, dtype, params) writes them straight into the packed patch stream (`PackedPatches`) the
    encoders accept, as `DynamicResize.to_patches` does.  Images that are not applied come back unchanged, bit for bit."""

    def __init__(self, transforms: Sequence, p: float = 0.5, device=None, generator=None):
        super().__init__()
        stages = [t.stage for t in transforms]
        if not stages or len(set(stages)) != len(stages) or stages != sorted(stages, key=STAGE_ORDER.index):
            raise ValueError(f"CameraAugment: stages must be a non-empty subset of {STAGE_ORDER} in that order, got {stages}")
        if not 0.0 <= p <= 1.0:
            raise ValueError("CameraAugment: p lies in [0, 1]")
        self.transforms, self.p = list(transforms), float(p)
        self.device = device         # target GPU for CPU inputs (default: the current device)
        self.generator = generator   # host generator of sample_params when none is passed

    def _stage(self, name):
        return next((t for t in self.transforms if t.stage == name), None)

    def sample_params(self, sizes, generator=None) -> List[ImageParams]:
        """One `ImageParams` per (H, W) of `sizes`, drawn from `generator` (default: the module's, else torch's global CPU generator)."""
        g = generator if generator is not None else self.generator
        out = []
        for h, w in sizes:
            p = ImageParams(apply=_rand(g) < self.p)
            if p.apply:
                for t in self.transforms:
                    t.sample(p, int(h), int(w), g)
            out.append(p)
        return out

    # ---- the device side ----------------------------------------------------------------------------------------------------------------
    def _run(self, imgs, params, patch_size=None, dtype=torch.float32):
        from . import _lib, ops
        single = torch.is_tensor(imgs)
        planes, shapes = zip(*[_as_image(im, self.device) for im in ([imgs] if single else list(imgs))])
        dev = planes[0].device
        if any(t.device != dev for t in planes):
            raise RuntimeError("CameraAugment: images on different devices")
        sizes = [tuple(t.shape) for t in planes]
        if params is None:
            params = self.sample_params(sizes)
        elif isinstance(params, ImageParams):
            params = [params]
        if len(params) != len(planes):
            raise ValueError(f"CameraAugment: {len(planes)} images against {len(params)} parameter sets")
        blur, P = self._stage("blur"), patch_size
        k = blur.kernel_size if blur is not None else 1
        for (h, w), p in zip(sizes, params):
            if min(h, w) <= k // 2:
                raise ValueError(f"CameraAugment: a {h} x {w} image cannot be reflect-padded by {k // 2} (each side must exceed it)")
            if p.apply and p.sigma is not None and not p.sigma > 0.0:
                raise ValueError("CameraAugment: blur sigma must be positive")
            if P is not None and (h % P or w % P):
                raise ValueError(f"CameraAugment.to_patches: {h} x {w} is not a multiple of the patch size {P}")
        stages = [t.stage for t in self.transforms]
        do_blur, do_noise, do_jitter = "blur" in stages, "noise" in stages, "jitter" in stages
        npix = [h * w for h, w in sizes]
        total, n = sum(npix), len(planes)
        with torch.cuda.device(dev):
            scratch = torch.empty(2 * total, dtype=torch.float32, device=dev)
            partials = torch.empty(n * _lib.AUG_MEAN_PARTS, dtype=torch.float64, device=dev)
            need_noise = [do_noise and p.apply and p.noise_sigma is not None and p.noise is None for p in params]
            drawn = torch.randn(sum(c for c, nd in zip(npix, need_noise) if nd), dtype=torch.float32, device=dev) if any(need_noise) else None
            if P is None:
                out = torch.empty(total, dtype=torch.float32, device=dev)
            else:
                if dtype not in (torch.float32, torch.bfloat16):
                    raise TypeError(f"CameraAugment.to_patches: fp32 or bf16 patch stream, got {dtype}")
                out = torch.empty(total // (P * P), P * P, dtype=dtype, device=dev)
            entries, off, noff, row0 = [], 0, 0, 0
            uploads = []   # uploaded noise planes stay alive until the launches that read them are enqueued
            warped = [i for i, p in enumerate(params) if p.apply and p.endpoints is not None]
            coeffs = dict(zip(warped, perspective_coeffs_batch([params[i].endpoints for i in warped], [sizes[i] for i in warped]))) if warped else {}
            for t, (h, w), p, c, nd in zip(planes, sizes, params, npix, need_noise):
                e = _lib.AcaiAugImage()
                e.src, e.H, e.W, e.apply = t.data_ptr(), h, w, int(bool(p.apply))
                e.buf[0], e.buf[1] = scratch.data_ptr() + 4 * off, scratch.data_ptr() + 4 * (total + off)
                e.partials = partials.data_ptr() + 8 * _lib.AUG_MEAN_PARTS * len(entries)
                e.out, e.row0 = (out.data_ptr() + 4 * off, 0) if P is None else (None, row0)
                e.ktaps, e.w[0] = 1, 1.0
                if do_blur and p.apply and p.sigma is not None:
                    e.ktaps = k
                    for j, v in enumerate(blur_weights(k, p.sigma).tolist()):
                        e.w[j] = v
                e.noise_sigma = 0.0
                if do_noise and p.apply and p.noise_sigma is not None:
                    if nd:
                        noise = drawn[noff:noff + c]
                        noff += c
                    else:
                        noise = p.noise
                        if not torch.is_tensor(noise) or noise.numel() != c:
                            raise ValueError(f"CameraAugment: the noise of a {h} x {w} image must hold {c} values")
                        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
                        uploads.append(noise)
                    e.noise, e.noise_sigma = noise.data_ptr(), float(p.noise_sigma)
                ang = math.radians(p.angle) if p.angle is not None else 0.0
                e.rot_cos, e.rot_sin = math.cos(ang), math.sin(ang)
                for j, v in enumerate(coeffs.get(len(entries), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])):
                    e.persp[j] = v
                e.fb = float(p.brightness) if p.brightness is not None else 1.0
                e.fc = float(p.contrast) if p.contrast is not None else 1.0
                e.jitter = ((_lib.AUG_BRIGHTNESS if p.brightness is not None else 0) | (_lib.AUG_CONTRAST if p.contrast is not None else 0)
                            | (_lib.AUG_BRIGHTNESS_FIRST if p.brightness_first else 0))
                entries.append(e)
                off += c
                row0 += c // (P * P) if P is not None else 0
            table = ops.augment_table(entries, dev)
            mh, mw = max(h for h, _ in sizes), max(w for _, w in sizes)
            cur = -1
            if do_blur or do_noise:
                ops.augment_blur_noise(table, n, mh, mw, cur, 0, 1, do_blur=do_blur, do_noise=do_noise)
                cur = 1
            for name in ("rotation", "perspective"):
                if name in stages:
                    nxt = 0 if cur != 0 else 1
                    ops.augment_warp(table, n, mh, mw, cur, nxt, name == "perspective")
                    cur = nxt
            if P is None:
                ops.augment_jitter_out(table, n, mh, mw, cur, do_jitter=do_jitter)
            else:
                ops.augment_jitter_out(table, n, mh, mw, cur, do_jitter=do_jitter, patches=out, patch_size=P)
        if P is not None:
            return PackedPatches(out, [(h // P, w // P) for h, w in sizes], P)
        res, off = [], 0
        for shape, c in zip(shapes, npix):
            res.append(out[off:off + c].view(shape))
            off += c
        return res[0] if single else res

    def forward(self, imgs, params=None):
        """One image ((1, H, W) or (H, W), float in [0, 1]) or a list of them -> the augmented image(s), GPU tensors of the input shapes.
        params: what `sample_params` returns for these sizes (one `ImageParams` per image), or None to draw them now."""
        return self._run(imgs, params)

    def to_patches(self, imgs, patch_size, dtype=torch.float32, params=None):
        """`forward` + the encoder's Unfold for a list of images in one call: the last stage writes the nn.Unfold(P, P) rows of every image
        into ONE packed [sum N, P*P] tensor (fp32 or bf16).  patchify(forward(img)) gives the same rows bit for bit (bf16: rounded once)."""
        return self._run(imgs, params, patch_size=int(patch_size), dtype=dtype)


# ---- the reference's recipes ---------------------------------------------------------------------------------------------------------------
def _camera(sigma, noise, degrees, distortion, brightness, contrast, p, **kw):
    return CameraAugment([GaussianBlur(15, sigma), GaussianNoise(sigma=noise), RandomRotation((-degrees, degrees)),
                          RandomPerspective(distortion, p=1.0), ColorJitter(brightness=brightness, saturation=0.2, contrast=contrast, hue=0)], p=p, **kw)


def _grandstaff(distortion, brightness, contrast, p, **kw):
    return CameraAugment([RandomPerspective(distortion, p=1.0), ColorJitter(brightness=brightness, saturation=0.2, contrast=contrast, hue=0)], p=p, **kw)


def pretrain_camera_augment(p=0.2, **kw):
    """pre_train.py:178-184 (AUGMENTATION_P = 0.2)."""
    return _camera(1.0, 0.03, 1.0, 0.06, 0.2, 0.2, p, **kw)


def pretrain_grandstaff_augment(p=0.2, **kw):
    """pre_train.py:187-190, applied with `augment_p` by the GrandStaff wrapper (:196)."""
    return _grandstaff(0.08, 0.2, 0.2, p, **kw)


def fine_tune_camera_augment(p=0.5, **kw):
    """omr_teacher_force_train.py:320-326 (AUGMENTATION_P = 0.5)."""
    return _camera((0.2, 0.7), 0.03, 2.0, 0.2, 0.15, 0.2, p, **kw)


def fine_tune_grandstaff_augment(p=0.5, **kw):
    """omr_teacher_force_train.py:328-331."""
    return _grandstaff(0.2, 0.15, 0.2, p, **kw)


def grpo_camera_augment(p=0.3, **kw):
    """omr_grpo_train.py:530-536 (AUGMENTATION_P = 0.3)."""
    return _camera((0.1, 0.5), 0.01, 2.0, 0.2, 0.1, 0.2, p, **kw)


def grpo_grandstaff_augment(p=0.3, **kw):
    """omr_grpo_train.py:538-541."""
    return _grandstaff(0.2, 0.1, 0.2, p, **kw)
