"""CPU checks of the camera augmentation (no GPU): parameter sampling (ranges, formulas, determinism, the apply probability), the CPU
restatement tests/augment_reference.py against itself where the answer is known, the recipe constructors, and the declarations of the new
C-ABI symbols."""
import math
import os
import re

import pytest
import torch

import augment_reference as R
from conftest import ROOT

from acai_omr_amd import augment as A


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- parameter sampling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 64), (512, 2048)])
def test_sampled_parameters_lie_in_the_recipe_ranges(h, w):
    aug = A.fine_tune_camera_augment(p=1.0)
    bh, bw = int(0.2 * (h // 2)) + 1, int(0.2 * (w // 2)) + 1
    assert (bh, bw) == {(32, 64): (4, 7), (512, 2048): (52, 205)}[(h, w)]
    first = set()
    for p in aug.sample_params([(h, w)] * 300, generator=_gen(1)):
        assert p.apply and 0.2 <= p.sigma <= 0.7 and p.noise_sigma == 0.03 and -2.0 <= p.angle <= 2.0
        assert 0.85 <= p.brightness <= 1.15 and 0.8 <= p.contrast <= 1.2
        (tlx, tly), (trx, try_), (brx, bry), (blx, bly) = p.endpoints
        assert 0 <= tlx < bw and 0 <= tly < bh and w - bw <= trx < w and 0 <= try_ < bh
        assert w - bw <= brx < w and h - bh <= bry < h and 0 <= blx < bw and h - bh <= bly < h
        first.add(p.brightness_first)
    assert first == {True, False}


def test_sampling_spreads_over_the_whole_range():
    aug = A.grpo_camera_augment(p=1.0)
    ps = aug.sample_params([(64, 128)] * 2000, generator=_gen(2))
    sig = torch.tensor([p.sigma for p in ps])
    ang = torch.tensor([p.angle for p in ps])
    assert sig.min() < 0.11 and sig.max() > 0.49 and abs(float(sig.mean()) - 0.3) < 0.02
    assert ang.min() < -1.9 and ang.max() > 1.9 and abs(float(ang.mean())) < 0.15
    share = sum(p.brightness_first for p in ps) / len(ps)
    assert abs(share - 0.5) < 5 * math.sqrt(0.25 / len(ps))
    xs = {p.endpoints[0][0] for p in ps}
    assert xs == set(range(int(0.2 * 64) + 1))   # randint[0, bw) reaches every value


def test_fixed_forms_and_single_number_arguments():
    aug = A.CameraAugment([A.GaussianBlur(15, sigma=1), A.RandomRotation(3), A.ColorJitter(brightness=0.25)], p=1.0)
    for p in aug.sample_params([(40, 40)] * 50, generator=_gen(3)):
        assert p.sigma == 1.0 and -3.0 <= p.angle <= 3.0 and 0.75 <= p.brightness <= 1.25
        assert p.contrast is None and p.noise_sigma is None and p.endpoints is None
    assert A.RandomRotation((-1, 1)).degrees == (-1.0, 1.0) and A.ColorJitter(contrast=(0.5, 1.5)).contrast == (0.5, 1.5)
    assert A.ColorJitter(brightness=1.5).brightness == (0.0, 2.5)   # clipped at 0 as torchvision does


def test_same_seed_same_parameters():
    aug = A.pretrain_camera_augment()
    sizes = [(32, 64), (48, 80), (512, 2048)] * 20
    a, b = aug.sample_params(sizes, generator=_gen(7)), aug.sample_params(sizes, generator=_gen(7))
    assert a == b and a != aug.sample_params(sizes, generator=_gen(8))
    assert any(p.apply for p in a) and not all(p.apply for p in a)
    for p in a:
        if not p.apply:
            assert p == A.ImageParams(apply=False)


def test_apply_probability():
    sizes = [(32, 64)] * 4000
    assert not any(p.apply for p in A.pretrain_camera_augment(p=0.0).sample_params(sizes[:500], generator=_gen(0)))
    assert all(p.apply for p in A.pretrain_camera_augment(p=1.0).sample_params(sizes[:500], generator=_gen(0)))
    n = sum(p.apply for p in A.fine_tune_camera_augment(p=0.5).sample_params(sizes, generator=_gen(11)))
    assert abs(n - 2000) <= 5 * math.sqrt(4000 * 0.25), n   # binomial 5-sigma band


def test_constructor_argument_errors():
    with pytest.raises(ValueError):
        A.GaussianBlur(14, 1.0)
    with pytest.raises(ValueError):
        A.GaussianBlur(15, 0.0)
    with pytest.raises(ValueError):
        A.GaussianBlur(15, (-0.1, 0.5))
    with pytest.raises(ValueError):
        A.ColorJitter(hue=0.1)
    with pytest.raises(ValueError):
        A.CameraAugment([A.RandomRotation(1), A.GaussianBlur(15, 1.0)])   # not the reference's order
    with pytest.raises(ValueError):
        A.CameraAugment([])


def test_no_cpu_fallback_and_input_type_errors():
    aug = A.pretrain_camera_augment(p=1.0)
    with pytest.raises(TypeError):
        aug([[0.0, 1.0]])
    with pytest.raises(TypeError):
        aug(torch.zeros(2, 3, 32, 32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            aug(torch.zeros(1, 32, 64))
        with pytest.raises(RuntimeError):
            aug.to_patches([torch.zeros(32, 64)], 16)


# ---- the restatement against itself -----------------------------------------------------------------------------------------------------------
def _img(h=32, w=48):
    return R.staff_image(h, w, seed=5).double()


def test_identity_parameters_return_the_image():
    img = _img()
    h, w = img.shape
    assert float((R.rotate(img, 0.0) - img).abs().max()) < 1e-12
    assert float((R.perspective(img, [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]) - img).abs().max()) < 1e-9
    assert torch.equal(R.color_jitter(img, 1.0, 1.0, True), img) and torch.equal(R.color_jitter(img, 1.0, 1.0, False), img)
    assert float((R.gaussian_blur(img, 15, 1e-3) - img).abs().max()) < 1e-12
    assert torch.equal(R.gaussian_noise(img, 0.0, torch.randn(h, w, generator=_gen(0))), img)
    p = A.ImageParams(apply=False, sigma=1.0, angle=2.0)
    assert torch.equal(R.augment(img, p), img)


def test_rotation_by_180_degrees_flips_an_even_sized_image():
    img = _img(32, 48)
    assert float((R.rotate(img, 180.0) - img.flip(0, 1)).abs().max()) < 1e-9


def test_blur_weights_and_reflect_padding():
    w = R.blur_weights(15, 1.0, torch.float64)
    assert abs(float(w.sum()) - 1.0) < 1e-14 and torch.equal(w, w.flip(0)) and int(w.argmax()) == 7
    assert torch.allclose(A.blur_weights(15, 0.37), R.blur_weights(15, 0.37, torch.float64), rtol=0, atol=1e-15)
    assert float((R.gaussian_blur(torch.full((20, 24), 0.3, dtype=torch.float64), 15, 2.0) - 0.3).abs().max()) < 1e-14
    # reflection without repeating the edge pixel: a ramp's blurred first pixel averages (1, 0, 1) around it, not (0, 0, 1)
    ramp = torch.arange(16, dtype=torch.float64)[None, :].repeat(16, 1)
    w3 = R.blur_weights(3, 1.0, torch.float64)
    assert abs(float(R.gaussian_blur(ramp, 3, 1.0)[8, 0]) - float(w3[0] * 1 + w3[1] * 0 + w3[2] * 1)) < 1e-14


def test_perspective_coefficients_map_end_points_onto_start_points():
    h, w = 512, 2048
    ends = [(150, 20), (1900, 3), (2047, 470), (7, 505)]
    for c in (R.perspective_coeffs(ends, h, w), A.perspective_coeffs(ends, h, w)):
        for (px, py), (sx, sy) in zip(ends, [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]):
            d = c[6] * px + c[7] * py + 1
            assert abs((c[0] * px + c[1] * py + c[2]) / d - sx) < 1e-7 and abs((c[3] * px + c[4] * py + c[5]) / d - sy) < 1e-7
    assert R.perspective_coeffs(ends, h, w) == A.perspective_coeffs(ends, h, w)


def test_jitter_order_is_observable_and_float32_tracks_float64():
    img = _img()
    a, b = R.color_jitter(img, 1.2, 0.8, True), R.color_jitter(img, 1.2, 0.8, False)
    assert float((a - b).abs().max()) > 1e-3
    p = A.ImageParams(sigma=0.7, noise_sigma=0.03, angle=1.5, endpoints=[(3, 2), (44, 1), (47, 30), (1, 29)], brightness=0.9, contrast=1.2,
                      brightness_first=False)
    noise = torch.randn(32, 48, generator=_gen(4))
    d = float((R.augment(img.float(), p, noise=noise, dtype=torch.float32).double() - R.augment(img, p, noise=noise)).abs().max())
    assert 0.0 < d < 1e-3


# ---- recipes and declarations -------------------------------------------------------------------------------------------------------------------
def _numbers(aug):
    out = {"p": aug.p, "stages": [t.stage for t in aug.transforms]}
    for t in aug.transforms:
        if t.stage == "blur":
            out["k"], out["sigma"] = t.kernel_size, t.sigma
        elif t.stage == "noise":
            out["noise"] = t.sigma
        elif t.stage == "rotation":
            out["degrees"] = t.degrees
        elif t.stage == "perspective":
            out["distortion"], out["pp"] = t.distortion_scale, t.p
        else:
            out["brightness"], out["contrast"] = t.brightness, t.contrast
    return out


def test_recipes_carry_the_reference_numbers():
    full = list(A.STAGE_ORDER)
    close = lambda a, b: all(abs(x - y) < 1e-12 for x, y in zip(a, b))   # noqa: E731
    n = _numbers(A.pretrain_camera_augment())
    assert (n["p"], n["stages"], n["k"], n["sigma"], n["noise"], n["degrees"], n["distortion"], n["pp"]) == (0.2, full, 15, (1.0, 1.0), 0.03, (-1.0, 1.0), 0.06, 1.0)
    assert close(n["brightness"], (0.8, 1.2)) and close(n["contrast"], (0.8, 1.2))
    n = _numbers(A.fine_tune_camera_augment())
    assert (n["p"], n["stages"], n["k"], n["sigma"], n["noise"], n["degrees"], n["distortion"], n["pp"]) == (0.5, full, 15, (0.2, 0.7), 0.03, (-2.0, 2.0), 0.2, 1.0)
    assert close(n["brightness"], (0.85, 1.15)) and close(n["contrast"], (0.8, 1.2))
    n = _numbers(A.grpo_camera_augment())
    assert (n["p"], n["stages"], n["k"], n["sigma"], n["noise"], n["degrees"], n["distortion"], n["pp"]) == (0.3, full, 15, (0.1, 0.5), 0.01, (-2.0, 2.0), 0.2, 1.0)
    assert close(n["brightness"], (0.9, 1.1)) and close(n["contrast"], (0.8, 1.2))
    for make, p, dist, b in ((A.pretrain_grandstaff_augment, 0.2, 0.08, 0.2), (A.fine_tune_grandstaff_augment, 0.5, 0.2, 0.15),
                             (A.grpo_grandstaff_augment, 0.3, 0.2, 0.1)):
        n = _numbers(make())
        assert (n["p"], n["stages"], n["distortion"], n["pp"]) == (p, ["perspective", "jitter"], dist, 1.0)
        assert close(n["brightness"], (1 - b, 1 + b)) and close(n["contrast"], (0.8, 1.2))


def test_new_symbols_are_declared_and_typed():
    import ctypes

    from acai_omr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acai_omr_hip.h")).read()
    for name in ("acai_augment_blur_noise", "acai_augment_warp", "acai_augment_jitter_out"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in _lib._SIGNATURES
    assert "augment.hip" in _lib.SOURCES
    body = hdr[hdr.index("typedef struct AcaiAugImage {"):hdr.index("} AcaiAugImage;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"[a-z0-9_]+\s+\**([^;{}]+);", body) for n in re.findall(r"\*?\s*([a-zA-Z_][a-zA-Z0-9_]*)(?:\[[^\]]*\])?\s*(?:,|$)", decl)]
    assert names == [f for f, _ in _lib.AcaiAugImage._fields_]
    assert ctypes.sizeof(_lib.AcaiAugImage) == 6 * 8 + 10 * 8 + 6 * 4 + 4 * 4 + 4 * _lib.AUG_MAX_TAPS
    assert int(re.search(r"#define ACAI_AUG_MAX_TAPS (\d+)", hdr).group(1)) == _lib.AUG_MAX_TAPS
    assert int(re.search(r"#define ACAI_AUG_MEAN_PARTS (\d+)", hdr).group(1)) == _lib.AUG_MEAN_PARTS
