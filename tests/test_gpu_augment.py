"""The camera augmentation kernels (csrc/augment.hip, acai_omr_amd/augment.py) against the CPU restatement tests/augment_reference.py with the
SAME injected parameters and noise.

Yardstick: the float64 restatement.  Allowance, per case: e_ref = max |stock aten float32 on the CPU - float64| on the same inputs, and the
kernel must stay within max(2 e_ref, 2e-6) of float64, in the maximum and in the mean.  Factor 2: the kernel may order the coordinate
arithmetic differently and a bilinear sample moves by the coordinate error times the local contrast; 2e-6 is the bar tests/test_resize.py
uses for float32 image arithmetic and covers stages whose e_ref is near zero.  Every figure is printed before it is asserted."""
import pytest
import torch

import augment_reference as R
from conftest import load_golden

from acai_omr_amd import augment as A

pytestmark = pytest.mark.gpu

K = 15
SIZES = [(512, 2048), (48, 80), (45, 77), (768, 3072)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from acai_omr_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _full():
    return A.CameraAugment([A.GaussianBlur(K, 1.0), A.GaussianNoise(sigma=0.03), A.RandomRotation(2), A.RandomPerspective(0.2, p=1.0),
                            A.ColorJitter(brightness=0.2, contrast=0.2)], p=1.0)


def _only(stage):
    return A.CameraAugment([{"blur": A.GaussianBlur(K, 1.0), "noise": A.GaussianNoise(sigma=0.03), "rotation": A.RandomRotation(2),
                             "perspective": A.RandomPerspective(0.2, p=1.0), "jitter": A.ColorJitter(brightness=0.2, contrast=0.2)}[stage]], p=1.0)


def _ends(h, w, scale, inward):
    """End points at the edge of RandomPerspective's ranges: every corner pulled in as far as the distortion scale allows (inward), or only the
    top-left one while the others stay where they are."""
    bh, bw = int(scale * (h // 2)) + 1, int(scale * (w // 2)) + 1
    if inward:
        return [(bw - 1, bh - 1), (w - bw, bh - 1), (w - bw, h - bh), (bw - 1, h - bh)]
    return [(bw - 1, bh - 1), (w - 1, 0), (w - 1, h - 1), (0, h - 1)]


def _noise(h, w, seed):
    return torch.randn(h, w, generator=torch.Generator().manual_seed(seed))


def _recipe_edges(h, w):
    """Both ends of every recipe's ranges (pre-train, fine-tune, GRPO), both jitter orders."""
    P = A.ImageParams
    return {
        "pretrain-lo": P(sigma=1.0, noise_sigma=0.03, angle=-1.0, endpoints=_ends(h, w, 0.06, True), brightness=0.8, contrast=0.8, brightness_first=True),
        "pretrain-hi": P(sigma=1.0, noise_sigma=0.03, angle=1.0, endpoints=_ends(h, w, 0.06, False), brightness=1.2, contrast=1.2, brightness_first=False),
        "finetune-lo": P(sigma=0.2, noise_sigma=0.03, angle=-2.0, endpoints=_ends(h, w, 0.2, True), brightness=0.85, contrast=0.8, brightness_first=False),
        "finetune-hi": P(sigma=0.7, noise_sigma=0.03, angle=2.0, endpoints=_ends(h, w, 0.2, False), brightness=1.15, contrast=1.2, brightness_first=True),
        "grpo-lo": P(sigma=0.1, noise_sigma=0.01, angle=-2.0, endpoints=_ends(h, w, 0.2, False), brightness=0.9, contrast=1.2, brightness_first=True),
        "grpo-hi": P(sigma=0.5, noise_sigma=0.01, angle=2.0, endpoints=_ends(h, w, 0.2, True), brightness=1.1, contrast=0.8, brightness_first=False),
    }


def _check(name, aug, img, p, dev):
    """Kernel against the float64 restatement, allowance from the float32 one.  Returns the figures."""
    noise = p.noise
    got = aug(img.to(dev), params=p).cpu().double()
    ref64 = R.augment(img, p, noise=noise, kernel_size=K, dtype=torch.float64)
    ref32 = R.augment(img, p, noise=noise, kernel_size=K, dtype=torch.float32).double()
    e_ref, e_ref_mean = float((ref32 - ref64).abs().max()), float((ref32 - ref64).abs().mean())
    e, e_mean = float((got - ref64).abs().max()), float((got - ref64).abs().mean())
    print(f"augment {name} {tuple(img.shape)}: kernel max {e:.3e} mean {e_mean:.3e} | aten fp32 max {e_ref:.3e} mean {e_ref_mean:.3e}")
    assert got.shape == img.shape
    assert e <= max(2 * e_ref, 2e-6), (name, e, e_ref)
    assert e_mean <= max(2 * e_ref_mean, 2e-6), (name, e_mean, e_ref_mean)
    return e, e_ref


@pytest.mark.parametrize("h,w", SIZES)
def test_each_stage_alone(dev, h, w):
    img = R.staff_image(h, w, seed=h)
    P = A.ImageParams
    for sigma in (0.1, 0.2, 0.5, 0.7, 1.0):
        _check(f"blur sigma={sigma}", _only("blur"), img, P(sigma=sigma), dev)
    for ns in (0.01, 0.03):
        _check(f"noise sigma={ns}", _only("noise"), img, P(noise_sigma=ns, noise=_noise(h, w, 3)), dev)
    for angle in (-2.0, -1.0, 1.0, 2.0, 0.37):
        _check(f"rotation {angle}", _only("rotation"), img, P(angle=angle), dev)
    for scale in (0.06, 0.08, 0.2):
        for inward in (True, False):
            _check(f"perspective {scale} inward={inward}", _only("perspective"), img, P(endpoints=_ends(h, w, scale, inward)), dev)
    for fb, fc in ((0.8, 1.2), (1.2, 0.8), (0.85, 0.8), (1.15, 1.2), (0.9, 1.0), (1.1, 1.2)):
        for first in (True, False):
            _check(f"jitter fb={fb} fc={fc} brightness_first={first}", _only("jitter"), img, P(brightness=fb, contrast=fc, brightness_first=first), dev)


@pytest.mark.parametrize("h,w", SIZES)
def test_full_pipeline_at_the_edges_of_every_recipe(dev, h, w):
    img = R.staff_image(h, w, seed=h + 1)
    for i, (name, p) in enumerate(_recipe_edges(h, w).items()):
        p.noise = _noise(h, w, 10 + i)
        _check(name, _full(), img, p, dev)
    # the GrandStaff pair
    pair = A.CameraAugment([A.RandomPerspective(0.2, p=1.0), A.ColorJitter(brightness=0.15, contrast=0.2)], p=1.0)
    _check("grandstaff pair", pair, img, A.ImageParams(endpoints=_ends(h, w, 0.2, True), brightness=1.15, contrast=0.8, brightness_first=False), dev)
    # a (1, H, W) input keeps its shape
    p = _recipe_edges(h, w)["pretrain-lo"]
    p.noise = _noise(h, w, 1)
    assert _full()(img[None].to(dev), params=p).shape == (1, h, w)


RAGGED = [(48, 80), (32, 96), (64, 64), (16, 208), (80, 48), (512, 2048), (96, 32)]


def _ragged(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    aug = _full()
    imgs = [R.staff_image(h, w, seed=i) for i, (h, w) in enumerate(RAGGED)]
    params = aug.sample_params(RAGGED, generator=g)
    for i, (p, (h, w)) in enumerate(zip(params, RAGGED)):
        p.noise = _noise(h, w, 40 + i)
    params[2].apply = params[5].apply = False
    return aug, [im.to(dev) for im in imgs], params


def test_ragged_batch_equals_one_by_one_and_is_reproducible(dev):
    aug, imgs, params = _ragged(dev)
    batch = aug(imgs, params=params)
    again = aug(imgs, params=params)
    assert len(batch) == len(imgs)
    for i, (im, p, b, b2) in enumerate(zip(imgs, params, batch, again)):
        assert b.shape == im.shape and b.is_cuda and b.dtype == torch.float32
        assert torch.equal(b, aug(im, params=p)), i          # one call for all = one call each, bit for bit
        assert torch.equal(b, b2), i                         # the contrast mean is order-fixed
        if not p.apply:
            assert torch.equal(b, im), i                     # not applied: unchanged, bit for bit
        else:
            assert float((b - im).abs().max()) > 1e-2
    # negative zero and values outside [0, 1] survive a pass-through untouched
    odd = torch.tensor([[-0.0, 1.5, -2.0, float("inf")] * 4] * 8, device=dev)
    back = aug(odd, params=A.ImageParams(apply=False))
    assert torch.equal(back.view(torch.int32), odd.view(torch.int32))


def test_noise_drawn_on_the_device_follows_the_generator_convention(dev):
    aug = A.CameraAugment([A.GaussianNoise(sigma=0.05)], p=1.0)
    img = torch.full((64, 128), 0.5, device=dev)
    p = A.ImageParams(noise_sigma=0.05)
    torch.manual_seed(3)
    a = aug([img, img], params=[p, p])
    torch.manual_seed(3)
    b = aug([img, img], params=[p, p])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], a[1])
    d = (a[0] - 0.5) / 0.05
    assert abs(float(d.mean())) < 0.05 and abs(float(d.std()) - 1.0) < 0.05


def test_to_patches_equals_patchify_of_forward(dev):
    from acai_omr_amd import ops
    from acai_omr_amd.models.models import OMREncoder
    from acai_omr_amd.utils import DynamicResize, PackedPatches
    P = 16
    aug, imgs, params = _ragged(dev, seed=1)
    pk = aug.to_patches(imgs, P, params=params)
    outs = aug(imgs, params=params)
    rows = []
    for o in outs:
        r = torch.empty((o.shape[-2] // P) * (o.shape[-1] // P), P * P, device=dev)
        ops.patchify(o.reshape(1, *o.shape[-2:]).contiguous(), P, r, 0)
        rows.append(r)
    want = torch.cat(rows)
    assert isinstance(pk, PackedPatches) and pk.patch_size == P and pk.dims == [(h // P, w // P) for h, w in RAGGED]
    assert pk.patches.shape == want.shape and torch.equal(pk.patches, want)
    assert torch.equal(aug.to_patches(imgs, P, dtype=torch.bfloat16, params=params).patches, want.to(torch.bfloat16))
    with pytest.raises(ValueError):
        aug.to_patches([torch.rand(40, 64, device=dev)], P)
    # the encoder takes the packed patches as it takes DynamicResize.to_patches' and as it takes the image tensors
    enc = OMREncoder(P, 60, 200, num_layers=2, hidden_dim=64, num_heads=2, mlp_dim=128).to(dev).eval()
    with torch.no_grad():
        a, ma = enc([o.reshape(1, *o.shape[-2:]) for o in outs])
        b, mb = enc(pk)
    assert torch.equal(ma, mb) and torch.equal(a, b)
    tr = DynamicResize(P, 512, 60, 200, True)
    pk0 = tr.to_patches([torch.rand(1, 300, 1100)])
    assert type(pk0) is type(pk) and pk0.patches.dtype == pk.patches.dtype


def test_argument_errors(dev):
    aug = _full()
    for shape in ((7, 64), (64, 7), (5, 5)):
        with pytest.raises(ValueError):
            aug(torch.rand(*shape, device=dev), params=A.ImageParams(sigma=1.0))
    assert aug(torch.rand(8, 8, device=dev), params=A.ImageParams(sigma=1.0)).shape == (8, 8)   # side 8 > 15 // 2
    with pytest.raises(ValueError):
        A.GaussianBlur(14, 1.0)
    with pytest.raises(ValueError):
        A.GaussianBlur(15, 0.0)
    with pytest.raises(ValueError):
        aug(torch.rand(32, 32, device=dev), params=A.ImageParams(sigma=-1.0))
    with pytest.raises(ValueError):
        aug(torch.rand(3, 32, 32, device=dev))
    with pytest.raises(ValueError):
        aug([torch.rand(32, 32, device=dev)] * 2, params=[A.ImageParams()])
    with pytest.raises(ValueError):
        aug(torch.rand(32, 32, device=dev), params=A.ImageParams(noise_sigma=0.1, noise=torch.randn(5)))
    with pytest.raises(TypeError):
        aug("image")
    with pytest.raises(TypeError):
        aug(torch.rand(1, 1, 32, 32, device=dev))
    with pytest.raises(TypeError):
        aug(torch.zeros(32, 32, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        aug.to_patches([torch.rand(32, 32, device=dev)], 16, dtype=torch.float16)
    from acai_omr_amd import ops
    with pytest.raises(RuntimeError):
        ops.augment_warp(torch.zeros(296, dtype=torch.uint8), 1, 8, 8, -1, 0, False)
    with pytest.raises(ValueError):
        ops.augment_warp(torch.zeros(100, dtype=torch.uint8, device=dev), 1, 8, 8, -1, 0, False)
    with pytest.raises(ValueError):
        ops.augment_warp(torch.zeros(296, dtype=torch.uint8, device=dev), 1, 8, 8, 0, 0, False)
    # a CPU image is uploaded once, as the resize transforms do
    cpu = R.staff_image(48, 80)
    p = A.ImageParams(angle=1.0)
    assert torch.equal(_only("rotation")(cpu, params=p), _only("rotation")(cpu.to(dev), params=p))


class _Loader(list):
    pass


def test_pretrain_epoch_augments_the_input_and_keeps_the_target_clean(dev):
    from acai_omr_amd.models.models import MAE, MAELoss
    from acai_omr_amd.optim import FusedAdamW
    from acai_omr_amd.train import loops
    from acai_omr_amd.utils import cosine_anneal_with_warmup
    fx = load_golden("mae_small")
    cfg = fx["cfg"]
    P = cfg["P"]
    g = torch.Generator().manual_seed(21)
    shapes = [[(8, 16), (24, 40)], [(12, 20), (16, 16), (24, 24)]]
    batches = _Loader([[(im, im.clone()) for im in (torch.rand(1, h, w, generator=g) for h, w in b)] for b in shapes])
    noises = [[torch.rand((im.shape[-2] // P) * (im.shape[-1] // P), generator=g) for im, _ in b] for b in batches]
    aug = _full()
    params = [aug.sample_params(b, generator=g) for b in shapes]
    for ps, b in zip(params, shapes):
        for p, (h, w) in zip(ps, b):
            p.noise = torch.randn(h, w, generator=g)
        ps[0].apply = False

    class Injected(torch.nn.Module):
        def __init__(self, inner, queue):
            super().__init__()
            self.inner, self.queue, self.seen = inner, list(queue), []

        def forward(self, batch):
            self.seen.append([(x.detach().clone(), y.detach().clone()) for x, y in batch])
            return self.inner(batch, noises=self.queue.pop(0))

    def epoch(loader, **kw):
        mae = MAE(cfg["mask_ratio"], P, cfg["pe_h"], cfg["pe_w"], encoder_hidden_dim=cfg["enc_dim"], decoder_hidden_dim=cfg["dec_dim"],
                  encoder_kwargs=cfg["enc_kwargs"], decoder_kwargs=cfg["dec_kwargs"])
        mae.load_state_dict(fx["state_dict"])
        mae = mae.to(dev)
        model = Injected(mae, noises)
        opt = FusedAdamW(mae.parameters(), lr=3e-3, betas=(0.9, 0.95), weight_decay=0.05)
        sch = cosine_anneal_with_warmup(opt, 1, 4, 1e-6)
        return loops.pretrain_epoch(model, loader, MAELoss(), opt, sch, dev, **kw), model.seen

    queue = list(params)
    got, seen = epoch(batches, augment=lambda imgs: aug(imgs, params=queue.pop(0)))
    by_hand = _Loader([[(a.cpu(), y) for a, (_, y) in zip(aug([x.to(dev) for x, _ in b], params=ps), b)] for b, ps in zip(batches, params)])
    want, seen_hand = epoch(by_hand)
    plain, seen_plain = epoch(batches)
    today, _ = epoch(batches, augment=None)
    print(f"pretrain_epoch: augmented {got:.8f} by hand {want:.8f} plain {plain:.8f}")
    for sb, hb, pb, b in zip(seen, seen_hand, seen_plain, batches):
        for (x, y), (hx, hy), (px, py), (cx, cy) in zip(sb, hb, pb, b):
            assert torch.equal(x, hx) and torch.equal(y, hy)                          # the model saw the augmented input ...
            assert torch.equal(y.cpu(), cy) and torch.equal(py.cpu(), cy)             # ... and the clean target
            assert torch.equal(px.cpu(), cx)                                          # without `augment` the batch is untouched
    assert not torch.equal(seen[0][1][0], seen_plain[0][1][0]) and torch.equal(seen[0][0][0], seen_plain[0][0][0])   # (image 0 of a batch: not applied)
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want)
    assert abs(got - plain) > 1e-5
    assert abs(today - plain) <= 1e-6 * max(1.0, abs(plain)), (today, plain)
