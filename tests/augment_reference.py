"""CPU restatement of the camera augmentation (acai_omr_amd/augment.py, csrc/augment.hip) as the stock aten ops torchvision's v2 tensor path
calls - F.pad(reflect) + conv2d, grid_sample on a grid built like `_affine_grid` / `_perspective_grid`, clamp arithmetic - in float32 or
float64.  torchvision is not installed where this project is tested, so this file (with the text of include/acai_omr_hip.h) IS the contract:
the float64 run is the yardstick of the GPU tests, the float32 run gives the allowance (what stock aten float32 loses against it)."""
import math

import torch
import torch.nn.functional as F


def blur_weights(kernel_size, sigma, dtype):
    lim = (kernel_size - 1) / (2.0 * math.sqrt(2.0))
    x = torch.linspace(-lim, lim, kernel_size, dtype=dtype)
    return torch.softmax(-(x / sigma) ** 2, dim=0)


def gaussian_blur(img, kernel_size, sigma):
    """img (H, W) -> (H, W): reflect padding by k // 2, convolution with w w^T."""
    w = blur_weights(kernel_size, sigma, img.dtype)
    k2 = (w[:, None] * w[None, :])[None, None]
    r = kernel_size // 2
    return F.conv2d(F.pad(img[None, None], (r, r, r, r), mode="reflect"), k2)[0, 0]


def gaussian_noise(img, noise_sigma, noise):
    return (img + noise_sigma * noise.to(img.dtype)).clamp(0.0, 1.0)


def _sample_fill0(img, grid):
    """grid_sample(bilinear, zeros, align_corners=False) of the image and of an all-ones mask, multiplied (the fill path with fill = 0)."""
    both = torch.stack([img, torch.ones_like(img)])[None]
    s = F.grid_sample(both, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]
    return s[0] * s[1]


def rotate(img, angle):
    H, W = img.shape
    dt = img.dtype
    t = math.radians(angle)
    theta = torch.tensor([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0]], dtype=dt)
    base = torch.empty(1, H, W, 3, dtype=dt)
    base[..., 0] = torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, W, dtype=dt)
    base[..., 1] = torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, H, dtype=dt)[:, None]
    base[..., 2] = 1
    rescaled = theta.t() / torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
    grid = (base.view(1, H * W, 3) @ rescaled[None]).view(1, H, W, 2)
    return _sample_fill0(img, grid)


def perspective_coeffs(endpoints, H, W):
    """float64 least squares: the coefficients that map every end point onto its start point."""
    start = [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)]
    a = torch.zeros(8, 8, dtype=torch.float64)
    for i, ((px, py), (sx, sy)) in enumerate(zip(endpoints, start)):
        a[2 * i] = torch.tensor([px, py, 1, 0, 0, 0, -sx * px, -sx * py], dtype=torch.float64)
        a[2 * i + 1] = torch.tensor([0, 0, 0, px, py, 1, -sy * px, -sy * py], dtype=torch.float64)
    b = torch.tensor(start, dtype=torch.float64).reshape(8)
    return torch.linalg.lstsq(a, b, driver="gelsd").solution.tolist()


def perspective(img, endpoints):
    H, W = img.shape
    dt = img.dtype
    c = perspective_coeffs(endpoints, H, W)
    theta1 = torch.tensor([[c[0], c[1], c[2]], [c[3], c[4], c[5]]], dtype=dt)
    theta2 = torch.tensor([[c[6], c[7], 1.0], [c[6], c[7], 1.0]], dtype=dt)
    base = torch.empty(1, H, W, 3, dtype=dt)
    base[..., 0] = torch.linspace(0.5, W + 0.5 - 1, W, dtype=dt)
    base[..., 1] = torch.linspace(0.5, H + 0.5 - 1, H, dtype=dt)[:, None]
    base[..., 2] = 1
    rescaled = theta1.t() / torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
    g1 = base.view(1, H * W, 3) @ rescaled[None]
    g2 = base.view(1, H * W, 3) @ theta2.t()[None]
    grid = (g1 / g2 - 1.0).view(1, H, W, 2)
    return _sample_fill0(img, grid)


def color_jitter(img, fb, fc, brightness_first):
    def bright(v):
        return v if fb is None else (v * fb).clamp(0.0, 1.0)

    def contrast(v):
        return v if fc is None else (fc * v + (1.0 - fc) * v.mean()).clamp(0.0, 1.0)
    return contrast(bright(img)) if brightness_first else bright(contrast(img))


def augment(img, p, noise=None, kernel_size=15, dtype=torch.float64):
    """The stages an `ImageParams`-like object `p` names, in the reference's order, on one (H, W) or (1, H, W) image."""
    shape = img.shape
    v = img.reshape(shape[-2], shape[-1]).to(dtype)
    if p.apply:
        if p.sigma is not None:
            v = gaussian_blur(v, kernel_size, p.sigma)
        if p.noise_sigma is not None:
            v = gaussian_noise(v, p.noise_sigma, (noise if noise is not None else p.noise).reshape(v.shape))
        if p.angle is not None:
            v = rotate(v, p.angle)
        if p.endpoints is not None:
            v = perspective(v, p.endpoints)
        if p.brightness is not None or p.contrast is not None:
            v = color_jitter(v, p.brightness, p.contrast, p.brightness_first)
    return v.reshape(shape)


def staff_image(H, W, seed=0):
    """A white page with sharp dark staff lines, stems and a few grey blobs: sharp edges expose coordinate rounding."""
    g = torch.Generator().manual_seed(seed)
    img = torch.ones(H, W, dtype=torch.float32)
    for top in range(max(2, H // 16), H - 10, max(12, H // 5)):
        for i in range(5):
            y = top + i * max(2, H // 64)
            if y + 1 < H:
                img[y:y + max(1, H // 256), :] = 0.0
    for x in torch.randint(0, W, (max(4, W // 24),), generator=g).tolist():
        y0 = int(torch.randint(0, max(1, H - H // 4), (1,), generator=g))
        img[y0:y0 + H // 4, x:x + 2] = 0.0
    for _ in range(max(3, W // 64)):
        y0, x0 = int(torch.randint(0, H - 4, (1,), generator=g)), int(torch.randint(0, W - 6, (1,), generator=g))
        img[y0:y0 + 4, x0:x0 + 6] = float(torch.rand(1, generator=g)) * 0.6
    return img
