"""Plain float64 restatement of clipping by the global gradient norm ahead of an AdamW step (`torch.nn.utils.clip_grad_norm_` followed by
`torch.optim.AdamW.step`): the global 2-norm over the gradients that are present, torch's coefficient min(1, max_norm / (norm + 1e-6)), and
the scaled gradients fed to `row_reference.adamw_run`.  Everything is CPU torch."""
import math

import torch

import row_reference as R

ULP32 = 2.0 ** -23      # one fp32 ulp, relative: the bar of every norm comparison
MAX_NORMS = (1.0, 300.0, 1e4)   # against gradient norms of ~285 (~2870 on the louder third step): always clips / only on step 3 / never


def tensor_norms(grads, grad_scale=1.0):
    """float64 2-norm of grad_scale * g for every gradient of the list (None where there is none)."""
    return [None if g is None else abs(grad_scale) * math.sqrt(float((g.double() * g.double()).sum())) for g in grads]


def global_norm(grads, grad_scale=1.0):
    """float64 2-norm of grad_scale * g over all gradients of the list that are present."""
    return abs(grad_scale) * math.sqrt(sum(float((g.double() * g.double()).sum()) for g in grads if g is not None))


def clip_coef(norm, max_norm):
    """torch's coefficient, in float64.  A max_norm that is not positive or is infinite does not clip."""
    if not (max_norm > 0.0 and math.isfinite(max_norm)):
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def clip_coef_fp32(norm32, max_norm):
    """The same formula in fp32 arithmetic from an fp32 norm (a 0-dim CPU tensor), in torch's order: add, divide, clamp."""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm32.float() + 1e-6), max=1.0)


def clipped_adamw_run(params, grads, hyper, max_norm, grad_scale=1.0):
    """`row_reference.adamw_run` over the gradients times grad_scale times each step's clip coefficient.
    Returns (params, exp_avg, exp_avg_sq, steps, per-step norms before clipping, per-step coefficients)."""
    norms = [global_norm(gs, grad_scale) for gs in grads]
    coefs = [clip_coef(n, max_norm) for n in norms]
    scaled = [[None if g is None else g.double() * (grad_scale * c) for g in gs] for gs, c in zip(grads, coefs)]
    p, m, v, steps = R.adamw_run(params, scaled, hyper)
    return p, m, v, steps, norms, coefs
