"""CPU emulation (plain torch, no GPU) of the mixed-precision pre-training step of mstg_hip/train_plain.py, and the seeded draws
its tests use.

The emulation is the DESIGN, not the kernels: filters rounded to fp16; activations rounded to fp16 where the kernels store them
(the stem's output, every ``z = conv + bias`` in front of a BatchNorm, every BatchNorm + activation output, the head image);
activation gradients rounded to fp16 at the same places and at the head's pre-activation, carrying the loss scale; fp32
accumulation everywhere else, fp32 BatchNorm statistics, fp32 parameter gradients divided by the scale.  The kernels differ
from it in fp32 summation order only.  fp16 overflow turns into inf here as it does there.

    python tools/emulate_plain_f16_train.py            # the draw of tests/test_gpu_f16_train.py::test_loss_scaling_earns_its_place

prints the relative L2 distance of the emulated parameter gradient from the same model in fp64 for loss scale "auto" and 1.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import restatement as R  # noqa: E402

DEAD_BIASES = ("encoder.2.bias", "encoder.5.bias", "encoder.8.bias", "decoder.0.bias", "decoder.3.bias", "decoder.6.bias")


def param_names(C):
    return [k for k, _ in R.plain_generator_spec(C) if "running" not in k and "num_batches" not in k]


def pretrain_draw(C, N, S, seed):
    """(state dict, masked input, real image, mask) of a seeded draw: weights ``make_state_dict(plain_generator_spec(C), seed)``,
    images ``make_input(.., 100 + seed)`` / ``make_input(.., 200 + seed)``, an 8 x 8 grid mask with 40 % of the cells masked
    (torch generator 300 + seed), the input masked as pretrain.py:52-55 does."""
    sd = R.make_state_dict(R.plain_generator_spec(C), seed)
    x = R.make_input((N, 3, S, S), 100 + seed)
    real = R.make_input((N, 3, S, S), 200 + seed)
    g = torch.Generator().manual_seed(300 + seed)
    m = (torch.rand(N, 1, 8, 8, generator=g) < 0.4).float()
    m = m.repeat_interleave(S // 8, 2).repeat_interleave(S // 8, 3).expand(N, 3, S, S).contiguous()
    return sd, x * (1 - m), real, m


def masked_l1(y, real, m):
    return (y * (1 - m) - real * (1 - m)).abs().mean()


def reference_grads(sd, x, real, m, dtype=torch.float64):
    """Loss and parameter gradients of the restated reference forward in ``dtype`` (train mode; ``sd`` is not modified)."""
    sd2 = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = [k for k in sd2 if sd2[k].is_floating_point() and "running" not in k]
    for k in names:
        sd2[k].requires_grad_(True)
    loss = masked_l1(R.plain_generator_forward(sd2, x.to(dtype), train=True), real.to(dtype), m.to(dtype))
    grads = torch.autograd.grad(loss, [sd2[k] for k in names])
    return float(loss), dict(zip(names, grads))


class _RoundFwd(torch.autograd.Function):  # store as fp16; the gradient passes
    @staticmethod
    def forward(ctx, t):
        return t.half().float()

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):  # the gradient is stored as fp16 here
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.half().float()


def _both(t):
    return _RoundFwd.apply(_RoundBwd.apply(t))


def emulated_grads(sd, x, real, m, loss_scale):
    """Loss (unscaled) and unscaled fp32 parameter gradients of the emulated mixed-precision step."""
    sd2 = {k: v.clone().float() for k, v in sd.items() if v.is_floating_point()}
    names = [k for k in sd2 if "running" not in k]
    for k in names:
        sd2[k].requires_grad_(True)

    def w16(k):
        return _RoundFwd.apply(sd2[k])

    def bn(z, p):
        mu = z.mean(dim=(0, 2, 3))
        var = z.var(dim=(0, 2, 3), unbiased=False)
        xh = (z - mu[None, :, None, None]) * torch.rsqrt(var[None, :, None, None] + 1e-5)
        return xh * sd2[p + ".weight"][None, :, None, None] + sd2[p + ".bias"][None, :, None, None]

    h = _RoundBwd.apply(F.conv2d(x.half().float(), w16("encoder.0.weight"), sd2["encoder.0.bias"], stride=2, padding=1))
    h = _both(F.leaky_relu(h, 0.2))
    for ci, bi in ((2, 3), (5, 6), (8, 9)):
        z = _both(F.conv2d(h, w16(f"encoder.{ci}.weight"), sd2[f"encoder.{ci}.bias"], stride=2, padding=1))
        h = _both(F.leaky_relu(bn(z, f"encoder.{bi}"), 0.2))
    for ci, bi in ((0, 1), (3, 4), (6, 7)):
        z = _both(F.conv_transpose2d(h, w16(f"decoder.{ci}.weight"), sd2[f"decoder.{ci}.bias"], stride=2, padding=1))
        h = _both(F.relu(bn(z, f"decoder.{bi}")))
    z = _RoundBwd.apply(F.conv_transpose2d(h, w16("decoder.9.weight"), sd2["decoder.9.bias"], stride=2, padding=1))
    y = _RoundFwd.apply(torch.tanh(z))
    loss = masked_l1(y, real, m)
    grads = torch.autograd.grad(loss * loss_scale, [sd2[k] for k in names])
    return float(loss), {k: g / loss_scale for k, g in zip(names, grads)}


def flat(grads, names, skip=()):
    return torch.cat([grads[k].double().flatten() for k in names if k not in skip])


def distance(grads, ref, names, skip=()):
    a, b = flat(grads, names, skip), flat(ref, names, skip)
    return float((a - b).norm() / b.norm())


LOSS_SCALE_DRAW = (8, 16, 256, 7)  # channels, batch, size, seed of test_loss_scaling_earns_its_place


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    C, N, S, seed = LOSS_SCALE_DRAW
    sd, x, real, m = pretrain_draw(C, N, S, seed)
    names = param_names(C)
    l64, g64 = reference_grads(sd, x, real, m)
    auto = float(2 ** (x.numel() - 1).bit_length())
    for name, scale in (("auto", auto), ("1", 1.0)):
        le, ge = emulated_grads(sd, x, real, m, scale)
        print(f"draw C{C} {N}x{S}x{S} seed {seed}: loss scale {name:5s} loss - fp64 {le - l64:+.2e}  "
              f"gradient distance from fp64 {distance(ge, g64, names):.4e}")


if __name__ == "__main__":
    main()
