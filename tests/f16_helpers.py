"""Helpers shared by the fp16 GPU tests (test_gpu_f16*.py): the parity report, operand generators and rounding, the CPU side of
the InstanceNorm statistics, the NHWC fp16 upload, the library fixture and the layer tables of the plain Generator."""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
ACT_NONE, ACT_RELU, ACT_LEAKY02, ACT_TANH = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    """imported by name into each test module, where it runs once per module"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def report(name, err, tol):
    print(f"  [parity] {name:64s} rel-L2 {err:.2e} (tol {tol:.0e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.0e}"


def h(t):
    """round to fp16 and back (CPU, fp32)"""
    return t.half().float()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def stats_of(y_nchw):
    mu = y_nchw.mean(dim=(2, 3))
    var = y_nchw.var(dim=(2, 3), unbiased=False)
    return torch.stack([mu, torch.rsqrt(var + 1e-5)], dim=-1)  # (N, C, 2)


def norm_relu(x_nchw, st):
    return F.relu((x_nchw - st[..., 0][:, :, None, None]) * st[..., 1][:, :, None, None])


def nhwc(x):
    """NCHW fp32 on the CPU -> NHWC fp16 on the device"""
    return x.permute(0, 2, 3, 1).contiguous().half().to(DEV)


nhwc16 = nhwc


LAYER_CASES = [
    # name, kind, N, H, W, Cin, Cout, act
    ("conv 8->8 leaky", 0, 2, 16, 16, 8, 8, ACT_LEAKY02),
    ("conv 8->64 none", 0, 1, 24, 40, 8, 64, ACT_NONE),
    ("conv 64->256 relu", 0, 2, 12, 20, 64, 256, ACT_RELU),
    ("conv 256->512 leaky, 2x2 -> 1x1", 0, 1, 2, 2, 256, 512, ACT_LEAKY02),
    ("conv 512->512 tanh, tiles span 5 images", 0, 5, 6, 10, 512, 512, ACT_TANH),
    ("conv 512->8 leaky", 0, 3, 8, 8, 512, 8, ACT_LEAKY02),
    ("conv 64->128 leaky, 64x64 (128-pixel tiles)", 0, 8, 64, 64, 64, 128, ACT_LEAKY02),
    ("convT 8->8 relu", 1, 2, 8, 8, 8, 8, ACT_RELU),
    ("convT 512->256 relu, 1x1 -> 2x2", 1, 1, 1, 1, 512, 256, ACT_RELU),
    ("convT 512->512 none, tiles span 5 images", 1, 5, 3, 5, 512, 512, ACT_NONE),
    ("convT 256->64 leaky", 1, 2, 6, 10, 256, 64, ACT_LEAKY02),
    ("convT 64->8 tanh", 1, 1, 12, 20, 64, 8, ACT_TANH),
    ("convT 8->512 relu", 1, 3, 4, 4, 8, 512, ACT_RELU),
    ("convT 128->64 relu, 64x64 (128-pixel tiles)", 1, 8, 64, 64, 128, 64, ACT_RELU),
    ("conv 24->48 leaky (other multiples of 8)", 0, 2, 10, 14, 24, 48, ACT_LEAKY02),
]

STEM_HEAD_CASES = [
    # name, N, H, W, C
    ("16x16 C8", 2, 16, 16, 8),
    ("48x80 C64", 1, 48, 80, 64),
    ("32x32 C16, tiles span 5 images", 5, 32, 32, 16),
    ("256x256 C64", 1, 256, 256, 64),
]
