"""CPU restatement of what scikit-image evaluates for the reference's metric calls (image_quality_comparison.py:11-34 and the
three scripts that repeat it): ``peak_signal_noise_ratio(a, b, data_range=1.0)`` and ``structural_similarity(a, b, channel_axis=2,
data_range=1.0)`` on ``uint8.astype(float) / 255.0`` images, plus ``np.mean((a - b) ** 2)``.

scikit-image is not a dependency of this repository: this module RESTATES its defaults for these calls (uniform 7x7 window through
``scipy.ndimage.uniform_filter``, the function skimage itself calls; sample covariance 49 / 48; K1 = 0.01, K2 = 0.03; the mean of
the map cropped by 3 on each side; per channel, then the mean over channels) and is not compared with skimage here.
tests/test_metrics_cpu.py pins it with closed forms instead.
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2


def ssim_channel(x, y):
    """mean SSIM of two float64 (H, W) planes in [0, 1]"""
    if min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    cov_norm = WIN * WIN / (WIN * WIN - 1.0)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (WIN - 1) // 2
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def metrics(a_u8, b_u8):
    """{'mse', 'psnr', 'ssim', 'ssim_channels'} of two uint8 (H, W, 3) arrays"""
    assert a_u8.dtype == np.uint8 and b_u8.dtype == np.uint8 and a_u8.shape == b_u8.shape and a_u8.shape[2] == 3
    x, y = a_u8.astype(float) / 255.0, b_u8.astype(float) / 255.0
    mse = np.mean((x - y) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(1.0 / mse)
    ch = [ssim_channel(x[..., c], y[..., c]) for c in range(3)]
    return {"mse": float(mse), "psnr": float(psnr), "ssim": float(np.mean(ch)), "ssim_channels": [float(c) for c in ch]}


# ---- seeded test images ---------------------------------------------------------------------------------------------------
def image(h, w, seed):
    """blocky image with texture"""
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, size=(h // 4 + 2, w // 4 + 2, 3)).astype(np.uint8)
    img = np.kron(base, np.ones((4, 4, 1), dtype=np.uint8))[:h, :w]
    return np.ascontiguousarray((img.astype(np.int32) + rs.randint(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8))


def pair(kind, h, w, seed=0):
    """the pairs the GPU tests use: 'noise' (image, image + uniform noise in +-30, clipped), 'identical', 'constant',
    'blackwhite' (all 0 against all 255), 'binary' (random {0, 255} against its inverse: the largest integer intermediates)"""
    rs = np.random.RandomState(1000 + seed)
    if kind == "noise":
        a = image(h, w, seed)
        b = (a.astype(np.int32) + rs.randint(-30, 31, size=a.shape)).clip(0, 255).astype(np.uint8)
    elif kind == "identical":
        a = image(h, w, seed)
        b = a.copy()
    elif kind == "constant":
        a, b = np.full((h, w, 3), 37 + seed, np.uint8), np.full((h, w, 3), 201 - seed, np.uint8)
    elif kind == "blackwhite":
        a, b = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    elif kind == "binary":
        a = (rs.randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
        b = 255 - a
    else:
        raise ValueError(kind)
    return a, b


KINDS = ("noise", "identical", "constant", "blackwhite", "binary")
