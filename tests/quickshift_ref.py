"""numpy restatement of the device quickshift segmentation (csrc/quickshift.hip) as include/mstg_hip.h defines it, written from the
definition and independently of the kernels: a loop over the window offsets in row-major order, int64 arithmetic for the colour
term, ``np.rint(np.exp(..) * 2**32)`` for the terms of the density, a strict ``<`` for the parent and a plain walk to the roots.
The features are this build's 8-bit Lab (advanced_transform_ref.lab_u8); the fixed-point density and the tie rule by raster index
are this build's own: NOTHING HERE HAS BEEN COMPARED WITH A SCIKIT-IMAGE BINARY.
"""
import math

import numpy as np

from advanced_transform_ref import lab_u8

F64, I64 = np.float64, np.int64
MAX_PIXELS, MAX_RADIUS = 1 << 20, 15
REFERENCE_PARAMS = (0.5, 3, 6)  # ratio, kernel_size, max_dist of the reference's call


class Refused(ValueError):
    pass


def window(kernel_size):
    return int(math.ceil(3 * kernel_size))


def check(H, W, ratio=0.5, kernel_size=3, max_dist=6):
    """raises Refused with the header's words for what is not built; returns (w, reach)"""
    if H < 1 or W < 1:
        raise Refused(f"H = {H}, W = {W}")
    if H * W > MAX_PIXELS:
        raise Refused(f"H * W = {H * W}")
    if not (math.isfinite(kernel_size) and kernel_size >= 1):
        raise Refused(f"kernel_size = {kernel_size}")
    if math.ceil(3 * kernel_size) > MAX_RADIUS:
        raise Refused(f"w = {math.ceil(3 * kernel_size)}")
    if not 0 <= ratio <= 1:
        raise Refused(f"ratio = {ratio}")
    if not (math.isfinite(max_dist) and max_dist > 0):
        raise Refused(f"max_dist = {max_dist}")
    w = window(kernel_size)
    return w, int(min(w, math.floor(max_dist)))


def _pairs(H, W, dr, dc):
    """(slices of the pixels p, slices of their taps p + (dr, dc)) for the pixels whose tap lies in the image, or None"""
    y0, y1, x0, x1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dr, y1 + dr), slice(x0 + dc, x1 + dc))


def _distance(lab, ps, ts, dr, dc, kc):
    d = lab[ts] - lab[ps]  # int64
    q = (100 * d[..., 0]) ** 2 + 65025 * (d[..., 1] ** 2 + d[..., 2] ** 2)
    D = q.astype(F64) * F64(kc)  # one rounding
    return D + F64(dr * dr + dc * dc)  # the second


def taps(H, W, w):
    """the number of taps of every pixel's clipped window, int64 (H, W)"""
    ny = np.minimum(np.arange(H) + w, H - 1) - np.maximum(np.arange(H) - w, 0) + 1
    nx = np.minimum(np.arange(W) + w, W - 1) - np.maximum(np.arange(W) - w, 0) + 1
    return ny[:, None].astype(I64) * nx[None, :].astype(I64)


def density(img, ratio=0.5, kernel_size=3):
    """steps 1 to 3: int64 (H, W)"""
    H, W = img.shape[:2]
    w, _ = check(H, W, ratio, kernel_size)
    lab = lab_u8(img).astype(I64)
    kc = (F64(ratio) * F64(ratio)) / F64(65025.0)
    inv = F64(-0.5) / (F64(kernel_size) * F64(kernel_size))
    T = np.zeros((H, W), dtype=I64)
    for dr in range(-w, w + 1):
        for dc in range(-w, w + 1):
            pr = _pairs(H, W, dr, dc)
            if pr is None:
                continue
            ps, ts = pr
            term = np.rint(np.exp(_distance(lab, ps, ts, dr, dc, kc) * inv) * F64(2.0 ** 32))  # ties to even
            T[ps] += term.astype(I64)
    return T


_density = density  # quickshift() has a parameter of that name


def parents(img, dens, ratio=0.5, kernel_size=3, max_dist=6, reach=None, stats=None):
    """step 4 on a given density: int32 (H, W) raster indices, a root its own parent.  ``reach`` None: the whole window, as the
    definition says; a number: that square only.  ``stats`` receives 'ties' (compared pairs of equal density, a pixel and itself
    not counted) and 'gap' (the smallest non-zero density difference among compared pairs; None if there is none)."""
    H, W = img.shape[:2]
    w, _ = check(H, W, ratio, kernel_size, max_dist)
    r = w if reach is None else int(reach)
    lab = lab_u8(img).astype(I64)
    kc = (F64(ratio) * F64(ratio)) / F64(65025.0)
    max2 = F64(max_dist) * F64(max_dist)
    idx = np.arange(H * W, dtype=I64).reshape(H, W)
    T = np.asarray(dens, dtype=I64)
    best = np.full((H, W), np.inf, dtype=F64)
    par = idx.copy()
    ties, gap = 0, None
    for dr in range(-r, r + 1):  # row-major: ascending index of the tap
        for dc in range(-r, r + 1):
            pr = _pairs(H, W, dr, dc)
            if pr is None:
                continue
            ps, ts = pr
            diff = T[ts] - T[ps]
            if (dr, dc) != (0, 0):
                ties += int((diff == 0).sum())
                nz = np.abs(diff[diff != 0])
                if nz.size:
                    gap = int(nz.min()) if gap is None else min(gap, int(nz.min()))
            higher = (diff > 0) | ((diff == 0) & (idx[ts] < idx[ps]))
            D = _distance(lab, ps, ts, dr, dc, kc)
            better = higher & (D < best[ps])  # strict: among equal D the first of the scan stays
            best[ps][better] = D[better]
            par[ps][better] = idx[ts][better]
    root = best > max2  # inf where no tap is higher
    par[root] = idx[root]
    if stats is not None:
        stats.update(ties=ties, gap=gap)
    return par.astype(np.int32)


def labels_of(parent, stats=None):
    """step 5: (labels int32 (H, W) in 0 .. count - 1, count).  ``stats`` receives 'roots' and 'depth' (the longest walk)."""
    H, W = parent.shape
    par = parent.ravel().astype(I64)
    cur, depth = np.arange(H * W, dtype=I64), 0
    while True:
        nxt = par[cur]
        if (nxt == cur).all():
            break
        cur, depth = nxt, depth + 1
        assert depth <= H * W, "the parent links cycle"
    roots = np.flatnonzero(par == np.arange(H * W))  # ascending index
    number = np.full(H * W, -1, dtype=np.int32)
    number[roots] = np.arange(len(roots), dtype=np.int32)
    if stats is not None:
        stats.update(roots=len(roots), depth=depth)
    return number[cur].reshape(H, W), len(roots)


def quickshift(img, ratio=0.5, kernel_size=3, max_dist=6, density=None, stats=None):
    """steps 1 to 5 -> {'density', 'parent', 'labels', 'count'}; ``density``: run steps 4 and 5 on this density instead"""
    dens = _density(img, ratio, kernel_size) if density is None else np.asarray(density, dtype=I64)
    par = parents(img, dens, ratio, kernel_size, max_dist, stats=stats)
    labels, count = labels_of(par, stats)
    return dict(density=dens, parent=par, labels=labels, count=count)


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
def case(name):
    from advanced_transform_ref import noise, smooth
    from color_blocks_ref import blocks
    from enhanced_local_style_ref import smooth_noise
    if name == "flat":  # the interior densities tie: the raster index decides every parent
        return np.full((40, 48, 3), 97, dtype=np.uint8)
    if name == "flat_small":  # smaller than the window
        return np.full((7, 11, 3), 201, dtype=np.uint8)
    if name == "one":
        return np.full((1, 1, 3), 5, dtype=np.uint8)
    if name == "strip_h":
        return np.ascontiguousarray(smooth(1, 70, 3))
    if name == "strip_w":
        return np.ascontiguousarray(smooth(70, 1, 3))
    if name == "blocks96":  # crosses tile edges
        return blocks(96, 80, 5, cell=16)
    if name == "smooth":  # no tile divides it
        return smooth(37, 53, 2)
    if name == "noise":  # nearly every pixel a root
        return noise(40, 70, 1)
    if name == "smooth_noise":
        return smooth_noise(64, 72, 4)
    if name == "smooth_noise48":  # the one the other parameter sets run on
        return smooth_noise(48, 56, 4)
    raise ValueError(name)


CASES = ("flat", "flat_small", "one", "strip_h", "strip_w", "blocks96", "smooth", "noise", "smooth_noise")
EXACT_CASES = ("flat", "flat_small", "blocks96")  # the smallest density gap exceeds twice the taps: test_quickshift_cpu.py
OTHER_PARAMS = ((1.0, 5, 10), (0.5, 1, 2), (0.0, 3, 6))
RUNS = tuple((name, REFERENCE_PARAMS) for name in CASES) + tuple(("smooth_noise48", p) for p in OTHER_PARAMS)
_results = {}


def reference(name, params=REFERENCE_PARAMS):
    """{'img', 'params', 'density', 'parent', 'labels', 'count', 'stats'} of a named input, computed once; read-only arrays"""
    key = (name, tuple(float(v) for v in params))
    if key not in _results:
        img = case(name)
        stats = {}
        r = quickshift(img, *params, stats=stats)
        for a in (img, r["density"], r["parent"], r["labels"]):
            a.setflags(write=False)
        _results[key] = dict(img=img, params=tuple(params), stats=stats, **r)
    return _results[key]
