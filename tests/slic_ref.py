"""numpy restatement of the device SLIC segmentation (csrc/slic.hip) as include/mstg_hip.h defines it, written from the definition and
independently of the kernels: a per-centre window loop with a strict ``<`` in ascending k for the assignment, float32 numpy
arithmetic one operation at a time, ``scipy.ndimage.label`` and a plain walk along the parent links for the connectivity step.
The features are this build's 8-bit Lab (advanced_transform_ref.lab_u8), the connectivity rule is this build's own: NOTHING HERE HAS
BEEN COMPARED WITH A SCIKIT-IMAGE BINARY.
"""
import math

import numpy as np
from scipy import ndimage

from advanced_transform_ref import lab_u8

F32, F64 = np.float32, np.float64
MAX_PIXELS, MAX_CENTRES, ROUNDS = 1 << 20, 4096, 10


class Refused(ValueError):
    pass


def _rint_even(x):
    f = math.floor(x)
    d = x - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


def grid(H, W, n_segments):
    """(step, ny, nx, start) of the initial centres; raises Refused with the header's words for what is not built"""
    if n_segments < 1:
        raise Refused(f"n_segments = {n_segments}")
    if H < 1 or W < 1:
        raise Refused(f"H = {H}, W = {W}")
    if H * W > MAX_PIXELS:
        raise Refused(f"H * W = {H * W}")
    if H * W <= n_segments:
        raise Refused(f"n_segments = {n_segments}")
    s = math.sqrt(float(H * W) / float(n_segments))
    step, start = _rint_even(s), int(math.floor(s / 2))
    if H < step or W < step:
        raise Refused(f"step = {step}")
    ny, nx = len(range(start, H, step)), len(range(start, W, step))
    if ny * nx > MAX_CENTRES:
        raise Refused(f"K = {ny * nx}")
    return step, ny, nx, start


def min_size_of(H, W, K):
    return int(0.5 * (float(H * W) / float(K)))


def segment_bound(H, W, n_segments):
    """the most segments the connectivity step can leave: every component that is not small has min_size pixels, but the first"""
    _, ny, nx, _ = grid(H, W, n_segments)
    return H * W // max(min_size_of(H, W, ny * nx), 1) + 1


def assign(img, n_segments=100, compactness=10.0, rounds=ROUNDS, stats=None):
    """steps 1 to 3: (labels int32 (H, W) in 0 .. K - 1, centres float32 (K, 5): y, x, L, a, b after the last update).
    ``stats`` (a dict) receives 'orphans': the pixels without a candidate, per round."""
    H, W = img.shape[:2]
    if not compactness > 0:
        raise Refused(f"compactness = {compactness}")
    step, ny, nx, start = grid(H, W, n_segments)
    K = ny * nx
    lab = lab_u8(img)
    yy, xx = np.mgrid[0:H, 0:W]
    feat = np.stack([yy, xx, lab[..., 0], lab[..., 1], lab[..., 2]], axis=-1).astype(np.int64)
    ff = feat.astype(F32)
    cy, cx = np.meshgrid(start + step * np.arange(ny), start + step * np.arange(nx), indexing="ij")
    cen = feat[cy.ravel(), cx.ravel()].astype(F32)  # (K, 5), row-major
    ws = F32(1) / F32(step * step)
    m = F32(compactness)
    wc = F32(1) / (m * m)
    kL = F32(100) / F32(255)
    labels = np.zeros((H, W), dtype=np.int32)
    orphans = []
    for _ in range(rounds):
        best = np.full((H, W), np.inf, dtype=F32)
        has = np.zeros((H, W), dtype=bool)
        for k in range(K):
            iy, ix = int(cen[k, 0]), int(cen[k, 1])
            y0, y1, x0, x1 = max(iy - 2 * step, 0), min(iy + 2 * step, H - 1), max(ix - 2 * step, 0), min(ix + 2 * step, W - 1)
            if y0 > y1 or x0 > x1:
                continue
            f = ff[y0:y1 + 1, x0:x1 + 1]
            dy, dx = f[..., 0] - cen[k, 0], f[..., 1] - cen[k, 1]
            dL, da, db = f[..., 2] - cen[k, 2], f[..., 3] - cen[k, 3], f[..., 4] - cen[k, 4]
            sp = (dy * dy + dx * dx) * ws
            t = dL * kL
            co = ((t * t + da * da) + db * db) * wc
            d = sp + co
            assert d.dtype == F32
            win = best[y0:y1 + 1, x0:x1 + 1]
            better = d < win  # strict: among equal distances the lowest k stays
            win[better] = d[better]
            labels[y0:y1 + 1, x0:x1 + 1][better] = k
            has[y0:y1 + 1, x0:x1 + 1] = True
        orphans.append(int((~has).sum()))
        flat = labels.ravel()
        n = np.bincount(flat, minlength=K)
        new = cen.copy()
        for c in range(5):
            s = np.zeros(K, dtype=np.int64)  # exact integer sums
            np.add.at(s, flat, feat[..., c].ravel())
            live = n > 0
            new[live, c] = (s[live].astype(F64) / n[live].astype(F64)).astype(F32)
        cen = new
    if stats is not None:
        stats["orphans"] = orphans
    return labels, cen


def connect(labels, min_size, stats=None):
    """step 4 on any integer labels (H, W): (labels int32 1 .. count, count).  ``stats`` receives 'components', 'small' and
    'deepest' (the longest walk along the parent links)."""
    labels = np.asarray(labels)
    H, W = labels.shape
    comp = np.zeros((H, W), dtype=np.int64)
    total = 0
    for v in np.unique(labels):
        c, n = ndimage.label(labels == v)  # the default structure: 4-connected
        comp[c > 0] = c[c > 0] + total
        total += n
    flat = comp.ravel() - 1
    root = np.full(total, H * W, dtype=np.int64)
    np.minimum.at(root, flat, np.arange(H * W))
    size = np.bincount(flat, minlength=total)
    small = (size < min_size) & (root > 0)
    owner = np.arange(total)
    deepest = 0
    for c in range(total):
        o, depth = c, 0
        while small[o]:
            r = root[o]
            o = flat[r - W] if r % W == 0 else flat[r - 1]
            depth += 1
        owner[c] = o
        deepest = max(deepest, depth)
    owners = np.unique(owner)
    owners = owners[np.argsort(root[owners])]
    number = np.zeros(total, dtype=np.int32)
    number[owners] = np.arange(1, len(owners) + 1)
    if stats is not None:
        stats.update(components=total, small=int(small.sum()), deepest=deepest)
    return number[owner[flat]].reshape(H, W), len(owners)


def slic(img, n_segments=100, compactness=10.0, stats=None):
    """steps 1 to 4: (labels int32 (H, W) in 1 .. count, count)"""
    H, W = img.shape[:2]
    raw, cen = assign(img, n_segments, compactness, stats=stats)
    return connect(raw, min_size_of(H, W, len(cen)), stats)


# ---- hand-made label planes ----------------------------------------------------------------------------------------------------------
def serpentine(h, w):
    """two labels: label 1 is one component that winds through every row (full rows joined alternately at the right and the left
    end), label 0 the gaps between its turns"""
    lab = np.zeros((h, w), dtype=np.int32)
    lab[0::2] = 1
    lab[1::4, w - 1] = 1
    lab[3::4, 0] = 1
    return lab


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) & 1).astype(np.int32)


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
def case(name):
    """(image (H, W, 3) uint8, n_segments) of a named input"""
    from advanced_transform_ref import noise, smooth
    from color_blocks_ref import blocks
    if name == "blocks96":
        return blocks(96, 80, 5, cell=16), 30
    if name == "blocks256":  # the workload's own shape
        return blocks(256, 256, 3), 100
    if name == "smooth":  # no tile divides it
        return smooth(37, 53, 2), 12
    if name == "noise":  # every component small: everything chains to the segment of pixel 0
        return noise(40, 70, 1), 15
    if name == "flat":  # the colour terms are all zero: spatial ties, the lowest k wins, no component is small
        return np.full((64, 48, 3), 97, dtype=np.uint8), 100
    raise ValueError(name)


CASES = ("blocks96", "blocks256", "smooth", "noise", "flat")
_results = {}


def reference(name, compactness=10.0):
    """{'img', 'n_segments', 'raw', 'centres', 'labels', 'count', 'stats'} of a named input, computed once; read-only arrays"""
    key = (name, float(compactness))
    if key not in _results:
        img, n_segments = case(name)
        stats = {}
        raw, cen = assign(img, n_segments, compactness, stats=stats)
        labels, count = connect(raw, min_size_of(img.shape[0], img.shape[1], len(cen)), stats)
        for a in (img, raw, cen, labels):
            a.setflags(write=False)
        _results[key] = dict(img=img, n_segments=n_segments, raw=raw, centres=cen, labels=labels, count=count, stats=stats)
    return _results[key]
