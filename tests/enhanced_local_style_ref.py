"""CPU restatement of the reference's segmentation-driven local style (enhanced_local_style.py:56-292) as include/mstg_hip.h defines
it, written independently of the kernels, with per-segment loops as the reference has them (no scatter): the Felzenszwalb
segmentation, ``analyze_segments`` (a masked copy, grey and two Sobel filters per segment), ``determine_blend_ratios``, the
``scipy.ndimage.gaussian_filter(sigma=3)`` of the map, the float32 blend, the 8-bit ``COLOR_RGB2HSV`` -> saturation * 1.2 -> CLAHE ->
``COLOR_HSV2RGB`` step, the sharpening filter and ``cv2.bilateralFilter(5, 50, 50)``.

OpenCV and scikit-image are not dependencies of this repository: this module RESTATES them from their definitions as recalled and
HAS NOT BEEN COMPARED WITH AN OPENCV OR SCIKIT-IMAGE BINARY.  tests/test_enhanced_local_style_cpu.py pins it with closed forms
instead, and compares ``gaussian_reflect`` with scipy itself, bit for bit.
"""
import math

import numpy as np

from app_local_style_ref import hsv_u8
from local_style_ref import gray_u8
from standard_mode_ref import bilateral, fma_f32, reflect101

F32, F64 = np.float32, np.float64
FIELDS = ("n", "R", "G", "B", "R2", "G2", "B2", "S", "y", "x", "E")
TILES = 8


# ---- 1. segment statistics and ratios ---------------------------------------------------------------------------------------------
def _pad101(plane):
    H, W = plane.shape
    ys = [reflect101(i, H) for i in range(-1, H + 1)]
    xs = [reflect101(i, W) for i in range(-1, W + 1)]
    return plane[np.ix_(ys, xs)]


def sobel101(gray):
    """3 x 3 Sobel of an (H, W) plane, BORDER_REFLECT_101 -> (gx, gy) int64"""
    H, W = gray.shape
    g = _pad101(gray.astype(np.int64))

    def at(dy, dx):
        return g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return gx, gy


def segment_sums(canvas, labels, num_segments):
    """(S, 11) Python integers (object array): the exact sums of include/mstg_hip.h per label, one masked pass per segment"""
    H, W = labels.shape
    gray = gray_u8(canvas)
    sat = hsv_u8(canvas)[1]
    c = canvas.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((num_segments, len(FIELDS)), dtype=object)
    for s in np.unique(labels):
        if not 0 <= s < num_segments:
            continue
        mask = labels == s
        gx, gy = sobel101(np.where(mask, gray, 0))
        m = np.sqrt((gx * gx + gy * gy).astype(F64))
        e = int(np.rint(m * 4294967296.0).astype(np.uint64).astype(object).sum())
        row = [int(mask.sum())] + [int(c[..., k][mask].sum()) for k in range(3)] + [int((c[..., k][mask] ** 2).sum()) for k in range(3)]
        row += [int(sat[mask].sum()), int(yy[mask].sum()), int(xx[mask].sum()), e]
        out[s] = row
    return out


def ratio_of(row, H, W):
    """the float32 ratio of one row of sums, every operation rounded in float64 in the header's order; 0 for an empty label"""
    n = int(row[0])
    if n == 0:
        return F32(0)
    sd = [math.sqrt(float(n * int(row[4 + k]) - int(row[1 + k]) ** 2)) / float(n) for k in range(3)]
    mstd = ((sd[0] + sd[1]) + sd[2]) / 3.0
    ed = float(int(row[10])) / 4294967296.0 / float(H * W)
    py, px = float(int(row[8])) / float(n), float(int(row[9])) / float(n)
    cy, cx = H // 2, W // 2
    md = math.sqrt(float(cx * cx + cy * cy))
    dy, dx = py - cy, px - cx
    dist = math.sqrt(dy * dy + dx * dx)
    sm = float(int(row[7])) / float(n)
    adj = (((0.3 * (ed / 30) + 0.2 * (mstd / 50)) - 0.1 * (dist / md)) + (-0.1 * (float(n) / (H * W / 100.0)))) + 0.2 * (sm / 255)
    return F32(max(0.3, min(0.9, 0.7 + adj)))


def segment_ratios(canvas, labels, num_segments):
    """(sums (S, 11) object, ratio (S,) float32)"""
    H, W = labels.shape
    sums = segment_sums(canvas, labels, num_segments)
    return sums, np.array([ratio_of(r, H, W) for r in sums], dtype=F32)


def map_of(labels, ratio):
    S = len(ratio)
    ok = (labels >= 0) & (labels < S)
    return np.where(ok, ratio[np.clip(labels, 0, S - 1)], F32(0)).astype(F32)


def literal_ratios(canvas, labels):
    """{label: float32 ratio}: the reference's own numpy expressions (:88-171) with np.mean, np.std and the float64 Sobel magnitude,
    on the restated grey, saturation and Sobel"""
    H, W = labels.shape
    gray = gray_u8(canvas)
    hsv = np.stack(hsv_u8(canvas), axis=-1).astype(np.uint8)
    center_y, center_x = H // 2, W // 2
    max_dist = np.sqrt(center_x ** 2 + center_y ** 2)
    out = {}
    for segment_id in np.unique(labels):
        mask = labels == segment_id
        region_rgb, region_hsv = canvas[mask], hsv[mask]
        avg_hsv = np.mean(region_hsv, axis=0)
        std_color = np.std(region_rgb, axis=0)
        gx, gy = sobel101(np.where(mask, gray, 0))
        sobelx, sobely = gx.astype(F64), gy.astype(F64)
        edge_density = np.mean(np.sqrt(sobelx ** 2 + sobely ** 2))
        size = np.sum(mask)
        pos_y, pos_x = np.mean(np.argwhere(mask), axis=0)
        edge_factor = 0.3 * (edge_density / 30)
        color_var_factor = 0.2 * (np.mean(std_color) / 50)
        dist_to_center = np.sqrt((pos_y - center_y) ** 2 + (pos_x - center_x) ** 2)
        dist_factor = 0.1 * (dist_to_center / max_dist)
        size_factor = -0.1 * (size / (H * W / 100))
        saturation_factor = 0.2 * (avg_hsv[1] / 255)
        adjustment = edge_factor + color_var_factor - dist_factor + size_factor + saturation_factor
        out[int(segment_id)] = F32(max(0.3, min(0.9, 0.7 + adjustment)))
    return out


# ---- 2. scipy.ndimage.gaussian_filter on float32 ------------------------------------------------------------------------------------
def gaussian_weights(sigma, radius):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius), its expressions: the half from the centre outwards"""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[radius:]


def reflect_index(i, n):
    """scipy's 'reflect' (d c b a | a b c d | d c b a)"""
    i %= 2 * n
    return i if i < n else 2 * n - 1 - i


def _correlate_axis(a, w, axis):
    """float64 (H, W) -> float64: t = in[i] * w[0]; t += (in[i - k] + in[i + k]) * w[k], k = r .. 1"""
    r = len(w) - 1
    n = a.shape[axis]
    idx = np.array([reflect_index(i, n) for i in range(-r, n + r)])
    p = np.take(a, idx, axis=axis)

    def at(k):
        return np.take(p, np.arange(r + k, r + k + n), axis=axis)
    t = at(0) * w[0]
    for k in range(r, 0, -1):
        t = t + (at(-k) + at(k)) * w[k]
    return t


def gaussian_reflect(plane, sigma=3.0):
    """scipy.ndimage.gaussian_filter(plane, sigma) of a float32 (H, W) plane: axis 0 then axis 1, float32 between the passes"""
    w = gaussian_weights(sigma, int(4.0 * sigma + 0.5))
    a = _correlate_axis(plane.astype(F32).astype(F64), w, 0).astype(F32)
    return _correlate_axis(a.astype(F64), w, 1).astype(F32)


def segment_blend_map(canvas, labels, num_segments, smooth=True):
    sums, ratio = segment_ratios(canvas, labels, num_segments)
    m = map_of(labels, ratio)
    return (gaussian_reflect(m) if smooth else m), sums, ratio


# ---- 3. the blend -------------------------------------------------------------------------------------------------------------------
def blend_f32(canvas, styled, m):
    m = m.astype(F32)[..., None]
    x = styled.astype(F32) * m + canvas.astype(F32) * (F32(1) - m)
    x = np.where(np.isnan(x), F32(0), np.clip(x, 0, 255))
    return x.astype(np.uint8)


# ---- 4. colour and contrast ---------------------------------------------------------------------------------------------------------
def sat_scale(s, dtype=F64):
    return np.minimum(np.rint(np.asarray(s).astype(dtype) * dtype(1.2)), 255).astype(np.int64)


def clahe_luts(v, clip_limit=2.0):
    """(8, 8, 256) uint8: the tables of the v plane (H, W), H and W multiples of 8"""
    H, W = v.shape
    if H % TILES or W % TILES:
        raise NotImplementedError(f"H = {H}, W = {W}")
    th, tw = H // TILES, W // TILES
    area = th * tw
    clip = max(int(clip_limit * area / 256), 1)
    scale = F32(255.0) / F32(area)
    luts = np.zeros((TILES, TILES, 256), dtype=np.uint8)
    for ty in range(TILES):
        for tx in range(TILES):
            hist = np.bincount(v[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            excess = int(np.maximum(hist - clip, 0).sum())
            hist = np.minimum(hist, clip)
            batch = excess // 256
            residual = excess - batch * 256
            hist += batch
            if residual:
                step = max(256 // residual, 1)
                i = 0
                while i < 256 and residual > 0:
                    hist[i] += 1
                    i += step
                    residual -= 1
            luts[ty, tx] = np.clip(np.rint(np.cumsum(hist).astype(F32) * scale), 0, 255).astype(np.uint8)
    return luts


def _clahe_axis(n_px, t, dtype):
    p = np.arange(n_px).astype(dtype)
    tf = p * (dtype(1.0) / dtype(t)) - dtype(0.5)
    fl = np.floor(tf)
    t1 = fl.astype(np.int64)
    a = tf - fl
    return np.maximum(t1, 0), np.minimum(t1 + 1, TILES - 1), a, dtype(1.0) - a


def clahe(v, dtype=F32):
    """cv2.createCLAHE(2.0, (8, 8)).apply(v); ``dtype=F64`` evaluates the interpolation in float64 (not the definition)"""
    H, W = v.shape
    luts = clahe_luts(v)
    ty1, ty2, ya, ya1 = (q[:, None] for q in _clahe_axis(H, H // TILES, dtype))
    tx1, tx2, xa, xa1 = (q[None, :] for q in _clahe_axis(W, W // TILES, dtype))
    vi = v.astype(np.int64)
    l11, l12 = luts[ty1, tx1, vi].astype(dtype), luts[ty1, tx2, vi].astype(dtype)
    l21, l22 = luts[ty2, tx1, vi].astype(dtype), luts[ty2, tx2, vi].astype(dtype)
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


HSV_IDX = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2rgb_u8(h, s, v, how="definition"):
    """8-bit COLOR_HSV2RGB of integer arrays -> (..., 3) uint8.  ``how``: 'definition' (float32, every operation rounded), 'fused'
    (vf * (1 - sf * hf) with the inner product and subtraction fused, and the same for the fourth entry: NOT the definition),
    'float64' (NOT the definition)"""
    dt = F64 if how == "float64" else F32
    one = dt(1)
    hf = np.asarray(h).astype(dt)
    sf = np.asarray(s).astype(dt) * (one / dt(255))
    vf = np.asarray(v).astype(dt) * (one / dt(255))
    hf = hf * (dt(6) / dt(180))
    fl = np.floor(hf)
    sector = fl.astype(np.int64)
    hf = hf - fl
    bad = (sector < 0) | (sector > 5)
    sector = np.where(bad, 0, sector)
    hf = np.where(bad, dt(0), hf)
    if how == "fused":
        t2 = fma_f32(-sf, hf, np.ones_like(sf))
        t3 = fma_f32(-sf, one - hf, np.ones_like(sf))
    else:
        t2 = one - sf * hf
        t3 = one - sf * (one - hf)
    tab = np.stack([vf, vf * (one - sf), vf * t2, vf * t3], axis=-1)
    bgr = np.take_along_axis(tab, HSV_IDX[sector], axis=-1)
    grey = (sf == 0)[..., None]
    bgr = np.where(grey, vf[..., None], bgr)
    out = np.clip(np.rint(bgr * dt(255)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hsv_enhance(rgb):
    h, s, v = hsv_u8(rgb)
    return np.ascontiguousarray(hsv2rgb_u8(h, sat_scale(s), clahe(v.astype(np.uint8)).astype(np.int64)))


# ---- 5. sharpen and denoise ---------------------------------------------------------------------------------------------------------
def sharpen3(img):
    H, W = img.shape[:2]
    out = np.zeros(img.shape, dtype=np.int64)
    for c in range(3):
        g = _pad101(img[..., c].astype(np.int64))
        total = sum(g[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
        out[..., c] = 10 * g[1:1 + H, 1:1 + W] - total
    return np.clip(out, 0, 255).astype(np.uint8)


def enhanced_style_finish(canvas, styled, m):
    return bilateral(sharpen3(hsv_enhance(blend_f32(canvas, styled, m))), 5, 50, 50)


# ---- the segmentation ---------------------------------------------------------------------------------------------------------------
def felzenszwalb(img, scale=100, sigma=0.5, min_size=50):
    """skimage.segmentation.felzenszwalb as include/mstg_hip.h defines it -> int32 (H, W)"""
    H, W = img.shape[:2]
    w = gaussian_weights(sigma, int(4.0 * sigma + 0.5))
    a = img.astype(F64) / 255.0
    a = np.stack([_correlate_axis(_correlate_axis(a[..., c], w, 0), w, 1) for c in range(3)], axis=-1)
    sc = float(scale) / 255.0
    idx = np.arange(H * W).reshape(H, W)
    e0, e1, cost = [], [], []
    for dy, dx in ((0, 1), (1, 0), (1, 1), (-1, 1)):
        ys = slice(max(0, -dy), H - max(0, dy))
        yt = slice(max(0, dy), H + min(0, dy))
        p, q = idx[ys, 0:W - dx], idx[yt, dx:W]
        d = a[ys, 0:W - dx] - a[yt, dx:W]
        e0.append(p.ravel())
        e1.append(q.ravel())
        cost.append(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).ravel())
    e0, e1, cost = np.concatenate(e0), np.concatenate(e1), np.concatenate(cost)
    order = np.argsort(cost, kind="stable")
    parent, size, cint = list(range(H * W)), [1] * (H * W), [0.0] * (H * W)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def join(r0, r1):
        keep, gone = min(r0, r1), max(r0, r1)
        parent[gone] = keep
        size[keep] += size[gone]
        return keep
    for i in order:
        r0, r1 = find(int(e0[i])), find(int(e1[i]))
        if r0 != r1 and cost[i] < min(cint[r0] + sc / size[r0], cint[r1] + sc / size[r1]):
            cint[join(r0, r1)] = float(cost[i])
    for i in order:
        r0, r1 = find(int(e0[i])), find(int(e1[i]))
        if r0 != r1 and (size[r0] < min_size or size[r1] < min_size):
            join(r0, r1)
    roots = np.array([find(p) for p in range(H * W)])
    return np.unique(roots, return_inverse=True)[1].reshape(H, W).astype(np.int32)


# ---- the caller ---------------------------------------------------------------------------------------------------------------------
def geometry(width, height, target=256):
    """(new_w, new_h, crop box or None, resize back) of :184-203 and :270-281, as written"""
    if width > height:
        new_w, new_h = target, int(height * (target / width))
    else:
        new_h, new_w = target, int(width * (target / height))
    box = None
    if width != height:
        cw, ch = min(target, int(height * (width / height))), min(target, int(width * (height / width)))
        left, top = (target - cw) // 2, (target - ch) // 2
        box = (left, top, left + cw, top + ch)
    return new_w, new_h, box, (width > target or height > target) and width * height <= 1024 * 1024


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
def smooth_noise(h, w, seed, sigma=12.0):
    """(h, w, 3) uint8: a smooth field plus noise of ``sigma`` grey levels"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(yy / 9.0 + k) * np.cos(xx / 7.0 - k) for k in range(3)], axis=-1)
    return np.clip(np.rint(base + rs.normal(0, sigma, size=(h, w, 3))), 0, 255).astype(np.uint8)


def grid_labels(h, w, seed, cell=(9, 11), scattered=0.05):
    """(labels int32 (h, w), S): a block grid, ``scattered`` of the pixels relabelled from three columns away"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    nx = -(-w // cell[1])
    lab = (yy // cell[0]) * nx + xx // cell[1]
    pick = rs.rand(h, w) < scattered
    lab = np.where(pick, lab[yy, (xx + 3) % w], lab)
    return lab.astype(np.int32), int(lab.max()) + 1
