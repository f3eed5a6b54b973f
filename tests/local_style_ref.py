"""CPU restatement of the weight map of the reference's ``process_local_style(mode='enhanced', enhance_colors=False,
smooth=False)`` (batch_process_images.py:126-150, :312-342): the sky mask of ``detect_sky`` (``cv2.cvtColor(COLOR_RGB2HSV)``,
``v > 150 & s < 100``, ``has_sky`` above 70 % of the pixels), ``cv2.cvtColor(COLOR_RGB2GRAY)``, ``cv2.Canny(gray, 50, 150)``,
``scipy.ndimage.gaussian_filter(edges.astype(float), sigma=2) > 0.1`` and the three weight levels.

OpenCV is not a dependency of this repository: this module RESTATES OpenCV 4.x's 8-bit ``cvtColor`` (RGB2GRAY, S and V of
RGB2HSV) and ``Canny`` (aperture 3, L1 gradient: Sobel with replicated borders, non-maximum suppression with the 22.5 / 67.5 degree
sectors in 15-bit fixed point, hysteresis over 8-connected neighbours) from their definitions in integer numpy and HAS NOT BEEN
COMPARED WITH AN OPENCV BINARY.  tests/test_local_style_cpu.py pins it with closed forms instead.  The Gaussian is scipy's own
``gaussian_filter``: the reference's literal call.
"""
import numpy as np
from scipy.ndimage import gaussian_filter, label

LOW, HIGH = 50, 150


def sdiv_table():
    """OpenCV's saturation divisor table: sdiv[0] = 0, sdiv[i] = cvRound((255 << 12) / i) (round half to even); every value of
    this module fits int32"""
    t = np.zeros(256, dtype=np.int32)
    t[1:] = np.rint(1044480.0 / np.arange(1, 256)).astype(np.int32)
    return t


def gray_u8(rgb):
    """(..., 3) uint8 -> uint8: (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14"""
    c = rgb.astype(np.int32)
    return ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def sat_val(rgb):
    """(..., 3) uint8 -> (S, V) of the 8-bit RGB2HSV, int32"""
    c = rgb.astype(np.int32)
    v = c.max(axis=-1)
    diff = v - c.min(axis=-1)
    s = (diff * sdiv_table()[v] + 2048) >> 12
    return s, v


def sky_mask(rgb):
    s, v = sat_val(rgb)
    return (v > 150) & (s < 100)


def sobel(gray):
    """3x3 Sobel of a uint8 (H, W) plane with replicated borders -> (dx, dy) int32"""
    g = np.pad(gray.astype(np.int32), 1, mode="edge")
    H, W = gray.shape

    def at(dy, dx):
        return g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return gx, gy


def state_map(gray):
    """Canny's map before hysteresis: 2 = kept by the suppression and above HIGH, 0 = kept (a candidate), 1 = not an edge"""
    dx, dy = sobel(gray)
    H, W = gray.shape
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1, mode="constant")  # the magnitude counts as 0 outside the image

    def at(oy, ox):
        return mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x, y = np.abs(dx), np.abs(dy) << 15
    t = x * 13573
    horiz = y < t
    vert = ~horiz & (y > t + (x << 16))
    diag = ~horiz & ~vert
    neg = (dx ^ dy) < 0  # s = -1: compare with (y - 1, x + 1) and (y + 1, x - 1)
    keep_h = (m > at(0, -1)) & (m >= at(0, 1))
    keep_v = (m > at(-1, 0)) & (m >= at(1, 0))
    keep_d = np.where(neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    keep = (m > LOW) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    return np.where(keep, np.where(m > HIGH, 2, 0), 1).astype(np.uint8)


def hysteresis(state):
    """edge mask (bool): the 8-connected components of ``state != 1`` that contain a 2"""
    lab, n = label(state != 1, structure=np.ones((3, 3), dtype=int))
    strong = np.zeros(n + 1, dtype=bool)
    strong[np.unique(lab[state == 2])] = True
    strong[0] = False
    return strong[lab]


def canny(gray):
    return hysteresis(state_map(gray))


def gaussian(edge):
    """the reference's literal call"""
    return gaussian_filter(edge.astype(float), sigma=2)


def weights(strength, detail, detail_coeff=0.3):
    """(w_base, w_sky, w_detail) as the reference computes them (:330, :334, :337; coefficient 0.4 at :383)"""
    return float(strength), min(strength + 0.2, 1.0), max(strength - detail_coeff * detail, 0.0)


def enhanced_weight_map(canvas, strength=0.8, detail=0.7, detail_coeff=0.3):
    """(H, W, 3) uint8 -> dict(weight float64 (H, W), sky, edge, detail bool masks, has_sky, gauss float64, gray, state)"""
    H, W = canvas.shape[:2]
    sky = sky_mask(canvas)
    has_sky = bool(np.sum(sky) / (H * W) > 0.7)
    gray = gray_u8(canvas)
    state = state_map(gray)
    edge = hysteresis(state)
    g = gaussian(edge)
    det = g > 0.1
    w_base, w_sky, w_detail = weights(strength, detail, detail_coeff)
    weight = np.ones((H, W), dtype=float) * w_base
    if has_sky:
        weight[sky] = w_sky
    weight[det] = w_detail
    return dict(weight=weight, sky=sky, edge=edge, detail=det, has_sky=has_sky, gauss=g, gray=gray, state=state)


# ---- test inputs (shared by the GPU tests and tools/bench_local_style.py) -------------------------------------------------------
def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def blocky(h, w, seed):
    """random colour cells upsampled by 6..9: flat cells make magnitudes tie, so the > / >= rule of the suppression decides"""
    f = 6 + seed % 4
    base = np.random.RandomState(seed).randint(0, 256, size=(h // f + 1, w // f + 1, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(base, np.ones((f, f, 1), dtype=np.uint8))[:h, :w])


def gradient_rects(h, w, seed):
    """a smooth gradient with a few rectangles"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 150 * xx // max(w - 1, 1), 60 + 120 * yy // max(h - 1, 1), 200 - 100 * (xx + yy) // max(h + w - 2, 1)], axis=-1)
    img = img.astype(np.uint8)
    for _ in range(4):
        y0, x0 = rs.randint(0, max(h - 4, 1)), rs.randint(0, max(w - 4, 1))
        img[y0:y0 + rs.randint(3, h // 2 + 4), x0:x0 + rs.randint(3, w // 2 + 4)] = rs.randint(0, 256, size=3)
    return np.ascontiguousarray(img)


def landscape(h, w, seed):
    """a letterboxed landscape: white bars, a bright low-saturation sky gradient, textured ground"""
    rs = np.random.RandomState(seed)
    img = np.full((h, w, 3), 255, dtype=np.uint8)
    top, bot = h // 6, h - h // 6
    mid = (top + bot) // 2
    yy = np.arange(top, mid)[:, None, None]
    img[top:mid] = (np.array([170, 200, 235]) + (yy - top) * np.array([60, 40, 15]) // max(mid - top, 1)).astype(np.uint8)
    ground = np.kron(rs.randint(30, 140, size=((bot - mid) // 4 + 1, w // 4 + 1, 3)), np.ones((4, 4, 1), dtype=np.int64))[:bot - mid, :w]
    img[mid:bot] = (ground + rs.randint(-12, 13, size=ground.shape)).clip(0, 255).astype(np.uint8)
    return img


def bright_low_saturation(h, w, seed):
    """bright, nearly grey 32 x 32 cells with a little noise and a few dark ones: at 256 x 256 more than 70 % of the pixels pass
    detect_sky, and the inside of a cell has no edge, so the sky weight survives there"""
    rs = np.random.RandomState(seed)
    cells = rs.randint(175, 250, size=(h // 32 + 1, w // 32 + 1, 1)) + rs.randint(-12, 13, size=(h // 32 + 1, w // 32 + 1, 3))
    cells[rs.rand(*cells.shape[:2]) < 0.12] = 70  # a few dark cells: not sky
    img = np.kron(cells, np.ones((32, 32, 1), dtype=np.int64))[:h, :w]
    return (img + rs.randint(-1, 2, size=img.shape)).clip(0, 255).astype(np.uint8)


def sky_threshold_canvas(h, w, n_sky, seed):
    """``n_sky`` pixels (151, 151, 151) (v = 151 > 150, s = 0: sky) placed pseudo-randomly among (150, 150, 150) (not sky); grays
    differ by one level, so there is no edge and no detail anywhere"""
    flat = np.full(h * w, 150, dtype=np.uint8)
    flat[np.random.RandomState(seed).permutation(h * w)[:n_sky]] = 151
    return np.ascontiguousarray(np.repeat(flat.reshape(h, w, 1), 3, axis=2))


def spiral_path(h, w):
    """cells of a one-pixel-wide rectangular spiral with one free pixel between its turns, from the corner inwards"""
    free = np.ones((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    free[0, 0] = False
    path = [(0, 0)]

    def ok(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and free[yy, xx]

    def clear(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or free[yy, xx]
    while True:
        for _ in range(2):
            if ok(y + dy, x + dx) and clear(y + 2 * dy, x + 2 * dx):
                break
            dy, dx = dx, -dy
        else:
            return path
        y, x = y + dy, x + dx
        free[y, x] = False
        path.append((y, x))


def spiral_state(h, w, strong=True):
    """the long-path case: the spiral as candidates, one strong pixel at its inner end"""
    st = np.ones((h, w), dtype=np.uint8)
    path = spiral_path(h, w)
    ys, xs = zip(*path)
    st[list(ys), list(xs)] = 0
    if strong:
        st[path[-1]] = 2
    return st


def serpentine_state(h, w):
    """full rows 0, 2, 4, ... joined alternately at the right and the left border, the last row too: runs along all four borders"""
    st = np.ones((h, w), dtype=np.uint8)
    st[0::2] = 0
    for r in range(0, h - 1, 2):
        st[r + 1, w - 1 if r % 4 == 0 else 0] = 0
    st[h - 1] = 0
    st[h - 1, w // 2] = 2
    return st


def diagonal_state(h, w):
    """two diagonal-only chains, one strong at its top end, the other at its bottom end"""
    st = np.ones((h, w), dtype=np.uint8)
    n = min(h, w)
    i = np.arange(n)
    st[i, i] = 0
    st[h - 1 - i, i] = 0
    st[0, 0] = 2
    st[h - 1, 0] = 2
    return st


def candidates_only_state(h, w, seed):
    """blobs of candidates that touch only candidates, and a strong pixel that touches none of them"""
    rs = np.random.RandomState(seed)
    st = np.where(rs.rand(h, w) < 0.45, 0, 1).astype(np.uint8)
    st[:3, :3] = 1
    st[1, 1] = 2
    return st


def random_state(h, w, seed):
    return np.random.RandomState(seed).choice(np.array([0, 1, 2], dtype=np.uint8), size=(h, w), p=[0.3, 0.62, 0.08])
