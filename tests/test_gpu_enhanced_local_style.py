"""The segmentation-driven local style on the device (csrc/segment_style.hip through mstg_segment_blend_map,
mstg_gaussian_reflect_f32, mstg_blend_map_f32_u8, mstg_clahe_u8, mstg_hsv_enhance_u8, mstg_sharpen3_u8 and
mstg_enhanced_style_finish; mstg_hip.image.process_enhanced_local_style and its stage functions; the drop-in
enhanced_local_style.py) against the numpy restatement of tests/enhanced_local_style_ref.py: bytes byte for byte, the sums exactly,
the ratios and the map bit for bit.  Every stage runs three different images per launch with 64 guard bytes behind every output
and the inputs unchanged; the chain against the composition of the stage entries; the launch counts; reproducibility; the
refusals by name.  The restatement has not been compared with an OpenCV or scikit-image binary (see its docstring)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import enhanced_local_style_ref as ER
import standard_mode_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
TILE_SLOTS = 128  # MSTG_SEGMENT_TILE_SLOTS: distinct labels a 16 x 64 tile of seg_stats_kernel combines in LDS
TILE_H, TILE_W = 16, 64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()
    assert _lib.SEGMENT_TILE_SLOTS == TILE_SLOTS


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


@lru_cache(maxsize=None)
def _images(shape, n=3):
    """n different images of one shape: smooth + noise, a blocky one (flat cells: zero gradients, equal samples), pure noise"""
    h, w = shape
    a = np.stack([ER.smooth_noise(h, w, 3 + h), SR.image("blocky", h, w, 5 + w), SR.image("noise", h, w, 7)][:n])
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def _styled(shape, n=3):
    a = np.array(_images(shape, 3)[::-1][:n])  # a copy
    a[..., 1] = 255 - a[..., 1]
    a.setflags(write=False)
    return a


def _guarded(nbytes):
    return torch.full((nbytes + GUARD,), 7, dtype=torch.uint8, device=DEV)


def _take(buf, nbytes, dtype, shape, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), f"{what} wrote behind its output"
    return out[:nbytes].view(dtype).reshape(shape)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} entries differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ---- the stage entries on numpy batches ----------------------------------------------------------------------------------------------
def _segment_map(x, labels, S, smooth):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    xin, lin = _dev(x), _dev(labels)
    N, H, W = xin.shape[:3]
    mb, sb, rb = N * H * W * 4, N * S * 11 * 8, N * S * 4
    bm, bs, br = _guarded(mb), _guarded(sb), _guarded(rb)
    need = lib.mstg_segment_blend_map_workspace_bytes(N, H, W, S, int(smooth))
    assert need > 0
    ws = _guarded(need)
    _lib.check(lib.mstg_segment_blend_map(_p(xin), _p(lin), N, H, W, S, int(smooth), _p(bm), _p(bs), _p(br), _p(ws), need, _stream()),
               "mstg_segment_blend_map")
    m = _take(bm, mb, np.float32, (N, H, W), "segment_blend_map (map)")
    s = _take(bs, sb, np.uint64, (N, S, 11), "segment_blend_map (sums)")
    r = _take(br, rb, np.float32, (N, S), "segment_blend_map (ratio)")
    _take(ws, need, np.uint8, (need,), "segment_blend_map (workspace)")
    assert torch.equal(xin, _dev(x)) and torch.equal(lin, _dev(labels)), "mstg_segment_blend_map changed an input"
    return m, s, r


def _gauss(planes):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    pin = _dev(planes)
    N, H, W = pin.shape
    nb = N * H * W * 4
    buf, ws = _guarded(nb), _guarded(nb)
    _lib.check(_lib.load().mstg_gaussian_reflect_f32(_p(pin), N, H, W, _p(buf), _p(ws), nb, _stream()), "mstg_gaussian_reflect_f32")
    out = _take(buf, nb, np.float32, (N, H, W), "gaussian_reflect_f32")
    _take(ws, nb, np.uint8, (nb,), "gaussian_reflect_f32 (workspace)")
    assert torch.equal(pin, _dev(planes)), "mstg_gaussian_reflect_f32 changed its input"
    return out


def _blend(c, s, m):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    cin, sin, min_ = _dev(c), _dev(s), _dev(m)
    N, H, W = cin.shape[:3]
    nb = N * H * W * 3
    buf = _guarded(nb)
    _lib.check(_lib.load().mstg_blend_map_f32_u8(_p(cin), _p(sin), _p(min_), N, H, W, _p(buf), _stream()), "mstg_blend_map_f32_u8")
    out = _take(buf, nb, np.uint8, (N, H, W, 3), "blend_map_f32_u8")
    assert torch.equal(cin, _dev(c)) and torch.equal(sin, _dev(s)) and torch.equal(min_.view(torch.int32), _dev(m).view(torch.int32))
    return out


def _with_luts(entry, x, channels):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    nb = N * H * W * channels
    need = lib.mstg_clahe_workspace_bytes(N, H, W)
    assert need == N * 64 * 256
    buf, ws = _guarded(nb), _guarded(need)
    _lib.check(getattr(lib, entry)(_p(xin), N, H, W, _p(buf), _p(ws), need, _stream()), entry)
    out = _take(buf, nb, np.uint8, x.shape, entry)
    luts = _take(ws, need, np.uint8, (N, 8, 8, 256), entry + " (tables)")
    assert torch.equal(xin, _dev(x)), entry + " changed its input"
    return out, luts


def _sharpen(x):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    nb = N * H * W * 3
    buf = _guarded(nb)
    _lib.check(_lib.load().mstg_sharpen3_u8(_p(xin), N, H, W, _p(buf), _stream()), "mstg_sharpen3_u8")
    out = _take(buf, nb, np.uint8, (N, H, W, 3), "sharpen3_u8")
    assert torch.equal(xin, _dev(x)), "mstg_sharpen3_u8 changed its input"
    return out


def _finish(c, s, m):
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    cin, sin, min_ = _dev(c), _dev(s), _dev(m)
    N, H, W = cin.shape[:3]
    nb = N * H * W * 3
    table = dimg._bilateral_table(5, 50, 50, cin.device)
    before = table.clone()
    need = lib.mstg_enhanced_style_finish_workspace_bytes(N, H, W)
    assert need > 0
    buf, ws = _guarded(nb), _guarded(need)
    _lib.check(lib.mstg_enhanced_style_finish(_p(cin), _p(sin), _p(min_), N, H, W, _p(table), _p(buf), _p(ws), need, _stream()),
               "mstg_enhanced_style_finish")
    out = _take(buf, nb, np.uint8, (N, H, W, 3), "enhanced_style_finish")
    _take(ws, need, np.uint8, (need,), "enhanced_style_finish (workspace)")
    assert torch.equal(cin, _dev(c)) and torch.equal(sin, _dev(s)) and torch.equal(table, before)
    assert torch.equal(min_.view(torch.int32), _dev(m).view(torch.int32)), "mstg_enhanced_style_finish changed an input"
    return out


# ---- 1. segment statistics, ratios and the map ---------------------------------------------------------------------------------------
def _label_maps(kind, h, w):
    """(labels (3, h, w) int32, S): three different label maps of one kind"""
    yy, xx = np.mgrid[0:h, 0:w]
    grids = [ER.grid_labels(h, w, seed, cell) for seed, cell in ((1, (9, 11)), (2, (5, 7)), (3, (16, 13)))]
    S = max(s for _, s in grids)
    g = np.stack([lab for lab, _ in grids])
    if kind == "one":
        return np.zeros((3, h, w), dtype=np.int32), 1
    if kind == "grid":
        return g, S
    if kind == "pixel":  # one label per pixel: every tile holds more labels than TILE_SLOTS
        p = (yy * w + xx).astype(np.int32)
        return np.stack([p, p[::-1].copy(), p[:, ::-1].copy()]), h * w
    if kind == "gaps":  # two of three labels have no pixel
        return g * 3 + 1, 3 * S
    if kind == "outside":  # negative labels, labels >= S, the largest int32
        o = g.copy()
        o[0][(yy + xx) % 7 == 0] = -5
        o[1][(yy * xx) % 11 == 3] = np.iinfo(np.int32).max
        o[2][yy % 5 == 0] = np.iinfo(np.int32).min
        return o, S - 3
    if kind == "borders":  # rings, columns and rows: segments that touch every border
        ring = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx)) // 3
        return np.stack([ring, xx // 5, yy // 4]).astype(np.int32), int(max(ring.max(), (w - 1) // 5, (h - 1) // 4)) + 1
    raise ValueError(kind)


def _check_map(x, labels, S, what):
    m, s, r = _segment_map(x, labels, S, smooth=False)
    ms, s2, r2 = _segment_map(x, labels, S, smooth=True)
    assert np.array_equal(s, s2) and np.array_equal(r.view(np.uint32), r2.view(np.uint32))
    for i in range(len(x)):
        want_sums, want_ratio = ER.segment_ratios(x[i], labels[i], S)
        assert (want_sums < (1 << 63)).all()
        _same(s[i], want_sums.astype(np.uint64), f"{what}: sums of image {i}")
        _same(r[i], want_ratio, f"{what}: ratios of image {i}")
        want_map = ER.map_of(labels[i], want_ratio)
        _same(m[i], want_map, f"{what}: map of image {i}")
        _same(ms[i], ER.gaussian_reflect(want_map), f"{what}: smoothed map of image {i}")


@pytest.mark.parametrize("shape", [(37, 53), (64, 64)])
@pytest.mark.parametrize("kind", ["one", "grid", "gaps", "outside", "borders"])
def test_segment_map(shape, kind):
    labels, S = _label_maps(kind, *shape)
    _check_map(_images(shape), labels, S, f"{kind} {shape}")


def test_segment_map_one_label_per_pixel():
    """1961 labels at 37 x 53: every tile overflows its TILE_SLOTS slots, most sums go straight to the global sums"""
    labels, S = _label_maps("pixel", 37, 53)
    assert S == 1961
    _check_map(_images((37, 53)), labels, S, "one label per pixel")


@pytest.mark.parametrize("extra", [0, 1, TILE_SLOTS])
def test_segment_map_around_the_tile_slot_limit(extra):
    """one 16 x 64 tile with exactly TILE_SLOTS labels (runs of eight pixels: the table is full, nothing overflows), one more
    (a single overflowing label) and twice as many (runs of four)"""
    h, w = TILE_H, TILE_W
    yy, xx = np.mgrid[0:h, 0:w]
    run = 4 if extra == TILE_SLOTS else 8
    lab = (yy * (w // run) + xx // run).astype(np.int32)
    if extra == 1:
        lab[7, 33] = TILE_SLOTS
    S = int(lab.max()) + 1
    assert S == TILE_SLOTS + extra
    _check_map(_images((h, w)), np.stack([lab, lab[::-1].copy(), lab[:, ::-1].copy()]), S, f"{S} labels in one tile")


def test_segment_map_is_reproducible_and_independent_of_n():
    x = _images((64, 64))
    labels, S = _label_maps("grid", 64, 64)
    a, b = _segment_map(x, labels, S, True), _segment_map(x, labels, S, True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    for i in range(3):
        one = _segment_map(x[i:i + 1], labels[i:i + 1], S, True)
        for u, v in zip(one, a):
            assert np.array_equal(u[0].view(np.uint8), v[i].view(np.uint8)), f"image {i} alone differs from image {i} of three"


# ---- 2 .. 5: the other stages --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (64, 64), (5, 3)])
def test_gaussian(shape):
    rs = np.random.RandomState(shape[0])
    planes = np.stack([rs.rand(*shape), 0.3 + 0.6 * (rs.rand(*shape) < 0.3), np.full(shape, 0.7)]).astype(np.float32)
    _same(_gauss(planes), np.stack([ER.gaussian_reflect(p) for p in planes]), f"gaussian {shape}")


@lru_cache(maxsize=None)
def _maps(shape, n=3):
    h, w = shape
    rs = np.random.RandomState(h + w)
    m = np.stack([ER.gaussian_reflect((0.3 + 0.6 * (rs.rand(h, w) < 0.4)).astype(np.float32)), rs.rand(h, w).astype(np.float32),
                  np.where(rs.rand(h, w) < 0.5, np.float32(0), np.float32(1))])[:n].astype(np.float32)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("shape", [(37, 53), (64, 64)])
def test_blend(shape):
    c, s, m = _images(shape), _styled(shape), _maps(shape)
    _same(_blend(c, s, m), np.stack([ER.blend_f32(*t) for t in zip(c, s, m)]), f"blend {shape}")
    wild = np.array(m)  # a caller's map outside [0, 1], with a NaN: clipped, the NaN gives 0
    wild[0, 0, :4] = (-0.5, 1.5, np.nan, 1e30)
    _same(_blend(c, s, wild), np.stack([ER.blend_f32(*t) for t in zip(c, s, wild)]), f"blend {shape} outside [0, 1]")


@pytest.mark.parametrize("shape", [(37, 53), (64, 64), (2, 2)])
def test_sharpen(shape):
    x = _images(shape)
    _same(_sharpen(x), np.stack([ER.sharpen3(im) for im in x]), f"sharpen {shape}")


TILED = [((64, 64), 3), ((40, 72), 3), ((256, 256), 1)]  # tiles 8 x 8, 5 x 9 (the inexact float32 interpolation), 32 x 32


@pytest.mark.parametrize("shape,n", TILED)
def test_clahe(shape, n):
    x = _images(shape, n)
    planes = np.ascontiguousarray(x.max(axis=-1))
    planes[0, : shape[0] // 2] //= 4  # a dark half: tiles with few levels and a large excess
    out, luts = _with_luts("mstg_clahe_u8", planes, 1)
    _same(luts, np.stack([ER.clahe_luts(p) for p in planes]), f"clahe tables {shape}")
    _same(out, np.stack([ER.clahe(p) for p in planes]), f"clahe {shape}")


@pytest.mark.parametrize("shape,n", TILED)
def test_hsv_enhance(shape, n):
    x = np.array(_images(shape, n))
    x[0, :8, :8] = 0                      # black: s = 0, v = 0
    x[0, :8, 8:16] = (200, 200, 200)      # grey: s = 0
    x[0, 8:16, :8] = (255, 0, 0)          # the pure hues
    x[0, 8:16, 8:16] = (0, 255, 255)
    out, _ = _with_luts("mstg_hsv_enhance_u8", x, 3)
    _same(out, np.stack([ER.hsv_enhance(im) for im in x]), f"hsv_enhance {shape}")


@pytest.mark.parametrize("shape,n", TILED)
def test_chain_equals_the_restatement_and_the_stages(shape, n):
    c, s, m = _images(shape, n), _styled(shape, n), _maps(shape, n)
    got = _finish(c, s, m)
    _same(got, np.stack([ER.enhanced_style_finish(*t) for t in zip(c, s, m)]), f"chain {shape}")
    from mstg_hip import image as dimg
    staged = dimg.bilateral_u8(_dev(_sharpen(_with_luts("mstg_hsv_enhance_u8", _blend(c, s, m), 3)[0])), 5, 50, 50)
    _same(got, staged.cpu().numpy(), f"chain {shape} against the stage entries")
    if n == 3:
        again = _finish(c, s, m)
        assert np.array_equal(got, again)
        for i in range(3):
            assert np.array_equal(_finish(c[i:i + 1], s[i:i + 1], m[i:i + 1])[0], got[i]), f"image {i} alone differs"


def _launches(fn):
    from mstg_hip import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        return lib.mstg_prof_count()
    finally:
        lib.mstg_prof_enable(0)


def test_launch_counts_are_the_headers():
    from mstg_hip import image as dimg
    shape = (64, 64)
    c, s, m = _dev(_images(shape)), _dev(_styled(shape)), _dev(_maps(shape))
    dimg.enhanced_style_finish(c[:1], s[:1], m[:1])  # the bilateral table is uploaded here, outside the counts
    for n in (1, 3):
        assert _launches(lambda: dimg.enhanced_style_finish(c[:n], s[:n], m[:n])) == 5
        for kind in ("one", "pixel" if n == 1 else "grid"):
            labels, S = _label_maps(kind, *shape)
            lab = _dev(labels)
            assert _launches(lambda: dimg.segment_blend_map(c[:n], lab[:n], S, smooth=False)) == 4
            assert _launches(lambda: dimg.segment_blend_map(c[:n], lab[:n], S, smooth=True)) == 6
        assert _launches(lambda: dimg.hsv_enhance_u8(c[:n])) == 2 and _launches(lambda: dimg.sharpen3_u8(c[:n])) == 1
        assert _launches(lambda: dimg.gaussian_reflect_f32(m[:n])) == 2 and _launches(lambda: dimg.blend_map_u8(c[:n], s[:n], m[:n])) == 1


# ---- the Python surface --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import enhanced_generator as eg
    torch.manual_seed(11)
    g = eg.EnhancedGenerator(16, 1).to(DEV)
    g.eval()
    return g


@pytest.mark.parametrize("size", [(90, 60), (60, 90), (64, 64), (300, 280)])  # (height, width): portrait, landscape, square, uncropped
def test_process_end_to_end_equals_the_stages_composed_by_hand(model, size):
    from mstg_hip import image as dimg
    h, w = size
    img = _dev(ER.smooth_noise(h, w, h + w))
    got = dimg.process_enhanced_local_style(model, img)
    new_w, new_h, box, back = ER.geometry(w, h)
    resized = dimg.resize_u8(img, (new_w, new_h), dimg.LANCZOS)
    canvas = dimg.paste_u8(resized, (0, 0, new_h, new_w), (256, 256), ((256 - new_h) // 2, (256 - new_w) // 2), fill=0)
    if new_h < 256:
        assert int(canvas[0].max()) == 0  # black bars
    with torch.no_grad():
        styled = dimg.to_u8(model(dimg.to_tensor(canvas).unsqueeze(0))[0])
    labels = dimg.felzenszwalb_labels(canvas)
    assert labels.dtype == np.int32 and labels.min() == 0 and len(np.unique(labels)) == labels.max() + 1
    m, sums, ratio = dimg.segment_blend_map(canvas, labels, return_stats=True)
    assert int(sums[:, 0].sum()) == 256 * 256 and float(ratio.min()) >= 0.3 and float(ratio.max()) <= 0.9
    out = dimg.bilateral_u8(dimg.sharpen3_u8(dimg.hsv_enhance_u8(dimg.blend_map_u8(canvas, styled, m))), 5, 50, 50)
    if box is not None:
        out = dimg.crop_u8(out, *box)
    if size == (300, 280):
        assert box == (0, 0, 256, 256) and back  # larger than the canvas in both directions: the crop as written takes everything
    if back:
        out = dimg.resize_u8(out, (w, h), dimg.LANCZOS)
    assert back == (max(h, w) > 256)
    assert got.shape == out.shape and torch.equal(got, out)
    # a small square image stays the 256 x 256 canvas: the reference resizes back only an image larger than the canvas (:280)
    assert tuple(got.shape) == ((h, w, 3) if back else (256, 256, 3) if box is None else (box[3] - box[1], box[2] - box[0], 3))
    other = torch.from_numpy(ER.grid_labels(256, 256, 1, (32, 40))[0]).to(DEV)  # a caller's own labels
    got2 = dimg.process_enhanced_local_style(model, img, segments=other)
    assert got2.shape == got.shape and not torch.equal(got2, got)


def test_drop_in_command_line_and_stage_functions(model, tmp_path):
    from PIL import Image
    import enhanced_local_style as E
    from mstg_hip import image as dimg
    img = ER.smooth_noise(120, 80, 4)
    Image.fromarray(img).save(tmp_path / "in.png")
    torch.save({"G_AB_state_dict": model.state_dict()}, tmp_path / "ckpt.pth")
    E.main(["--image", str(tmp_path / "in.png"), "--model", str(tmp_path / "ckpt.pth"), "--output", str(tmp_path / "out" / "o.png")])
    got = np.asarray(Image.open(tmp_path / "out" / "o.png"))
    want = dimg.process_enhanced_local_style(model, _dev(img)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # analyze_segments and determine_blend_ratios: the reference's two calls give the device's map, bit for bit
    canvas = ER.smooth_noise(64, 64, 9)
    segments = E.get_segmentation_mask(Image.fromarray(canvas))
    stats = E.analyze_segments(Image.fromarray(canvas), segments)
    assert set(stats) == set(np.unique(segments).tolist())
    assert set(next(iter(stats.values()))) == {"avg_color_rgb", "avg_color_hsv", "std_color", "edge_density", "size", "position"}
    m = E.determine_blend_ratios(stats, segments, canvas.shape)
    assert m.dtype == np.float32
    _same(m, dimg.segment_blend_map(_dev(canvas), segments).cpu().numpy(), "determine_blend_ratios")
    for method in ("slic", "quickshift"):
        with pytest.raises(NotImplementedError, match=method):
            E.get_segmentation_mask(canvas, method=method)
    t = E.preprocess_image(Image.fromarray(canvas), 32)
    back = np.asarray(E.standard_postprocess(E.preprocess_image(canvas, 64))).astype(int)  # the output conversion truncates
    assert tuple(t.shape) == (1, 3, 32, 32) and back.shape == canvas.shape and np.abs(back - canvas).max() <= 1


def test_refusals_name_the_value():
    from mstg_hip import image as dimg
    x = _dev(_images((37, 53)))
    for fn in (dimg.hsv_enhance_u8, lambda t: dimg.clahe_u8(t[..., 0]), lambda t: dimg.enhanced_style_finish(t, t, torch.zeros(3, 37, 53, device=DEV))):
        with pytest.raises(RuntimeError, match="H = 37, W = 53"):
            fn(x)
    with pytest.raises(RuntimeError, match="H = 1, W = 53"):
        dimg.segment_blend_map(x[:, :1], np.zeros((3, 1, 53), dtype=np.int32))
    with pytest.raises(RuntimeError, match="num_segments = 0"):
        dimg.segment_blend_map(x, np.zeros((3, 37, 53), dtype=np.int32), num_segments=0)
    with pytest.raises(RuntimeError, match=r"labels of shape \(3, 37, 53\)"):
        dimg.segment_blend_map(x, np.zeros((3, 37, 52), dtype=np.int32))
    with pytest.raises(RuntimeError, match=r"blend map of shape"):
        dimg.blend_map_u8(x, x, np.zeros((37, 53), dtype=np.float32))
    with pytest.raises(RuntimeError, match="sigma = 0.8"):
        dimg.felzenszwalb_labels(_images((37, 53))[0], sigma=0.8)
    with pytest.raises(RuntimeError, match="overlaps"):
        from mstg_hip import _lib
        from mstg_hip.ops import _p, _stream
        _lib.check(_lib.load().mstg_sharpen3_u8(_p(x), 3, 37, 53, _p(x), _stream()), "mstg_sharpen3_u8")
