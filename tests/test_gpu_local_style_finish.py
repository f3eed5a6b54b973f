"""The finish of the 'enhanced' local-style mode on the device (csrc/local_style.hip local_style_finish_kernel through
mstg_local_style_finish / mstg_local_style_enhanced, mstg_hip.image.local_style_finish and mode="enhanced" of process_local_style
/ process_local_style_batch) against the numpy restatement of tests/local_style_finish_ref.py, byte for byte: the colour step
over all byte pairs, the smoothing on crafted detail masks at sizes around the tile, the four launches from the canvas, the two
callers end to end, the launch count and reproducibility.  The restatement has not been compared with an OpenCV binary (see its
docstring)."""
import numpy as np
import pytest
import torch

import local_style_finish_ref as FR
import local_style_ref as LR
from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_H, TILE_W = 32, 64  # the kernel's tile
LEVELS = np.array(LR.weights(0.8, 0.7))  # 0.8, 1.0, 0.59


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _finish(orig, styled, weight, detail, enhance, smooth):
    """mstg_local_style_finish on (N, H, W, 3) / (N, H, W) numpy arrays -> numpy; 64 guard bytes behind ``out`` must survive and
    the inputs must not change"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    o, s, w = _dev(orig), _dev(styled), _dev(weight)
    d = _dev(detail.astype(np.uint8)) if detail is not None else None
    N, H, W = o.shape[:3]
    nbytes = N * H * W * 3
    buf = torch.full((nbytes + 64,), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mstg_local_style_finish(_p(o), _p(s), _p(w), _p(d), N, H, W, int(enhance), int(smooth), _p(buf), _stream()),
               "mstg_local_style_finish")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), "the kernel wrote behind its output"
    assert torch.equal(o, _dev(orig)) and torch.equal(s, _dev(styled)) and torch.equal(w, _dev(weight)), "the kernel changed an input"
    assert d is None or torch.equal(d, _dev(detail.astype(np.uint8))), "the kernel changed the detail mask"
    return out[:nbytes].reshape(N, H, W, 3)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}"


# ---- 1. the colour step over all byte pairs -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def byte_pairs():
    r, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    orig = np.stack([r, c, r], axis=-1)[None]          # every (orig, styled) pair in channel 0, swapped in channel 1,
    styled = np.stack([c, r, 255 - c], axis=-1)[None]  # against the complement in channel 2
    return np.ascontiguousarray(orig), np.ascontiguousarray(styled)


@pytest.mark.parametrize("w", [0.8, 1.0, 0.59, 0.0, "random"])
def test_colour_step_all_byte_pairs(byte_pairs, w):
    from mstg_hip import image as dimg
    orig, styled = byte_pairs
    if w == "random":  # uniform in [1/16, 15/16]: every non-zero blend value is at least 1/16 (the restatement's exact range)
        wm = 0.0625 + 0.875 * np.random.RandomState(5).rand(1, 256, 256)
    else:
        wm = np.full((1, 256, 256), LEVELS[2] if w == 0.59 else w)
    x = FR.blend_f64(orig, styled, wm)
    _same(_finish(orig, styled, wm, None, 1, 0), FR.enhance_u8(x), f"enhance, w = {w}")
    plain = _finish(orig, styled, wm, None, 0, 0)
    _same(plain, np.clip(x, 0, 255).astype(np.uint8), f"blend, w = {w}")
    blend = dimg.blend_u8(_dev(orig[0]), _dev(styled[0]), weight_map=_dev(wm[0]))  # mstg_blend_u8 itself
    assert np.array_equal(plain[0], blend.cpu().numpy())
    both = dimg.local_style_finish(_dev(orig[0]), _dev(styled[0]), _dev(wm[0]), None, enhance_colors=True, smooth=False)
    assert both.shape == (256, 256, 3) and np.array_equal(both.cpu().numpy(), FR.enhance_u8(x)[0])


# ---- 2. smoothing on crafted masks ----------------------------------------------------------------------------------------------------
def _mask(kind, h, w, seed):
    m = np.zeros((h, w), dtype=bool)
    if kind == "pixels":  # single pixels in the corners and on both sides of every tile seam the image has
        pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
        for y in (TILE_H - 1, TILE_H, 4 * TILE_H - 1, 4 * TILE_H):
            for x in (TILE_W - 1, TILE_W, 2 * TILE_W - 1, 2 * TILE_W):
                pts.append((y, x))
        for y, x in pts:
            if y < h and x < w:
                m[y, x] = True
    elif kind == "frame":  # a one-pixel frame on the image border
        m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    elif kind == "checker":  # cells of 10 x 10
        yy, xx = np.mgrid[0:h, 0:w]
        m = ((yy // 10 + xx // 10) % 2).astype(bool)
    else:
        m = np.random.RandomState(seed).rand(h, w) < 0.02
    return m


@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (7, 9), (TILE_H + 1, TILE_W + 1), (67, 93), (256, 256)])
@pytest.mark.parametrize("kinds", [("pixels", "frame", "checker"), ("random", "checker", "pixels")])
def test_smoothing_on_crafted_masks(kinds, shape):
    h, w = shape
    rs = np.random.RandomState(h * 1000 + w)
    masks = [_mask(k, h, w, 7 + i) for i, k in enumerate(kinds)]
    share = float(np.mean([FR.boundary(m).mean() for m in masks]))
    print(f"{kinds} {shape}: boundary share {100 * share:.1f} %")
    if shape != (1, 1):  # a one-pixel image has no boundary; every other case takes both branches
        assert 0.05 < share < 0.95, share
    for order in ((0, 1, 2), (2, 1, 0)):  # different masks per image, both ways round
        detail = np.stack([masks[i] for i in order])
        orig = rs.randint(0, 256, size=(3, h, w, 3)).astype(np.uint8)
        styled = rs.randint(0, 256, size=(3, h, w, 3)).astype(np.uint8)
        weight = LEVELS[rs.randint(0, 3, size=(3, h, w))]
        got = _finish(orig, styled, weight, detail, 1, 1)
        for i in range(3):
            _same(got[i], FR.finish(orig[i], styled[i], weight[i], detail[i]), f"{kinds[order[i]]} {shape} image {i}")
    # smooth off does not read the mask
    _same(_finish(orig, styled, weight, None, 1, 0)[0], FR.finish(orig[0], styled[0], weight[0], None, True, False), "smooth off")


def test_smooth_without_enhance_is_refused_by_name():
    from mstg_hip import image as dimg
    z = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="smooth without enhance_colors"):
        dimg.local_style_finish(z, z.clone(), torch.zeros(8, 8, dtype=torch.float64, device=DEV), torch.zeros(8, 8, dtype=torch.bool, device=DEV),
                                enhance_colors=False, smooth=True)


# ---- 3. four launches from the canvas -------------------------------------------------------------------------------------------------
def _enhanced(canvases, styled, enhance=1, smooth=1, strength=0.8, detail=0.7):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    c, s = _dev(canvases), _dev(styled)
    N, H, W = c.shape[:3]
    need = lib.mstg_local_style_enhanced_workspace_bytes(N, H, W)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full_like(c, 9)
    w_base, w_sky, w_detail = LR.weights(strength, detail)
    _lib.check(lib.mstg_local_style_enhanced(_p(c), _p(s), N, H, W, w_base, w_sky, w_detail, enhance, smooth, _p(out), _p(ws), need, _stream()),
               "mstg_local_style_enhanced")
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def canvas_cases():
    """canvases, styled images and the restatement's results per shape, computed once.  gradient_rects is the case that must
    exercise both branches of the smoothing (its boundary share is asserted to lie between 5 % and 95 %); blocky, whose detail
    mask covers nearly everything, and the bright low-saturation canvas with has_sky are the degenerate ones and carry no such
    assertion."""
    out = {}
    for shape in ((96, 80), (256, 256)):
        h, w = shape
        third = LR.bright_low_saturation(h, w, 22) if shape == (256, 256) else LR.gradient_rects(h, w, 31)
        canvases = np.stack([LR.gradient_rects(h, w, 25), LR.blocky(h, w, 24), third])
        styled = np.random.RandomState(h).randint(0, 256, size=canvases.shape).astype(np.uint8)
        refs = [FR.enhanced_ref(c, s) for c, s in zip(canvases, styled)]
        for i, (_, m) in enumerate(refs):
            assert np.abs(m["gauss"] - 0.1).min() > 1e-9, (shape, i)  # the precondition of an exact detail mask
        assert 0.05 < FR.boundary(refs[0][1]["detail"]).mean() < 0.95
        out[shape] = (canvases, styled, refs)
    assert out[(256, 256)][2][2][1]["has_sky"] and (out[(256, 256)][2][2][1]["weight"] == 1.0).any()  # the 70 % sky case
    return out


@pytest.mark.parametrize("shape", [(96, 80), (256, 256)])
def test_enhanced_from_the_canvas(canvas_cases, shape):
    from mstg_hip import _lib
    canvases, styled, refs = canvas_cases[shape]
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        got = _enhanced(canvases, styled)
        assert lib.mstg_prof_count() == 4
    finally:
        lib.mstg_prof_enable(0)
    got = got.cpu().numpy()
    for i, (want, m) in enumerate(refs):
        _same(got[i], want, f"{shape} image {i}")
    e_only = _enhanced(canvases, styled, 1, 0).cpu().numpy()
    plain = _enhanced(canvases, styled, 0, 0).cpu().numpy()
    for i, (_, m) in enumerate(refs):
        _same(e_only[i], FR.finish(canvases[i], styled[i], m["weight"], None, True, False), f"{shape} image {i}, smooth off")
        _same(plain[i], IR.blend_weight_map(canvases[i], styled[i], m["weight"]), f"{shape} image {i}, both off")


# ---- 4. the callers -------------------------------------------------------------------------------------------------------------------
def _img(h, w, seed):
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, size=(h // 4 + 2, w // 4 + 2, 3)).astype(np.uint8)
    img = np.kron(base, np.ones((4, 4, 1), dtype=np.uint8))[:h, :w]
    return np.ascontiguousarray((img.astype(np.int32) + rs.randint(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8))


def _pil_or_numpy():
    try:
        import PIL  # noqa: F401
        return IR.pil_resize
    except ImportError:
        return IR.resample_numpy


def stub(x):  # exact in fp32 and not symmetric: a swapped image or axis shows
    return -x.flip(3)


def stub_np(x):
    return -np.asarray(x)[:, :, :, ::-1]


MIXED = [(300, 420), (420, 300), (256, 256), (97, 301), (64, 48)]  # landscape, portrait, square, two small ones


@pytest.fixture(scope="module")
def mixed():
    arrays = [_img(h, w, 50 + i) for i, (h, w) in enumerate(MIXED)]
    return arrays, [_dev(a) for a in arrays]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_process_local_style_enhanced_defaults(mixed, k):
    from mstg_hip import image as dimg
    rz = _pil_or_numpy()
    arr, dev = mixed[0][k], mixed[1][k]
    out = dimg.process_local_style(stub, dev, mode="enhanced").cpu().numpy()
    ref, m = FR.process_local_style_enhanced_ref(stub_np, arr, resize=rz)
    assert np.abs(m["gauss"] - 0.1).min() > 1e-9 and m["detail"].any() and not m["detail"].all()
    _same(out, ref, f"image {k}")
    e_only = dimg.process_local_style(stub, dev, mode="enhanced", enhance_colors=True, smooth=False).cpu().numpy()
    _same(e_only, FR.process_local_style_enhanced_ref(stub_np, arr, smooth=False, resize=rz)[0], f"image {k}, smooth off")
    assert (e_only != out).any()


def test_flags_off_raise_and_other_modes(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    rz = _pil_or_numpy()
    for im in images[:3]:
        off = dimg.process_local_style(stub, im, mode="enhanced", enhance_colors=False, smooth=False)
        assert torch.equal(off, dimg.process_local_style(stub, im, mode="weight_map", weight_map=None))
    offs = dimg.process_local_style_batch(stub, images, mode="enhanced", enhance_colors=False, smooth=False)
    for a, b in zip(offs, dimg.process_local_style_batch(stub, images, mode="weight_map")):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="smooth without enhance_colors"):
        dimg.process_local_style(stub, images[0], mode="enhanced", enhance_colors=False, smooth=True)
    with pytest.raises(RuntimeError, match="smooth without enhance_colors"):
        dimg.process_local_style_batch(stub, images, mode="enhanced", enhance_colors=False)
    adv = dimg.process_local_style(stub, images[0], mode="advanced")  # every other name: the styled image, as before
    assert np.array_equal(adv.cpu().numpy(), IR.process_local_style_ref(stub_np, arrays[0], mode="advanced", resize=rz))
    advb = dimg.process_local_style_batch(stub, images[:2], mode="advanced", enhance_colors=False, smooth=True)  # keywords ignored there
    assert torch.equal(advb[0], adv)
    with pytest.raises(RuntimeError, match="at most 147456 pixels"):
        dimg.process_local_style_batch(stub, images[:1], mode="enhanced", target=385)


def test_batch_equals_the_one_image_function(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    loop = [dimg.process_local_style(stub, im, mode="enhanced") for im in images]
    calls = []

    def model(x):
        calls.append(x.shape[0])
        return stub(x)
    for bs, want_calls in ((2, [2, 2, 1]), (5, [5])):  # chunked and unchunked
        del calls[:]
        outs = dimg.process_local_style_batch(model, images, mode="enhanced", batch_size=bs)
        assert calls == want_calls
        for i, (a, b) in enumerate(zip(loop, outs)):
            assert a.shape == b.shape and torch.equal(a, b), f"batch_size {bs} image {i}: {int((a != b).sum())} of {a.numel()} bytes differ"


# ---- 5. launch count ------------------------------------------------------------------------------------------------------------------
def test_enhanced_costs_the_launches_of_weight_map(mixed):
    from mstg_hip import _lib, image as dimg
    lib = _lib.load()
    images = mixed[1]

    def launches(fn):
        torch.cuda.synchronize()
        lib.mstg_prof_enable(1)
        try:
            fn()
            torch.cuda.synchronize()
            return lib.mstg_prof_count()
        finally:
            lib.mstg_prof_enable(0)
    for imgs in (images[:1], images):  # 1 and 5 images
        assert launches(lambda: dimg.process_local_style_batch(stub, imgs, mode="enhanced")) == \
            launches(lambda: dimg.process_local_style_batch(stub, imgs, mode="weight_map")) == 9
    assert launches(lambda: dimg.process_local_style(stub, images[0], mode="enhanced")) == \
        launches(lambda: dimg.process_local_style(stub, images[0], mode="weight_map"))


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(96, 80), (256, 256)])
def test_reproducible(canvas_cases, shape):
    canvases, styled, _ = canvas_cases[shape]
    assert torch.equal(_enhanced(canvases, styled), _enhanced(canvases, styled))
