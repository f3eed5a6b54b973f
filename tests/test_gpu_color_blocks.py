"""The colour-block repair on the device (csrc/color_blocks.hip through mstg_color_block_mask, mstg_color_correct_u8,
mstg_bilateral_wide_u8, mstg_detail_blend_u8 and mstg_color_block_fix; mstg_hip.image.fix_color_blocks and its stage functions; the
drop-in improved_smooth.py) against the numpy restatement of tests/color_blocks_ref.py, byte for byte and the mask bit for bit:
every stage with three different images per launch, 64 guard bytes behind the output and the inputs unchanged; the wide bilateral
filter also against the existing mstg_bilateral_u8 at d = 3, 5, 7, 9; the chain against the composition of the stage entries; the
launch count; reproducibility; the refusals by name.  The restatement has not been compared with an OpenCV binary (see its
docstring)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import color_blocks_ref as CR
import standard_mode_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
BAND_ROWS, BAND_COLS = 4, 256  # the tiling of cb_bilateral_wide_kernel: a wave per row of a band, four pixels per lane


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


def _make(kind, h, w, seed):
    return CR.blocks(h, w, seed) if kind == "blocks" else SR.image(kind, h, w, seed)


TRIPLES = (("noise", "blocks", "gradient"), ("constant", "blocks", "noise"))


@lru_cache(maxsize=None)
def _images(shape, which):
    """three different images of one shape, (3, H, W, 3); read-only so that the cached references stay valid"""
    h, w = shape
    a = np.stack([_make(kind, h, w, seed=7 * which + i + h) for i, kind in enumerate(TRIPLES[which])])
    a.setflags(write=False)
    return a


def _guarded(nbytes):
    return torch.full((nbytes + GUARD,), 7, dtype=torch.uint8, device=DEV)


def _take(buf, nbytes, shape, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), f"{what} wrote behind its output"
    return out[:nbytes].reshape(shape)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}: "
                                                       f"{got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


# ---- the stage entries on numpy batches ----------------------------------------------------------------------------------------------
def _mask(x, threshold=30.0, kernel_size=11):
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    buf, ws = _guarded(N * H * W), torch.empty(N * H * W, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mstg_color_block_mask(_p(xin), N, H, W, _p(dimg._lab_table(xin.device)), threshold, kernel_size, _p(buf), _p(ws),
                                                 ws.numel(), _stream()), "mstg_color_block_mask")
    out = _take(buf, N * H * W, (N, H, W), "mstg_color_block_mask")
    assert torch.equal(xin, _dev(x)), "mstg_color_block_mask changed its input"
    return out


def _correct(x, mask, radius=50):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    xin, m = _dev(x), _dev(mask.astype(np.uint8))
    N, H, W = xin.shape[:3]
    nb = N * H * W * 3
    buf, ws = _guarded(nb), torch.empty(nb, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mstg_color_correct_u8(_p(xin), _p(m), N, H, W, radius, _p(buf), _p(ws), nb * 4, _stream()), "mstg_color_correct_u8")
    out = _take(buf, nb, (N, H, W, 3), "mstg_color_correct_u8")
    assert torch.equal(xin, _dev(x)) and torch.equal(m, _dev(mask.astype(np.uint8))), "mstg_color_correct_u8 changed an input"
    return out


def _wide(x, d, sigma_color, sigma_space):
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    nb = N * H * W * 3
    radius, table = dimg._bilateral_wide_table(d, sigma_color, sigma_space, xin.device)
    assert radius == CR.bilateral_radius(d, sigma_space)
    before = table.clone()
    buf = _guarded(nb)
    _lib.check(_lib.load().mstg_bilateral_wide_u8(_p(xin), N, H, W, radius, _p(table), _p(buf), _stream()), "mstg_bilateral_wide_u8")
    out = _take(buf, nb, (N, H, W, 3), "mstg_bilateral_wide_u8")
    assert torch.equal(xin, _dev(x)) and torch.equal(table, before), "mstg_bilateral_wide_u8 changed an input"
    return out


def _blend(x, orig, alpha, beta, sigma=3.0):
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    xin, oin = _dev(x), _dev(orig)
    N, H, W = xin.shape[:3]
    nb = N * H * W * 3
    ksize = CR.detail_ksize(sigma)
    kern = dimg._detail_kernel(ksize, sigma, xin.device)
    buf, ws = _guarded(nb), torch.empty(nb, dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().mstg_detail_blend_u8(_p(xin), _p(oin), N, H, W, _p(kern), ksize, 1 - alpha, alpha, beta, _p(buf), _p(ws), nb * 8,
                                                _stream()), "mstg_detail_blend_u8")
    out = _take(buf, nb, (N, H, W, 3), "mstg_detail_blend_u8")
    assert torch.equal(xin, _dev(x)) and torch.equal(oin, _dev(orig)), "mstg_detail_blend_u8 changed an input"
    return out


# ---- 1. the mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 5), (16, 64), (67, 93), (130, 150)])
def test_mask(shape):
    """bit for bit on noise, blocks, gradient and constant images.  Checked on the restatement's mask so that all three branches of
    the kernels are exercised: a constant image flags nothing; from 16 x 64 pixels on (below that an image is too small for the
    shares to mean anything: a 1 x 1 image has no gradient at all) noise flags everything and the block images flag between 5 %
    and 95 % of their pixels."""
    for which in (0, 1):
        x = _images(shape, which)
        want = np.stack([CR.block_mask(im) for im in x])
        for kind, m in zip(TRIPLES[which], want):
            if kind == "constant":
                assert not m.any()
            elif shape[0] >= 16 and shape[1] >= 64 and kind == "noise":
                assert m.all()
            elif shape[0] >= 16 and shape[1] >= 64 and kind == "blocks":
                assert 0.05 < m.mean() < 0.95, m.mean()
        _same(_mask(x), want.astype(np.uint8), f"mask {shape} {TRIPLES[which]}")
    x = _images(shape, 0)
    for threshold, k in ((12.5, 1), (30.0, 15), (300.0, 5)):  # other arguments: a fractional threshold, no dilation, the widest asked for
        _same(_mask(x, threshold, k), np.stack([CR.block_mask(im, threshold, k) for im in x]).astype(np.uint8), f"mask {shape} {threshold} {k}")


# ---- 2. the correction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (30, 40), (101, 102), (130, 150)])
def test_correction(shape):
    x = _images(shape, 0)
    masks = {"restatement": np.stack([CR.block_mask(im) for im in x]), "none": np.zeros((3,) + shape, dtype=bool),
             "random": np.random.RandomState(shape[0]).rand(3, *shape) < 0.5, "all": np.ones((3,) + shape, dtype=bool)}
    for name, m in masks.items():
        got = _correct(x, m)
        _same(got, np.stack([CR.correct(im, mi) for im, mi in zip(x, m)]), f"correction {shape} mask {name}")
        if name == "none":
            _same(got, x, f"correction {shape} without a flagged pixel is the identity")
    m = masks["random"]
    _same(_correct(x, m, 3), np.stack([CR.correct(im, mi, 3) for im, mi in zip(x, m)]), f"correction {shape} radius 3")


# ---- 3. the wide bilateral filter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 5, 7, 9])
def test_wide_equals_the_existing_kernel(d):
    """(a) an independent implementation on the device that covers every band: 256 x 256 has 64 bands, 5 x 300 two columns of them"""
    from mstg_hip import image as dimg
    for shape in ((67, 93), (256, 256), (5, 300)):
        x = _images(shape, 0)
        for sc, ss in ((75, 75), (10, 3)):
            want = dimg.bilateral_u8(_dev(x), d, sc, ss).cpu().numpy()
            _same(_wide(x, d, sc, ss), want, f"wide d = {d} ({sc}, {ss}) {shape}")


@pytest.mark.parametrize("shape", [(67, 93), (130, 150), (6, 261)])
def test_wide_radius_12(shape):
    """(b) whole images at radius 12 (d = 0, sigma_space 8); 6 x 261 crosses the seam between two columns of bands"""
    x = _images(shape, 0)
    _same(_wide(x, 0, 102.0, 8), CR.bilateral_wide(x, 0, 102.0, 8), f"wide radius 12 {shape}")


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (40, 33), (24, 100)])
def test_wide_radius_90_whole_images(shape):
    """(c) sides shorter than the radius: mirrored again and again.  Three images per launch; up to 7 x 5 the restatement filters
    all of them whole, above that the first one whole and 48 pixels (the corners among them) of the other two: numpy needs three
    seconds for one whole image of 24 x 100 at 25 445 taps."""
    x = _images(shape, 0)
    got = _wide(x, 0, 0.4 * 255, 60)
    whole = 3 if shape[0] * shape[1] <= 35 else 1
    _same(got[:whole], CR.bilateral_wide(x[:whole], 0, 0.4 * 255, 60), f"wide radius 90 {shape}")
    if whole < 3:
        H, W = shape
        rs = np.random.RandomState(H)
        coords = sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} | {(int(y), int(c)) for y, c in zip(rs.randint(0, H, 44), rs.randint(0, W, 44))})
        yy, xx = np.array([c[0] for c in coords]), np.array([c[1] for c in coords])
        _same(got[1:, yy, xx], CR.bilateral_wide(x[1:], 0, 0.4 * 255, 60, coords), f"wide radius 90 {shape}, images 1 and 2 at {len(coords)} pixels")


def _chosen(H, W):
    """pixels for (d): the corners, both sides of every seam between two bands, 89, 90 and 91 from each border, the centre"""
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)}
    for k, y in enumerate(range(BAND_ROWS, H, BAND_ROWS)):  # rows y - 1 | y; the column moves across the lanes' groups of four pixels
        pts |= {(y - 1, (37 * k) % W), (y, (37 * k + 3) % W)}
    for x in range(BAND_COLS, W, BAND_COLS):
        pts |= {(H // 3, x - 1), (H // 3, x)}
    for t in (89, 90, 91):
        pts |= {(t, W // 2), (H - 1 - t, W // 2 + 1), (H // 2, t), (H // 2 + 1, W - 1 - t), (t, t), (H - 1 - t, W - 1 - t)}
    return sorted(pts)


@pytest.mark.parametrize("shape", [(200, 256), (256, 256)])
def test_wide_radius_90_chosen_pixels(shape):
    """(d) the flagship size: the device filters whole images, the restatement the chosen pixels"""
    coords = _chosen(*shape)
    assert len(coords) >= 64
    x = _images(shape, 0)
    got = _wide(x, 0, 0.4 * 255, 60)
    yy, xx = np.array([c[0] for c in coords]), np.array([c[1] for c in coords])
    want = CR.bilateral_wide(x, 0, 0.4 * 255, 60, coords)
    bad = np.argwhere(got[:, yy, xx] != want)
    assert len(bad) == 0, f"wide radius 90 {shape}: {len(bad)} of {want.size} bytes differ, first at image {bad[0][0]} pixel {coords[bad[0][1]]}"


# ---- 4. the detail blend --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (12, 13), (67, 93), (130, 150)])
def test_detail_blend(shape):
    x, other = _images(shape, 0), np.ascontiguousarray(_images(shape, 1)[::-1])
    for orig, name in ((x, "orig equal to img"), (other, "orig different")):
        for alpha, beta in ((0.1, 0.5), (0.3, 1.5)):
            want = np.stack([CR.detail_blend(a, b, alpha, beta) for a, b in zip(x, orig)])
            _same(_blend(x, orig, alpha, beta), want, f"detail blend {shape} {name} ({alpha}, {beta})")
    want = np.stack([CR.detail_blend(a, b, 0.1, 0.5, 3.7) for a, b in zip(x, other)])  # 31 taps: the largest size built
    assert CR.detail_ksize(3.7) == 31
    _same(_blend(x, other, 0.1, 0.5, 3.7), want, f"detail blend {shape} sigma 3.7")


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------------
CHAIN_SHAPE = (67, 93)


@pytest.fixture(scope="module")
def chain_inputs():
    return _images(CHAIN_SHAPE, 0), np.ascontiguousarray(_images(CHAIN_SHAPE, 1)[::-1])


def _composed(x, orig):
    from mstg_hip import image as dimg
    y = dimg.edge_preserving_smoothing(dimg.adaptive_color_correction(x, dimg.detect_color_blocks(x)))
    return y if orig is None else dimg.detail_enhancing_blend(y, orig, alpha=0.1, beta=0.5)


@pytest.mark.parametrize("with_orig", [False, True])
def test_chain_equals_the_composed_stages(chain_inputs, with_orig):
    from mstg_hip import image as dimg
    x, o = _dev(chain_inputs[0]), (_dev(chain_inputs[1]) if with_orig else None)
    got = dimg.fix_color_blocks(x, o)
    want = _composed(x, o)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} bytes differ"
    assert torch.equal(x, _dev(chain_inputs[0])) and (o is None or torch.equal(o, _dev(chain_inputs[1]))), "the chain changed an input"
    assert torch.equal(got, dimg.fix_color_blocks(x, o)), "two runs differ"
    one = dimg.fix_color_blocks(x[:1], None if o is None else o[:1])
    assert torch.equal(one[0], got[0]), "N = 1 differs from the first image of N = 3"
    assert torch.equal(dimg.adaptive_color_correction(x), dimg.adaptive_color_correction(x, dimg.detect_color_blocks(x)))


def test_chain_against_the_restatement(chain_inputs):
    from mstg_hip import image as dimg
    img, orig = chain_inputs[0][1], chain_inputs[1][1]  # the block image, whose mask has flagged and unflagged pixels
    rs = np.random.RandomState(9)
    coords = sorted({(int(y), int(x)) for y, x in zip(rs.randint(0, CHAIN_SHAPE[0], 24), rs.randint(0, CHAIN_SHAPE[1], 24))})
    yy, xx = np.array([c[0] for c in coords]), np.array([c[1] for c in coords])
    got = dimg.fix_color_blocks(_dev(img), _dev(orig)).cpu().numpy()
    _same(got[yy, xx], CR.fix_color_blocks(img, orig, coords), "chain with an original")
    got = dimg.fix_color_blocks(_dev(img)).cpu().numpy()
    _same(got[yy, xx], CR.fix_color_blocks(img, None, coords), "chain without an original")


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


def test_launch_count_is_the_headers(chain_inputs):
    from mstg_hip import image as dimg
    x, o = _dev(chain_inputs[0]), _dev(chain_inputs[1])
    dimg.fix_color_blocks(x[:1], o[:1])  # the tables are uploaded here, outside the counts
    for n in (1, 3):
        assert _launches(lambda: dimg.fix_color_blocks(x[:n])) == 5
        assert _launches(lambda: dimg.fix_color_blocks(x[:n], o[:n])) == 7


# ---- 6. the Python surface ------------------------------------------------------------------------------------------------------------
def test_python_surface_3d_and_4d(chain_inputs):
    from mstg_hip import image as dimg
    x, o = _dev(chain_inputs[0]), _dev(chain_inputs[1])
    m = dimg.detect_color_blocks(x)
    assert m.dtype == torch.bool and m.shape == (3,) + CHAIN_SHAPE
    assert np.array_equal(m.cpu().numpy(), np.stack([CR.block_mask(im) for im in chain_inputs[0]]))
    m1 = dimg.detect_color_blocks(x[1])
    assert m1.shape == CHAIN_SHAPE and torch.equal(m1, m[1])
    calls = ((dimg.adaptive_color_correction, (m,), (m[1],)), (dimg.adaptive_color_correction, (), ()),
             (dimg.edge_preserving_smoothing, (8, 0.2), (8, 0.2)), (dimg.detail_enhancing_blend, (o,), (o[1],)),
             (dimg.fix_color_blocks, (o,), (o[1],)))
    for fn, a4, a3 in calls:
        y4, y3 = fn(x, *a4), fn(x[1], *a3)
        assert y4.shape == x.shape and y3.shape == x.shape[1:] and y4.dtype == torch.uint8, fn.__name__
        assert torch.equal(y4[1], y3), fn.__name__
    big = torch.stack([dimg.resize_u8(im, (40, 31), dimg.LANCZOS) for im in o])  # an original of another size: resized first
    back = torch.stack([dimg.resize_u8(im, (CHAIN_SHAPE[1], CHAIN_SHAPE[0]), dimg.LANCZOS) for im in big])
    assert torch.equal(dimg.detail_enhancing_blend(x, big), dimg.detail_enhancing_blend(x, back))
    _same(dimg.edge_preserving_smoothing(x, 8, 0.2).cpu().numpy(), CR.bilateral_wide(chain_inputs[0], 0, 0.2 * 255, 8), "sigma_s 8")


def test_refusals_by_name():
    from mstg_hip import image as dimg
    z = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="radius = 92 "):  # cvRound(61 * 1.5) = cvRound(91.5) = 92: half to even
        dimg.edge_preserving_smoothing(z, sigma_s=61)
    with pytest.raises(RuntimeError, match="radius = 91 "):
        dimg.edge_preserving_smoothing(z, sigma_s=60.7)
    with pytest.raises(RuntimeError, match="radius = 91 "):
        dimg.bilateral_wide_u8(z, d=183)
    with pytest.raises(RuntimeError, match="kernel_size = 10 "):
        dimg.detect_color_blocks(z, kernel_size=10)
    with pytest.raises(RuntimeError, match="ksize = 33 "):
        dimg.detail_enhancing_blend(z, z.clone(), sigma=4)
    with pytest.raises(RuntimeError, match="d = 11 "):  # the narrow entry still refuses what it never built
        dimg.bilateral_u8(z, d=11)
    out = dimg.edge_preserving_smoothing(z)  # radius 90 on 8 x 8 zeros: zeros
    assert not out.any()


# ---- 7. the drop-in module ------------------------------------------------------------------------------------------------------------
def test_drop_in_from_files(tmp_path):
    from PIL import Image

    import improved_smooth as IS
    from mstg_hip import image as dimg
    img, orig = CR.blocks(40, 33, 5, cell=16), SR.image("noise", 50, 41, seed=6)  # the original of another size
    Image.fromarray(img).save(tmp_path / "in.png")
    Image.fromarray(orig).save(tmp_path / "orig.png")
    out = IS.fix_color_blocks_improved(str(tmp_path / "in.png"), str(tmp_path / "orig.png"), str(tmp_path / "sub" / "out.png"))
    assert isinstance(out, Image.Image)
    want = dimg.fix_color_blocks(_dev(img), _dev(orig)).cpu().numpy()
    _same(np.array(out), want, "fix_color_blocks_improved with an original")
    _same(np.array(Image.open(tmp_path / "sub" / "out.png")), want, "the saved file")
    plain = IS.fix_color_blocks_improved(str(tmp_path / "in.png"), str(tmp_path / "missing.png"))
    _same(np.array(plain), dimg.fix_color_blocks(_dev(img)).cpu().numpy(), "fix_color_blocks_improved without an original")
    # the four stage functions: the kind that goes in comes out
    m = IS.detect_color_blocks(img)
    assert m.dtype == bool and np.array_equal(m, CR.block_mask(img)) and np.array_equal(IS.detect_color_blocks(Image.fromarray(img)), m)
    c = IS.adaptive_color_correction(img, m)
    assert isinstance(c, np.ndarray) and np.array_equal(c, CR.correct(img, m))
    assert np.array_equal(np.array(IS.adaptive_color_correction(Image.fromarray(img))), c)
    s = IS.edge_preserving_smoothing(Image.fromarray(img), sigma_s=8)
    assert isinstance(s, Image.Image) and np.array_equal(np.array(s), CR.bilateral_wide(img[None], 0, 0.4 * 255, 8)[0])
    same = Image.fromarray(SR.image("gradient", 40, 33, seed=2))
    b = IS.detail_enhancing_blend(Image.fromarray(img), same)
    assert np.array_equal(np.array(b), CR.detail_blend(img, np.array(same), 0.3, 1.5))
    assert IS.detail_enhancing_blend(img, np.array(same)) is img  # as in the reference: only two PIL images are blended
