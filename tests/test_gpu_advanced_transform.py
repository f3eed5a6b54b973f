"""The advanced transform on the device (csrc/advanced_transform.hip through mstg_lab_u8, mstg_lab2rgb_u8, mstg_gaussian_sigma_u8,
mstg_hsv_gain_u8, mstg_kmeans_u8, mstg_region_blend_u8, mstg_fuse_scales_u8 and the three chains; mstg_hip.image.process_advanced)
against the numpy restatement of tests/advanced_transform_ref.py: bytes byte for byte, the K-means centres and compactness bit
for bit.  Every stage at (37, 53), (64, 64), (5, 3) and at (17, 65) with three images per launch (the shape crosses a 16 x 64 tile
in both directions); the chains against the composition of their stage functions; the launch counts; the refusals by name.  The
restatement has not been compared with an OpenCV binary (see its docstring)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import advanced_transform_ref as AR
import enhanced_local_style_ref as ER
from local_style_ref import gray_u8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SHAPES = [((37, 53), 1), ((64, 64), 1), ((5, 3), 1), ((17, 65), 3)]
CHAIN_SHAPES = [((64, 64), 1), ((40, 72), 1), ((64, 64), 3), ((40, 72), 3)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


@lru_cache(maxsize=None)
def _images(shape, n, seed=0):
    """n different images of one shape: a smooth field with a flat patch, pure noise, the smooth field of another seed"""
    h, w = shape
    a = np.stack([AR.smooth(h, w, 3 + h + seed), AR.noise(h, w, 7 + seed), AR.smooth(h, w, 11 + w + seed)][:n])
    a.setflags(write=False)
    return a


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}
    g, w = (got.view(bits[got.itemsize]), want.view(bits[got.itemsize])) if got.dtype.kind == "f" else (got, want)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} entries differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


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


# ---- the point-wise stages ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", SHAPES)
def test_lab_round_trip_and_gains(shape, n):
    from mstg_hip import image as dimg
    imgs = _images(shape, n)
    x = _dev(imgs)
    lab = dimg.lab_u8(x)
    _same(lab, AR.lab_u8(imgs), "lab_u8")
    _same(dimg.lab2rgb_u8(lab), AR.lab2rgb_u8(AR.lab_u8(imgs)), "lab2rgb_u8 of Lab")
    _same(dimg.lab2rgb_u8(x), AR.lab2rgb_u8(imgs), "lab2rgb_u8 of arbitrary bytes")
    for sg, vg in ((1.2, 1.0), (1.2, 1.1), (1.0, 1.0), (0.0, 2.5)):
        _same(dimg.hsv_gain_u8(x, sg, vg), np.stack([AR.hsv_gain_u8(i, sg, vg) for i in imgs]), f"hsv_gain_u8({sg}, {vg})")
    assert torch.equal(x.cpu(), torch.from_numpy(np.array(imgs)))  # the input is unchanged
    _same(dimg.lab_u8(x[0]), AR.lab_u8(imgs[0]), "lab_u8 of one image")


def test_lab2rgb_on_a_table_of_triples():
    from mstg_hip import image as dimg
    edge = [0, 1, 127, 128, 129, 254, 255]
    corners = np.array([[L, a, b] for L in edge for a in edge for b in edge], dtype=np.uint8)
    table = np.concatenate([corners, AR.noise(1, 681, 5)[0]]).reshape(32, 32, 3)
    _same(dimg.lab2rgb_u8(_dev(table)), AR.lab2rgb_u8(table), "lab2rgb_u8 on the corners of the cube")


def test_hsv_gain_with_clahe_put_back_is_hsv_enhance():
    from mstg_hip import image as dimg
    imgs = _images((64, 64), 3)
    x = _dev(imgs)
    _same(dimg.hsv_enhance_u8(x), np.stack([ER.hsv_enhance(i) for i in imgs]), "hsv_enhance_u8")
    # the gain alone leaves v as it is: the kernel's HSV -> RGB of (h, s * 1.2, v)
    h, s, v = AR.hsv_u8(imgs)
    _same(dimg.hsv_gain_u8(x, 1.2, 1.0), np.ascontiguousarray(ER.hsv2rgb_u8(h, ER.sat_scale(s), v)), "hsv_gain_u8 against sat_scale")


# ---- the Gaussian -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", SHAPES + [((1, 7), 2), ((7, 1), 1), ((1, 1), 1)])
def test_gaussian_sigma(shape, n):
    from mstg_hip import image as dimg
    planes = np.ascontiguousarray(_images(shape, n)[..., 1])
    x = _dev(planes)
    for sigma in (3.0, 1.0, 5.0):
        _same(dimg.gaussian_sigma_u8(x, sigma), np.stack([AR.gaussian_sigma_u8(p, sigma) for p in planes]), f"gaussian_sigma_u8({sigma})")
    flat = torch.full((n,) + shape, 201, dtype=torch.uint8, device=DEV)
    assert int(dimg.gaussian_sigma_u8(flat, 3.0).min()) == 201 and int(dimg.gaussian_sigma_u8(flat[0], 3.0).max()) == 201


# ---- K-means ------------------------------------------------------------------------------------------------------------------------
def _km_same(got, want, what):
    labels, cen, comp, best = got
    _same(labels, want[0], what + ": labels")
    _same(cen, want[1], what + ": centres")
    assert float(comp) == want[2] and int(best) == want[3], (what, float(comp), want[2], int(best), want[3])


@lru_cache(maxsize=None)
def _km_ref(seed_img, K, attempts, seed):
    return AR.kmeans_u8(_images((37, 53), 3)[seed_img], K=K, attempts=attempts, seed=seed)


def test_kmeans_solo_batch_and_winner():
    from mstg_hip import image as dimg
    imgs = _images((37, 53), 3)
    x = _dev(imgs)
    batch = dimg.kmeans_u8(x, seed=0, return_attempt=True)
    assert batch[0].dtype == torch.int32 and batch[1].dtype == torch.float32 and batch[2].dtype == torch.float64
    for i in range(3):
        want = _km_ref(i, 5, 10, 0)
        _km_same(tuple(t[i] for t in batch), want, f"kmeans_u8 image {i} of the batch")
        solo = dimg.kmeans_u8(x[i], seed=0, return_attempt=True)
        _km_same(solo, want, f"kmeans_u8 image {i} alone")
        # the winning attempt alone, from its initial centres
        px = imgs[i].reshape(-1, 3)
        lo, hi = px.min(axis=0).astype(F32), px.max(axis=0).astype(F32)
        start = lo + AR.uniforms(0, 10, 5)[want[3]] * (hi - lo)
        one = dimg.kmeans_u8(x[i], attempts=1, centers0=_dev(start), return_attempt=True)
        _km_same(one, want[:3] + (0,), f"kmeans_u8 image {i}, the winner's centres as centers0")
    again = dimg.kmeans_u8(x, seed=0, return_attempt=True)
    assert all(torch.equal(a, b) for a, b in zip(batch, again))  # reproducible
    other = dimg.kmeans_u8(x[0], K=7, attempts=3, iters=4, eps=0.0, seed=5, return_attempt=True)
    _km_same(other, AR.kmeans_u8(imgs[0], K=7, attempts=3, iters=4, eps=0.0, seed=5), "kmeans_u8 K = 7, 3 attempts, 4 iterations")
    assert _launches(lambda: dimg.kmeans_u8(x, seed=0)) == 26 == _launches(lambda: dimg.kmeans_u8(x[0], seed=0))


def test_kmeans_edge_cases():
    from mstg_hip import image as dimg
    img = _images((37, 53), 1)[0]
    x = _dev(img)
    _km_same(dimg.kmeans_u8(x, K=1, attempts=2, return_attempt=True), AR.kmeans_u8(img, K=1, attempts=2), "K = 1")
    flat = np.full((37, 53, 3), 93, dtype=np.uint8)  # lo == hi: K - 1 empty clusters
    got = dimg.kmeans_u8(_dev(flat), K=5, attempts=3, return_attempt=True)
    _km_same(got, AR.kmeans_u8(flat, K=5, attempts=3), "one colour")
    assert not got[0].any() and float(got[2]) == 0.0 and torch.equal(got[1].cpu(), torch.full((5, 3), 93.0))
    yy, xx = np.mgrid[0:37, 0:53]
    two = np.ascontiguousarray(np.repeat(np.where((yy + xx) % 3 == 0, 10, 200).astype(np.uint8)[..., None], 3, axis=2))
    want = AR.kmeans_u8(two, K=5, attempts=10, seed=2)
    got = dimg.kmeans_u8(_dev(two), K=5, attempts=10, seed=2, return_attempt=True)
    _km_same(got, want, "two colours, K = 5")
    assert len(np.unique(want[0])) == 2  # three clusters stay empty and keep their centres
    # an exact distance tie: (10, 10, 10) lies 10 from centre 0 and from centre 1; centres 2 and 3 coincide
    c0 = np.array([[0, 10, 10], [20, 10, 10], [200, 190, 200], [200, 190, 200], [90, 90, 90]], dtype=F32)
    want = AR.kmeans_u8(two, K=5, attempts=1, iters=1, centers0=c0)
    got = dimg.kmeans_u8(_dev(two), K=5, attempts=1, iters=1, centers0=_dev(c0), return_attempt=True)
    _km_same(got, want, "an exact tie")
    first = AR.km_assign(two.reshape(-1, 3), c0)
    assert set(np.unique(first)) == {0, 2}  # the lowest index won both ties


# ---- region blend and fusion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", SHAPES)
def test_region_blend_and_fusion(shape, n):
    from mstg_hip import image as dimg
    styled, orig = _images(shape, n), _images(shape, n, seed=1)
    h, w = shape
    labels = np.random.RandomState(h).randint(-1, 7, size=(n, h, w)).astype(np.int32)
    got = dimg.region_blend_u8(_dev(styled), _dev(orig), _dev(labels))
    _same(got, AR.region_blend_u8(styled, orig, labels), "region_blend_u8")
    got = dimg.region_blend_u8(_dev(styled), _dev(orig), _dev(labels), ratios=(0.25, 1.0, 0.0, 0.7, 0.1, 0.33, 0.9))
    _same(got, AR.region_blend_u8(styled, orig, labels, (0.25, 1.0, 0.0, 0.7, 0.1, 0.33, 0.9)), "region_blend_u8, seven ratios")
    third = _images(shape, n, seed=2)
    stack = np.stack([styled, orig, third])
    _same(dimg.fuse_scales_u8(_dev(stack)), AR.fuse_scales_u8(stack), "fuse_scales_u8")
    _same(dimg.fuse_scales_u8(_dev(stack[:2]), (0.9, 0.6), 0.8), AR.fuse_scales_u8(stack[:2], (0.9, 0.6), 0.8), "fuse_scales_u8, two scales")
    _same(dimg.fuse_scales_u8(_dev(stack[:, 0])), AR.fuse_scales_u8(stack[:, 0]), "fuse_scales_u8 of single images")


# ---- the chains ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", CHAIN_SHAPES)
def test_chains_equal_their_stages(shape, n):
    from mstg_hip import image as dimg
    styled_np, orig_np = _images(shape, n), _images(shape, n, seed=1)
    styled, orig = _dev(styled_np), _dev(orig_np)
    # contrast
    lab = dimg.lab_u8(styled)
    lab[..., 0] = dimg.clahe_u8(lab[..., 0].contiguous())
    want = dimg.hsv_gain_u8(dimg.lab2rgb_u8(lab), 1.2, 1.0)
    got = dimg.contrast_enhanced_finish(styled)
    assert torch.equal(got, want)
    _same(got[0], AR.contrast_enhanced_finish(styled_np[0]), "contrast_enhanced_finish against the restatement")
    # detail
    grey = _dev(np.stack([gray_u8(o).astype(np.uint8) for o in orig_np]))
    detail = grey - dimg.gaussian_sigma_u8(grey, 3.0)  # uint8: wraps
    lab = dimg.lab_u8(styled)
    lab[..., 0] = torch.clamp(lab[..., 0].float() + detail.float() * 0.5, 0, 255).to(torch.uint8)
    want = dimg.hsv_gain_u8(dimg.lab2rgb_u8(lab), 1.2, 1.1)
    got = dimg.detail_enhanced_finish(styled, orig)
    assert torch.equal(got, want)
    _same(got[n - 1], AR.detail_enhanced_finish(styled_np[n - 1], orig_np[n - 1]), "detail_enhanced_finish against the restatement")
    # regions
    labels = dimg.kmeans_u8(orig, seed=3)[0]
    want = dimg.hsv_gain_u8(dimg.region_blend_u8(styled, orig, labels), 1.2, 1.0)
    got = dimg.local_regions_finish(styled, orig, seed=3)
    assert torch.equal(got, want)
    _same(got[0], AR.local_regions_finish(styled_np[0], orig_np[0], seed=3), "local_regions_finish against the restatement")
    assert _launches(lambda: dimg.contrast_enhanced_finish(styled)) == 2 == _launches(lambda: dimg.detail_enhanced_finish(styled, orig))
    assert _launches(lambda: dimg.local_regions_finish(styled, orig, seed=3)) == 27


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value():
    from mstg_hip import image as dimg
    x = _dev(_images((37, 53), 1))
    with pytest.raises(RuntimeError, match="H = 37, W = 53.*multiples of 8"):
        dimg.contrast_enhanced_finish(x)
    with pytest.raises(RuntimeError, match="ksize = 33"):
        dimg.gaussian_sigma_u8(x[..., 0].contiguous(), 5.2)
    for kw, name in (({"K": 0}, "K = 0"), ({"K": 17}, "K = 17"), ({"attempts": 0}, "attempts = 0"), ({"attempts": 17}, "attempts = 17"),
                     ({"iters": 0}, "iters = 0")):
        with pytest.raises(RuntimeError, match=name):
            dimg.kmeans_u8(x, **kw)
    with pytest.raises(RuntimeError, match="centers0"):
        dimg.kmeans_u8(x, K=2, attempts=2, centers0=torch.zeros((2, 3)))
    with pytest.raises(RuntimeError, match="S = 9"):
        dimg.fuse_scales_u8(x.expand(9, 37, 53, 3), [0.1] * 9)
    with pytest.raises(RuntimeError, match="count = 17"):
        dimg.region_blend_u8(x, x, torch.zeros((1, 37, 53), dtype=torch.int32, device=DEV), [0.5] * 17)
    with pytest.raises(RuntimeError, match="s_gain = -0.5"):
        dimg.hsv_gain_u8(x, -0.5)
    from mstg_hip import _lib
    lib = _lib.load()
    p = x.data_ptr()
    assert lib.mstg_hsv_gain_u8(p, 1, 37, 53, 1.2, 1.0, p + 3, None) == -1 and b"overlaps" in lib.mstg_last_error()


# ---- the caller ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import enhanced_generator as eg
    torch.manual_seed(11)
    g = eg.EnhancedGenerator(16, 1).to(DEV)
    g.eval()
    return g


@pytest.mark.parametrize("size", [(90, 60), (64, 64)])  # (height, width)
def test_process_advanced_equals_the_stages(model, size):
    from mstg_hip import image as dimg
    h, w = size
    img = _dev(AR.smooth(h, w, h + w))

    def forward(inputs):
        with torch.no_grad():
            return [dimg.to_u8(t) for t in model(torch.stack([dimg.to_tensor(i) for i in inputs]))]
    styled = forward([dimg.resize_u8(img, (256, 256), dimg.BILINEAR)])[0]
    orig = dimg.resize_u8(img, (256, 256), dimg.LANCZOS)
    assert torch.equal(dimg.process_advanced(model, img, "standard"), styled)
    lab = dimg.lab_u8(styled)
    lab[..., 0] = dimg.clahe_u8(lab[..., 0].contiguous())
    assert torch.equal(dimg.process_advanced(model, img, "contrast"), dimg.hsv_gain_u8(dimg.lab2rgb_u8(lab), 1.2, 1.0))
    grey = _dev(gray_u8(orig.cpu().numpy()).astype(np.uint8))
    detail = grey - dimg.gaussian_sigma_u8(grey, 3.0)
    lab = dimg.lab_u8(styled)
    lab[..., 0] = torch.clamp(lab[..., 0].float() + detail.float() * 0.5, 0, 255).to(torch.uint8)
    assert torch.equal(dimg.process_advanced(model, img, "detail"), dimg.hsv_gain_u8(dimg.lab2rgb_u8(lab), 1.2, 1.1))
    labels = dimg.kmeans_u8(orig, seed=4)[0]
    want = dimg.hsv_gain_u8(dimg.region_blend_u8(styled, orig, labels), 1.2, 1.0)
    assert torch.equal(dimg.process_advanced(model, img, "regions", seed=4), want)
    scaled = [dimg.resize_u8(dimg.resize_u8(img, (int(w * s), int(h * s)), dimg.LANCZOS), (256, 256), dimg.BILINEAR) for s in (0.5, 0.75, 1.0)]
    singles = [forward([s])[0] for s in scaled]
    got = dimg.process_advanced(model, img, "multi_scale")
    assert got.shape == (256, 256, 3) and got.dtype == torch.uint8
    assert torch.equal(got, dimg.fuse_scales_u8(torch.stack(singles)))
    # The three inputs run singly: one forward pass of the batch of three does not give the bytes of three single passes (the
    # counts are printed below), so process_advanced does what the reference does.
    batch = forward(scaled)
    print(f"multi_scale {size}: bytes of a batch-of-three forward that differ from single forwards: "
          f"{[int((a != b).sum()) for a, b in zip(batch, singles)]} of {singles[0].numel()}")
