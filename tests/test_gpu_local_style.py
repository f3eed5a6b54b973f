"""The 'enhanced' local-style weight map built on the device (csrc/local_style.hip, mstg_hip.image.enhanced_weight_map and the
``weight_map=None`` path of process_local_style / process_local_style_batch) against the numpy / scipy restatement of
tests/local_style_ref.py, byte for byte: the colour stage over all 2^24 colours, the state map before hysteresis, the hysteresis
alone on crafted maps (long spiral paths included), the 70 % sky rule at its threshold, the float64 map and the detail mask, and
the two callers end to end.  The restatement has not been compared with an OpenCV binary (see its docstring)."""
import numpy as np
import pytest
import torch

import local_style_ref as LR
from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _prepare(canvases, gray=True):
    """mstg_local_style_prepare on an (N, H, W, 3) uint8 array -> (state, sky, count, gray) as numpy; the count starts at -1: the
    entry point zeroes it"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    c = _dev(canvases)
    N, H, W = c.shape[:3]
    state, sky, g = (torch.full((N, H, W), 9, dtype=torch.uint8, device=DEV) for _ in range(3))
    count = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mstg_local_style_prepare(_p(c), N, H, W, _p(state), _p(sky), _p(count), _p(g) if gray else None, _stream()),
               "mstg_local_style_prepare")
    torch.cuda.synchronize()
    return state.cpu().numpy(), sky.cpu().numpy(), count.cpu().numpy(), g.cpu().numpy()


def _hysteresis(states):
    """mstg_local_style_hysteresis on an (N, H, W) uint8 array -> edge mask; 64 guard bytes behind the output must survive"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    s = _dev(states)
    N, H, W = s.shape
    buf = torch.full((N * H * W + 64,), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mstg_local_style_hysteresis(_p(s), N, H, W, _p(buf), _stream()), "mstg_local_style_hysteresis")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[N * H * W:] == 7).all(), "the kernel wrote behind its output"
    assert torch.equal(s, _dev(states)), "the kernel changed its input"
    return out[:N * H * W].reshape(N, H, W)


# ---- 1. colour stage, exhaustive ------------------------------------------------------------------------------------------------
def test_all_colours_gray_and_sky():
    idx = np.arange(1 << 24, dtype=np.uint32)
    canvas = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    _, sky, count, gray = _prepare(canvas)
    assert np.array_equal(gray[0], LR.gray_u8(canvas[0]))
    ref_sky = LR.sky_mask(canvas[0])
    assert np.array_equal(sky[0].astype(bool), ref_sky) and set(np.unique(sky).tolist()) == {0, 1}
    assert int(count[0]) == int(sky.sum()) == int(ref_sky.sum())


# ---- 2. the state map before hysteresis -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(67, 93), (96, 80), (256, 256)])
@pytest.mark.parametrize("kind", ["noise", "blocky", "gradient_rects"])
def test_state_map(kind, shape):
    gen = getattr(LR, kind)
    canvases = np.stack([gen(shape[0], shape[1], 11 + 5 * i) for i in range(3)])
    state, sky, count, gray = _prepare(canvases)
    state2 = _prepare(canvases, gray=False)[0]  # the gray plane is optional
    for i in range(3):
        ref_gray = LR.gray_u8(canvases[i])
        ref = LR.state_map(ref_gray)
        assert np.array_equal(gray[i], ref_gray), i
        bad = np.argwhere(state[i] != ref)
        assert len(bad) == 0, f"image {i}: {len(bad)} of {ref.size} states differ, first at {bad[0].tolist()}"
        assert np.array_equal(sky[i].astype(bool), LR.sky_mask(canvases[i])) and int(count[i]) == int(sky[i].sum()), i
        if kind != "gradient_rects":
            assert (ref == 0).any() and (ref == 2).any()  # the case exercises candidates and seeds
    assert np.array_equal(state, state2)


# ---- 3. hysteresis alone ----------------------------------------------------------------------------------------------------------
def _crafted(pair, h, w):
    if pair == "spirals":
        return [LR.spiral_state(h, w), LR.spiral_state(h, w, strong=False)]
    if pair == "serpentine_diagonal":
        return [LR.serpentine_state(h, w), LR.diagonal_state(h, w)]
    return [LR.candidates_only_state(h, w, 3), LR.random_state(h, w, 4)]


@pytest.mark.parametrize("shape", [(48, 64), (65, 130), (384, 384)])
@pytest.mark.parametrize("pair", ["spirals", "serpentine_diagonal", "candidates_random"])
def test_hysteresis_crafted_maps(pair, shape):
    maps = _crafted(pair, *shape)
    for order in (maps, maps[::-1]):  # different maps per image, both ways round: nothing leaks from one image's LDS to the next
        states = np.stack(order)
        edge = _hysteresis(states)
        for i in range(2):
            ref = LR.hysteresis(states[i])
            assert set(np.unique(edge[i]).tolist()) <= {0, 1}
            bad = np.argwhere(edge[i].astype(bool) != ref)
            assert len(bad) == 0, f"{pair} image {i}: {len(bad)} pixels differ ({int(ref.sum())} edge pixels expected), first {bad[0].tolist()}"
    if pair == "spirals":
        assert _hysteresis(np.stack(maps))[0].sum() == (maps[0] != 1).sum() and not LR.hysteresis(maps[1]).any()


def test_hysteresis_size_limit():
    from mstg_hip import image as dimg
    _hysteresis(np.ones((1, 1, 147456), dtype=np.uint8))  # exactly the limit, one row
    assert _hysteresis(np.array([[[0, 2, 0]]], dtype=np.uint8)).tolist() == [[[1, 1, 1]]]
    assert _hysteresis(np.array([[[0], [1], [2], [0]]], dtype=np.uint8)).reshape(-1).tolist() == [0, 0, 1, 1]
    with pytest.raises(RuntimeError, match="385 x 384"):
        dimg.enhanced_weight_map(torch.zeros(385, 384, 3, dtype=torch.uint8, device=DEV))


# ---- 4. the 70 % rule at its threshold --------------------------------------------------------------------------------------------
def test_sky_threshold():
    from mstg_hip import image as dimg
    counts = [6999, 7000, 7001]
    canvases = np.stack([LR.sky_threshold_canvas(100, 100, k, 5) for k in counts])
    wm, sky, edge, det, has_sky = dimg.enhanced_weight_map(_dev(canvases), strength=0.8, detail=0.7, return_masks=True)
    assert has_sky.cpu().tolist() == [False, False, True]  # 7000 / 10000 > 0.7 is false
    wm = wm.cpu().numpy()
    for i, k in enumerate(counts):
        ref = LR.enhanced_weight_map(canvases[i], 0.8, 0.7)
        assert int(sky[i].sum()) == k and not bool(edge[i].any()) and not bool(det[i].any())
        assert np.array_equal(wm[i], ref["weight"])
        assert bool((wm[i] == 1.0).any()) == (k == 7001)  # w_sky = min(0.8 + 0.2, 1.0) only where has_sky
    assert int((wm[2] == 1.0).sum()) == 7001 and (wm[:2] == 0.8).all()


# ---- 5. the full map ----------------------------------------------------------------------------------------------------------------
def _full_inputs(shape):
    h, w = shape
    if shape == (256, 256):
        return np.stack([LR.landscape(h, w, 21), LR.bright_low_saturation(h, w, 22), LR.noise(h, w, 23)])
    return np.stack([LR.blocky(h, w, 24), LR.gradient_rects(h, w, 25)])


@pytest.fixture(scope="module")
def full_refs():
    """masks of the restatement per shape (they do not depend on the weights), with the precondition of the exact comparison:
    no value of the reference's Gaussian lies within 1e-9 of the 0.1 threshold on these inputs"""
    out = {}
    for shape in ((256, 256), (96, 80)):
        canvases = _full_inputs(shape)
        refs = [LR.enhanced_weight_map(c) for c in canvases]
        for i, r in enumerate(refs):
            assert np.abs(r["gauss"] - 0.1).min() > 1e-9, (shape, i)
        out[shape] = (canvases, refs)
    assert out[(256, 256)][1][1]["has_sky"] and not out[(256, 256)][1][0]["has_sky"]
    return out


@pytest.mark.parametrize("shape", [(256, 256), (96, 80)])
@pytest.mark.parametrize("coeff", [0.3, 0.4])
@pytest.mark.parametrize("strength,detail", [(0.8, 0.7), (0.65, 1.0), (0.1, 0.7)])
def test_full_map(full_refs, strength, detail, coeff, shape):
    from mstg_hip import image as dimg
    canvases, refs = full_refs[shape]
    c = _dev(canvases)
    wm, sky, edge, det, has_sky = dimg.enhanced_weight_map(c, strength, detail, coeff, return_masks=True)
    one_call = dimg.enhanced_weight_map(c, strength, detail, coeff)  # the three stages on one workspace
    assert wm.dtype == torch.float64 and torch.equal(wm, one_call)
    if (strength, detail) == (0.1, 0.7):
        assert LR.weights(strength, detail, coeff)[2] == 0.0  # w_detail clamps
    for i, r in enumerate(refs):
        want = LR.enhanced_weight_map(canvases[i], strength, detail, coeff)
        assert np.array_equal(want["detail"], r["detail"])
        assert np.array_equal(sky[i].cpu().numpy(), r["sky"]) and bool(has_sky[i]) == r["has_sky"], i
        assert np.array_equal(edge[i].cpu().numpy(), r["edge"]), i
        assert np.array_equal(det[i].cpu().numpy(), r["detail"]), i
        got = wm[i].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want["weight"].view(np.uint64)), f"image {i}: {int((got != want['weight']).sum())} weights differ"
    single = dimg.enhanced_weight_map(c[0], strength, detail, coeff)
    assert single.shape == shape and torch.equal(single, wm[0])


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
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


def _ref_canvas(img, resize, target=256):
    """the letterboxed canvas of process_local_style (batch_process_images.py:183-199), as oracle/image_ref.py builds it"""
    height, width = img.shape[:2]
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    canvas = np.full((target, target, 3), 255, dtype=np.uint8)
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    canvas[off_y:off_y + new_height, off_x:off_x + new_width] = resize(img, (new_width, new_height), IR.LANCZOS)
    return canvas


MIXED = [(300, 420), (420, 300), (256, 256), (97, 301), (64, 48)]


@pytest.fixture(scope="module")
def mixed():
    arrays = [_img(h, w, 50 + i) for i, (h, w) in enumerate(MIXED)]
    return arrays, [_dev(a) for a in arrays]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("strength,detail,coeff", [(0.8, 0.7, 0.3), (0.65, 1.0, 0.4)])
def test_process_local_style_builds_the_map(mixed, k, strength, detail, coeff):
    from mstg_hip import image as dimg
    rz = _pil_or_numpy()
    arr, dev = mixed[0][k], mixed[1][k]
    out = dimg.process_local_style(stub, dev, mode="weight_map", weight_map=None, strength=strength, detail=detail, detail_coeff=coeff)
    ref_map = LR.enhanced_weight_map(_ref_canvas(arr, rz), strength, detail, coeff)
    assert np.abs(ref_map["gauss"] - 0.1).min() > 1e-9 and ref_map["detail"].any() and not ref_map["detail"].all()
    ref = IR.process_local_style_ref(stub_np, arr, mode="weight_map", strength=strength, weight_map=ref_map["weight"], resize=rz)
    out = out.cpu().numpy()
    assert out.shape == ref.shape and np.array_equal(out, ref), f"{int((out != ref).sum())} of {ref.size} bytes differ"


def test_batch_equals_the_one_image_function(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    loop = [dimg.process_local_style(stub, im, mode="weight_map") for im in images]
    calls = []

    def model(x):
        calls.append(x.shape[0])
        return stub(x)
    for bs, want_calls in ((1, [1] * 5), (2, [2, 2, 1]), (5, [5])):
        del calls[:]
        outs = dimg.process_local_style_batch(model, images, mode="weight_map", batch_size=bs)
        assert calls == want_calls
        for i, (a, b) in enumerate(zip(loop, outs)):
            assert a.shape == b.shape and torch.equal(a, b), f"batch_size {bs} image {i}: {int((a != b).sum())} of {a.numel()} bytes differ"


def test_explicit_maps_and_other_modes_are_unchanged(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    rs = np.random.RandomState(9)
    maps = [rs.rand(256, 256) for _ in arrays]
    rz = _pil_or_numpy()
    outs = dimg.process_local_style_batch(stub, images, mode="weight_map", weight_maps=maps)
    for i, a in enumerate(arrays):
        ref = IR.process_local_style_ref(stub_np, a, mode="weight_map", weight_map=maps[i], resize=rz)
        assert np.array_equal(outs[i].cpu().numpy(), ref), i
        one = dimg.process_local_style(stub, images[i], mode="weight_map", weight_map=maps[i])
        assert np.array_equal(one.cpu().numpy(), ref), i
    styled = dimg.process_local_style_batch(stub, images, mode="advanced", detail=0.2, detail_coeff=0.4)  # other names: the styled image
    for i, a in enumerate(arrays):
        assert np.array_equal(styled[i].cpu().numpy(), IR.process_local_style_ref(stub_np, a, mode="advanced", resize=rz)), i
    with pytest.raises(RuntimeError, match="one weight map per image"):
        dimg.process_local_style_batch(stub, images, mode="weight_map", weight_maps=maps[:2])


def test_three_launches_whatever_n(mixed):
    from mstg_hip import _lib, image as dimg
    lib = _lib.load()
    canvases = _dev(np.stack([LR.landscape(256, 256, i) for i in range(64)]))

    def launches(fn):
        torch.cuda.synchronize()
        lib.mstg_prof_enable(1)
        try:
            fn()
            torch.cuda.synchronize()
            return lib.mstg_prof_count()
        finally:
            lib.mstg_prof_enable(0)
    for n in (1, 2, 17, 64):
        assert launches(lambda: dimg.enhanced_weight_map(canvases[:n])) == 3, n
    images = mixed[1]
    simple = launches(lambda: dimg.process_local_style_batch(stub, images[:3], mode="simple"))
    for imgs in (images[:1], images[:3], (images + images + images)[:12]):
        assert launches(lambda: dimg.process_local_style_batch(stub, imgs, mode="weight_map")) == simple + 3 <= 9


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------------------
def test_reproducible(full_refs):
    from mstg_hip import image as dimg
    c = _dev(full_refs[(256, 256)][0])
    a = dimg.enhanced_weight_map(c, return_masks=True)
    b = dimg.enhanced_weight_map(c, return_masks=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(dimg.enhanced_weight_map(c), a[0])
