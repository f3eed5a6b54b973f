"""The application's local-style and compare tabs on the device (csrc/app_local_style.hip through mstg_app_sky_mask,
mstg_app_edge_weight, mstg_app_chain and mstg_app_local_style_finish; mstg_hip.image.app_sky_mask, app_edge_weight,
app_local_style_finish, process_app_local_style(_batch) and process_compare(_batch)) against the numpy restatement of
tests/app_local_style_ref.py: bytes byte for byte, the float64 edge weight bit for bit.  Shapes below both filter radii (the mirror
repeats), ragged tiles, tile seams with a batch offset and one 256 x 256; canvases with sky and edge pixels, one without sky, and a
styled image that equals the canvas on half of its area; the point-wise kernel over every flag combination; the chain against the
composed stage functions and against the restatement over the modes, both directions, two strengths and every option off in turn;
launch counts; the callers end to end with stub models; refusals by name.  The restatement has not been compared with an OpenCV
binary (see its docstring)."""
import itertools
from functools import lru_cache

import numpy as np
import pytest
import torch

import app_local_style_ref as AR
import local_style_ref as LR
from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 9), (5, 3), (37, 70), (64, 130), (256, 256)]
TRIPLES = (("noise", "landscape", "blocky"), ("gradient_rects", "bright_low_saturation", "landscape"))
CHAIN_SHAPE = (37, 70)
MODEL_TYPES = ("photo_to_monet", "monet_to_photo")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def _canvases(shape, which):
    """three different canvases of one shape, (3, H, W, 3)"""
    h, w = shape
    return _ro(np.stack([getattr(LR, kind)(h, w, 7 * which + i + 1) for i, kind in enumerate(TRIPLES[which])]))


@lru_cache(maxsize=None)
def _styled(shape, which):
    """noise on the left half, the canvas itself on the right half"""
    return _ro(np.stack([AR.half_equal(c, 50 + i) for i, c in enumerate(_canvases(shape, which))]))


@lru_cache(maxsize=None)
def _ref_sky(shape, which):
    return _ro(np.stack([AR.sky_mask(c) for c in _canvases(shape, which)]))


@lru_cache(maxsize=None)
def _ref_edge(shape, which, detail=0.6):
    return _ro(np.stack([AR.edge_weight(c, detail) for c in _canvases(shape, which)]))


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} values differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def _which(shape):
    return (0,) if shape == (256, 256) else (0, 1)  # one launch at the large size


# ---- 1. the stages --------------------------------------------------------------------------------------------------------------------
def test_inputs_give_every_stage_work():
    c = _canvases((64, 130), 0)
    assert all(AR.blue_mask(x).sum() > 50 for x in c) and all(AR.edge_mask(x).sum() > 50 for x in c)
    assert AR.blue_mask(LR.bright_low_saturation(64, 64, 1)).sum() == 0  # the empty-mask case
    m = _ref_sky((64, 130), 0)
    assert ((m > 0) & (m < 255)).any() and (m == 255).any() and (m == 0).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_sky_mask(shape):
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    for which in _which(shape):
        x = _dev(_canvases(shape, which))
        n = x.shape[0] * shape[0] * shape[1]
        buf = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)  # guard bytes behind the output
        _lib.check(_lib.load().mstg_app_sky_mask(_p(x), 3, shape[0], shape[1], _p(buf), _stream()), "mstg_app_sky_mask")
        out = buf.cpu().numpy()
        assert (out[n:] == 7).all() and torch.equal(x, _dev(_canvases(shape, which)))
        _same(out[:n].reshape(3, *shape), _ref_sky(shape, which), f"sky mask {shape} {TRIPLES[which]}")
    one = dimg.app_sky_mask(_dev(_canvases(shape, 0)[1]))  # the Python entry on one image: no batch offset
    _same(one.cpu().numpy(), _ref_sky(shape, 0)[1], f"sky mask {shape}, one image")


@pytest.mark.parametrize("shape", SHAPES)
def test_edge_weight_bit_for_bit(shape):
    from mstg_hip import image as dimg
    for which in _which(shape):
        got = dimg.app_edge_weight(_dev(_canvases(shape, which)), 0.6)
        assert got.dtype == torch.float64
        _same(got.cpu().numpy().view(np.int64), _ref_edge(shape, which).view(np.int64), f"edge weight {shape} {TRIPLES[which]}")
    one = dimg.app_edge_weight(_dev(_canvases(shape, 0)[2]), 0.35)
    _same(one.cpu().numpy().view(np.int64), AR.edge_weight(_canvases(shape, 0)[2], 0.35).view(np.int64), f"edge weight {shape}, one image")


def _chain(canvas, styled, sky, edge, use_strength, w_styled, w_canvas, lut):
    """mstg_app_chain on device tensors; 64 guard bytes behind ``out`` must survive"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    N, H, W = styled.shape[:3]
    nb = N * H * W * 3
    buf = torch.full((nb + 64,), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mstg_app_chain(_p(canvas), _p(styled), N, H, W, _p(sky), _p(edge), int(use_strength), w_styled, w_canvas, _p(lut),
                                          _p(buf), _stream()), "mstg_app_chain")
    assert (buf[nb:] == 7).all(), "mstg_app_chain wrote behind its output"
    return buf[:nb].view(N, H, W, 3)


@pytest.mark.parametrize("shape", [CHAIN_SHAPE, (5, 3)])  # 5 x 3 x 3 images = 45 pixels: the tail of the four-pixel items
def test_chain_every_flag_combination(shape):
    from mstg_hip import image as dimg
    canvas, styled = _canvases(shape, 0), _styled(shape, 0)
    m, a = _ref_sky(shape, 0), _ref_edge(shape, 0)
    c, s, md, ad = _dev(canvas), _dev(styled), _dev(m), _dev(a)
    bf = 0.1 / 0.3
    for sky, edge, strength, colour in itertools.product((False, True), (False, True), (False, True), (None,) + MODEL_TYPES):
        lut = dimg._color_lut(colour, torch.device(DEV)) if colour else None
        got = _chain(c, s, md if sky else None, ad if edge else None, strength, bf, 1 - bf, lut).cpu().numpy()
        for i in range(3):
            x = styled[i]
            if sky:
                x = AR.blend(x, canvas[i], m[i].astype(float) / 255.0)
            if edge:
                x = AR.blend(x, canvas[i], a[i])
            if strength:
                x = AR.strength_blend(x, canvas[i], 0.1)
            if colour:
                x = AR.apply_color(x, colour)
            _same(got[i], x, f"chain sky={sky} edge={edge} strength={strength} colour={colour} image {i}")
    assert torch.equal(c, _dev(canvas)) and torch.equal(s, _dev(styled)), "the chain changed an input"
    odd = _chain(c.view(-1)[3:].view(1, -1, 1, 3), s.view(-1)[3:].view(1, -1, 1, 3), None, None, True, bf, 1 - bf, None)  # unaligned pointers
    want = torch.stack([torch.from_numpy(AR.strength_blend(x, y, 0.1)) for x, y in zip(styled, canvas)]).view(-1)[3:]
    assert torch.equal(odd.cpu().view(-1), want)


# ---- 2. the chain entry ---------------------------------------------------------------------------------------------------------------
def _composed(canvas, styled, model_type, strength, detail, auto_select, ignore_sky, enhance_colors, smooth_transitions):
    """the 'enhanced' mode from the stage functions, one after the other"""
    from mstg_hip import image as dimg
    sky = dimg.app_sky_mask(canvas) if ignore_sky and model_type == "photo_to_monet" else None
    edge = dimg.app_edge_weight(canvas, detail) if auto_select else None
    low = strength < 0.3
    bf = strength / 0.3 if low else 1.0
    x = _chain(canvas, styled, sky, edge, low, bf, 1 - bf, dimg._color_lut(model_type, canvas.device) if enhance_colors else None)
    return dimg.bilateral_u8(x, 9, 75, 75) if smooth_transitions else x


OPTION_SETS = [dict(), dict(strength=0.1), dict(ignore_sky=False), dict(auto_select=False), dict(enhance_colors=False),
               dict(smooth_transitions=False), dict(auto_select=False, ignore_sky=False, enhance_colors=False, smooth_transitions=False),
               dict(auto_select=False, ignore_sky=False, enhance_colors=False), dict(detail=0.9, strength=0.29)]


@pytest.mark.parametrize("model_type", MODEL_TYPES)
def test_finish_equals_the_composed_stages(model_type):
    from mstg_hip import image as dimg
    for which in (0, 1):
        c, s = _dev(_canvases(CHAIN_SHAPE, which)), _dev(_styled(CHAIN_SHAPE, which))
        for opts in OPTION_SETS:
            kw = dict(strength=0.5, detail=0.6, auto_select=True, ignore_sky=True, enhance_colors=True, smooth_transitions=True)
            kw.update(opts)
            got = dimg.app_local_style_finish(c, s, model_type, "enhanced", **kw)
            want = _composed(c, s, model_type, **kw)
            assert torch.equal(got, want), f"{model_type} {opts}: {int((got != want).sum())} of {got.numel()} bytes differ"
        assert torch.equal(c, _dev(_canvases(CHAIN_SHAPE, which))) and torch.equal(s, _dev(_styled(CHAIN_SHAPE, which)))


CASES = [(mode, mt, st, {}) for mode in AR.MODES for mt in MODEL_TYPES for st in (0.1, 0.5)]
CASES += [("enhanced", mt, 0.5, {flag: False}) for mt in MODEL_TYPES
          for flag in ("ignore_sky", "auto_select", "enhance_colors", "smooth_transitions")]
CASES += [("something else", "photo_to_monet", 0.5, {})]


@pytest.mark.parametrize("mode,model_type,strength,opts", CASES)
def test_finish_against_the_restatement(mode, model_type, strength, opts):
    from mstg_hip import image as dimg
    which = 0 if model_type == "photo_to_monet" else 1
    canvas, styled = _canvases(CHAIN_SHAPE, which), _styled(CHAIN_SHAPE, which)
    got = dimg.app_local_style_finish(_dev(canvas), _dev(styled), model_type, mode, strength, **opts).cpu().numpy()
    for i in range(3):
        _same(got[i], AR.app_local_style_finish(canvas[i], styled[i], model_type, mode, strength, **opts), f"{mode} {model_type} image {i}")
    single = dimg.app_local_style_finish(_dev(canvas[2]), _dev(styled[2]), model_type, mode, strength, **opts)
    assert single.shape == CHAIN_SHAPE + (3,) and np.array_equal(single.cpu().numpy(), got[2])  # independent of N


def test_finish_on_a_full_canvas():
    from mstg_hip import image as dimg
    shape = (256, 256)
    canvas, styled = _canvases(shape, 0)[1], _styled(shape, 0)[1]  # the landscape
    c, s = _dev(canvas), _dev(styled)
    got = dimg.app_local_style_finish(c, s, "photo_to_monet")
    _same(got.cpu().numpy(), AR.app_local_style_finish(canvas, styled, "photo_to_monet"), "defaults at 256 x 256")
    assert torch.equal(got, dimg.app_local_style_finish(c, s, "photo_to_monet"))  # two runs are bit-identical


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


def test_launch_counts_do_not_depend_on_n():
    from mstg_hip import image as dimg
    c = _dev(np.concatenate([_canvases(CHAIN_SHAPE, 0), _canvases(CHAIN_SHAPE, 1)]))[:5]
    s = c.flip(2).contiguous()
    for mt in MODEL_TYPES:
        dimg.app_local_style_finish(c[:1], s[:1], mt)  # the tables are uploaded here, outside the counts
    off = dict(auto_select=False, ignore_sky=False, enhance_colors=False, smooth_transitions=False)
    for mt, mode, kw, want in (("photo_to_monet", "enhanced", dict(), 6), ("monet_to_photo", "enhanced", dict(), 5),
                               ("photo_to_monet", "enhanced", dict(auto_select=False), 3), ("photo_to_monet", "enhanced", off, 1),
                               ("photo_to_monet", "enhanced", dict(off, smooth_transitions=True), 1),
                               ("photo_to_monet", "enhanced", dict(off, strength=0.1, smooth_transitions=True), 2),
                               ("monet_to_photo", "simple", dict(), 1), ("monet_to_photo", "advanced", dict(strength=0.1), 1)):
        counts = [_launches(lambda: dimg.app_local_style_finish(c[:n], s[:n], mt, mode, **kw)) for n in (1, 5)]
        assert counts[0] == counts[1] == want <= 6, (mt, mode, kw, counts)


# ---- 3. the callers -------------------------------------------------------------------------------------------------------------------
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


def stub2(x):
    return x.flip(2)


def stub2_np(x):
    return np.asarray(x)[:, :, ::-1, :]


MIXED = [(150, 210), (210, 150), (97, 301)]  # landscape, portrait, a wide strip


@pytest.fixture(scope="module")
def mixed():
    arrays = [np.ascontiguousarray(LR.landscape(h, w, 70 + i)[:, :, ::-1] if i == 1 else LR.landscape(h, w, 70 + i)) for i, (h, w) in enumerate(MIXED)]
    return arrays, [_dev(a) for a in arrays]


def test_process_app_local_style_and_its_batch(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    calls = []

    def model(x):
        calls.append(x.shape[0])
        return stub(x)
    batch = dimg.process_app_local_style_batch(model, images, "photo_to_monet")
    assert calls == [3]
    chunked = dimg.process_app_local_style_batch(model, images, "photo_to_monet", batch_size=2)
    assert calls == [3, 2, 1]
    for k, (arr, im) in enumerate(zip(arrays, images)):
        one = dimg.process_app_local_style(stub, im, "photo_to_monet")
        _same(one.cpu().numpy(), AR.process_app_local_style(stub_np, arr, "photo_to_monet", resize=_pil_or_numpy()), f"image {k}")
        assert one.shape == arr.shape and torch.equal(one, batch[k]) and torch.equal(one, chunked[k])
    low = dimg.process_app_local_style(stub, images[0], "monet_to_photo", "simple", 0.2)
    _same(low.cpu().numpy(), AR.process_app_local_style(stub_np, arrays[0], "monet_to_photo", mode="simple", strength=0.2,
                                                        resize=_pil_or_numpy()), "simple")
    for a, b in zip(dimg.process_app_local_style_batch(stub, images[:2], "monet_to_photo", "other"),
                    dimg.process_local_style_batch(stub, images[:2], mode="other")):  # the styled image: the plain local-style pipeline
        assert torch.equal(a, b)
    assert _launches(lambda: dimg.process_app_local_style_batch(stub, images[:1], "photo_to_monet")) == \
        _launches(lambda: dimg.process_app_local_style_batch(stub, images, "photo_to_monet")) == 5 + 6


def test_process_compare(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    local, plain = dimg.process_compare(stub, stub2, images[1], "photo_to_monet", blend_strength=0.2)
    want_local, want_plain = AR.process_compare(stub_np, stub2_np, arrays[1], "photo_to_monet", 0.2, resize=_pil_or_numpy())
    _same(local.cpu().numpy(), want_local, "compare: local style")
    _same(plain.cpu().numpy(), want_plain, "compare: cyclegan")
    assert torch.equal(plain, dimg.process_local_style(stub2, images[1], mode="other"))  # the plain pipeline with the tab's crop
    seen = []

    def first(x):
        seen.append(x.clone())
        return stub(x)

    def second(x):
        seen.append(x.clone())
        return stub2(x)
    locals_b, plains_b = dimg.process_compare_batch(first, second, images, "monet_to_photo", sky_handling=False)
    assert len(seen) == 2 and torch.equal(seen[0], seen[1]) and seen[0].shape == (3, 3, 256, 256)  # both models on the same batch
    for k, im in enumerate(images):
        a, b = dimg.process_compare(stub, stub2, im, "monet_to_photo", sky_handling=False)
        assert torch.equal(a, locals_b[k]) and torch.equal(b, plains_b[k]) and a.shape == b.shape == im.shape
    assert _launches(lambda: dimg.process_compare_batch(stub, stub2, images, "photo_to_monet")) == \
        _launches(lambda: dimg.process_compare_batch(stub, stub2, images[:1], "photo_to_monet")) == 2 + 2 + 6 + 4


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    big = torch.zeros(400, 400, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="400 x 400"):
        dimg.app_local_style_finish(big, big.clone(), "photo_to_monet")
    out = dimg.app_local_style_finish(big, big.clone(), "photo_to_monet", auto_select=False)  # any size without auto_select
    assert out.shape == big.shape
    with pytest.raises(RuntimeError, match="auto_select"):
        dimg.process_app_local_style(stub, big, "photo_to_monet", target=400)
    z = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="model_type"):
        dimg.app_local_style_finish(z, z.clone(), "monet")
    with pytest.raises(ValueError, match="model_type"):
        dimg.process_compare(stub, stub2, z, "photo")
    lib = _lib.load()
    both = torch.zeros(2 * 8 * 8 * 3, dtype=torch.uint8, device=DEV)
    ws = torch.empty(lib.mstg_app_local_style_workspace_bytes(1, 8, 8), dtype=torch.uint8, device=DEV)
    rc = lib.mstg_app_local_style_finish(_p(both), _p(z), 1, 8, 8, 0, 0, 1, 0, 0.6, 0.5, 0.5, None, None, None, both.data_ptr() + 96, _p(ws),
                                         ws.numel(), _stream())
    assert rc == -1 and "overlaps" in lib.mstg_last_error().decode()  # out inside the canvas: MSTG_E_BADARG
