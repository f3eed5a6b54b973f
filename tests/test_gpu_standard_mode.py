"""The finish of the application's standard mode on the device (csrc/standard_mode.hip through mstg_median3_u8, mstg_bilateral_u8,
mstg_lut_u8, mstg_gaussian_u8 and mstg_standard_finish; mstg_hip.image.standard_finish, process_standard and
process_standard_batch) against the numpy restatement of tests/standard_mode_ref.py, byte for byte: every stage on noise, blocky,
gradient, constant and 0 / 255 step images at sizes around the tiles and below the filter radius, three different images per
launch, guard bytes behind the output and the inputs unchanged; the chain against the composition of the stage entries over its
switches; the launch count; the two callers end to end; reproducibility.  The restatement has not been compared with an OpenCV
binary (see its docstring)."""
import itertools
from functools import lru_cache

import numpy as np
import pytest
import torch

import standard_mode_ref as SR
from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRIPLES = (("noise", "blocky", "step"), ("gradient", "constant", "step"))
BILATERAL_PARAMS = ((9, 75, 75), (5, 10, 3))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


@lru_cache(maxsize=None)
def _images(shape, which):
    """three different images of one shape, (3, H, W, 3); read-only so that the cached references stay valid"""
    h, w = shape
    a = np.stack([SR.image(kind, h, w, seed=11 * which + i + h) for i, kind in enumerate(TRIPLES[which])])
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def _ref(stage, shape, which, *params):
    fn = {"median": SR.median3, "bilateral": SR.bilateral, "gaussian": SR.gaussian}[stage]
    out = np.stack([fn(im, *params) for im in _images(shape, which)])
    out.setflags(write=False)
    return out


def _stage(name, x, *args):
    """one stage entry on an (N, H, W, 3) numpy batch -> numpy; 64 guard bytes behind ``out`` must survive, the input must not
    change.  ``args`` go between the shape and ``out`` (device tensors are passed as pointers)."""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    nbytes = N * H * W * 3
    buf = torch.full((nbytes + 64,), 7, dtype=torch.uint8, device=DEV)
    _lib.check(getattr(_lib.load(), name)(_p(xin), N, H, W, *[_p(a) if torch.is_tensor(a) else a for a in args], _p(buf), _stream()), name)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), f"{name} wrote behind its output"
    assert torch.equal(xin, _dev(x)), f"{name} changed its input"
    return out[:nbytes].reshape(N, H, W, 3)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}: "
                                                       f"{got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


# ---- 1. the stages --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (2, 5), (33, 65), (67, 93)])
def test_median(shape):
    for which in (0, 1):
        _same(_stage("mstg_median3_u8", _images(shape, which)), _ref("median", shape, which), f"median {shape} {TRIPLES[which]}")


@pytest.mark.parametrize("params", BILATERAL_PARAMS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (33, 65), (67, 93), (256, 256)])
def test_bilateral(shape, params):
    from mstg_hip import image as dimg
    table = dimg._bilateral_table(*params, torch.device(DEV))
    for which in ((0,) if shape == (256, 256) else (0, 1)):  # one launch at the large size: the reference takes a second per image
        got = _stage("mstg_bilateral_u8", _images(shape, which), params[0], table)
        _same(got, _ref("bilateral", shape, which, *params), f"bilateral {params} {shape} {TRIPLES[which]}")
    one = dimg.bilateral_u8(_dev(_images(shape, 0)[2]), *params)  # the Python entry on a single image
    assert one.shape == shape + (3,) and np.array_equal(one.cpu().numpy(), _ref("bilateral", shape, 0, *params)[2])


@pytest.mark.parametrize("model_type", SR.MODEL_TYPES)
def test_table_lookup_all_values(model_type):
    from mstg_hip import image as dimg
    v = np.arange(256, dtype=np.uint8)
    x = np.stack([np.stack([np.roll(v, s), np.roll(v[::-1], 3 * s), np.roll(v, -7 * s)], axis=-1).reshape(16, 16, 3) for s in (0, 1, 5)])
    assert all(len(np.unique(x[..., c])) == 256 for c in range(3))  # all 256 values in every channel
    got = _stage("mstg_lut_u8", x, dimg._color_lut(model_type, torch.device(DEV)))
    _same(got, np.stack([SR.apply_lut(im, SR.color_lut(model_type)) for im in x]), f"lookup {model_type}")
    odd = x.reshape(1, 3, 256, 3)[:, :, :251]  # a byte count that is no multiple of 12: the tail path
    _same(_stage("mstg_lut_u8", odd, dimg._color_lut(model_type, torch.device(DEV))), SR.apply_lut(odd, SR.color_lut(model_type)), "tail")


@pytest.mark.parametrize("ksize", [3, 5, 7])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (33, 65), (67, 93), (256, 256)])
def test_blur(shape, ksize):
    from mstg_hip import image as dimg
    for which in (0, 1):
        _same(_stage("mstg_gaussian_u8", _images(shape, which), ksize), _ref("gaussian", shape, which, ksize), f"blur {ksize} {shape}")
    one = dimg.gaussian_u8(_dev(_images(shape, 1)[0]), ksize)
    assert np.array_equal(one.cpu().numpy(), _ref("gaussian", shape, 1, ksize)[0])


def test_refusals_by_name():
    from mstg_hip import image as dimg
    z = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="d = 11 "):
        dimg.bilateral_u8(z, d=11)
    with pytest.raises(RuntimeError, match="smooth_level = 4"):
        dimg.gaussian_u8(z, 9)
    with pytest.raises(RuntimeError, match="smooth_level = 4"):
        dimg.standard_finish(z, z.clone(), "photo_to_monet", smooth_level=4)
    with pytest.raises(ValueError, match="model_type"):
        dimg.standard_finish(z, z.clone(), "monet")


# ---- 2. the chain ---------------------------------------------------------------------------------------------------------------------
CHAIN_SHAPE = (67, 93)


def _composed(canvas, styled, model_type, blend_ratio, fix_blocks, enhance_colors, smooth_level):
    """the stage entries one after the other, (N, H, W, 3) device tensors"""
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    x = styled
    if blend_ratio > 0:  # mstg_blend_u8 with the operands swapped
        x = torch.stack([dimg.blend_u8(s, c, strength=blend_ratio) for s, c in zip(styled, canvas)])
    if fix_blocks:
        x = dimg.bilateral_u8(dimg.median3_u8(x), 9, 75, 75)
    if enhance_colors:
        y = torch.empty_like(x)
        N, H, W = x.shape[:3]
        _lib.check(_lib.load().mstg_lut_u8(_p(x), N, H, W, _p(dimg._color_lut(model_type, x.device)), _p(y), _stream()), "mstg_lut_u8")
        x = y
    if smooth_level:
        x = dimg.gaussian_u8(x, 2 * smooth_level + 1)
    return x


@pytest.fixture(scope="module")
def chain_inputs():
    canvas, styled = _images(CHAIN_SHAPE, 0), _images(CHAIN_SHAPE, 1)[::-1]
    return canvas, np.ascontiguousarray(styled)


@pytest.mark.parametrize("fix_blocks", [True, False])
@pytest.mark.parametrize("blend_ratio", [0, 0.3])
def test_chain_equals_the_composed_stages(chain_inputs, blend_ratio, fix_blocks):
    from mstg_hip import image as dimg
    canvas, styled = chain_inputs
    c, s = _dev(canvas), _dev(styled)
    for colour, level in itertools.product(("photo_to_monet", "monet_to_photo", None), (0, 1, 3)):
        kw = dict(model_type=colour or "photo_to_monet", blend_ratio=blend_ratio, fix_blocks=fix_blocks, enhance_colors=colour is not None,
                  smooth_level=level)
        got = dimg.standard_finish(c, s, **kw)
        want = _composed(c, s, kw["model_type"], blend_ratio, fix_blocks, colour is not None, level)
        assert torch.equal(got, want), f"{kw}: {int((got != want).sum())} of {got.numel()} bytes differ"
        assert torch.equal(c, _dev(canvas)) and torch.equal(s, _dev(styled)), "the chain changed an input"
    assert torch.equal(dimg.standard_finish(c, s, "photo_to_monet", blend_ratio, fix_blocks, adaptive_smooth=False),
                       dimg.standard_finish(c, s, "photo_to_monet", blend_ratio, fix_blocks, smooth_level=0))


@pytest.mark.parametrize("model_type", SR.MODEL_TYPES)
def test_chain_defaults_against_the_restatement(chain_inputs, model_type):
    from mstg_hip import image as dimg
    canvas, styled = chain_inputs
    got = dimg.standard_finish(_dev(canvas), _dev(styled), model_type).cpu().numpy()
    for i in range(3):
        _same(got[i], SR.standard_finish(canvas[i], styled[i], model_type), f"{model_type} image {i}")
    single = dimg.standard_finish(_dev(canvas[1]), _dev(styled[1]), model_type)
    assert single.shape == CHAIN_SHAPE + (3,) and np.array_equal(single.cpu().numpy(), got[1])


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


def test_launch_count_does_not_depend_on_n():
    from mstg_hip import image as dimg
    x = _dev(np.concatenate([_images(CHAIN_SHAPE, 0), _images(CHAIN_SHAPE, 1)]))[:5]
    dimg.standard_finish(x[:1], x[:1].flip(1).contiguous(), "monet_to_photo")  # the tables are uploaded here, outside the counts
    for kw, want in ((dict(), 3), (dict(smooth_level=0), 2), (dict(fix_blocks=False), 2), (dict(fix_blocks=False, smooth_level=0), 1),
                     (dict(fix_blocks=False, blend_ratio=0, enhance_colors=False), 1)):
        counts = [_launches(lambda: dimg.standard_finish(x[:n], x[:n].flip(1).contiguous(), "monet_to_photo", **kw)) for n in (1, 5)]
        assert counts[0] == counts[1] == want <= 3, (kw, counts)


# ---- 3. the callers -------------------------------------------------------------------------------------------------------------------
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
    arrays = [_img(h, w, 70 + i) for i, (h, w) in enumerate(MIXED)]
    return arrays, [_dev(a) for a in arrays]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_process_standard_defaults(mixed, k):
    from mstg_hip import image as dimg
    arr, dev = mixed[0][k], mixed[1][k]
    model_type = SR.MODEL_TYPES[k % 2]
    out = dimg.process_standard(stub, dev, model_type).cpu().numpy()
    _same(out, SR.process_standard(stub_np, arr, model_type, resize=_pil_or_numpy()), f"image {k} {model_type}")
    assert out.shape == arr.shape


def test_batch_equals_the_one_image_function(mixed):
    from mstg_hip import image as dimg
    arrays, images = mixed
    loop = [dimg.process_standard(stub, im, "photo_to_monet") for im in images]
    calls = []

    def model(x):
        calls.append(x.shape[0])
        return stub(x)
    for bs, want_calls in ((2, [2, 2, 1]), (5, [5])):  # chunked and unchunked
        del calls[:]
        outs = dimg.process_standard_batch(model, images, "photo_to_monet", batch_size=bs)
        assert calls == want_calls
        for i, (a, b) in enumerate(zip(loop, outs)):
            assert a.shape == b.shape and torch.equal(a, b), f"batch_size {bs} image {i}: {int((a != b).sum())} of {a.numel()} bytes differ"
    off = dimg.process_standard_batch(stub, images[:2], "monet_to_photo", blend_ratio=0, fix_blocks=False, enhance_colors=False, smooth_level=0)
    for a, b in zip(off, dimg.process_cyclegan_batch(stub, images[:2])):  # every step off: the plain pipeline
        assert torch.equal(a, b)
    assert _launches(lambda: dimg.process_standard_batch(stub, images[:1], "photo_to_monet")) == \
        _launches(lambda: dimg.process_standard_batch(stub, images, "photo_to_monet")) == 8


# ---- 4. reproducibility ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(chain_inputs, mixed):
    from mstg_hip import image as dimg
    c, s = _dev(chain_inputs[0]), _dev(chain_inputs[1])
    assert torch.equal(dimg.standard_finish(c, s, "monet_to_photo"), dimg.standard_finish(c, s, "monet_to_photo"))
    a = dimg.process_standard_batch(stub, mixed[1], "monet_to_photo")
    b = dimg.process_standard_batch(stub, mixed[1], "monet_to_photo")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
