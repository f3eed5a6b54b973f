"""Batched device image pipeline (csrc/image_batch.hip, mstg_hip.image.*_batch, pretrain.MonetPhotoDataset.get_batch): N images of
different sizes per call, a number of library launches that does not depend on N, and every byte equal to the per-image
references of oracle/image_ref.py (Pillow where it is importable, else the numpy restatement tests/test_image_cpu.py pins to it)."""
import random

import numpy as np
import pytest
import torch

from oracle import image_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(300, 420), (420, 300), (256, 256), (256, 171), (512, 256), (97, 301), (64, 48), (1100, 1000)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


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


def stub_half(x):
    return (-x.flip(3)).half()


def stub_np(x):
    return -np.asarray(x)[:, :, :, ::-1]


def stub_half_np(x):  # the reference fed the fp16-rounded values
    return stub_np(x).astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def arrays():
    return [_img(h, w, 30 + i) for i, (h, w) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def images(arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


@pytest.fixture(scope="module")
def cyclegan_refs(arrays):
    rz = _pil_or_numpy()
    return {"fp32": [IR.process_cyclegan_ref(stub_np, a, resize=rz) for a in arrays],
            "fp16": [IR.process_cyclegan_ref(stub_half_np, a, resize=rz) for a in arrays]}


def _same(outs, refs):
    assert len(outs) == len(refs)
    for i, (o, r) in enumerate(zip(outs, refs)):
        o = o.cpu().numpy()
        assert o.dtype == np.uint8 and o.shape == r.shape, (i, o.shape, r.shape)
        assert np.array_equal(o, r), f"image {i} {SHAPES[i] if i < len(SHAPES) else ''}: {int((o != r).sum())} of {o.size} bytes differ"


@pytest.mark.parametrize("kind", ["fp32", "fp16"])
def test_mixed_batch_in_one_call(images, cyclegan_refs, kind):
    from mstg_hip import image as dimg
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return (stub if kind == "fp32" else stub_half)(x)
    outs = dimg.process_cyclegan_batch(model, images)
    assert calls == [(8, 3, 256, 256)]
    _same(outs, cyclegan_refs[kind])
    assert outs[7].shape[:2] != SHAPES[7]  # 1100 x 1000 keeps its cropped canvas


@pytest.mark.parametrize("mode,strength", [("simple", 0.8), ("simple", 1.0 / 3.0), ("weight_map", None), ("styled", None)])
def test_local_style_same_batch(arrays, images, mode, strength):
    from mstg_hip import image as dimg
    rs = np.random.RandomState(9)
    maps = [rs.rand(256, 256) for _ in arrays] if mode == "weight_map" else None
    kw = {} if strength is None else {"strength": strength}
    outs = dimg.process_local_style_batch(stub, images, mode=mode, weight_maps=maps, **kw)
    refs = [IR.process_local_style_ref(stub_np, a, mode=mode, weight_map=None if maps is None else maps[i], resize=_pil_or_numpy(), **kw)
            for i, a in enumerate(arrays)]
    _same(outs, refs)


def test_chunking(images, cyclegan_refs):
    from mstg_hip import image as dimg
    calls = []

    def model(x):
        calls.append(x.shape[0])
        return stub(x)
    outs = dimg.process_cyclegan_batch(model, images, batch_size=3)
    assert calls == [3, 3, 2]
    whole = dimg.process_cyclegan_batch(stub, images, batch_size=64)
    for a, b in zip(outs, whole):
        assert torch.equal(a, b)
    _same(outs, cyclegan_refs["fp32"])


def test_real_network_equals_the_per_image_loop():
    """The plain fp16 generator documents that a pixel's result does not depend on the batch or tile (infer_f16_plain.hip), so
    the batched pipeline around ONE forward of five images equals five per-image calls byte for byte."""
    import plain_generator
    from mstg_hip import image as dimg
    torch.manual_seed(1234)
    m = plain_generator.Generator(8).to(DEV).half_inference().eval()
    imgs = [torch.from_numpy(_img(h, w, 70 + i)).to(DEV) for i, (h, w) in enumerate([(300, 420), (420, 300), (256, 256), (97, 301), (64, 48)])]
    loop = [dimg.process_cyclegan(m, im) for im in imgs]
    batch = dimg.process_cyclegan_batch(m, imgs)
    for i, (a, b) in enumerate(zip(loop, batch)):
        assert a.shape == b.shape and torch.equal(a, b), f"image {i}: {int((a != b).sum())} of {a.numel()} bytes differ"


def test_launch_count_does_not_depend_on_n(images):
    from mstg_hip import _lib, image as dimg
    lib = _lib.load()
    counts = []
    for imgs in (images[:3], (images + images)[:12]):
        torch.cuda.synchronize()
        lib.mstg_prof_enable(1)
        try:
            dimg.process_cyclegan_batch(stub, imgs)
            torch.cuda.synchronize()
            counts.append(lib.mstg_prof_count())
        finally:
            lib.mstg_prof_enable(0)
    assert counts[0] == counts[1] and 0 < counts[0] <= 6, counts
    lib.mstg_prof_enable(1)
    try:
        dimg.process_local_style_batch(stub, images[:3], mode="simple")
        torch.cuda.synchronize()
        assert lib.mstg_prof_count() <= 6
    finally:
        lib.mstg_prof_enable(0)


def test_dataset_batch():
    from mstg_hip import image as dimg
    arrs = [_img(300, 420, 3), _img(512, 384, 4), _img(256, 256, 5)]
    rng = random.Random(42)
    grids = [IR.draw_grid_mask(rng) for _ in arrs]
    masked, image, mask = dimg.dataset_batch(dimg.upload_u8(arrs, DEV), grids)
    assert masked.shape == image.shape == mask.shape == (3, 3, 256, 256)
    for i, (a, g) in enumerate(zip(arrs, grids)):
        m_ref, i_ref, k_ref = IR.dataset_item_ref(a, g, resize=_pil_or_numpy())
        assert np.array_equal(image[i].cpu().numpy(), i_ref), i
        assert np.array_equal(mask[i].cpu().numpy(), k_ref), i
        assert np.array_equal(masked[i].cpu().numpy(), m_ref), i


def test_loader_equivalence():
    import pretrain
    arrs = [_img(130 + 7 * i, 150 - 9 * i, 80 + i) for i in range(5)]
    ds = pretrain.MonetPhotoDataset(arrays=arrs, device=DEV, img_size=64)
    random.seed(7)
    got = list(pretrain.DeviceLoader(ds, batch_size=2, shuffle=True))
    random.seed(7)
    order = list(range(5))
    random.shuffle(order)
    items = [ds[i] for i in order]
    assert [g[0].shape[0] for g in got] == [2, 2, 1]
    for b, fields in enumerate(got):
        want = tuple(torch.stack(f) for f in zip(*items[2 * b:2 * b + 2]))
        for f, w in zip(fields, want):
            assert f.shape == w.shape and torch.equal(f, w), b


def test_determinism(images):
    from mstg_hip import image as dimg
    a = dimg.process_cyclegan_batch(stub, images)
    b = dimg.process_cyclegan_batch(stub, images)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
