"""CPU: the geometry the batched image pipeline plans (mstg_hip.image.letterbox_plan / dataset_plan) is the geometry of the
per-image references in oracle/image_ref.py, and the host-side descriptor validation of csrc/image_batch.hip refuses bad
descriptors by image index.  No kernel is launched here.

The references are run with an identity-like ``model_fn`` and a ``resize`` stub that records what it is asked for and returns
coordinate-coded pixels, so every size, offset, crop box and resize-back decision they take is read from their own execution."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import image_ref as IR

EDGE = [(256, 256), (256, 171), (512, 256), (64, 48), (1100, 1000), (1024, 1024), (171, 256), (1000, 1100), (1024, 1025), (3, 700)]


def _sizes():
    rng = random.Random(2024)
    return EDGE + [(rng.randint(8, 1300), rng.randint(8, 1300)) for _ in range(200)]


def _coded(h, w):
    """(h, w, 3) bytes that spell their own coordinates: x % 256, y % 256, x // 256 + 16 * (y // 256)"""
    y, x = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([x % 256, y % 256, x // 256 + 16 * (y // 256)], axis=2).astype(np.uint8))


def _decode(px):
    return int(px[1]) + 256 * (int(px[2]) // 16), int(px[0]) + 256 * (int(px[2]) % 16)  # (y, x)


def _coded_long(h, w):
    """the same for one long side (a dataset resize can be tens of thousands of pixels long): byte 2 = max(x, y) // 256"""
    y, x = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([x % 256, y % 256, np.maximum(x, y) // 256], axis=2).astype(np.uint8))


class _Resize:
    def __init__(self, coded=_coded):
        self.calls, self.coded = [], coded

    def __call__(self, img, size, filt):
        self.calls.append((img.shape[:2], tuple(size), filt, _decode(img[0, 0])))
        return self.coded(size[1], size[0])


def _canvas_coded_model(x):
    """a 'model' whose output bytes are the canvas coordinates: (b + 0.5) / 255 survives (y + 1) / 2 * 255 truncation exactly"""
    T = x.shape[2]
    assert T <= 256
    b = _coded(T, T).transpose(2, 0, 1).astype(np.float32)
    return ((b + np.float32(0.5)) / np.float32(255) * 2 - 1)[None]


@pytest.mark.parametrize("local_style", [False, True])
def test_letterbox_plan_is_the_references_geometry(local_style):
    from mstg_hip import image as dimg
    sizes = _sizes()
    plan = dimg.letterbox_plan(sizes, 256, local_style=local_style)
    assert len(plan) == len(sizes)
    for (h, w), g in zip(sizes, plan):
        rz, seen = _Resize(), {}

        def model_fn(x):
            seen["canvas"] = x
            return _canvas_coded_model(x)
        img = np.zeros((h, w, 3), dtype=np.uint8)
        img[0, 0] = (0, 0, 0)
        if local_style:
            out = IR.process_local_style_ref(model_fn, img, mode="styled", resize=rz)
        else:
            out = IR.process_cyclegan_ref(model_fn, img, resize=rz)
        assert (g.height, g.width) == (h, w)
        # the letterbox resize and where it landed: the stub's bytes are the resized image's own coordinates
        assert rz.calls[0][:3] == ((h, w), (g.new_w, g.new_h), IR.LANCZOS)
        canvas = np.rint((seen["canvas"][0] * 0.5 + 0.5) * 255).astype(np.uint8).transpose(1, 2, 0)
        ref_canvas = np.full((256, 256, 3), 255, dtype=np.uint8)
        ref_canvas[g.off_y:g.off_y + g.new_h, g.off_x:g.off_x + g.new_w] = _coded(g.new_h, g.new_w)
        assert np.array_equal(canvas, ref_canvas), (h, w)
        # the crop box of the output canvas and the resize back
        left, top, crop_w, crop_h = g.crop
        assert g.resize_back == (w * h <= 1024 * 1024)
        if g.resize_back:
            assert len(rz.calls) == 2
            assert rz.calls[1] == ((crop_h, crop_w), (w, h), IR.LANCZOS, (top, left)), (h, w)
            assert (g.out_h, g.out_w) == (h, w) == out.shape[:2]
        else:
            assert len(rz.calls) == 1
            assert out.shape[:2] == (crop_h, crop_w) == (g.out_h, g.out_w) and _decode(out[0, 0]) == (top, left), (h, w)


def test_letterbox_plan_edge_decisions():
    from mstg_hip import image as dimg
    sq, same, wide, up, big, limit = dimg.letterbox_plan([(256, 256), (256, 171), (512, 256), (64, 48), (1100, 1000), (1024, 1024)], 256)
    assert (sq.new_h, sq.new_w, sq.off_y, sq.off_x, sq.crop, sq.resize_back) == (256, 256, 0, 0, (0, 0, 256, 256), True)
    assert (same.new_h, same.new_w) == (256, 171) and same.crop[2:] == (171, 256)  # neither pass changes a size, either way
    assert (wide.new_h, wide.new_w, wide.off_x) == (256, 128, 64)
    assert (up.new_h, up.new_w) == (256, 192)                                      # an upscale
    assert not big.resize_back and (big.out_h, big.out_w) == (big.crop[3], big.crop[2])
    assert limit.resize_back and (limit.out_h, limit.out_w) == (1024, 1024)


@pytest.mark.parametrize("size", [(1, 300), (300, 1)])
def test_a_side_of_zero_raises_and_names_the_image(size):
    from mstg_hip import image as dimg
    with pytest.raises(ValueError, match="image 2"):
        dimg.letterbox_plan([(256, 256), (64, 48), size], 256)
    with pytest.raises(ValueError, match="image 2"):
        dimg.letterbox_plan([(256, 256), (64, 48), size], 256, local_style=True)
    with pytest.raises(ValueError, match="image 1"):
        dimg.dataset_plan([(256, 256), (0, 4)], 256)


@pytest.mark.parametrize("img_size", [256, 64])
def test_dataset_plan_is_the_references_geometry(img_size):
    from mstg_hip import image as dimg
    sizes = [s for s in _sizes()[:110] if s != (3, 700)] + [(300, 420), (512, 384)]
    for (h, w), g in zip(sizes, dimg.dataset_plan(sizes, img_size)):
        rz = _Resize(_coded_long)
        _, image, _ = IR.dataset_item_ref(_coded_long(h, w), 0, img_size, resize=rz)
        if (g.new_w, g.new_h) == (w, h):
            assert not rz.calls
        else:
            assert rz.calls == [((h, w), (g.new_w, g.new_h), IR.BILINEAR, (0, 0))]
        first = np.rint((image[:, 0, 0] * 0.5 + 0.5) * 255).astype(np.uint8)
        # the shorter side becomes img_size, so the crop origin is 0 along it and byte 2 belongs to the other coordinate
        origin = (int(first[1]) + 256 * int(first[2]), int(first[0])) if w <= h else (int(first[1]), int(first[0]) + 256 * int(first[2]))
        assert image.shape == (3, img_size, img_size) and origin == (g.top, g.left), (h, w)
        assert (g.left == 0 and g.new_w == img_size) if w <= h else (g.top == 0 and g.new_h == img_size)
        assert g.top + img_size <= g.new_h and g.left + img_size <= g.new_w


# ---- the validation entry -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _descs(lib):
    """three valid letterbox descriptors (fake, never dereferenced source pointers) and their packed table"""
    from mstg_hip import _lib, image as dimg
    sizes, T = [(300, 420), (97, 301), (64, 48)], 256
    parts, index, tlen, descs, inter = [], {}, 0, (_lib.ImgDesc * 3)(), 0

    def table(i, o):
        nonlocal tlen
        if (i, o) not in index:
            _, kk, b = dimg._coeff_tables_host(i, o, dimg.LANCZOS)
            index[(i, o)] = (tlen, tlen + kk.size)
            parts.extend([kk.reshape(-1), b.reshape(-1)])
            tlen += kk.size + b.size
        return index[(i, o)]

    for d, g in zip(descs, dimg.letterbox_plan(sizes, T)):
        ks_h, ks_v, y_first, irows = dimg._axes(g.height, g.width, g.new_h, g.new_w, dimg.LANCZOS, 0, g.new_h)
        d.src, d.src_h, d.src_w, d.box_h, d.box_w = 4096, g.height, g.width, g.height, g.width
        d.rs_h, d.rs_w, d.filter, d.win_h, d.win_w = g.new_h, g.new_w, dimg.LANCZOS, g.new_h, g.new_w
        d.dst_y, d.dst_x, d.fill, d.ks_h, d.ks_v, d.y_first, d.irows = g.off_y, g.off_x, 255, ks_h, ks_v, y_first, irows
        d.ipitch = (3 * g.new_w + 3) & ~3
        d.kk_h, d.bounds_h = table(g.width, g.new_w)
        d.kk_v, d.bounds_v = table(g.height, g.new_h)
        d.inter_off = inter
        inter += irows * d.ipitch
    return descs, np.concatenate(parts), inter, T


def test_validation_accepts_good_descriptors_and_builds_tiles(lib):
    from mstg_hip import _lib
    descs, table, inter, T = _descs(lib)
    assert lib.mstg_img_batch_validate(descs, 3, table.ctypes.data, table.size, inter, T, 0) == 0, lib.mstg_last_error()
    for p, canvas in ((_lib.IMG_PASS_H, 0), (_lib.IMG_PASS_V_TENSOR, T)):
        cnt = lib.mstg_img_batch_tiles(descs, 3, table.ctypes.data, table.size, p, canvas, None, 0)
        assert cnt > 0, lib.mstg_last_error()
        tiles = np.full((cnt, 4), -1, dtype=np.int32)
        assert lib.mstg_img_batch_tiles(descs, 3, table.ctypes.data, table.size, p, canvas, tiles.ctypes.data, cnt) == cnt
        assert set(tiles[:, 0]) == {0, 1, 2} and tiles.min() >= 0
        if p == _lib.IMG_PASS_V_TENSOR:  # the canvas tiles of every image cover T x T exactly once
            assert sum(int(e) * 64 for e in tiles[:, 3]) == 3 * T * T
        assert lib.mstg_img_batch_tiles(descs, 3, table.ctypes.data, table.size, p, canvas, tiles.ctypes.data, cnt - 1) == -4
    # every launch entry validates before it touches the device: a bad descriptor is refused without a GPU
    descs[1].win_w += 1
    assert lib.mstg_img_batch_resample_h(descs, 3, table.ctypes.data, table.size, 4096, 4096, 1, 4096, 4096, inter, None) == -1
    assert b"image 1" in lib.mstg_last_error()
    assert lib.mstg_img_batch_resample_v_tensor(descs, 3, table.ctypes.data, table.size, 4096, 4096, 1, 4096, 4096, inter, T, 4096, None, None,
                                                None, 0, None) == -1
    assert lib.mstg_img_batch_resample_v_u8(descs, 3, table.ctypes.data, table.size, 4096, 4096, 1, 4096, 4096, inter, 4096, 1 << 30, None) == -1
    assert lib.mstg_img_batch_tensor_to_u8(None, 0, 1, 4, 4, 4096, None) == -1


BAD = {
    "window outside its image": lambda d: setattr(d, "win_x", d.rs_w - d.win_w + 1),
    "window taller than the resized image": lambda d: setattr(d, "win_h", d.rs_h + 1),
    "source box outside the image": lambda d: setattr(d, "box_y", 1),
    "zero size": lambda d: setattr(d, "rs_w", 0),
    "zero window": lambda d: setattr(d, "win_h", 0),
    "negative source size": lambda d: setattr(d, "src_h", -5),
    "table offset past the buffer": lambda d: setattr(d, "kk_h", 1 << 40),
    "bounds offset past the buffer": lambda d: setattr(d, "bounds_v", 1 << 40),
    "negative table offset": lambda d: setattr(d, "kk_v", -8),
    "null pointer": lambda d: setattr(d, "src", None),
    "intermediate past the buffer": lambda d: setattr(d, "inter_off", 1 << 40),
    "window placed outside the canvas": lambda d: setattr(d, "dst_x", 200),
    "tap count that does not belong to the sizes": lambda d: setattr(d, "ks_h", d.ks_h + 2),
    "rows the intermediate does not hold": lambda d: setattr(d, "y_first", d.y_first + 1),
}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("which", [0, 2])
def test_validation_refuses_a_bad_descriptor_and_names_the_image(lib, what, which):
    descs, table, inter, T = _descs(lib)
    BAD[what](descs[which])
    assert lib.mstg_img_batch_validate(descs, 3, table.ctypes.data, table.size, inter, T, 0) == -1, what
    assert f"image {which}:".encode() in lib.mstg_last_error(), (what, lib.mstg_last_error())
    if what != "intermediate past the buffer":  # the tile builder is not told the buffer sizes; the launch entries are
        assert lib.mstg_img_batch_tiles(descs, 3, table.ctypes.data, table.size, 1, T, None, 0) < 0


def test_validation_reads_the_bounds_tables(lib):
    descs, table, inter, T = _descs(lib)
    table = table.copy()
    table[descs[1].bounds_h + 2 * 5] = descs[1].box_w  # column 5 of image 1 would start past its source row
    assert lib.mstg_img_batch_validate(descs, 3, table.ctypes.data, table.size, inter, T, 0) == -1
    assert b"image 1:" in lib.mstg_last_error()
    assert lib.mstg_img_batch_validate(None, 3, table.ctypes.data, table.size, inter, T, 0) == -1
    assert lib.mstg_img_batch_validate(descs, 0, table.ctypes.data, table.size, inter, T, 0) == -1


def test_descriptor_layout():
    from mstg_hip import _lib, image as dimg
    assert C.sizeof(_lib.ImgDesc) == 152 == dimg._DESC.itemsize
    for name, _ in _lib.ImgDesc._fields_:
        assert getattr(_lib.ImgDesc, name).offset == dimg._DESC.fields[name][1], name
