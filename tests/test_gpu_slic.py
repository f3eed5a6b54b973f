"""The device SLIC segmentation (csrc/slic.hip through mstg_slic_u8, mstg_slic_assign_u8 and mstg_connect_labels;
mstg_hip.image.slic_labels, slic_assign, connect_labels and process_enhanced_local_style(segmentation="slic"); the drop-in's
--segmentation option) against the numpy restatement of tests/slic_ref.py: labels and counts equal, the centres bit for bit, no
tolerance anywhere.  Every entry runs with 64 guard bytes behind every output and its inputs unchanged.  The restatement has not
been compared with a scikit-image binary (see its docstring)."""
import numpy as np
import pytest
import torch

import enhanced_local_style_ref as ER
import slic_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


def _guarded(nbytes):
    return torch.full((nbytes + GUARD,), 7, dtype=torch.uint8, device=DEV)


def _take(buf, nbytes, dtype, shape, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), f"{what} wrote behind its output"
    return out[:nbytes].view(dtype).reshape(shape)


# ---- the entries on numpy batches -------------------------------------------------------------------------------------------------
def _slic(x, n_segments, compactness=10.0):
    """mstg_slic_u8 of a numpy batch (N, H, W, 3) -> (labels (N, H, W), count (N,))"""
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    table = dimg._lab_table(xin.device)
    before = table.clone()
    need = lib.mstg_slic_workspace_bytes(N, H, W, n_segments)
    assert need > 0
    bl, bc, ws = _guarded(N * H * W * 4), _guarded(N * 4), _guarded(need)
    _lib.check(lib.mstg_slic_u8(_p(xin), N, H, W, n_segments, compactness, _p(table), _p(bl), _p(bc), _p(ws), need, _stream()), "mstg_slic_u8")
    labels = _take(bl, N * H * W * 4, np.int32, (N, H, W), "slic_u8 (labels)")
    count = _take(bc, N * 4, np.int32, (N,), "slic_u8 (count)")
    _take(ws, need, np.uint8, (need,), "slic_u8 (workspace)")
    assert torch.equal(xin, _dev(x)) and torch.equal(table, before), "mstg_slic_u8 changed an input"
    return labels, count


def _assign(x, n_segments, compactness=10.0):
    """mstg_slic_assign_u8 of a numpy batch -> (raw labels (N, H, W), centres (N, K, 5))"""
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    _, ny, nx = dimg.slic_grid(H, W, n_segments)
    K = ny * nx
    need = lib.mstg_slic_workspace_bytes(N, H, W, n_segments)
    bl, bc, ws = _guarded(N * H * W * 4), _guarded(N * K * 20), _guarded(need)
    _lib.check(lib.mstg_slic_assign_u8(_p(xin), N, H, W, n_segments, compactness, _p(dimg._lab_table(xin.device)), _p(bl), _p(bc), _p(ws), need,
                                       _stream()), "mstg_slic_assign_u8")
    labels = _take(bl, N * H * W * 4, np.int32, (N, H, W), "slic_assign_u8 (labels)")
    centres = _take(bc, N * K * 20, np.float32, (N, K, 5), "slic_assign_u8 (centres)")
    _take(ws, need, np.uint8, (need,), "slic_assign_u8 (workspace)")
    assert torch.equal(xin, _dev(x)), "mstg_slic_assign_u8 changed its input"
    return labels, centres


def _connect(labels, min_size):
    """mstg_connect_labels of a numpy batch (N, H, W) -> (labels, count)"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    lin = _dev(labels)
    N, H, W = lin.shape
    need = lib.mstg_connect_labels_workspace_bytes(N, H, W)
    assert need > 0
    bl, bc, ws = _guarded(N * H * W * 4), _guarded(N * 4), _guarded(need)
    _lib.check(lib.mstg_connect_labels(_p(lin), N, H, W, min_size, _p(bl), _p(bc), _p(ws), need, _stream()), "mstg_connect_labels")
    out = _take(bl, N * H * W * 4, np.int32, (N, H, W), "connect_labels (labels)")
    count = _take(bc, N * 4, np.int32, (N,), "connect_labels (count)")
    _take(ws, need, np.uint8, (need,), "connect_labels (workspace)")
    assert torch.equal(lin, _dev(labels)), "mstg_connect_labels changed its input"
    return out, count


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} entries differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ---- steps 1 to 3, and the whole -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.CASES)
def test_assign_and_labels_equal_the_restatement(name):
    r = SR.reference(name)
    x = r["img"][None]
    raw, centres = _assign(x, r["n_segments"])
    _same(raw[0], r["raw"], f"{name}: raw labels")
    _same(centres[0], r["centres"], f"{name}: centres")
    labels, count = _slic(x, r["n_segments"])
    assert int(count[0]) == r["count"], (name, int(count[0]), r["count"])
    _same(labels[0], r["labels"], f"{name}: labels")


@pytest.mark.parametrize("name", ["blocks96", "smooth"])
@pytest.mark.parametrize("compactness", [1.0, 40.0])
def test_compactness(name, compactness):
    """the 96 x 80 image (its cells lie on the grid: the labels are the cells at any compactness) and the smooth one, where the
    weight between colour and distance decides the labels"""
    r = SR.reference(name, compactness)
    x = r["img"][None]
    raw, centres = _assign(x, r["n_segments"], compactness)
    _same(raw[0], r["raw"], f"{name}, compactness {compactness}: raw labels")
    _same(centres[0], r["centres"], f"{name}, compactness {compactness}: centres")
    labels, count = _slic(x, r["n_segments"], compactness)
    assert int(count[0]) == r["count"]
    _same(labels[0], r["labels"], f"{name}, compactness {compactness}: labels")
    if name == "smooth":
        assert not np.array_equal(r["raw"], SR.reference(name)["raw"])  # the parameter reaches the result


# ---- step 4 alone ----------------------------------------------------------------------------------------------------------------
def _check_connect(labels, min_size, what):
    want, want_count = SR.connect(labels, min_size)
    got, count = _connect(labels[None], min_size)
    assert int(count[0]) == want_count, (what, int(count[0]), want_count)
    _same(got[0], want, what)
    return want_count


def test_connect_serpentine():
    """one component winding through every row: the case that defeats neighbour-minimum propagation"""
    lab = SR.serpentine(33, 47)
    assert _check_connect(lab, 50, "serpentine, the gaps small") == 1
    assert _check_connect(lab, 10, "serpentine, nothing small") == 17


def test_connect_checkerboard():
    """every component one pixel: with min_size 2 everything chains to pixel 0, along each row and up the first column (the case
    that defeats a per-thread walk at full size); with min_size 1 nothing is small and every pixel is a segment"""
    lab = SR.checkerboard(32, 64)
    assert _check_connect(lab, 2, "checkerboard, min_size 2") == 1
    assert _check_connect(lab, 1, "checkerboard, min_size 1") == 32 * 64
    assert _check_connect(lab, 0, "checkerboard, min_size 0") == 32 * 64


@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (1, 1)])
def test_connect_strips(shape):
    h, w = shape
    lab = (np.arange(h * w).reshape(h, w) // 3 % 2).astype(np.int32)  # runs of three
    _check_connect(lab, 1, f"strip {shape}, nothing small")
    _check_connect(lab, 4, f"strip {shape}, every run small")
    _check_connect(np.zeros(shape, dtype=np.int32), 5, f"strip {shape}, one label")


def test_connect_components_across_tile_corners():
    lab, _ = ER.grid_labels(40, 130, 3)
    for min_size in (1, 3, 40, 120):
        _check_connect(lab, min_size, f"grid labels, min_size {min_size}")
    wild = lab.copy()  # any int32 is a label: only equality counts
    wild[lab % 3 == 0] = np.iinfo(np.int32).min
    wild[lab % 3 == 1] = -7
    _check_connect(wild, 3, "negative labels")


# ---- batches, reproducibility ----------------------------------------------------------------------------------------------------
def test_a_batch_equals_the_single_calls_and_repeats_itself():
    from advanced_transform_ref import noise, smooth
    from color_blocks_ref import blocks
    x = np.stack([blocks(48, 80, 2, cell=16), smooth(48, 80, 4), noise(48, 80, 6)])
    labels, count = _slic(x, 20)
    again, count2 = _slic(x, 20)
    assert np.array_equal(labels, again) and np.array_equal(count, count2)
    raw, centres = _assign(x, 20)
    for i in range(3):
        one, c1 = _slic(x[i:i + 1], 20)
        assert np.array_equal(one[0], labels[i]) and c1[0] == count[i], f"image {i} alone differs from image {i} of three"
        r1, cen1 = _assign(x[i:i + 1], 20)
        assert np.array_equal(r1[0], raw[i]) and np.array_equal(cen1[0].view(np.uint32), centres[i].view(np.uint32))
    want, want_count = SR.slic(x[1], 20)
    assert int(count[1]) == want_count
    _same(labels[1], want, "image 1 of three")
    lab3 = np.stack([SR.serpentine(32, 64), SR.checkerboard(32, 64), ER.grid_labels(32, 64, 5)[0]])
    got, cnt = _connect(lab3, 3)
    for i in range(3):
        want, want_count = SR.connect(lab3[i], 3)
        assert int(cnt[i]) == want_count
        _same(got[i], want, f"connect, image {i} of three")


def test_python_surface():
    from mstg_hip import image as dimg
    r = SR.reference("blocks96")
    x = _dev(r["img"])
    labels, count = dimg.slic_labels(x, r["n_segments"], return_count=True)
    assert labels.dtype == torch.int32 and labels.is_cuda and tuple(labels.shape) == (96, 80) and int(count) == r["count"]
    _same(labels.cpu().numpy(), r["labels"], "slic_labels")
    assert torch.equal(dimg.slic_labels(x.unsqueeze(0), r["n_segments"])[0], labels)
    raw, centres = dimg.slic_assign(x, r["n_segments"])
    _same(raw.cpu().numpy(), r["raw"], "slic_assign (labels)")
    _same(centres.cpu().numpy(), r["centres"], "slic_assign (centres)")
    H, W = 96, 80
    _, ny, nx = dimg.slic_grid(H, W, r["n_segments"])
    assert dimg.slic_min_size(H, W, r["n_segments"]) == SR.min_size_of(H, W, ny * nx)
    staged, c2 = dimg.connect_labels(raw, dimg.slic_min_size(H, W, r["n_segments"]), return_count=True)
    assert torch.equal(staged, labels) and int(c2) == int(count)
    assert torch.equal(dimg.connect_labels(np.array(r["raw"]), dimg.slic_min_size(H, W, r["n_segments"])), labels)  # numpy labels
    assert int(count) <= dimg.slic_segment_bound(H, W, r["n_segments"])
    with pytest.raises(RuntimeError, match="step = 10"):
        dimg.slic_labels(x[:5].repeat(1, 3, 1)[:, :200].contiguous(), 10)
    with pytest.raises(RuntimeError, match="compactness = -1"):
        dimg.slic_labels(x, 30, compactness=-1)
    with pytest.raises(RuntimeError, match="n_segments = 0"):
        dimg.slic_labels(x, 0)


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
    x = _dev(np.stack([SR.case("blocks96")[0], SR.case("blocks96")[0][::-1].copy()]))  # 96 x 80: ceil(log16(7680)) = 4
    dimg.slic_labels(x[0], 30)  # the Lab table is uploaded here, outside the counts
    for n in (1, 2):
        assert _launches(lambda: dimg.slic_assign(x[:n], 30)) == 22
        assert _launches(lambda: dimg.slic_labels(x[:n], 30)) == 22 + 9 + 4
        assert _launches(lambda: dimg.connect_labels(torch.zeros((n, 96, 80), dtype=torch.int32, device=DEV), 5)) == 9 + 4


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import enhanced_generator as eg
    torch.manual_seed(11)
    g = eg.EnhancedGenerator(16, 1).to(DEV)
    g.eval()
    return g


def test_pipeline_with_slic_equals_the_stages_composed_by_hand(model, tmp_path):
    from PIL import Image
    import enhanced_local_style as E
    from mstg_hip import image as dimg
    h, w = 120, 80
    img_np = ER.smooth_noise(h, w, 4)
    img = _dev(img_np)
    got = dimg.process_enhanced_local_style(model, img, segmentation="slic")
    new_w, new_h, box, back = ER.geometry(w, h)
    resized = dimg.resize_u8(img, (new_w, new_h), dimg.LANCZOS)
    canvas = dimg.paste_u8(resized, (0, 0, new_h, new_w), (256, 256), ((256 - new_h) // 2, (256 - new_w) // 2), fill=0)
    with torch.no_grad():
        styled = dimg.to_u8(model(dimg.to_tensor(canvas).unsqueeze(0))[0])
    labels, count = dimg.slic_labels(canvas, return_count=True)
    bound = dimg.slic_segment_bound(256, 256)
    assert bound == 201 and 1 <= int(count) <= bound and int(labels.min()) == 1 and int(labels.max()) == int(count)
    m = dimg.segment_blend_map(canvas, labels, num_segments=bound + 1)  # labels 1 .. count <= bound
    assert torch.equal(m, dimg.segment_blend_map(canvas, labels))  # the bound drops no segment
    out = dimg.enhanced_style_finish(canvas, styled, m)
    assert box is not None and not back
    out = dimg.crop_u8(out, *box)
    assert got.shape == out.shape and torch.equal(got, out)
    # the default is the host segmentation, byte for byte, and the two segmentations give different images
    default = dimg.process_enhanced_local_style(model, img)
    assert torch.equal(default, dimg.process_enhanced_local_style(model, img, segmentation="felzenszwalb"))
    assert default.shape == got.shape and not torch.equal(default, got)
    # a caller's labels win over the keyword
    other = torch.from_numpy(ER.grid_labels(256, 256, 1, (32, 40))[0]).to(DEV)
    assert torch.equal(dimg.process_enhanced_local_style(model, img, segments=other, segmentation="slic"),
                       dimg.process_enhanced_local_style(model, img, segments=other))
    with pytest.raises(ValueError, match="quickshift"):
        dimg.process_enhanced_local_style(model, img, segmentation="quickshift")
    # the drop-in's command line writes that image
    Image.fromarray(img_np).save(tmp_path / "in.png")
    torch.save({"G_AB_state_dict": model.state_dict()}, tmp_path / "ckpt.pth")
    E.main(["--image", str(tmp_path / "in.png"), "--model", str(tmp_path / "ckpt.pth"), "--output", str(tmp_path / "o.png"), "--segmentation", "slic"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o.png")), got.cpu().numpy())
