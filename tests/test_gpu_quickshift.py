"""The device quickshift segmentation (csrc/quickshift.hip through mstg_quickshift_density_u8, mstg_quickshift_parents_u8 and
mstg_quickshift_u8; mstg_hip.image.quickshift_density, quickshift_parents, quickshift_labels, quickshift_segmenter and the callable
``segments`` of process_enhanced_local_style; the drop-in's --device-segmentation option) against the numpy restatement of
tests/quickshift_ref.py.

The density is compared within the number of taps of each pixel's window: a term is rint(exp(x) * 2^32), and two float64 exp that
differ by a few ulp (relative 1e-15, against one unit's 2.3e-10) move a term by at most one unit.  The parents are computed from the
RESTATEMENT's density and must be equal; the labels must equal the restatement run on the DEVICE's own density.  Together that pins
the pipeline without resting on two exp being equal bit for bit; on the three cases whose density gaps exceed twice the tap count
(test_quickshift_cpu.py) the labels must also equal the plain restatement.  The Python surface runs under
``guard_helpers.memory_contract``: red zones around every output and workspace, the inputs unchanged.  The restatement has not been
compared with a scikit-image binary (see its docstring)."""
import numpy as np
import pytest
import torch

import enhanced_local_style_ref as ER
import quickshift_ref as QR
from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{name}-{params}" for name, params in QR.RUNS]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib, image as dimg
    _lib.load()
    dimg._lab_table(torch.device(DEV))  # uploaded once, outside the guards and the launch counts


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


_density_cache = {}


def _device_density(name, params):
    """quickshift_density of a named run -> int64 numpy, computed once"""
    from mstg_hip import image as dimg
    key = (name, params)
    if key not in _density_cache:
        with memory_contract(check_inputs=True) as g:
            d = dimg.quickshift_density(_dev(QR.reference(name, params)["img"]), params[0], params[1])
            assert g.outputs >= 1
            assert d.dtype == torch.int64 and d.is_cuda
            _density_cache[key] = d.cpu().numpy()
    return _density_cache[key]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} entries differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ---- 1. density ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", QR.RUNS, ids=IDS)
def test_density_is_within_the_tap_count_of_the_restatement(run):
    name, params = run
    r = QR.reference(name, params)
    H, W = r["img"].shape[:2]
    got = _device_density(name, params)
    assert got.shape == (H, W)
    diff = np.abs(got - r["density"])
    print(f"{name} {params}: {int((diff != 0).sum())} of {H * W} densities differ from the restatement's, the largest by {int(diff.max())}")
    bound = QR.taps(H, W, QR.window(params[1]))
    bad = np.argwhere(diff > bound)
    assert len(bad) == 0, f"{name}: {len(bad)} densities off by more than their tap count, first at {bad[0].tolist()}: {diff[tuple(bad[0])]}"


# ---- 2. parents ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", QR.RUNS, ids=IDS)
def test_parents_of_the_restatements_density_equal_the_restatements(run):
    from mstg_hip import image as dimg
    name, params = run
    r = QR.reference(name, params)
    with memory_contract(check_inputs=True):
        got = dimg.quickshift_parents(_dev(r["img"]), _dev(r["density"]), *params)
        assert got.dtype == torch.int32 and got.is_cuda
        got = got.cpu().numpy()
    _same(got, r["parent"], f"{name} {params}: parents")


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", QR.RUNS, ids=IDS)
def test_labels_equal_the_restatement_on_the_devices_density(run):
    from mstg_hip import image as dimg
    name, params = run
    r = QR.reference(name, params)
    with memory_contract(check_inputs=True) as g:
        labels, count = dimg.quickshift_labels(_dev(r["img"]), *params, return_count=True)
        assert g.outputs >= 3  # labels, count, the workspace
        assert labels.dtype == torch.int32 and labels.is_cuda and count.dtype == torch.int32 and count.dim() == 0
        labels, count = labels.cpu().numpy(), int(count)
    want = QR.quickshift(r["img"], *params, density=_device_density(name, params))
    assert count == want["count"], (name, count, want["count"])
    _same(labels, want["labels"], f"{name} {params}: labels on the device's density")
    if name in QR.EXACT_CASES and params == QR.REFERENCE_PARAMS:
        assert count == r["count"]
        _same(labels, r["labels"], f"{name}: labels against the plain restatement")
    if params[0] == 0.0:
        assert count == 1


# ---- 4. position independence --------------------------------------------------------------------------------------------------------
def test_a_flat_image_is_one_segment_wherever_its_tiles_fall():
    from mstg_hip import image as dimg
    x = np.full((64, 200, 3), 143, dtype=np.uint8)
    with memory_contract(check_inputs=True):
        xin = _dev(x)
        labels, count = dimg.quickshift_labels(xin, 0.5, 3, 6, return_count=True)
        dens = dimg.quickshift_density(xin, 0.5, 3)
        labels, count, dens = labels.cpu().numpy(), int(count), dens.cpu().numpy()
    assert count == 1 and not labels.any()
    interior = dens[9:-9, 9:-9]
    assert (interior == interior[0, 0]).all(), "interior densities of a flat image differ"
    assert np.array_equal(dens, dens[::-1]) and np.array_equal(dens, dens[:, ::-1])  # mirror-image windows tie exactly


def test_both_ways_of_splitting_a_window_give_the_same_bits(monkeypatch):
    """MSTG_QUICKSHIFT_SPLIT forces one lane or four lanes per pixel: the density is an integer sum, so nothing may change"""
    from mstg_hip import image as dimg
    out = {}
    for split in ("1", "4"):
        monkeypatch.setenv("MSTG_QUICKSHIFT_SPLIT", split)
        for name in ("smooth", "flat_small", "strip_w"):
            with memory_contract(check_inputs=True):
                out[split, name] = dimg.quickshift_density(_dev(QR.case(name)), 0.5, 3).cpu().numpy()
    monkeypatch.delenv("MSTG_QUICKSHIFT_SPLIT")
    for name in ("smooth", "flat_small", "strip_w"):
        _same(out["1", name], out["4", name], f"{name}: one lane against four lanes per pixel")
        _same(out["1", name], _device_density(name, QR.REFERENCE_PARAMS), f"{name}: forced against chosen")


# ---- 5. batching and reproducibility ----------------------------------------------------------------------------------------------
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


def _batch():
    from advanced_transform_ref import noise, smooth
    return np.stack([noise(40, 70, 1), smooth(40, 70, 2), np.full((40, 70, 3), 60, dtype=np.uint8)])


def test_a_batch_equals_the_single_calls_and_repeats_itself():
    from mstg_hip import image as dimg
    x = _batch()
    with memory_contract(check_inputs=True):
        xin = _dev(x)
        labels, count = dimg.quickshift_labels(xin, 0.5, 3, 6, return_count=True)
        again, count2 = dimg.quickshift_labels(xin, 0.5, 3, 6, return_count=True)
        dens = dimg.quickshift_density(xin, 0.5, 3)
        par = dimg.quickshift_parents(xin, dens, 0.5, 3, 6)
        assert tuple(labels.shape) == (3, 40, 70) and tuple(count.shape) == (3,)
        assert torch.equal(labels, again) and torch.equal(count, count2)
        for i in range(3):
            one, c1 = dimg.quickshift_labels(xin[i], 0.5, 3, 6, return_count=True)
            assert torch.equal(one, labels[i]) and int(c1) == int(count[i]), f"image {i} alone differs from image {i} of three"
            assert torch.equal(dimg.quickshift_density(xin[i], 0.5, 3), dens[i])
            assert torch.equal(dimg.quickshift_parents(xin[i], dens[i], 0.5, 3, 6), par[i])
        assert int(par.min()) >= 0 and int(par.max()) < 40 * 70  # indices inside the pixel's own image
        labels, count, dens = labels.cpu().numpy(), count.cpu().numpy(), dens.cpu().numpy()
    assert np.array_equal(dens[0], _device_density("noise", QR.REFERENCE_PARAMS))  # the same image alone, earlier
    for i in range(3):
        want = QR.quickshift(x[i], 0.5, 3, 6, density=dens[i])
        assert int(count[i]) == want["count"]
        _same(labels[i], want["labels"], f"image {i} of three")
    assert int(count[2]) == 1 and int(count[0]) == QR.reference("noise")["count"] > 1400


def test_launch_counts_are_the_headers():
    from mstg_hip import image as dimg
    x = _dev(_batch())  # 40 x 70: ceil(log16(2800)) = 3
    dens = dimg.quickshift_density(x, 0.5, 3)
    for n in (1, 3):
        assert _launches(lambda: dimg.quickshift_density(x[:n], 0.5, 3)) == 1
        assert _launches(lambda: dimg.quickshift_parents(x[:n], dens[:n], 0.5, 3, 6)) == 1
        assert _launches(lambda: dimg.quickshift_labels(x[:n], 0.5, 3, 6)) == 6 + 3
    big = torch.zeros((1, 256, 256, 3), dtype=torch.uint8, device=DEV)
    assert _launches(lambda: dimg.quickshift_labels(big, 0.5, 3, 6)) == 10  # the header's figure for 256 x 256


def test_python_surface_refuses_by_name():
    from mstg_hip import image as dimg
    x = _dev(QR.case("flat_small"))
    with pytest.raises(RuntimeError, match="kernel_size = 0.5"):
        dimg.quickshift_labels(x, kernel_size=0.5)
    with pytest.raises(RuntimeError, match="w = 18"):
        dimg.quickshift_density(x, kernel_size=6)
    with pytest.raises(RuntimeError, match="max_dist = -2"):
        dimg.quickshift_labels(x, max_dist=-2)
    with pytest.raises(RuntimeError, match="ratio = 2"):
        dimg.quickshift_labels(x, ratio=2)
    with pytest.raises(RuntimeError, match="density of shape"):
        dimg.quickshift_parents(x, torch.zeros((3, 3), dtype=torch.int64, device=DEV))
    # scikit-image's defaults (1.0, 5, 10) are the surface's
    assert torch.equal(dimg.quickshift_labels(x), dimg.quickshift_labels(x, 1.0, 5, 10))


# ---- 6. the pipeline -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import enhanced_generator as eg
    torch.manual_seed(11)
    g = eg.EnhancedGenerator(16, 1).to(DEV)
    g.eval()
    return g


def test_pipeline_with_quickshift_equals_the_stages_composed_by_hand(model, tmp_path):
    from PIL import Image
    import enhanced_local_style as E
    from mstg_hip import image as dimg
    h, w = 120, 80
    img_np = ER.smooth_noise(h, w, 4)
    img = _dev(img_np)
    got = dimg.process_enhanced_local_style(model, img, segments=dimg.quickshift_segmenter())
    new_w, new_h, box, back = ER.geometry(w, h)
    resized = dimg.resize_u8(img, (new_w, new_h), dimg.LANCZOS)
    canvas = dimg.paste_u8(resized, (0, 0, new_h, new_w), (256, 256), ((256 - new_h) // 2, (256 - new_w) // 2), fill=0)
    with torch.no_grad():
        styled = dimg.to_u8(model(dimg.to_tensor(canvas).unsqueeze(0))[0])
    labels, count = dimg.quickshift_labels(canvas, 0.5, 3, 6, return_count=True)  # the reference's call
    assert 1 <= int(count) <= 256 * 256 and int(labels.min()) == 0 and int(labels.max()) == int(count) - 1
    m = dimg.segment_blend_map(canvas, labels, num_segments=256 * 256)
    assert torch.equal(m, dimg.segment_blend_map(canvas, labels))  # the bound the host knows drops and changes nothing
    out = dimg.enhanced_style_finish(canvas, styled, m)
    assert box is not None and not back
    out = dimg.crop_u8(out, *box)
    assert got.shape == out.shape and torch.equal(got, out)
    # a callable that returns labels alone, and the keyword's default next to it
    assert torch.equal(got, dimg.process_enhanced_local_style(model, img, segments=lambda c: dimg.quickshift_labels(c, 0.5, 3, 6)))
    assert torch.equal(got, dimg.process_enhanced_local_style(model, img, segments=dimg.quickshift_segmenter(), segmentation="slic"))
    # the slic segmenter is the keyword, and the two segmentations give different images
    slic = dimg.process_enhanced_local_style(model, img, segmentation="slic")
    assert torch.equal(slic, dimg.process_enhanced_local_style(model, img, segments=dimg.slic_segmenter()))
    assert slic.shape == got.shape and not torch.equal(slic, got)
    # labels as an array and None behave as before
    assert torch.equal(got, dimg.process_enhanced_local_style(model, img, segments=labels))
    assert torch.equal(dimg.process_enhanced_local_style(model, img), dimg.process_enhanced_local_style(model, img, segments=None, segmentation="felzenszwalb"))
    # the drop-in's command line writes that image
    Image.fromarray(img_np).save(tmp_path / "in.png")
    torch.save({"G_AB_state_dict": model.state_dict()}, tmp_path / "ckpt.pth")
    base = ["--image", str(tmp_path / "in.png"), "--model", str(tmp_path / "ckpt.pth")]
    E.main(base + ["--output", str(tmp_path / "q.png"), "--device-segmentation", "quickshift"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "q.png")), got.cpu().numpy())
    E.main(base + ["--output", str(tmp_path / "s.png"), "--device-segmentation", "slic", "--segmentation", "felzenszwalb"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "s.png")), slic.cpu().numpy())
