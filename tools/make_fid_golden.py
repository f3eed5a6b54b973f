"""Writes tests/golden/fid_cases.npz: the results of the REFERENCE'S OWN ``calculate_fid`` (its m_test.py, imported by path) on
the seeded draws of tests/fid_ref.py.  Results only: the inputs are regenerated from the seeds by the test, and no text of the
reference is stored.  Runs only where a checkout of the reference exists; the test-suite reads the stored file.

usage: python tools/make_fid_golden.py --reference DIR     (DIR holds the reference's m_test.py)

The reference's module imports torchvision, cv2, matplotlib, tqdm and two of its own modules at the top; none of them takes part
in ``calculate_fid`` (numpy and scipy.linalg do), so whatever is missing here is replaced by an empty placeholder module."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLACEHOLDERS = {"torchvision": (), "torchvision.models": ("inception_v3", "Inception_V3_Weights"), "torchvision.transforms": (),
                "cv2": (), "matplotlib": (), "matplotlib.pyplot": (), "tqdm": ("tqdm",), "pretrain": ("MonetPhotoDataset",),
                "enhanced_train": ("EnhancedCycleGAN",)}


def load_reference(directory):
    for name, attrs in PLACEHOLDERS.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_m_test", os.path.join(directory, "m_test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    """(name, x1, x2) in the order stored: the shapes of fid_ref.CASES in float32 and float64, then the two special draws"""
    import fid_ref as FR
    out = []
    for n1, n2, d in FR.CASES:
        if d < 2:
            continue  # np.cov of one feature is a scalar and the reference's sqrtm refuses it
        for dt in (np.float32, np.float64):
            out.append((f"{(n1, n2, d)} {dt.__name__}",) + FR.draw(n1, n2, d, 7 + n1 + d, dt))
    x1, x2 = FR.draw(48, 40, 13, 5, np.float64)
    x1[:, 4] = 0.25
    x2[:, 4] = 0.25
    y1, _ = FR.draw(24, 24, 64, 3, np.float64)
    return out + [("constant column", x1, x2), ("identical sets", y1, y1.copy())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference's m_test.py")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    names, fids = [], []
    for name, x1, x2 in cases():
        names.append(name)
        fids.append(float(ref.calculate_fid(x1, x2)))
        print(f"{name}: {fids[-1]!r}")
    import scipy
    out = os.path.join(ROOT, "tests", "golden", "fid_cases.npz")
    np.savez(out, names=np.array(names), fid=np.array(fids, np.float64), numpy_version=np.array(np.__version__),
             scipy_version=np.array(scipy.__version__))
    print(out)


if __name__ == "__main__":
    main()
