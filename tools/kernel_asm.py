#!/usr/bin/env python3
"""Dump the gfx950 assembly of every csrc/*.hip to OUTDIR/<name>.s, compiled with exactly the flags of mstg_hip/build.py
(MSTG_HIPCC_FLAGS and the per-source switches included).  Needs no GPU.  A refactor that must not change a kernel is checked by

    python tools/kernel_asm.py before/     # in a checkout of the parent
    python tools/kernel_asm.py after/      # in the branch
    diff -r before after

The lines that carry the __hip_cuid_<hash> symbol (a hash of the source text) are dropped.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multi-style-transfer-gan_amd"))
from mstg_hip import build  # noqa: E402


def dump(src, outdir):
    cmd = build.compile_cmd(src) + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    with open(os.path.join(outdir, os.path.basename(src)[:-4] + ".s"), "w") as f:
        f.writelines(ln for ln in asm.splitlines(keepends=True) if "__hip_cuid_" not in ln)


if __name__ == "__main__":
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(lambda s: dump(s, outdir), build.sources()))
