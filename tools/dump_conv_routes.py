"""Routing table of the fp32 convolution passes: for every entry of CONV_CASES and STREAM_CASES (tests/test_gpu_ops.py) the kernel
names of the three passes, the two workspace queries and the four fusion probes, under the default switches and under each switch
of SETTINGS.  The queries need no GPU.  The switches are read when the library is loaded, so every setting gets a child process.

usage: dump_conv_routes.py [-o FILE]     (MSTG_LIB selects another build of the library)

Output (what tests/golden/conv_routes.json holds and tests/test_conv_routes.py compares against):
    {"default": {case: row}, "<SWITCH>=<value>": {case: row, only where it differs from the default row}, ...}
    row = {"names": [fwd, dgrad, wgrad], "ws": bytes, "wgrad_ws": bytes,
           "probes": [fwd_norm_supported, fwd_stats_pays, dgrad_bsums_supported, wgrad_norm_supported]}
"""
import ast
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-style-transfer-gan_amd")]

SETTINGS = ["default", "MSTG_P32=0", "MSTG_WGRAD_OLD=1", "MSTG_WGRAD_1X1=0", "MSTG_WGRAD_PLAIN=1", "MSTG_NO_DPACK=1", "MSTG_CONV_IMG=0",
            "MSTG_STREAM=1f", "MSTG_IGEMM=h", "MSTG_P32_TH=4"]
PROBES = ["mstg_conv2d_fwd_norm_supported", "mstg_conv2d_fwd_stats_pays", "mstg_conv2d_dgrad_bsums_supported",
          "mstg_conv2d_wgrad_norm_supported"]


def cases():
    """CONV_CASES + STREAM_CASES, read from the test module's source (importing it would pull in torch and pytest)."""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_ops.py")).read())
    found = {n.targets[0].id: ast.literal_eval(n.value) for n in tree.body
             if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in ("CONV_CASES", "STREAM_CASES")}
    return found["CONV_CASES"] + found["STREAM_CASES"]


def desc_of(case):
    from mstg_hip._lib import ConvDesc
    _, N, H, W, Cin, Cout, k, s, p, d, tr, x_nchw, y_nchw, act = case
    Ho, Wo = (2 * H, 2 * W) if tr else ((H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1)
    return ConvDesc(N, H, W, Cin, Ho, Wo, Cout, k, k, s, p, d, tr, x_nchw, y_nchw, Cin, 0, Cout, 0, act, 0)


def rows():
    """{case: row} under the switches this process was started with."""
    from mstg_hip import _lib
    lib = _lib.load()
    out = {}
    for case in cases():
        d = ctypes.byref(desc_of(case))
        out[case[0]] = {"names": [lib.mstg_conv2d_kernel_name(d, ps).decode() for ps in (0, 1, 2)],
                        "ws": lib.mstg_conv2d_workspace_bytes(d), "wgrad_ws": lib.mstg_conv2d_wgrad_workspace_bytes(d),
                        "probes": [getattr(lib, p)(d) for p in PROBES]}
    return out


def dump():
    table = {}
    for setting in SETTINGS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("MSTG_") or k == "MSTG_LIB"}
        if setting != "default":
            env.update([setting.split("=")])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE, text=True)
        got = json.loads(r.stdout)
        table[setting] = got if setting == "default" else {c: row for c, row in got.items() if row != table["default"][c]}
    return table


if __name__ == "__main__":
    if "--child" in sys.argv:
        print(json.dumps(rows()))
    else:
        text = json.dumps(dump(), indent=1)
        if "-o" in sys.argv:
            open(sys.argv[sys.argv.index("-o") + 1], "w").write(text + "\n")
        else:
            print(text)
