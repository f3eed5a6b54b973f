"""The routing of the fused MultiScaleBlock and LocalAttention passes (which kernel, how much workspace) is a pure function of the
shape, the width and the switches: no GPU needed.  tests/golden/fused_routes.json holds what the commit before the routing was
gathered into one function per family did (PROVENANCE_fused_routes.txt): the answers of its workspace queries, and the kernel symbols
each pass launched on the GPU.  Every later build must answer the same workspace bytes, and its name queries must name a kernel of
that pass's launch list -- a kernel change that moves a route changes the golden file on purpose, with its own reasons.
tests/test_gpu_ops.py compares the launches themselves against the same file.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_fused_routes", os.path.join(ROOT, "tools", "dump_fused_routes.py"))
dump_fused_routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_fused_routes)

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "fused_routes.json")))


def test_golden_covers_every_setting_and_case():
    assert list(GOLD) == dump_fused_routes.SETTINGS
    assert list(GOLD["default"]) == [c[0] for c in dump_fused_routes.cases()]


def test_golden_shows_every_route():
    names = {n for rows in GOLD.values() for row in rows.values() for launches in row["launches"] for n in launches}
    stems = ["ms_fwd_kernel<", "ms_fwd4_kernel<", "ms_fwd4b_kernel<", "ms_dgrad_kernel<", "wgrad_ms_kernel<", "wgrad_msp_kernel<",
             "wgrad_ms_sync_kernel<", "wgrad_msp_sync_kernel<"]
    stems += [f"attn_core_{d}{k}_kernel<" for d in ("fwd", "bwd") for k in ("", "_blk", "_blk4")]
    for stem in stems:
        assert any(n.startswith(stem) for n in names), stem
    for stem in [f"attn_{k}_{d}_kernel<" for k in ("reg", "big", "fused") for d in ("fwd", "bwd")]:
        for norm in (", true", ", false"):  # <C, NORM> / <C, NORM, WAVES>
            assert any(n.startswith(stem) and norm in n for n in names), stem + norm


@pytest.mark.parametrize("setting", dump_fused_routes.SETTINGS)
def test_routes_match_golden(setting, monkeypatch):
    from mstg_hip import _lib
    lib = _lib.load()
    for k in [k for k in os.environ if k.startswith("MSTG_") and k != "MSTG_LIB"]:
        monkeypatch.delenv(k)
    for kv in setting.split(",") if setting != "default" else []:
        monkeypatch.setenv(*kv.split("="))
    lib.mstg_env_refresh()
    try:
        got = {case: (dump_fused_routes.workspaces(family, shape), dump_fused_routes.names(family, shape))
               for case, family, shape in dump_fused_routes.cases()}
    finally:
        monkeypatch.undo()
        lib.mstg_env_refresh()
    for case, (ws, names) in got.items():
        want = GOLD[setting].get(case, GOLD["default"][case])
        assert ws == want["ws"], (setting, case)
        if not want["launches"]:  # a width without a fused path
            assert set(names) == {""} and set(ws) == {0}, (setting, case, names)
            continue
        for ps, name in enumerate(names):
            assert name in want["launches"][ps], (setting, case, ps, name)
