"""The routing of the fp32 convolution passes (which kernel, how much workspace, which fusions) is a pure function of the descriptor
and the switches: no GPU needed.  tests/golden/conv_routes.json holds that table as the commit before the routing was gathered into
one function per file computed it (PROVENANCE_conv_routes.txt: numbers and flags untouched, two families of names corrected); every
later build must reproduce it exactly -- a kernel change that moves a route changes the golden file on purpose, with its own reasons.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_conv_routes", os.path.join(ROOT, "tools", "dump_conv_routes.py"))
dump_conv_routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_conv_routes)

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")))


def test_golden_covers_every_setting_and_case():
    assert list(GOLD) == dump_conv_routes.SETTINGS
    assert list(GOLD["default"]) == [c[0] for c in dump_conv_routes.cases()]


def test_golden_shows_every_route():
    names = {n for rows in GOLD.values() for row in rows.values() for n in row["names"]}
    for stem in ("igemm_light_kernel<4, 1, 2>", "igemm_light_kernel<4, 1, 4>", "igemm_heavy_kernel<", "igemm_stream_kernel<",
                 "conv_img_dgrad_kernel<", "conv_co1_kernel", "conv_p32i_kernel", "conv_p32d_kernel<4, 8>", "conv_p32d_kernel<2, 6>",
                 "conv_p32_kernel<", "wgrad_1x1_kernel<", "wgrad_p32_kernel", "wgrad_ts_kernel<", "wgrad7_kernel<1>", "wgrad7_kernel<2>",
                 "wgrad_kernel<"):
        assert any(n.startswith(stem) for n in names), stem
    # the 1x1 weight gradient in one channel block and in several
    assert GOLD["default"]["1x1 16->48"]["names"][2].startswith("wgrad_1x1") and GOLD["default"][
        "1x1 128->384 (wgrad in 2x2 channel blocks)"]["names"][2].startswith("wgrad_1x1")


@pytest.mark.parametrize("setting", dump_conv_routes.SETTINGS)
def test_routes_match_golden(setting, monkeypatch):
    from mstg_hip import _lib
    lib = _lib.load()
    for k in [k for k in os.environ if k.startswith("MSTG_") and k != "MSTG_LIB"]:
        monkeypatch.delenv(k)
    if setting != "default":
        monkeypatch.setenv(*setting.split("="))
    lib.mstg_env_refresh()
    try:
        got = dump_conv_routes.rows()
    finally:
        monkeypatch.undo()
        lib.mstg_env_refresh()
    for case, row in got.items():
        assert row == GOLD[setting].get(case, GOLD["default"][case]), (setting, case)
