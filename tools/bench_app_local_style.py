"""MI355X: the application's local-style tab (csrc/app_local_style.hip through mstg_hip.image.app_local_style_finish) on a chunk of 64
canvases at 256 x 256 that are already on the device: each stage alone, the chain, the tab end to end, and the host path the
chain replaces.

usage: python tools/bench_app_local_style.py [--n 64] [--seconds 0.5] [--repeats 7] [--host-repeats 3] [--json FILE]

  sky_mask, edge_weight_kernel, point_wise, bilateral   one stage entry alone on the chunk, one launch each (edge_weight_kernel on
                                    a precomputed Canny mask; point_wise with all three blends and the table);
  canny                             mstg_local_style_prepare + mstg_local_style_hysteresis, the two launches in front of the edge weight;
  chain                             app_local_style_finish with the tab's defaults for photo_to_monet: six launches;
  chain_batch1                      the same on one canvas;
  end_to_end                        process_app_local_style_batch with Generator(64).half_inference() on 64 images of 256 x 256:
                                    letterbox, forward in fp16, output conversion, the chain, resize back; ``forward_only`` is
                                    process_cyclegan_batch on the same images;
  host                              what a caller had to do before: device -> host copy of canvases and styled images,
                                    tests/app_local_style_ref.py (numpy; OpenCV is not installed) per canvas, host -> device copy
                                    of the result; ``host_batch1`` the same for one canvas.
The chain's bytes are checked against the host path on the first ``--check`` canvases.  Device timings are device events around
windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends; the host path is wall time around a
call that ends in a synchronise.  Each figure is reported as min / median / max over its repeats.  Prints one JSON line.  Needs a
GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-style-transfer-gan_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from bench_standard_mode import DEV, T, device_stats, wall_stats  # noqa: E402  (the same timing windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--model-type", default="photo_to_monet")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_app_local_style.py needs a GPU")
    import app_local_style_ref as AR
    import local_style_ref as LR
    import plain_generator
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    N, mt = args.n, args.model_type
    gens = [LR.landscape, LR.blocky, LR.gradient_rects, LR.noise]
    canv_np = np.stack([gens[i % 4](T, T, 100 + i) for i in range(N)])
    styled_np = np.ascontiguousarray(255 - canv_np[:, :, ::-1])
    canvas, styled = torch.from_numpy(canv_np).to(DEV), torch.from_numpy(styled_np).to(DEV)
    dev = torch.device(DEV)
    lut, kern = dimg._color_lut(mt, dev), dimg._edge_kernel(dev)
    scratch = torch.empty_like(canvas)
    state, sky_bits, edge, mask = (torch.empty((N, T, T), dtype=torch.uint8, device=DEV) for _ in range(4))
    count = torch.empty(N, dtype=torch.int32, device=DEV)
    weight = torch.empty((N, T, T), dtype=torch.float64, device=DEV)

    def canny():
        _lib.check(lib.mstg_local_style_prepare(_p(canvas), N, T, T, _p(state), _p(sky_bits), _p(count), None, _stream()), "prepare")
        _lib.check(lib.mstg_local_style_hysteresis(_p(state), N, T, T, _p(edge), _stream()), "hysteresis")

    def sky_mask():
        _lib.check(lib.mstg_app_sky_mask(_p(canvas), N, T, T, _p(mask), _stream()), "mstg_app_sky_mask")

    def edge_weight():
        _lib.check(lib.mstg_app_edge_weight(_p(edge), N, T, T, _p(kern), 0.6, _p(weight), _stream()), "mstg_app_edge_weight")

    def point_wise():
        _lib.check(lib.mstg_app_chain(_p(canvas), _p(styled), N, T, T, _p(mask), _p(weight), 1, 0.5, 0.5, _p(lut), _p(scratch), _stream()),
                   "mstg_app_chain")

    def chain(n=N):
        return dimg.app_local_style_finish(canvas[:n], styled[:n], mt)

    def host_path(n=N):
        c, s = canvas[:n].cpu().numpy(), styled[:n].cpu().numpy()
        out = np.stack([AR.app_local_style_finish(c[i], s[i], mt) for i in range(n)])
        return torch.from_numpy(out).to(DEV)

    canny(), sky_mask(), edge_weight()  # the inputs of the later stages
    k = max(1, min(args.check, N))
    same = bool(torch.equal(chain(k), host_path(k)))
    torch.manual_seed(0)
    model = plain_generator.Generator(64).to(DEV).half_inference().eval()
    images = [canvas[i] for i in range(N)]
    stages = {"canny": canny, "sky_mask": sky_mask, "edge_weight_kernel": edge_weight, "point_wise": point_wise,
              "bilateral": lambda: dimg.bilateral_u8(canvas), "chain": chain, "chain_batch1": lambda: chain(1),
              "end_to_end": lambda: dimg.process_app_local_style_batch(model, images, mt),
              "forward_only": lambda: dimg.process_cyclegan_batch(model, images)}
    result = {"N": N, "H": T, "W": T, "model_type": mt, "chain_equals_host_restatement": same, "checked_canvases": k}
    for name, fn in stages.items():
        result[name] = device_stats(fn, args.seconds, args.repeats)
    result["host_batch1"] = wall_stats(lambda: host_path(1), args.host_repeats)
    result["host"] = wall_stats(host_path, args.host_repeats)
    result["host_over_chain"] = result["host"]["median_ms"] / result["chain"]["median_ms"]
    result["host_over_chain_batch1"] = result["host_batch1"]["median_ms"] / result["chain_batch1"]["median_ms"]
    px = N * T * T
    result["sky_mask_bytes_per_s"] = px * 4 / (result["sky_mask"]["median_ms"] * 1e-3)            # 3 bytes read, 1 written per pixel
    result["edge_weight_bytes_per_s"] = px * 9 / (result["edge_weight_kernel"]["median_ms"] * 1e-3)  # 1 byte read, 8 written
    result["point_wise_bytes_per_s"] = px * 18 / (result["point_wise"]["median_ms"] * 1e-3)       # 3 + 3 + 1 + 8 read, 3 written
    result["end_to_end_images_per_s"] = N / (result["end_to_end"]["median_ms"] * 1e-3)
    result["forward_only_images_per_s"] = N / (result["forward_only"]["median_ms"] * 1e-3)
    for key in list(stages) + ["host_batch1", "host"]:
        r = result[key]
        print(f"{key:20s} {r['median_ms']:12.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]", file=sys.stderr)
    print(f"host / chain = {result['host_over_chain']:.0f}x (batch 1: {result['host_over_chain_batch1']:.0f}x)   chain equal: {same}   "
          f"sky {result['sky_mask_bytes_per_s'] / 1e9:.1f} GB/s, edge weight {result['edge_weight_bytes_per_s'] / 1e9:.1f} GB/s, "
          f"point-wise {result['point_wise_bytes_per_s'] / 1e9:.1f} GB/s", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
