"""MI355X: folder inference and data loading through the batched image pipeline (csrc/image_batch.hip,
mstg_hip.image.process_cyclegan_batch / dataset_batch) against the per-image functions, on 64 seeded synthetic images of mixed
sizes and orientations (already decoded and on the device: file decode / encode is host I/O outside this library).

usage: python tools/bench_image_batch.py [--seconds 0.4] [--rounds 5] [--json FILE]

Per model -- ``Generator(64).half_inference()``, ``EnhancedGenerator(16, 1).half_inference(fp16_blocks=True)`` and an identity
model (the pre / post stages alone) -- the variants are: the per-image loop over ``process_cyclegan`` and
``process_cyclegan_batch`` at batch 1 / 16 / 64.  The pipeline is host-bound at small batches, so the time is host wall time
around whole passes over the 64 images with a device synchronise at both ends; a window repeats the pass until ``--seconds`` are
filled, the variants alternate inside each of ``--rounds`` rounds in one process, and the median / min / max over the rounds
are reported, after one warm-up pass of every variant.  Outputs of the loop and of every batch size are compared byte for byte.
The loader part times ``DeviceLoader(batch_size=32)`` epochs over the same images with and without ``get_batch``.
Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multi-style-transfer-gan_amd"), ROOT):
    sys.path.insert(0, p)

DEV = "cuda:0"
N_IMAGES = 64


def make_images(seed=2024):
    """64 images: portrait, landscape and square, 160..1000 pixels a side, two above the 1024 x 1024 no-resize-back limit"""
    rs = np.random.RandomState(seed)
    sizes = [(256, 256), (512, 512), (1100, 1000), (1000, 1100)]
    while len(sizes) < N_IMAGES:
        h, w = int(rs.randint(160, 1001)), int(rs.randint(160, 1001))
        sizes.append((h, w))
    out = []
    for h, w in sizes:
        base = rs.randint(0, 256, size=(h // 8 + 2, w // 8 + 2, 3)).astype(np.uint8)
        out.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]))
    return out


def timed_pass(fn, passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / passes


def compare(variants, seconds, rounds):
    """variants: name -> callable doing one pass; returns name -> {s, min_s, max_s, passes_per_window}"""
    passes = {}
    for name, fn in variants.items():
        fn()  # warm-up: code objects, plans, allocator
        passes[name] = max(1, int(seconds / max(timed_pass(fn, 1), 1e-6)) + 1)
    samples = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            samples[name].append(timed_pass(fn, passes[name]))
    return {name: {"s": statistics.median(v), "min_s": min(v), "max_s": max(v), "passes_per_window": passes[name]}
            for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_batch.py needs a GPU")
    import enhanced_generator
    import plain_generator
    import pretrain
    from mstg_hip import image as dimg
    arrays = make_images()
    images = dimg.upload_u8(arrays, DEV)
    torch.manual_seed(0)
    models = {
        "plain_c64_f16": plain_generator.Generator(64).to(DEV).half_inference().eval(),
        "enhanced_c16_b1_f16": enhanced_generator.EnhancedGenerator(16, 1).to(DEV).half_inference(fp16_blocks=True).eval(),
        "identity": lambda x: x,
    }
    result = {"images": N_IMAGES, "target": 256, "pixels": int(sum(a.shape[0] * a.shape[1] for a in arrays)), "models": {}}
    for mname, model in models.items():
        variants = {"loop": lambda: [dimg.process_cyclegan(model, im) for im in images]}
        for bs in (1, 16, 64):
            variants[f"batch{bs}"] = (lambda bs=bs: dimg.process_cyclegan_batch(model, images, batch_size=bs))
        ref = variants["loop"]()
        same = {name: all(torch.equal(a, b) for a, b in zip(ref, fn())) for name, fn in variants.items() if name != "loop"}
        rows = compare(variants, args.seconds, args.rounds)
        for name, r in rows.items():
            r["images_per_s"] = N_IMAGES / r["s"]
            r["speedup_over_loop"] = rows["loop"]["s"] / r["s"]
            if name in same:
                r["bytes_equal_loop"] = same[name]
            print(f"{mname:22s} {name:8s} {r['s'] * 1e3:9.2f} ms / 64 images [{r['min_s'] * 1e3:.2f} .. {r['max_s'] * 1e3:.2f}]  "
                  f"{r['images_per_s']:9.0f} images/s  x{r['speedup_over_loop']:.2f}  equal={same.get(name, '-')}", file=sys.stderr)
        result["models"][mname] = rows

    class ItemOnly:  # the same dataset without get_batch: DeviceLoader falls back to stacking items
        def __init__(self, ds):
            self.ds = ds

        def __len__(self):
            return len(self.ds)

        def __getitem__(self, i):
            return self.ds[i]

    ds = pretrain.MonetPhotoDataset(arrays=arrays, device=DEV, img_size=256)
    loaders = {"get_batch": pretrain.DeviceLoader(ds, batch_size=32, shuffle=True),
               "items": pretrain.DeviceLoader(ItemOnly(ds), batch_size=32, shuffle=True)}
    random.seed(1)
    rows = compare({name: (lambda ld=ld: list(ld)) for name, ld in loaders.items()}, args.seconds, args.rounds)
    for name, r in rows.items():
        r["batches_per_s"] = len(loaders[name]) / r["s"]
        print(f"DeviceLoader batch 32  {name:10s} {r['s'] * 1e3:9.2f} ms / epoch of 64 [{r['min_s'] * 1e3:.2f} .. {r['max_s'] * 1e3:.2f}]  "
              f"{r['batches_per_s']:8.1f} batches/s", file=sys.stderr)
    result["loader_batch32"] = rows
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
