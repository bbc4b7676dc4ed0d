#!/usr/bin/env python
"""Region clean-up: the device route of ``tidy`` (vpu_regions_tidy_batched through ``DeviceRegionOps``) against the host route
it replaces (``HostRegionOps``: the fp32 map copied to the host, ``host_regions_tidy`` with scipy's labelling, the edited map
copied back up), in one process on the same map.  No network is involved: the map is synthetic, one fp32 probability map per
image size, written in place as ``SessionPool.tidy`` does.

Two maps per size: "speckled", a filled ellipse with pinholes and a few hundred specks around it (what a predicted mask looks
like before clean-up), and "checkerboard", the same with a checkerboard band across the middle, every clear cell of which is a
4-connected region of its own: the worst case for per-component bookkeeping.  Both routes alternated after three warm-up turns
of each; the median over ``--ops`` operations of the time between two device events around the operation, its read-back
included (the device is idle at the first event, so the span covers the host's own work too).  The map is restored (untimed)
before every operation.  Prints one JSON line and writes it to ``--out`` (default profiles/tidy.json).
usage: python tools/bench_tidy.py [--ops N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvpuformer_amd.isegm.inference.regions import DeviceRegionOps, HostRegionOps, TidyItem      # noqa: E402

SIZES = [(480, 640), (1024, 1365)]
THR = 0.49
PARAMS = dict(min_area=32, max_hole=32, keep="all")


def map_of(H, W, kind, seed):
    """fp32 [H, W]: an ellipse of high values with pinholes, specks of 1 .. 9 pixels around it, and for "checkerboard" a band of
    H / 8 rows of alternating pixels across the middle."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    on = ((yy - H // 2) / (0.3 * H)) ** 2 + ((xx - W // 2) / (0.3 * W)) ** 2 <= 1.0
    on &= rs.rand(H, W) > 0.002                                 # pinholes
    for _ in range(300):                                        # specks
        r, c, h, w = rs.randint(H - 3), rs.randint(W - 3), rs.randint(1, 4), rs.randint(1, 4)
        on[r:r + h, c:c + w] = True
    if kind == "checkerboard":
        band = slice(H // 2 - H // 16, H // 2 + H // 16)
        on[band] = ((yy + xx) % 2 == 0)[band]
    return np.where(on, 0.55 + 0.4 * rs.rand(H, W), 0.4 * rs.rand(H, W)).astype(np.float32)


def span(op):
    """Milliseconds between device events around ``op()``; the device is idle before the first."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    op()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(H, W, kind, ops):
    source = torch.from_numpy(map_of(H, W, kind, seed=H)).cuda()
    work = source.clone()
    routes = {"device": DeviceRegionOps("cuda"), "host": HostRegionOps()}
    seeds = [(H // 2, W // 2, True)]
    times, got = {name: [] for name in routes}, {}
    for turn in range(ops + 3):                                 # three warm-up turns of each route
        for name, route in routes.items():
            work.copy_(source)
            item = TidyItem(H, W, add=work, add_out=work, seeds=seeds, **PARAMS)
            t = span(lambda: got.__setitem__(name, route.tidy([item], THR, "masks")[0]))
            got[name + " map"] = work.clone()
            if turn >= 3:
                times[name].append(t)
    (rec_d, mask_d), (rec_h, mask_h) = got["device"], got["host"]
    assert np.array_equal(rec_d, rec_h) and np.array_equal(mask_d, mask_h) and torch.equal(got["device map"], got["host map"])
    res = {name + "_ms": round(statistics.median(ts), 4) for name, ts in times.items()}
    res["host_over_device"] = round(res["host_ms"] / res["device_ms"], 2)
    res["record"] = dict(area=int(rec_d[0]), removed=int(rec_d[1]), filled=int(rec_d[2]), kept_components=int(rec_d[7]))
    res["bytes_to_host"] = {"device": (H * W + 63) // 64 * 8 + 32, "host": 4 * H * W}
    res["bytes_to_device"] = {"device": 96 + 12 * len(seeds), "host": 4 * H * W}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tidy.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tidy: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_tidy: --ops must be at least 30")
    line = {"bench": "tidy", "thr": THR, "params": PARAMS, "ops_per_route": args.ops,
            "statistic": "median ms between device events around the operation, read-back included; routes alternated",
            "sizes": {f"{H}x{W}": {kind: measure(H, W, kind, args.ops) for kind in ("speckled", "checkerboard")} for H, W in SIZES},
            "not_measured": "several maps per launch, the kernels one by one, pinned host buffers for the host route's copies; the "
                            "kernels are untuned and this is a single run"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
