#!/usr/bin/env python
"""Simplified polygons: the device route (count, trace and vpu_outline_simplify_batched behind ``DeviceOutlineOps.trace(items,
tolerance)``, three read-backs, only the kept corners cross) against the route it replaces (the exact device trace, two
read-backs, then ``host_simplify`` on the host), in one process on the six maps of tools/bench_outlines.py (ellipse_holes,
eight_ellipses and model at 480 x 640 and 1024 x 1365) at tolerances 0.5, 1 and 2 pixels.

Per map and tolerance both routes are alternated after a warm-up of each; the figure is the median over ``--ops`` operations of
the time between two device events around the operation, read-backs and host work included.  Both routes must give the same
points.  Also recorded: the vertices and bytes that cross to the host, the rounds the longest-running loop took, the
intersection over union of the simplified polygons filled again (even-odd, at pixel centres) with the mask -- reported, not
gated -- and, on the model maps, the launches of one simplify call alone with form A and with form B for the short loops,
alternated.  Prints one JSON line and writes it to ``--out`` (default profiles/simplify.json).
usage: python tools/bench_simplify.py [--ops N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_outlines as bo                                                    # noqa: E402
from pvpuformer_amd import ops                                                 # noqa: E402
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool            # noqa: E402
from pvpuformer_amd.isegm.inference.outlines import DeviceOutlineOps, _binary   # noqa: E402
from pvpuformer_amd.isegm.inference.polygons import host_simplify, quantise, same_polygons, simplify_loops   # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import vitb_model_kwargs                             # noqa: E402

TOLERANCES = [0.5, 1.0, 2.0]


def fill(polygons):
    """bool [H, W]: the pixels whose centres lie inside the loops, even-odd, holes included."""
    H, W = polygons.size
    flips = np.zeros((H, W + 1), dtype=np.int32)
    for loop in polygons.loops():
        p = loop.astype(np.float64)
        q = np.roll(p, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(p, q):
            if y0 == y1:
                continue
            rows = np.arange(int(min(y0, y1)), int(max(y0, y1)))           # the centres y = r + 0.5 the edge passes
            x = x0 + (rows + 0.5 - y0) * (x1 - x0) / (y1 - y0)
            cols = np.clip(np.ceil(x - 0.5).astype(np.int64), 0, W)        # the first pixel whose centre lies beyond the edge
            np.add.at(flips, (rows, cols), 1)
    return (np.cumsum(flips, axis=1)[:, :W] % 2) == 1


def iou(a, b):
    union = int((a | b).sum())
    return 1.0 if union == 0 else round(int((a & b).sum()) / union, 6)


def alternate(first, second, n):
    """Median milliseconds of two routes, alternated, after three warm-up turns of each, and the spread inside this run: the
    10th and 90th percentiles."""
    times = ([], [])
    for turn in range(n + 3):
        a, b = bo.span(first), bo.span(second)
        if turn >= 3:
            times[0].append(a)
            times[1].append(b)
    return [{"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4),
             "p90": round(float(np.percentile(v, 90)), 4)} for v in times]


def routes(tracer, items, masks, tolerance, n):
    k, keep = len(items), {}

    def device():
        keep["device"] = tracer.trace(items, tolerance)

    def host():
        keep["exact"] = tracer.trace(items)
        keep["host"] = [host_simplify(o, tolerance) for o in keep["exact"]]

    times = dict(zip(("device", "host"), alternate(device, host, n)))
    assert all(same_polygons(d, h) for d, h in zip(keep["device"], keep["host"]))
    exact, got = keep["exact"], keep["device"]
    V, L = sum(len(o.points) for o in exact), sum(len(o) for o in exact)
    kept, alive = sum(len(p.points) for p in got), sum(len(p) for p in got)
    t = quantise(tolerance)
    return {"ms": times, "vertices": [V, kept], "loops": [L, alive],
            "rounds": max([simplify_loops(o.points, o.offsets, t)[3] for o in exact if len(o)] or [0]),
            "bytes_to_host": {"device": 4 * (k + 1) + ((12 * (k + 1) + 16) + 8 * kept + 4 * (alive + 1) + alive if V else 0),
                              "host": 4 * (k + 1) + (4 * (2 * V + V // 4 + 1 + k + 1) if V else 0)},
            "iou": [iou(fill(p), m) for p, m in zip(got, masks)] if k == 1 else round(float(np.mean([iou(fill(p), m) for p, m in zip(got, masks)])), 6)}


def forms_alone(tracer, items, tolerance, n):
    """The launches of one simplify call on the trace's device outputs, form A against form B for the short loops, alternated."""
    exact = tracer.trace(items)
    k = len(items)
    V, L = sum(len(o.points) for o in exact), sum(len(o) for o in exact)
    starts = np.concatenate(([0], np.cumsum([len(o.points) for o in exact])))
    points = torch.from_numpy(np.concatenate([o.points for o in exact])).cuda()
    loop_max = V // 4
    offsets = torch.zeros(loop_max + 1, dtype=torch.int32, device="cuda")
    offsets[:L + 1] = torch.from_numpy(np.concatenate([o.offsets[:-1] + s for o, s in zip(exact, starts)] + [[V]]).astype(np.int32)).cuda()
    item_loops = torch.from_numpy(np.concatenate(([0], np.cumsum([len(o) for o in exact]))).astype(np.int32)).cuda()
    work = torch.empty(ops.outline_simplify_work_len(V, loop_max), device="cuda", dtype=torch.int32)
    out_points = torch.empty(V, 2, device="cuda", dtype=torch.int32)
    out_offsets = torch.empty(loop_max + 2, device="cuda", dtype=torch.int32)
    out_hole = torch.empty(loop_max + 1, device="cuda", dtype=torch.uint8)
    firsts = torch.empty(2 * (k + 1) + 4, device="cuda", dtype=torch.int32)
    t = quantise(tolerance)

    def run(form):
        ops.outline_simplify_batched(points, offsets, item_loops, k, V, loop_max, t, work, out_points, out_offsets, out_hole, firsts,
                                     loop_cap=loop_max + 1, short_form=form)

    a, b = alternate(lambda: run(ops.SIMPLIFY_FORM_A), lambda: run(ops.SIMPLIFY_FORM_B), n)
    short = sum(int((np.diff(o.offsets) <= ops.SIMPLIFY_SHORT).sum()) for o in exact)
    return {"form_a_ms": a, "form_b_ms": b, "loops": L, "short_loops": short, "corners": V,
            "tolerance": tolerance}


def measure(ann, tracer, H, W, n):
    res = {}
    prob = torch.from_numpy(bo.ellipse_with_holes(H, W)).cuda()
    labels = torch.from_numpy(bo.blob_labels(H, W).view(np.int16)).cuda()
    aid = ann.open(bo.image_of(H, W, seed=H))
    ann.click({aid: (True, (H // 2, W // 2))})
    model = ann.pool.probs(aid)[0, 0].clone()
    maps = {"ellipse_holes": [(prob, 0, bo.THR, 0)], "eight_ellipses": [(labels, 1, 0.0, k) for k in range(1, 9)],
            "model": [(model, 0, ann.pool.pred_thr, 0)]}
    for name, items in maps.items():
        masks = [_binary(t.cpu().numpy(), kind, thr, label) for t, kind, thr, label in items]
        res[name] = {str(tol): routes(tracer, items, masks, tol, n) for tol in TOLERANCES}
    res["model"]["forms"] = forms_alone(tracer, maps["model"], 1.0, n)
    ann.close(aid)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_simplify: --ops must be at least 30")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    predictor = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    ann = AnnotationPool(predictor, max_images=1)
    tracer = DeviceOutlineOps("cuda")
    line = {"bench": "simplify", "model": "vitb448", "dtype": "bf16", "flip": True, "ops_per_route": args.ops,
            "threads": ops.SIMPLIFY_THREADS, "short": ops.SIMPLIFY_SHORT, "short_form": "AB"[ops.SIMPLIFY_SHORT_FORM],
            "statistic": "median (and 10th / 90th percentile) ms between device events around the operation, read-backs included; routes alternated (device "
                         "first, then host, per turn); forms: the launches of one simplify call alone, A first, then B",
            "sizes": {f"{H}x{W}": measure(ann, tracer, H, W, args.ops) for H, W in bo.SIZES},
            "not_measured": "other workgroup sizes, a short-loop limit other than 64, several sessions per trace, pinned host buffers, "
                            "a Douglas-Peucker in C on the host (none ships here), the spread between runs"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
