#!/usr/bin/env python
"""Tiled prediction: per-click latency of a ``BasePredictor`` whose input is cut into 448 x 448 tiles by ``Crops``, ViT-B/448
bf16, flip TTA, synthetic images (pvpuformer_amd.synth).  Rows:

* ``zoom672``: ZoomIn to 672 x 672 cut into 4 tiles (8 network rows), beside the plain 672 x 672 forward (2 rows);
* ``zoom896``: ZoomIn to 896 x 896 cut into 9 tiles (18 rows), beside the plain 896 x 896 forward;
* ``whole1024x1365``: a 1024 x 1365 image without ZoomIn, 12 tiles (24 rows); no plain forward exists for it (not square).

Every row runs three variants on the same images and click scripts, alternated session by session in one process after a
warm-up of each variant's shapes: ``device`` (the ``vpu_crops_gather`` / ``vpu_crops_blend`` kernels), ``standin`` (the torch
restatement of the reference's transform, tests/crops_cases.py: one slice per tile, a float64 coverage map built in numpy and
uploaded per click) and ``plain`` (no tiling).  A click is one ``get_prediction`` call, timed with device events around it (the
call ends in a device-to-host copy of the map, so the window is complete); reported: median and mean milliseconds per click
over all timed clicks, and from a pass of its own the share of a click's device time between the start of the gather / blend
call and its end (events around the two operations).  Nothing is asserted; one JSON line is printed and written to ``--out``
(default profiles/tiled_predict.json).

usage: python tools/bench_tiled.py [--sessions N] [--clicks C] [--rows NAME ...] [--out FILE]"""
import argparse
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crops_cases                                                             # noqa: E402
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker              # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import BasePredictor            # noqa: E402
from pvpuformer_amd.isegm.inference.transforms import Crops, ZoomIn, _device   # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import synth_batch, vitb_model_kwargs                # noqa: E402

TILE = 448
ROWS = {  # name: (image (H, W), ZoomIn target side or None, tiles expected)
    "zoom672": ((480, 640), 672, 4),
    "zoom896": ((720, 960), 896, 9),
    "whole1024x1365": ((1024, 1365), None, 12),
}


def make_session(H, W, clicks, seed):
    """(uint8 image [H, W, 3], [(positive, row, col)]): a synthetic object, a positive click inside it, then seeded clicks."""
    b = synth_batch(1, max(H, W), seed=seed)
    image = (b["images"][0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    rows, cols = np.nonzero(b["instances"][0, 0, :H, :W].numpy() > 0)
    first = (int(np.median(rows)), int(np.median(cols))) if len(rows) else (H // 2, W // 2)
    rs = np.random.RandomState(seed)
    return image, [(True,) + first] + [(bool(k % 2 == 0), int(rs.randint(H)), int(rs.randint(W))) for k in range(1, clicks)]


def predictor(model, variant, side):
    zoom = None if side is None else ZoomIn(target_size=(side, side), skip_clicks=-1)
    crops = {"device": Crops, "standin": crops_cases.StandInCrops}[variant](crop_size=(TILE, TILE)) if variant != "plain" else None
    return BasePredictor(model, "cuda", with_flip=True, zoom_in=zoom, crops=crops)


def run_session(pred, image, script):
    """-> milliseconds of every click of the script (device events around ``get_prediction``)."""
    pred.set_input_image(image)
    clicker = Clicker(device=None)
    out = []
    for positive, r, c in script:
        clicker.add_click(Click(positive, (r, c)))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pred.get_prediction(clicker)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def transform_share(pred, variant, image, script):
    """Share of the clicks' device time spent between the start and the end of the gather and blend calls."""
    spans = []

    def timed(fn):
        def call(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            spans.append((s, e))
            return out
        return call
    where = _device if variant == "device" else crops_cases
    names = ("crops_gather", "crops_blend") if variant == "device" else ("host_gather", "host_blend")
    with mock.patch.object(where, names[0], timed(getattr(where, names[0]))), \
            mock.patch.object(where, names[1], timed(getattr(where, names[1]))):
        total = sum(run_session(pred, image, script))
    assert len(spans) == 2 * len(script)
    return sum(s.elapsed_time(e) for s, e in spans) / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=6)
    ap.add_argument("--clicks", type=int, default=10)
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_predict.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled: needs a GPU (nothing here is measured without one)")
    if args.sessions * args.clicks < 50:
        raise SystemExit("bench_tiled: at least 50 timed clicks per variant (--sessions x --clicks)")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    res = {}
    for name in args.rows:
        (H, W), side, tiles = ROWS[name]
        variants = ["device", "standin"] + (["plain"] if side is not None else [])
        preds = {v: predictor(model, v, side) for v in variants}
        data = [make_session(H, W, args.clicks, seed=500 + i) for i in range(args.sessions)]
        for v in variants:                                   # warm-up: this variant's shapes and row counts
            run_session(preds[v], data[0][0], data[0][1][:3])
            if v != "plain":
                assert preds[v].crops.num_tiles == tiles, (name, v, preds[v].crops.num_tiles)
        ms = {v: [] for v in variants}
        for image, script in data:                           # alternated session by session
            for v in variants:
                ms[v] += run_session(preds[v], image, script)
        row = {"image": [H, W], "zoom_target": side, "tiles": tiles, "network_rows": 2 * tiles, "clicks_timed": len(ms["device"])}
        for v in variants:
            row[v] = {"ms_per_click_median": round(float(np.median(ms[v])), 3), "ms_per_click_mean": round(float(np.mean(ms[v])), 3)}
            if v != "plain":
                row[v]["gather_blend_share"] = round(transform_share(preds[v], v, *data[0]), 4)
        if "plain" in variants:
            row["device_over_plain"] = round(row["device"]["ms_per_click_median"] / row["plain"]["ms_per_click_median"], 3)
        row["device_over_standin"] = round(row["device"]["ms_per_click_median"] / row["standin"]["ms_per_click_median"], 3)
        res[name] = row
    line = {"bench": "tiled_predict", "model": "vitb448", "dtype": "bf16", "tile": TILE, "flip": True, "sessions": args.sessions,
            "clicks_per_session": args.clicks, "rows": res}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
