#!/usr/bin/env python
"""Multi-object annotation: the device compose of ``AnnotationPool`` (vpu_annot_compose_batched) against the host route it
replaces, in one process on the same object.  ViT-B/448 bf16, flip TTA, ZoomIn to 448 x 448; per image size one annotation
whose object has parts (a click and a partial finish) and a prediction (a second click), so both maps are in play.

Per operation, both routes alternated after a warm-up of each, the median over ``--ops`` operations of the time between two
device events around the operation, its read-back included (the device is idle at the first event, so the span covers the
host's own work too):

* mask: R1's mask, what a click on an object with parts costs beyond the pool -- device: one compose launch, the packed
  mask back (H * W / 8 bytes); host: ``probs`` and parts copied to the host (4 * H * W bytes each), ``np.maximum``, ``>``;
* preview: R2's label map -- device: ``label_map(preview=True)`` (a copy of the labels, one launch, 2 * H * W bytes back);
  host: the two copies, ``np.maximum``, ``>`` and the assignment into a copy of the host's label map;
* partial_finish: R4's parts = current -- device: ``partially_finish`` (no read-back); host: the two copies and ``np.maximum``;
* finish: R5 -- device: ``finish`` (one launch, 32 bytes back); host: the two copies, ``np.maximum``, ``>``, the assignment.

After each timed partial finish or finish the object is put back (untimed).  Prints one JSON line and writes it to ``--out``
(default profiles/annotation.json).
usage: python tools/bench_annotation.py [--ops N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool            # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import vitb_model_kwargs                             # noqa: E402

SIZES = [(480, 640), (1024, 1365)]


def image_of(H, W, seed):
    """uint8 [H, W, 3]: noise with a bright ellipse in the middle."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = rs.rand(H, W, 3) * 0.35
    img[((yy - H // 2) / (0.25 * H)) ** 2 + ((xx - W // 2) / (0.25 * W)) ** 2 <= 1.0] += 0.55
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def span(op):
    """Milliseconds between device events around ``op()``; the device is idle before the first."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    op()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(ann, H, W, ops):
    aid = ann.open(image_of(H, W, seed=H))
    ann.click({aid: (True, (H // 2, W // 2))})
    ann.partially_finish(aid)
    ann.click({aid: (True, (H // 2 + H // 8, W // 2 - W // 8))})
    a = ann._held[aid]
    thr = np.float32(ann.prob_thresh)
    host_labels = np.zeros((H, W), dtype=np.uint16)
    keep = {}

    def two_maps():
        return ann.pool.probs(aid)[0, 0].cpu().numpy(), a.parts.cpu().numpy()

    def host_mask():
        add, parts = two_maps()
        keep["mask"] = np.maximum(parts, add) > thr

    def host_preview():
        add, parts = two_maps()
        out = host_labels.copy()
        out[np.maximum(parts, add) > thr] = a.object_count + 1
        keep["preview"] = out

    def host_partial():
        add, parts = two_maps()
        keep["parts"] = np.maximum(parts, add)

    def host_finish():
        add, parts = two_maps()
        host_labels[np.maximum(parts, add) > thr] = a.object_count + 1

    def put_back(snapshot):
        a.undo = [snapshot]
        ann.undo(aid)

    def held():
        return (a.clicker.get_state(), ann.pool.get_states(aid), a.parts, a.mask)

    device = {"mask": lambda: keep.__setitem__("dmask", ann._masks([a])[aid]),
              "preview": lambda: keep.__setitem__("dpreview", ann.label_map(aid, preview=True)),
              "partial_finish": lambda: ann.partially_finish(aid),
              "finish": lambda: ann.finish(aid)}
    host = {"mask": host_mask, "preview": host_preview, "partial_finish": host_partial, "finish": host_finish}
    res = {"device": {}, "host": {}}
    for name in device:
        times = {"device": [], "host": []}
        for turn in range(ops + 3):                        # three warm-up turns of each route
            snapshot = held()
            d = span(device[name])
            if name in ("partial_finish", "finish"):
                put_back(snapshot)
            h = span(host[name])
            if turn >= 3:
                times["device"].append(d)
                times["host"].append(h)
        for route in times:
            res[route][name + "_ms"] = round(statistics.median(times[route]), 4)
    assert np.array_equal(keep["dmask"], keep["mask"])                     # the two routes show the same object
    res["bytes_to_host"] = {"device": {"mask": (H * W + 63) // 64 * 8 + 32, "preview": 2 * H * W, "partial_finish": 0, "finish": 32},
                            "host": {name: 8 * H * W for name in host}}
    res["host_over_device"] = {name: round(res["host"][name + "_ms"] / res["device"][name + "_ms"], 2) for name in device}
    ann.close(aid)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotation.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_annotation: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_annotation: --ops must be at least 30")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    predictor = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    ann = AnnotationPool(predictor, max_images=1)
    line = {"bench": "annotation", "model": "vitb448", "dtype": "bf16", "flip": True, "ops_per_route": args.ops,
            "statistic": "median ms between device events around the operation, read-back included; routes alternated",
            "sizes": {f"{H}x{W}": measure(ann, H, W, args.ops) for H, W in SIZES},
            "not_measured": "the click's forward (the same in both routes), several annotations per compose launch, pinned "
                            "host buffers for the host route's copies, and the kernel's time per launch apart from its read-back"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
