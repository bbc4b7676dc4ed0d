#!/usr/bin/env python
"""Run-length objects onto the device: ``AnnotationPool.load`` and ``set_mask`` in run-length form (the host merge
``stack_objects`` and the device decoder vpu_runs_decode_batched) against the host routes they replace, in one process on the
same objects.  ViT-B/448 bf16, flip TTA, ZoomIn to 448 x 448, random weights; per image size one annotation.

Per operation both routes are alternated after a warm-up of each; the figure is the median over ``--ops`` operations of the
time between two device events around the operation, the host's own work included (the device is idle at the first event;
the annotation is put back to what ``open`` left between operations, outside the span):

* load: device: ``load(aid, objects)`` -- the objects read, merged on the host from their runs, one copy of 40 + 8 bytes per run
  of the merged map, one launch; host: every object read and ``RunMap.decode()``d, painted into one uint16 map with numpy, and
  that map uploaded into the annotation's labels (2 * H * W bytes);
* set_mask: device: ``set_mask(aid, rm, label)``; host: ``rm.decode() == label`` and ``set_mask(aid, raster)`` as it stands
  (H * W bytes of bool up, the fp32 conversion on the device).

Two sets of eight objects per size: synthetic filled ellipses, and what ``export`` gives after eight objects of the model's own
(random weights: noisy masks with many runs).  Also: the host time of ``stack_objects`` alone (wall clock), and ``kernel``: the
single decode launch of the merged label map from entries already on the device beside a device-to-device copy of the same
destination bytes.  Prints one JSON line and writes it to ``--out`` (default profiles/load.json).
usage: python tools/bench_load.py [--ops N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_runs import SIZES, alternate, image_of                              # noqa: E402
from pvpuformer_amd import _lib, ops                                           # noqa: E402
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool            # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.inference.runs import as_run_map, host_runs_encode, stack_objects   # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import vitb_model_kwargs                             # noqa: E402


def ellipse_objects(H, W, count=8):
    """``count`` filled ellipses as COCO dicts, placed as bench_runs.blob_labels places them."""
    rs = np.random.RandomState(H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(count):
        cy, cx = rs.uniform(0.15, 0.85) * H, rs.uniform(0.15, 0.85) * W
        ry, rx = rs.uniform(0.06, 0.2) * H, rs.uniform(0.06, 0.2) * W
        mask = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        out.append(host_runs_encode(mask.astype(np.uint16), 1).to_coco())
    return out


def model_objects(ann, H, W):
    """``export`` of eight objects of the model's own on a 3 x 3 grid of clicks."""
    aid = ann.open(image_of(H, W, seed=H))
    for k in (4, 0, 1, 2, 3, 5, 6, 7):
        ann.click({aid: (True, (H // 2 + (k % 3 - 1) * H // 5, W // 2 + (k // 3 - 1) * W // 5))})
        assert ann.finish(aid) is not None
    out = ann.export(aid)
    ann.close(aid)
    return out


def fresh(a):
    """The annotation as ``open`` left it (``load`` writes every pixel of the labels)."""
    a.records, a.object_count = [], 0
    a.start()


def decode_alone(rm, labels, n):
    """One decode launch of ``rm`` into ``labels`` from a staged buffer beside a device-to-device copy of the same bytes."""
    H, W = rm.size
    entries = torch.from_numpy(np.ascontiguousarray(np.stack((rm.starts, rm.values), axis=1))).cuda()
    d = _lib.UnrunObj()
    d.dst, d.entries, d.H, d.W, d.n_runs, d.kind, d.label, d.pad = labels.data_ptr(), entries.data_ptr(), H, W, len(rm), 1, 0, 0
    host = torch.frombuffer(bytearray(bytes((_lib.UnrunObj * 1)(d))), dtype=torch.uint8).pin_memory()
    desc = host.cuda()
    want = labels.clone()
    other = torch.empty_like(labels)
    out = alternate(lambda: ops.runs_decode_batched(desc, host, 1), lambda: other.copy_(labels), n)
    assert torch.equal(labels, want)
    return {"one_launch_ms": out["device"], "device_copy_ms": out["host"], "destination_bytes": 2 * H * W}


def measure_objects(ann, aid, objects, n):
    a = ann._held[aid]
    H, W = a.H, a.W
    keep = {}

    def device_load():
        fresh(a)
        keep["records"] = ann.load(aid, objects)

    def host_load():
        fresh(a)
        out = np.zeros((H, W), dtype=np.uint16)
        for k, obj in enumerate(objects):
            out[as_run_map(obj["segmentation"] if "segmentation" in obj else obj).decode() != 0] = k + 1
        a.labels.copy_(torch.from_numpy(out.view(np.int16)))
        keep["host"] = out

    # the resets run inside the spans of both routes alike: three attribute writes
    res = {"load_ms": alternate(device_load, host_load, n)}
    device_load()
    assert np.array_equal(a.labels.cpu().numpy().view(np.uint16), keep["host"])
    maps = [as_run_map(obj["segmentation"] if "segmentation" in obj else obj) for obj in objects]
    rm, _ = stack_objects((H, W), maps)
    took = []
    for _ in range(n + 3):
        t = time.perf_counter()
        stack_objects((H, W), maps)
        took.append(1e3 * (time.perf_counter() - t))
    res["stack_objects_host_ms"] = round(statistics.median(took[3:]), 4)
    res["runs"] = {"objects": [len(m) for m in maps], "merged": len(rm)}
    res["load_bytes_to_device"] = {"device": 40 + 8 * len(rm), "host": 2 * H * W}
    res["kernel"] = decode_alone(rm, a.labels, n)
    # set_mask: the largest object of the merged map
    label = max(range(1, len(maps) + 1), key=rm.area)

    def host_set_mask():
        ann.set_mask(aid, rm.decode() == label)

    res["set_mask_ms"] = alternate(lambda: ann.set_mask(aid, rm, label), host_set_mask, n)
    ann.set_mask(aid, rm, label)
    got = a.mask.clone()
    host_set_mask()
    assert torch.equal(got, a.mask)
    res["set_mask_bytes_to_device"] = {"device": 40 + 8 * len(rm), "host": H * W}
    fresh(a)
    ann._reset_session(a)
    return res


def measure(ann, H, W, n):
    given = {"ellipses_8": ellipse_objects(H, W), "model_8": model_objects(ann, H, W)}
    aid = ann.open(image_of(H, W, seed=H))
    res = {name: measure_objects(ann, aid, objects, n) for name, objects in given.items()}
    ann.close(aid)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_load: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_load: --ops must be at least 30")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    predictor = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    ann = AnnotationPool(predictor, max_images=1)
    line = {"bench": "load", "model": "vitb448", "dtype": "bf16", "flip": True, "ops_per_route": args.ops,
            "band_rows": ops.RUNS_BAND_ROWS, "cols": ops.RUNS_COLS,
            "statistic": "median ms between device events around the operation, the host's work included; routes alternated "
                         "(device first, then host, per turn); stack_objects_host_ms is wall clock; a single run",
            "sizes": {f"{H}x{W}": measure(ann, H, W, args.ops) for H, W in SIZES},
            "not_measured": "16-byte stores (four columns per lane), other band heights and column-group widths, several "
                            "annotations per decode, the spread between runs, pinned host buffers for the host route's upload"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
