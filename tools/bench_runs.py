#!/usr/bin/env python
"""Run-length read-back: ``SessionPool.mask_runs`` / ``AnnotationPool.label_runs`` / ``AnnotationPool.export`` (the device
encoder, vpu_runs_count_batched + vpu_runs_write_batched) against the host route they replace, in one process on the same
maps.  ViT-B/448 bf16, flip TTA, ZoomIn to 448 x 448, random weights; per image size one annotation.

Per operation both routes are alternated after a warm-up of each; the figure is the median over ``--ops`` operations of the
time between two device events around the operation, its read-backs and the host's own work included (the device is idle at
the first event):

* mask_runs: device: one encode of the session's probability map, two read-backs (4 * 2 + 8 bytes per run); host: the packed
  mask copied to the host (H * W / 8 bytes, as ``predict`` hands it back), unpacked, ``host_runs_encode`` and ``counts``;
* label_runs (committed labels): device: one encode of the label map; host: ``label_map`` (2 * H * W bytes) and
  ``host_runs_encode``;
* export_1 / export_8, with 1 and with 8 finished objects: device: ``export``; host: ``label_map``, ``host_runs_encode`` and
  ``counts`` per object.

Random weights give noisy maps with many runs, so the same three label-map operations are also timed on a synthetic blob
label map (eight filled ellipses) of the same size; the run counts of both are reported.  ``kernels``: the three launches of an
encode of the label map without any read-back (the entry buffer sized beforehand), beside a device-to-device copy of the same
source bytes.  Prints one JSON line and writes it to ``--out`` (default profiles/runs.json).
usage: python tools/bench_runs.py [--ops N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvpuformer_amd import _lib, ops                                           # noqa: E402
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool            # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.inference.runs import host_runs_encode               # noqa: E402
from pvpuformer_amd.isegm.inference.sessions import pack_mask, unpack_mask      # noqa: E402
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


def blob_labels(H, W, count=8):
    """uint16 [H, W]: ``count`` filled ellipses with labels 1 .. count, later ones over earlier ones."""
    rs = np.random.RandomState(H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), dtype=np.uint16)
    for label in range(1, count + 1):
        cy, cx = rs.uniform(0.15, 0.85) * H, rs.uniform(0.15, 0.85) * W
        ry, rx = rs.uniform(0.06, 0.2) * H, rs.uniform(0.06, 0.2) * W
        out[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = label
    return out


def span(op):
    """Milliseconds between device events around ``op()``; the device is idle before the first."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    op()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(device, host, n):
    """Median milliseconds of the two routes, alternated, after three warm-up turns of each."""
    times = {"device": [], "host": []}
    for turn in range(n + 3):
        d, h = span(device), span(host)
        if turn >= 3:
            times["device"].append(d)
            times["host"].append(h)
    return {route: round(statistics.median(v), 4) for route, v in times.items()}


def kernels_alone(labels, n):
    """The three launches of one encode of ``labels`` (no read-back) beside a device-to-device copy of its bytes."""
    H, W = labels.shape
    d = _lib.RunsObj()
    d.src, d.H, d.W, d.kind, d.thr = labels.data_ptr(), H, W, 1, 0.0
    host = torch.frombuffer(bytearray(bytes((_lib.RunsObj * 1)(d))), dtype=torch.uint8).pin_memory()
    desc = host.cuda()
    scratch = torch.empty(ops.runs_scratch_len([(H, W)]), device="cuda", dtype=torch.int32)
    header = torch.empty(2, device="cuda", dtype=torch.int32)
    ops.runs_count_batched(desc, host, 1, scratch, header)
    entries = torch.empty(int(header.cpu()[1]), 2, device="cuda", dtype=torch.int32)
    other = torch.empty_like(labels)

    def encode():
        ops.runs_count_batched(desc, host, 1, scratch, header)
        ops.runs_write_batched(desc, host, 1, scratch, entries)

    out = alternate(encode, lambda: other.copy_(labels), n)
    return {"three_launches_ms": out["device"], "device_copy_ms": out["host"], "source_bytes": 2 * H * W}


def label_ops(ann, aid, n, with_export):
    """label_runs and export of the annotation's committed labels, both routes; -> (figures, runs, objects)."""
    keep = {}
    labels = [r["label"] for r in ann.objects(aid)]

    def host_label_runs():
        keep["host"] = host_runs_encode(ann.label_map(aid, preview=False), 1)

    def host_export():
        rm = host_runs_encode(ann.label_map(aid, preview=False), 1)
        keep["host_export"] = [rm.to_coco(label) for label in labels]

    res = {"label_runs_ms": alternate(lambda: keep.__setitem__("device", ann.label_runs(aid, preview=False)), host_label_runs, n)}
    assert np.array_equal(keep["device"].starts, keep["host"].starts) and np.array_equal(keep["device"].values, keep["host"].values)
    if with_export:
        res["export_ms"] = alternate(lambda: keep.__setitem__("device_export", ann.export(aid)), host_export, n)
        assert [e["segmentation"] for e in keep["device_export"]] == keep["host_export"]
    runs = len(keep["device"])
    H, W = keep["device"].size
    res["runs"] = runs
    res["bytes_to_host"] = {"device": 8 + 8 * runs, "host": 2 * H * W}
    return res


def measure(ann, H, W, n):
    aid = ann.open(image_of(H, W, seed=H))
    a = ann._held[aid]
    res = {}

    def add_object(k):
        ann.click({aid: (True, (H // 2 + (k % 3 - 1) * H // 5, W // 2 + (k // 3 - 1) * W // 5))})
        assert ann.finish(aid) is not None

    add_object(4)                                                           # the centre
    res["objects_1"] = label_ops(ann, aid, n, with_export=True)
    # a prediction in progress: the session's mask
    mask = ann.click({aid: (True, (H // 2 + H // 8, W // 2 - W // 8))})[aid]
    packed = torch.from_numpy(pack_mask(mask).view(np.int64)).cuda()
    keep = {}

    def host_mask_runs():
        m = unpack_mask(packed.cpu().numpy(), H, W)
        rm = host_runs_encode(m.astype(np.uint16), 1)
        keep["host"] = rm.to_coco(1)

    res["mask_runs_ms"] = alternate(lambda: keep.__setitem__("device", ann.pool.mask_runs([aid])[aid]), host_mask_runs, n)
    assert keep["device"].to_coco() == keep["host"]
    res["mask_runs"] = {"runs": len(keep["device"]), "bytes_to_host": {"device": 8 + 8 * len(keep["device"]), "host": (H * W + 63) // 64 * 8}}
    assert ann.finish(aid) is not None
    for k in (0, 1, 2, 3, 5, 6):
        add_object(k)
    assert len(ann.objects(aid)) == 8
    res["objects_8"] = label_ops(ann, aid, n, with_export=True)
    res["kernels_model_labels"] = kernels_alone(a.labels, n)
    # the synthetic blobs: the label map and the records set directly
    blobs = blob_labels(H, W)
    a.labels.copy_(torch.from_numpy(blobs.view(np.int16)))
    a.records = [dict(label=k, area=int((blobs == k).sum()), box=(0, 0, 0, 0), overwritten=0) for k in range(1, 9)]
    res["blobs_8"] = label_ops(ann, aid, n, with_export=True)
    res["kernels_blob_labels"] = kernels_alone(a.labels, n)
    ann.close(aid)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runs.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_runs: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_runs: --ops must be at least 30")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    predictor = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    ann = AnnotationPool(predictor, max_images=1)
    line = {"bench": "runs", "model": "vitb448", "dtype": "bf16", "flip": True, "ops_per_route": args.ops,
            "band_rows": ops.RUNS_BAND_ROWS, "cols": ops.RUNS_COLS,
            "statistic": "median ms between device events around the operation, read-backs included; routes alternated "
                         "(device first, then host, per turn)",
            "sizes": {f"{H}x{W}": measure(ann, H, W, args.ops) for H, W in SIZES},
            "not_measured": "16-byte loads (four columns per lane), other band heights and column-group widths, several sessions "
                            "or annotations per encode, label_runs with an object in progress (its compose launch is "
                            "bench_annotation's preview), pinned host buffers for the host route's copies, the compressed counts string"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
