#!/usr/bin/env python
"""Outline read-back: the device tracer (vpu_outline_count_batched + vpu_outline_trace_batched behind ``DeviceOutlineOps`` /
``SessionPool.mask_outlines``) against the host route it replaces, in one process on the same maps, at 480 x 640 and
1024 x 1365:

* ellipse_holes: an fp32 probability map of one filled ellipse with three holes; device: one trace, two read-backs; host: the
  packed mask copied to the host (H * W / 8 bytes, as ``predict`` hands it back), unpacked, ``host_outline``;
* eight_ellipses: a 16-bit label map of eight filled ellipses; device: one trace of eight items (one per label); host: the
  label map copied to the host (2 * H * W bytes) and ``host_outline`` per label;
* model: the mask of a session after one click, ViT-B/448 bf16, flip TTA, ZoomIn to 448 x 448, random weights (a noisy map with
  many small loops); device: ``mask_outlines``; host: the packed mask as above.

Per map both routes are alternated after a warm-up of each; the figure is the median over ``--ops`` operations of the time
between two device events around the operation, its read-backs and the host's own work included (the device is idle at the
first event).  Both routes must agree element for element.  ``kernels``: the launches of one count and one trace without any
read-back (the header read beforehand), beside a device-to-device copy of the same source bytes.  Prints one JSON line and
writes it to ``--out`` (default profiles/outlines.json).
usage: python tools/bench_outlines.py [--ops N] [--out FILE]"""
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
from pvpuformer_amd.isegm.inference.outlines import DeviceOutlineOps, host_outline   # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.inference.sessions import pack_mask, unpack_mask      # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import vitb_model_kwargs                             # noqa: E402

SIZES = [(480, 640), (1024, 1365)]
THR = 0.5


def image_of(H, W, seed):
    """uint8 [H, W, 3]: noise with a bright ellipse in the middle."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = rs.rand(H, W, 3) * 0.35
    img[((yy - H // 2) / (0.25 * H)) ** 2 + ((xx - W // 2) / (0.25 * W)) ** 2 <= 1.0] += 0.55
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2 <= 1.0


def ellipse_with_holes(H, W):
    """fp32 [H, W]: 0.9 on a filled ellipse, 0.1 elsewhere and on three holes in it."""
    m = ellipse(H, W, 0.5, 0.5, 0.4, 0.4)
    for cy, cx in ((0.35, 0.4), (0.6, 0.6), (0.55, 0.3)):
        m &= ~ellipse(H, W, cy, cx, 0.06, 0.05)
    return np.where(m, np.float32(0.9), np.float32(0.1))


def blob_labels(H, W, count=8):
    """uint16 [H, W]: ``count`` filled ellipses with labels 1 .. count, later ones over earlier ones."""
    rs = np.random.RandomState(H + W)
    out = np.zeros((H, W), dtype=np.uint16)
    for label in range(1, count + 1):
        out[ellipse(H, W, rs.uniform(0.15, 0.85), rs.uniform(0.15, 0.85), rs.uniform(0.06, 0.2), rs.uniform(0.06, 0.2))] = label
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


def same(a, b):
    return a.size == b.size and np.array_equal(a.points, b.points) and np.array_equal(a.offsets, b.offsets)


def report(times, outlines, n_items, host_bytes):
    corners, loops = sum(len(o.points) for o in outlines), sum(len(o) for o in outlines)
    most = corners // 4 + 1
    return {"ms": times, "corners": corners, "loops": loops,
            "bytes_to_host": {"device": 4 * (n_items + 1) + (4 * (2 * corners + most + n_items + 1) if corners else 0), "host": host_bytes}}


def mask_routes(trace, packed, H, W, n):
    """One binary map: ``trace()`` -> Outline on the device route, the packed mask on the host route."""
    keep = {}

    def host():
        keep["host"] = host_outline(unpack_mask(packed.cpu().numpy(), H, W))

    times = alternate(lambda: keep.__setitem__("device", trace()), host, n)
    assert same(keep["device"], keep["host"])
    return report(times, [keep["device"]], 1, (H * W + 63) // 64 * 8)


def label_routes(tracer, labels, n):
    """Eight labels of one label map: one trace of eight items, against the map on the host and eight ``host_outline``."""
    H, W = labels.shape
    names, keep = list(range(1, 9)), {}

    def host():
        got = labels.cpu().numpy().view(np.uint16)
        keep["host"] = [host_outline(got == k) for k in names]

    times = alternate(lambda: keep.__setitem__("device", tracer.trace([(labels, 1, 0.0, k) for k in names])), host, n)
    assert all(same(d, h) for d, h in zip(keep["device"], keep["host"]))
    return report(times, keep["device"], len(names), 2 * H * W)


def kernels_alone(items, n):
    """The launches of one count and one trace of ``items`` [(tensor, kind, thr, label)] (no read-back) beside a
    device-to-device copy of the source bytes (each source once)."""
    rows = []
    for tensor, kind, thr, label in items:
        d = _lib.OutlineObj()
        d.src, d.H, d.W, d.kind, d.thr, d.label, d.pad = tensor.data_ptr(), tensor.shape[0], tensor.shape[1], kind, thr, label, 0
        rows.append(d)
    k = len(rows)
    host = torch.frombuffer(bytearray(bytes((_lib.OutlineObj * k)(*rows))), dtype=torch.uint8).pin_memory()
    desc = host.cuda()
    scratch = torch.empty(ops.outline_scratch_len([tuple(t.shape) for t, _, _, _ in items]), device="cuda", dtype=torch.int32)
    header = torch.empty(k + 1, device="cuda", dtype=torch.int32)
    ops.outline_count_batched(desc, host, k, scratch, header)
    head = header.cpu()
    V = int(head[k])
    work = torch.empty(ops.outline_work_len(V), device="cuda", dtype=torch.int32)
    points = torch.empty(V, 2, device="cuda", dtype=torch.int32)
    offsets = torch.empty(V // 4 + 1, device="cuda", dtype=torch.int32)
    item_loops = torch.empty(k + 1, device="cuda", dtype=torch.int32)
    sources = list({t.data_ptr(): t for t, _, _, _ in items}.values())
    others = [torch.empty_like(t) for t in sources]
    most = max(int(head[i + 1] - head[i]) for i in range(k))

    def trace():
        ops.outline_count_batched(desc, host, k, scratch, header)
        ops.outline_trace_batched(desc, host, k, scratch, header, head, work, points, offsets, item_loops)

    def copy():
        for o, t in zip(others, sources):
            o.copy_(t)

    out = alternate(trace, copy, n)
    return {"launches": 2 + (4 + max(most - 1, 0).bit_length() if V else 0), "launches_ms": out["device"], "device_copy_ms": out["host"],
            "source_bytes": sum(t.numel() * t.element_size() for t in sources), "corners": V}


def measure(ann, tracer, H, W, n):
    res = {}
    prob = torch.from_numpy(ellipse_with_holes(H, W)).cuda()
    packed = torch.from_numpy(pack_mask(prob.cpu().numpy() > np.float32(THR)).view(np.int64)).cuda()
    res["ellipse_holes"] = mask_routes(lambda: tracer.trace([(prob, 0, THR, 0)])[0], packed, H, W, n)
    res["ellipse_holes"]["kernels"] = kernels_alone([(prob, 0, THR, 0)], n)
    labels = torch.from_numpy(blob_labels(H, W).view(np.int16)).cuda()
    res["eight_ellipses"] = label_routes(tracer, labels, n)
    res["eight_ellipses"]["kernels"] = kernels_alone([(labels, 1, 0.0, k) for k in range(1, 9)], n)
    aid = ann.open(image_of(H, W, seed=H))
    mask = ann.click({aid: (True, (H // 2, W // 2))})[aid]
    packed = torch.from_numpy(pack_mask(mask).view(np.int64)).cuda()
    res["model"] = mask_routes(lambda: ann.pool.mask_outlines([aid])[aid], packed, H, W, n)
    res["model"]["kernels"] = kernels_alone([(ann.pool.probs(aid)[0, 0], 0, ann.pool.pred_thr, 0)], n)
    ann.close(aid)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=40, help="timed operations per route (at least 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlines.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_outlines: needs a GPU (nothing here is measured without one)")
    if args.ops < 30:
        raise SystemExit("bench_outlines: --ops must be at least 30")
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    predictor = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    ann = AnnotationPool(predictor, max_images=1)
    tracer = DeviceOutlineOps("cuda")
    line = {"bench": "outlines", "model": "vitb448", "dtype": "bf16", "flip": True, "ops_per_route": args.ops,
            "band_rows": ops.OUTLINE_BAND_ROWS, "cols": ops.OUTLINE_COLS,
            "statistic": "median ms between device events around the operation, read-backs included; routes alternated "
                         "(device first, then host, per turn)",
            "sizes": {f"{H}x{W}": measure(ann, tracer, H, W, args.ops) for H, W in SIZES},
            "not_measured": "other band heights and column-group widths, wider loads, several sessions per trace, label_outlines "
                            "with an object in progress (its compose launch is bench_annotation's preview), pinned host buffers for "
                            "the host route's copies, a tracer in C on the host (none ships here), the spread between runs"}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
