#!/usr/bin/env python
"""Interactive sessions: ``SessionPool.predict`` against ``BasePredictor.get_prediction`` per session, in one process on
the same sessions.  ViT-B/448 bf16, flip TTA, ZoomIn to 448 x 448 from the first click; N synthetic sessions on images of
mixed sizes (448 x 448, 480 x 640, 375 x 500), each with the same scripted click list (a positive click inside the object,
then seeded positive / negative clicks).  Each run comes after a warm-up of its own shapes:

* sequential: one private predictor per session, ``get_prediction`` and the caller's ``> pred_thr`` per click;
* the pool with K = 1, 4, 8 sessions per ``predict`` call (one forward and one read-back per call).

Per run: milliseconds per click (host clock; every click ends in a device-to-host copy, so the window is synchronised), the
share of the time spent in the model forward (a second pass with the forward synchronised on both sides), and from a
profiler pass of its own the device-to-host copies and bytes per click.  Then the time per launch (device events around a replayed graph) of
``vpu_session_paste_batched`` in both forms beside ``vpu_roi_paste_batched`` on the same canvases and maps, alternated.
Prints one JSON line and writes it to ``--out`` (default profiles/sessions.json).

``--prompts box-first | mixed``: drawn prompts on every session's FIRST call (``SessionPool.predict(boxes=, strokes=)``), clicks
afterwards -- ``box-first``: every session draws the box around its object; ``mixed``: a third of the sessions a box, a third
a stroke through the object, a third clicks only.  The yardstick is the click-only pool on the same sessions in the same
process (``pool_kK``, as without the option); the drawn runs are ``pool_kK_<prompts>``.  Same columns, plus the forwards per
round (a round ends in one read-back; 1.0 = one forward per network input size, as the click-only round).  Default ``--out``
then: profiles/sessions_prompts.json.
usage: python tools/bench_sessions.py [--sessions N] [--clicks C] [--prompts P] [--out FILE] [--kernels-only] [K ...]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvpuformer_amd.isegm.inference import batched, sessions                   # noqa: E402
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker              # noqa: E402
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.inference.transforms import Roi                      # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import synth_batch, vitb_model_kwargs                # noqa: E402

SIZES = [(448, 448), (480, 640), (375, 500)]
PRED_THR = 0.49


def make_sessions(n, clicks):
    """n (image uint8 [H, W, 3], click script) on SIZES in turn; the script: (positive, row, col) per click."""
    out = []
    for i in range(n):
        H, W = SIZES[i % len(SIZES)]
        b = synth_batch(1, max(H, W), seed=300 + i)
        image = (b["images"][0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
        rows, cols = np.nonzero(b["instances"][0, 0, :H, :W].numpy() > 0)
        first = (int(np.median(rows)), int(np.median(cols))) if len(rows) else (H // 2, W // 2)
        rs = np.random.RandomState(i)
        script = [(True,) + first] + [(bool(k % 2 == 0), int(rs.randint(H)), int(rs.randint(W))) for k in range(1, clicks)]
        out.append((image, script))
        # what an annotator would draw on this object: the box around it, a 64-point stroke along its diagonal
        r0, r1, c0, c1 = (int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())) if len(rows) else (H // 4, H // 2, W // 4, W // 2)
        t = np.linspace(0.0, 1.0, 64)
        DRAWN[id(image)] = ((r0, c0, r1, c1), np.stack([r0 + t * (r1 - r0), c0 + t * (c1 - c0)], 1).astype(np.int64))
    return out


DRAWN = {}           # id(image) -> (box, stroke) of make_sessions' sessions


def drawn_on_first_call(sids, data, prompts):
    """(boxes, strokes) of ``predict`` for the first call of these sessions under ``--prompts``."""
    boxes, strokes = {}, {}
    for sid, (image, _) in zip(sids, data):
        kind = {"clicks": 2, "box-first": 0, "mixed": sid % 3}[prompts]
        if kind == 0:
            boxes[sid] = DRAWN[id(image)][0]
        elif kind == 1:
            strokes[sid] = DRAWN[id(image)][1]
    return boxes or None, strokes or None


def run_sequential(mk, data, clicks):
    """Click by click over all sessions, one private predictor each -> the masks of the last click."""
    preds = []
    for image, _ in data:
        p = mk()
        p.set_input_image(image)
        preds.append((p, Clicker(device=None)))
    masks = None
    for k in range(clicks):
        masks = []
        for (p, clicker), (_, script) in zip(preds, data):
            clicker.add_click(Click(script[k][0], script[k][1:]))
            masks.append(p.get_prediction(clicker) > PRED_THR)
    return masks


def run_pool(mk, data, clicks, K, prompts="clicks", stats=None):
    """The same clicks, K sessions per ``predict`` call -> the masks of the last click.  ``prompts``: what the sessions draw on
    their first call; ``stats``: a dict that receives the pool's forwards and rounds."""
    pool = sessions.SessionPool(mk(), max_sessions=len(data), pred_thr=PRED_THR, max_batch=K)
    sids = [pool.open(image, seed=i) for i, (image, _) in enumerate(data)]
    lists = {sid: [] for sid in sids}
    masks = None
    for k in range(clicks):
        got = {}
        for sid, (_, script) in zip(sids, data):
            lists[sid].append(Click(script[k][0], script[k][1:], k))
        for at in range(0, len(sids), K):
            part = sids[at:at + K]
            if k == 0 and prompts != "clicks":
                boxes, strokes = drawn_on_first_call(part, data[at:at + K], prompts)
                got.update(pool.predict({sid: lists[sid] for sid in part}, boxes=boxes, strokes=strokes))
            else:
                got.update(pool.predict({sid: lists[sid] for sid in part}))
        masks = [got[sid] for sid in sids]
    if stats is not None:
        stats.update(forwards=pool.forwards, rounds=pool.readbacks)
    return masks


def timed(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def forward_share(model, run):
    """Share of a run's time inside model.forward, both measured in a pass with the forward synchronised on both sides."""
    fwd, orig = [], model.forward

    def wrapped(*a, **k):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = orig(*a, **k)
        torch.cuda.synchronize(); fwd.append(time.perf_counter() - t)
        return out
    model.forward = wrapped
    try:
        secs, _ = timed(run)
    finally:
        model.forward = orig
    return round(sum(fwd) / secs, 3), len(fwd)


def d2h_traffic(run):
    """(device-to-host copies, their bytes or None) of ``run()`` from the profiler's memcpy events; (None, None) when the
    profiler reported no copies at all (nothing can be said then)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    is_d2h = lambda n: "dtoh" in n.lower().replace(" ", "") or "device -> host" in n.lower() or "devicetohost" in n.lower()
    names = [e.name for e in prof.events() if "memcpy" in e.name.lower()]
    if not names:
        return None, None
    copies, nbytes = sum(1 for n in names if is_d2h(n)), None
    try:                      # the byte counts are in the trace's memcpy records only
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "trace.json")
            prof.export_chrome_trace(path)
            events = json.load(open(path)).get("traceEvents", [])
        sizes = [e.get("args", {}).get("bytes") for e in events
                 if "memcpy" in str(e.get("cat", "")).lower() and is_d2h(str(e.get("name", "")))]
        if sizes and all(s is not None for s in sizes):
            nbytes = int(sum(sizes))
    except Exception as e:    # noqa: BLE001 -- a trace that cannot be exported only loses the byte figure
        sys.stderr.write(f"bench_sessions: no byte counts from the profiler trace ({e})\n")
    return copies, nbytes


def kernel_times(data, launches=100, replays=10, repeats=3):
    """Microseconds per launch (device events around ``replays`` replays of a captured graph of ``launches`` launches, best of
    ``repeats`` alternated turns) of vpu_roi_paste_batched and of vpu_session_paste_batched in both forms: the same canvases,
    rois and maps."""
    from pvpuformer_amd import _lib, ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    objs = []
    for j, (image, _) in enumerate(data):
        H, W = image.shape[:2]
        objs.append(batched._Object(j, torch.zeros(3, H, W, device=dev), np.zeros((H, W), np.int32), dev))
    rois = [Roi(o.H // 8, o.H - o.H // 8 - 1, o.W // 6, o.W - o.W // 6 - 1) for o in objs]
    n = len(objs)
    probs = torch.rand(n, 1, 448, 448, generator=g).to(dev)
    max_hw = max(o.H * o.W for o in objs)
    eval_ops = batched._DeviceOps(dev)
    eval_ops.begin(n)
    for j, (o, roi) in enumerate(zip(objs, rois)):
        eval_ops.add(o, roi, j, j)
    eval_ops.upload()
    layout = sessions._Round([type("S", (), dict(sid=j, H=o.H, W=o.W)) for j, o in enumerate(objs)])
    out = torch.zeros(layout.size, device=dev, dtype=torch.int64)
    desc = []
    for j, (o, roi) in enumerate(zip(objs, rois)):
        d = _lib.SessionObj()
        d.canvas, d.bits, d.rec = o.canvas[1].data_ptr(), out.data_ptr() + 8 * layout.at[j], out.data_ptr() + 32 * j
        d.H, d.W = o.H, o.W
        d.r0, d.r1, d.c0, d.c1 = roi
        d.src = j
        desc.append(d)
    sdesc = torch.frombuffer(bytearray(bytes((_lib.SessionObj * n)(*desc))), dtype=torch.uint8).to(dev)
    calls = {
        "vpu_roi_paste_batched": lambda: ops.roi_paste_batched(eval_ops._at(0), n, probs, 448, 448, PRED_THR, 0.5, max_hw),
        "vpu_session_paste_batched[ballot]": lambda: ops.session_paste_batched(sdesc, n, probs, 448, 448, PRED_THR, 0.5, max_hw, 0),
        "vpu_session_paste_batched[quads]": lambda: ops.session_paste_batched(sdesc, n, probs, 448, 448, PRED_THR, 0.5, max_hw, 1),
    }
    # a captured graph of back-to-back launches, replayed: the device's time per launch without the host's enqueue cost (two
    # launches of some microseconds each are enqueued from Python more slowly than the device runs them)
    graphs = {}
    for name, call in calls.items():
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(launches):
                call()
        graphs[name].replay()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in calls}
    for _ in range(repeats):
        for name, graph in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            best[name] = min(best[name], a.elapsed_time(b) / (launches * replays) * 1e3)
    pixels = sum(o.H * o.W for o in objs)
    return {"sessions": n, "canvas_pixels": pixels, "launches": launches * replays, "us_per_launch": {k: round(v, 2) for k, v in best.items()},
            "note": "each figure covers the init launch and the main launch of its export"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=8)
    ap.add_argument("--clicks", type=int, default=10)
    ap.add_argument("--prompts", choices=["clicks", "box-first", "mixed"], default="clicks",
                    help="what the sessions draw on their first call (the click-only pool is always run beside it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the paste kernels' time per launch")
    ap.add_argument("ks", nargs="*", type=int)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sessions.json" if args.prompts == "clicks" else "sessions_prompts.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sessions: needs a GPU (nothing here is measured without one)")
    if args.kernels_only:
        print(json.dumps({"bench": "sessions", "paste_kernels": kernel_times(make_sessions(args.sessions, 1))}))
        return
    n, clicks, ks = args.sessions, args.clicks, args.ks or [1, 4, 8]
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    mk = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    data = make_sessions(n, clicks)
    total = n * clicks
    runs = [("sequential", lambda c=clicks: run_sequential(mk, data, c))]
    stats = {}
    for K in ks:
        runs.append((f"pool_k{K}", lambda c=clicks, K=K: run_pool(mk, data, c, K, stats=stats)))
        if args.prompts != "clicks":
            runs.append((f"pool_k{K}_{args.prompts}", lambda c=clicks, K=K: run_pool(mk, data, c, K, args.prompts, stats=stats)))
    res, last = {}, {}
    for name, run in runs:
        run(3)                                             # warm-up: the run's own shapes and batch sizes
        stats.clear()
        secs, last[name] = timed(run)
        per_round = round(stats["forwards"] / stats["rounds"], 3) if stats else None
        share, forwards = forward_share(model, run)
        copies, nbytes = d2h_traffic(lambda: run(2))       # the profiler pass: two clicks per session
        res[name] = dict(ms_per_click=round(secs / total * 1e3, 3), clicks=total, forwards=forwards, forward_share=share,
                         d2h_copies_per_click=None if copies is None else round(copies / (2 * n), 3),
                         d2h_bytes_per_click=None if nbytes is None else round(nbytes / (2 * n), 1),
                         forwards_per_round=per_round)
    # bf16: the pool's forward runs other GEMM instantiations than a batch of 2, so the masks are compared, not asserted
    agree = {name: round(float(np.mean([(a == b).mean() for a, b in zip(last[name], last["sequential"])])), 5)
             for name in last if name != "sequential" and not name.endswith("_" + args.prompts)}   # (drawn runs: other prompts)
    line = {"bench": "sessions", "prompts": args.prompts, "model": "vitb448", "dtype": "bf16", "sessions": n, "clicks_per_session": clicks,
            "sizes": SIZES, "results": res, "last_mask_pixel_agreement_with_sequential": agree,
            "pool_over_sequential_ms_per_click": {k: round(v["ms_per_click"] / res["sequential"]["ms_per_click"], 3)
                                                  for k, v in res.items() if k != "sequential"},
            "paste_kernels": kernel_times(data)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
