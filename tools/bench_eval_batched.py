#!/usr/bin/env python
"""Throughput of the NoBRS evaluation with K objects per forward (evaluate_dataset(batch_objects=K)): ViT-B/448 bf16,
flip TTA, ZoomIn to 448 x 448 from the first click, a 20-click budget that no object stops early (max_iou_thr=2), over a
synthetic set of objects on images of mixed sizes (448 x 448, 480 x 640, 375 x 500).  Prints one JSON line: object-clicks
per second and milliseconds per click for each K, and the share of the time spent in the model forward (a second,
synchronised pass).  K = 1 is the sequential loop (evaluate_sample per object).  ``--prompt-type 1`` evaluates with box
prompts (BasePredictor.get_vqu_prediction derives the box per click sequentially, vpu_box_prompts_batched per step batched)
and also counts, with the torch profiler, the device-to-host copies of a batched step (expected: exactly one).
``--prompt-type 1,0`` is a per-click schedule (a box on the first click, then clicks; the last element repeats): the batched
steps then run click and box rows in one forward, and ``forwards_per_step`` reports it.
usage: python tools/bench_eval_batched.py [--prompt-type {0,1,LIST}] [objects] [K ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvpuformer_amd.isegm.inference.predictors import get_predictor            # noqa: E402
from pvpuformer_amd.isegm.inference.vpu_evaluation import evaluate_dataset      # noqa: E402
from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model   # noqa: E402
from pvpuformer_amd.synth import synth_batch, vitb_model_kwargs                # noqa: E402

SIZES = [(448, 448), (480, 640), (375, 500)]


class Sample:
    def __init__(self, image, masks):
        self.image, self._masks, self.objects_ids = image, masks, list(range(len(masks)))

    def gt_mask(self, oid):
        return self._masks[oid]


class Dataset:
    def __init__(self, n_objects, per_image=2):
        self.samples = []
        for i in range((n_objects + per_image - 1) // per_image):
            H, W = SIZES[i % len(SIZES)]
            b = synth_batch(per_image, max(H, W), seed=100 + i)
            image = (b["images"][0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
            k = min(per_image, n_objects - i * per_image)
            self.samples.append(Sample(image, [b["instances"][j, 0, :H, :W].numpy().astype(np.int32) for j in range(k)]))

    def __len__(self):
        return len(self.samples)

    def get_sample(self, i):
        return self.samples[i]


def d2h_copies_per_step(run):
    """(device-to-host copies, batched steps) of ``run()``, the copies counted from the profiler's memcpy events."""
    from torch.profiler import ProfilerActivity, profile
    from pvpuformer_amd.isegm.inference import batched
    steps, orig = [], batched.BatchedEvaluator._step

    def counted(self, *a, **k):
        steps.append(1)
        return orig(self, *a, **k)
    batched.BatchedEvaluator._step = counted
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
    finally:
        batched.BatchedEvaluator._step = orig
    names = [e.name for e in prof.events() if "memcpy" in e.name.lower()]
    if not any("htod" in n.lower().replace(" ", "") or "host -> device" in n.lower() for n in names):
        return None, len(steps)              # the profiler reported no copies at all: nothing can be said
    return sum(1 for n in names if "dtoh" in n.lower().replace(" ", "") or "device -> host" in n.lower()), len(steps)


def prompt_type(text):
    """"1" -> 1; "1,0" -> (1, 0).  Types 0 and 1 only: scribble prompts are not batched."""
    types = tuple(int(v) for v in text.split(","))
    if not types or any(t not in (0, 1) for t in types):
        raise argparse.ArgumentTypeError("0, 1 or a comma list of them")
    return types[0] if len(types) == 1 else types


def main():
    from pvpuformer_amd.isegm.inference import batched
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt-type", type=prompt_type, default=0)
    ap.add_argument("objects", nargs="?", type=int, default=32)
    ap.add_argument("ks", nargs="*", type=int)
    args = ap.parse_args()
    n_obj, ks, ptype = args.objects, args.ks or [1, 4, 8, 16], args.prompt_type
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype("bf16")
    model.eval()
    model.weights_frozen = True
    ds, warm = Dataset(n_obj), Dataset(max(ks) + 2)
    kw = dict(max_iou_thr=2.0, pred_thr=0.49, max_clicks=20, as_prompt_type=ptype)
    mk = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True,
                               zoom_in_params=dict(skip_clicks=-1, target_size=(448, 448)))
    res = {}
    for K in ks:
        evaluate_dataset(warm, mk(), batch_objects=K, batch_box_prompts=True, max_iou_thr=2.0, max_clicks=3,
                         as_prompt_type=ptype)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        series, _ = evaluate_dataset(ds, mk(), batch_objects=K, batch_box_prompts=True, **kw)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        clicks = sum(len(s) for s in series)
        # forward share: the same run with the forward synchronised on both sides
        fwd, steps = [], []
        orig, orig_step = model.forward, batched.BatchedEvaluator._step

        def counted_step(self, *a, **k):
            steps.append(1)
            return orig_step(self, *a, **k)

        def timed(*a, **k):
            torch.cuda.synchronize(); t = time.perf_counter()
            out = orig(*a, **k)
            torch.cuda.synchronize(); fwd.append(time.perf_counter() - t)
            return out
        model.forward = timed
        batched.BatchedEvaluator._step = counted_step
        try:
            t1 = time.perf_counter()
            evaluate_dataset(ds, mk(), batch_objects=K, batch_box_prompts=True, **kw)
            secs_sync = time.perf_counter() - t1
        finally:
            model.forward = orig
            batched.BatchedEvaluator._step = orig_step
        res[K] = dict(object_clicks_per_s=round(clicks / secs, 1), ms_per_click=round(secs / clicks * 1e3, 3),
                      ms_per_step=round(secs / len(fwd) * 1e3, 2),
                      forwards=len(fwd), forward_share=round(sum(fwd) / secs_sync, 3), object_clicks=clicks)
        if len(steps) > 1:       # (the first step of a run only computes click keys: it has no forward)
            res[K].update(steps=len(steps), forwards_per_step=round(len(fwd) / (len(steps) - 1), 3))
    k1 = res.get(1, {}).get("object_clicks_per_s")
    line = {"bench": "eval_batched", "model": "vitb448", "dtype": "bf16", "objects": n_obj, "max_clicks": 20, "prompt_type": ptype,
            "results": {str(k): v for k, v in res.items()}}
    if k1:
        line["speedup_vs_k1"] = {str(k): round(v["object_clicks_per_s"] / k1, 2) for k, v in res.items()}
    if 1 in res and len(res) > 1:
        line["batched_over_sequential_ms_per_click"] = {str(k): round(v["ms_per_click"] / res[1]["ms_per_click"], 3)
                                                        for k, v in res.items() if k != 1}
    if ptype != 0 and max(ks) > 1:
        copies, steps = d2h_copies_per_step(
            lambda: evaluate_dataset(warm, mk(), batch_objects=max(ks), batch_box_prompts=True, max_iou_thr=2.0, max_clicks=4,
                                     as_prompt_type=ptype))
        line["batched_step_d2h_copies"] = {"K": max(ks), "steps": steps, "device_to_host_copies": copies}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
