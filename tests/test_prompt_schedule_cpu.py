"""CPU: per-click prompt schedules (``as_prompt_type`` as an int, a sequence or a callable) through the sequential
``evaluate_sample`` and the batched NoBRS scheduler, with a stub network that reads the box prompt and treats a slot of -1 as
"this row carries no box", and the host stand-ins of the batched kernels.  Also: the predictor built from the dictionary
the reference's evaluation script passes (``cascade_step=1``), and the scribble prompt of ``as_prompt_type=2``."""
import random

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.engine.prompt_sim import cal_scribble
from pvpuformer_amd.isegm.inference import batched, vpu_evaluation
from pvpuformer_amd.isegm.inference.clicker import Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.transforms import crop_resize
from pvpuformer_amd.isegm.inference.vpu_evaluation import PromptSchedule, evaluate_dataset, evaluate_sample, prompt_schedule
from test_batched_eval_box_cpu import Dataset, host_transforms  # noqa: F401  (the mixed-size data set and the host transforms)


class StubNet:
    """BoxStubNet's logits (image brightness, previous mask, bumps at the clicks, a bump shaped by the box) with two
    additions: a box row whose slot is negative adds nothing (the model's "no box in this row"), and with scribble prompts
    a bump at the scribble's bounding rectangle.  Every call is recorded."""
    with_prev_mask = True

    def __init__(self):
        self.calls = []

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        assert as_prompt_type in (0, 1, 2)
        B, _, H, W = image.shape
        n = points.shape[1] // 2
        yy = torch.arange(H, dtype=torch.float32)[:, None]
        xx = torch.arange(W, dtype=torch.float32)[None, :]
        boxes = rects = None
        if as_prompt_type == 1:
            boxes = prompts[1]
            assert prompts[0] is points and prompts[2] is None
            assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 5)
        if as_prompt_type == 2:
            scr, rects = prompts[2]
            assert tuple(scr.shape) == (B, 1, 1000, 2) and tuple(rects.shape) == (B, 1, 4)
        self.calls.append(dict(type=as_prompt_type, size=(H, W), rows=B, prompts=prompts,
                               slots=None if boxes is None else [int(s) for s in boxes[:, 4]]))
        out = []
        for b in range(B):
            x = image[b]
            logit = 8.0 * (x[:3].mean(0) - 0.5) + 2.0 * (x[3] - 0.5)
            for j in range(points.shape[1]):
                r, c, _ = (float(v) for v in points[b, j])
                if r < 0:
                    continue
                logit = logit + (6.0 if j < n else -6.0) * torch.exp(-((yy - r) ** 2 + (xx - c) ** 2) / 18.0)
            if boxes is not None and int(boxes[b, 4]) >= 0:
                xc, yc, bw, bh, slot = (int(v) for v in boxes[b])
                pol, within = (0, slot) if slot < n else (1, slot - n)
                bump = torch.exp(-((yy - yc) ** 2 / (bh * bh + 4.0) + (xx - xc) ** 2 / (bw * bw + 4.0)))
                logit = logit + (1.5 if pol == 0 else -1.5) * (1.0 + 0.5 * within) * bump
            if rects is not None:
                xc, yc, bw, bh = (int(v) for v in rects[b, 0])
                logit = logit + 1.5 * torch.exp(-((yy - yc) ** 2 / (bh * bh + 4.0) + (xx - xc) ** 2 / (bw * bw + 4.0)))
            out.append(logit[None, None])
        return {"instances": torch.cat(out, 0), "instances_aux": None}


ZOOM = dict(target_size=(32, 32), min_crop_size=12)
KW = dict(max_iou_thr=0.8, pred_thr=0.49, min_clicks=1, max_clicks=6)
SCHEDULES = {"box_first": (1, 0), "by_iou": lambda k, iou: int(iou < 0.3)}


def _predictor(skip_clicks=-1, net=None, **kw):
    return get_predictor(net or StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=dict(skip_clicks=skip_clicks, **ZOOM),
                         **kw)


def _tuples(clicks):
    return [(c.is_positive, int(c.coords[0]), int(c.coords[1]), c.indx) for c in clicks]


def _sequential(ds, pred, schedule, **kw):
    out = []
    for i in range(len(ds)):
        s = ds.get_sample(i)
        for oid in s.objects_ids:
            clicks, ious, _ = evaluate_sample(s.image, s.gt_mask(oid), pred, as_prompt_type=schedule, **kw)
            out.append((_tuples(clicks), ious))
    return out


_SEQ = {}


def _seq_reference(name, skip_clicks):
    """The sequential series of a schedule, computed once per zoom setting and shared by the K cases."""
    if (name, skip_clicks) not in _SEQ:
        net = StubNet()
        _SEQ[name, skip_clicks] = (_sequential(Dataset(), _predictor(skip_clicks, net), SCHEDULES[name], **KW), net)
    return _SEQ[name, skip_clicks]


# ---------------------------------------------------------------------------------------------- 1. cascade_step = 1
SCRIPT_PARAMS = dict(cascade_step=1, cascade_adaptive=False, cascade_clicks=1)      # evaluate_vpumodel.py:160-165, --cf-n 0


def test_predictor_from_the_evaluation_scripts_dictionary(host_transforms):
    ds = Dataset(sizes=((40, 56),), per_image=(1,))
    image, gt = ds.get_sample(0).image, ds.get_sample(0).gt_mask(0)
    with_keys = _predictor(predictor_params=dict(SCRIPT_PARAMS))
    assert (with_keys.cascade_step, with_keys.cascade_adaptive, with_keys.cascade_clicks) == (1, False, 1)
    assert get_predictor(StubNet(), "NoBRS", "cpu", predictor_params=dict(SCRIPT_PARAMS, cascade_adaptive=True)).cascade_adaptive
    a = evaluate_sample(image, gt, with_keys, max_iou_thr=2.0, max_clicks=3)
    b = evaluate_sample(image, gt, _predictor(), max_iou_thr=2.0, max_clicks=3)
    assert _tuples(a[0]) == _tuples(b[0]) and len(a[1]) == 3
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # the caller's prev_mask: dropped while len(clicks) <= cascade_clicks (base.py:111, :64), used afterwards
    given = torch.full((1, 1) + gt.shape, 0.75)
    for call in ("get_prediction", "get_vqu_prediction"):
        extra = dict(gt_mask=gt) if call == "get_vqu_prediction" else {}
        first = lambda x: x[0] if isinstance(x, tuple) else x

        def run(params, masks):
            pred = get_predictor(StubNet(), "NoBRS", "cpu", with_flip=False, zoom_in_params=None, predictor_params=params)
            pred.set_input_image(image)
            clicker, maps, mask = Clicker(gt_mask=gt), [], np.zeros(gt.shape, bool)
            for prev in masks:
                clicker.make_next_click(mask)
                maps.append(first(getattr(pred, call)(clicker, prev_mask=prev, **extra)))
                mask = maps[-1] > 0.49
            return maps
        plain = run(None, [None, None])
        plain_given = run(None, [given, given])
        cascade = run(dict(SCRIPT_PARAMS), [given, given])
        assert not np.array_equal(plain[0], plain_given[0])              # the stub reads the mask it is given
        assert np.array_equal(cascade[0], plain[0]), call                # first click: ignored
        second_used = run(None, [None, given])[1]
        assert np.array_equal(cascade[1], second_used), call             # second click: used
        assert not np.array_equal(cascade[1], plain[1])


# ---------------------------------------------------------------------------------------------- 2. the normaliser
def test_prompt_schedule_normaliser():
    s = prompt_schedule(1)
    assert isinstance(s, PromptSchedule) and s.constant == 1 and s.values == {1} and [s(k, 0.5) for k in range(3)] == [1, 1, 1]
    assert prompt_schedule(s) is s
    s = prompt_schedule((1, 0))
    assert s.constant is None and s.values == {0, 1} and [s(k, 0) for k in range(4)] == [1, 0, 0, 0]
    s = prompt_schedule([0, 0, 1])
    assert [s(k, 0) for k in range(5)] == [0, 0, 1, 1, 1]                # the last element repeats
    assert prompt_schedule(np.int64(2)).constant == 2 and prompt_schedule((0, 2)).values == {0, 2}
    seen = []
    s = prompt_schedule(lambda k, iou: seen.append((k, iou)) or (2 if iou > 0.5 else k % 2))
    assert s.constant is None and s.values is None
    assert [s(0, 0), s(1, 0.25), s(2, 0.75)] == [0, 1, 2] and seen == [(0, 0), (1, 0.25), (2, 0.75)]
    for bad in (3, "x", -1, (0, 3), (), [1, "x"], None, 1.0):
        with pytest.raises(ValueError):
            prompt_schedule(bad)
    with pytest.raises(ValueError):
        prompt_schedule(lambda k, iou: 3)(0, 0)
    with pytest.raises(ValueError):
        evaluate_sample(np.zeros((8, 8, 3), np.uint8), np.ones((8, 8), np.int32), _predictor(), 0.9, as_prompt_type=3)


# ---------------------------------------------------------------------------------------------- 3. sequential
def test_sequential_box_first_then_clicks(host_transforms):
    ds = Dataset(sizes=((60, 80), (48, 48)), per_image=(2, 1))
    for skip_clicks in (-1, 0):
        for i in range(len(ds)):
            sample = ds.get_sample(i)
            for oid in sample.objects_ids:
                net, seen = StubNet(), []
                pred = _predictor(skip_clicks, net)
                clicks, ious, _ = evaluate_sample(sample.image, sample.gt_mask(oid), pred, as_prompt_type=(1, 0),
                                                  callback=lambda *a: seen.append((a[5], a[10])), **KW)
                assert seen == [(k, 1 if k == 0 else 0) for k in range(len(ious))]
                types = [c["type"] for c in net.calls]
                if skip_clicks == -1:          # no recalculation: one network call per click
                    assert types == [1] + [0] * (len(ious) - 1)
                else:                          # a re-run click goes through get_prediction: click prompts
                    assert types[0] == 1 and types.count(1) == 1
    # a stateful callable is asked exactly once per click, also when ZoomIn re-runs a click
    reruns = 0
    for i in range(len(ds)):
        sample = ds.get_sample(i)
        for oid in sample.objects_ids:
            net, asked, seen = StubNet(), [], []
            schedule = lambda k, iou: asked.append((k, float(iou))) or len(asked) % 2
            clicks, ious, _ = evaluate_sample(sample.image, sample.gt_mask(oid), _predictor(0, net), as_prompt_type=schedule,
                                              callback=lambda *a: seen.append(a[10]), **KW)
            assert [k for k, _ in asked] == list(range(len(ious)))
            assert np.array_equal(np.float32([v for _, v in asked]), np.float32([0.0] + list(ious[:-1])))     # the IoU of the click before
            assert seen == [(k + 1) % 2 for k in range(len(ious))]
            reruns += len(net.calls) - len(ious)
    assert reruns > 0


# ---------------------------------------------------------------------------------------------- 4. batched = sequential
def _batched(ds, pred, K, schedule, **kw):
    runner = batched.BatchedEvaluator(pred, K, as_prompt_type=schedule, **kw)
    return [(_tuples(clicks), ious) for clicks, ious in runner.run(vpu_evaluation.dataset_objects(ds))]


def _mark_steps(monkeypatch, net):
    orig = batched.BatchedEvaluator._step

    def step(self, *a, **k):
        net.calls.append("step")
        return orig(self, *a, **k)
    monkeypatch.setattr(batched.BatchedEvaluator, "_step", step)


def _steps(net):
    steps = [[]]
    for c in net.calls:
        if c == "step":
            steps.append([])
        else:
            steps[-1].append(c)
    return steps


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("skip_clicks", [-1, 0])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_batched_schedule_equals_sequential(host_transforms, monkeypatch, name, skip_clicks, K):
    seq, seq_net = _seq_reference(name, skip_clicks)
    lens = [len(i) for _, i in seq]
    assert len(seq) == 8 and min(lens) < 6 and max(lens) == 6, lens         # early stops and full budgets: refill, tail
    assert {c["type"] for c in seq_net.calls} == {0, 1}
    net = StubNet()
    _mark_steps(monkeypatch, net)
    got = _batched(Dataset(), _predictor(skip_clicks, net), K, SCHEDULES[name], **KW)
    assert len(got) == len(seq)
    for (cs, i_s), (cb, i_b) in zip(seq, got):
        assert cs == cb
        assert i_s.dtype == i_b.dtype and np.array_equal(i_s, i_b)
    # one forward per (step, network size); a forward is type 1 exactly when one of its rows carries a box
    mixed = 0
    for calls in _steps(net):
        sizes = [c["size"] for c in calls]
        assert len(sizes) == len(set(sizes)), sizes
        for c in calls:
            assert (c["type"] == 1) == (c["slots"] is not None and any(s >= 0 for s in c["slots"]))
            mixed += c["slots"] is not None and min(c["slots"]) < 0 <= max(c["slots"])
    print(f"[schedule] {name} skip_clicks={skip_clicks} K={K}: forwards with box rows and -1 rows: {mixed}")
    # every forward of a run that zooms from the first click on has the target size, and K < 8 objects means refills: the
    # box click of a refilled object shares its forward with the click rows of the others
    if skip_clicks == -1 and K < 8:
        assert mixed > 0
    series, secs = evaluate_dataset(Dataset(), _predictor(skip_clicks), batch_objects=K, as_prompt_type=SCHEDULES[name],
                                    batch_box_prompts=True, **KW)
    assert [s.tolist() for s in series] == [i.tolist() for _, i in seq] and secs >= 0


# ---------------------------------------------------------------------------------------------- 5. overflow
def test_overflow_repeats_only_the_objects_of_its_sub_batch(host_transforms, monkeypatch):
    seq, _ = _seq_reference("box_first", -1)
    net = StubNet()
    flagged, repeated, state = [], [], dict(inside=False, n=0)
    orig_boxes, orig_host = batched._HostOps.boxes, batched._host_boxes

    def overflowing(self, rows, first, points_nd, n_batch, size, target_size, flag):
        state["n"] += 1
        if state["n"] >= 2 and len(flagged) < 3:      # (the first call holds the first K objects: a whole forward)
            self.flags[flag] = 1
            flagged.append((sorted({r[0].order for r in rows}), len(rows), len(net.calls)))
            return torch.full((len(rows), 5), 7, dtype=torch.int32)           # boxes of a truncated table: never used
        state["inside"] = True
        try:
            return orig_boxes(self, rows, first, points_nd, n_batch, size, target_size, flag)
        finally:
            state["inside"] = False

    def host(rows, *a, **k):
        if not state["inside"]:             # called by the step itself: the repeat of a flagged sub-batch
            repeated.append(sorted({r[0].order for r in rows}))
        return orig_host(rows, *a, **k)
    monkeypatch.setattr(batched._HostOps, "boxes", overflowing)
    monkeypatch.setattr(batched, "_host_boxes", host)
    got = _batched(Dataset(), _predictor(-1, net), 3, (1, 0), **KW)
    assert len(flagged) == 3 and repeated == [f[0] for f in flagged]
    # a flagged sub-batch shared its forward with rows that kept their results
    assert any(net.calls[at]["rows"] > n_rows for _, n_rows, at in flagged)
    for (cs, i_s), (cb, i_b) in zip(seq, got):
        assert cs == cb and np.array_equal(i_s, i_b)


# ---------------------------------------------------------------------------------------------- 6. dispatch
def test_dispatch_of_schedules(host_transforms, monkeypatch):
    seq, _ = _seq_reference("box_first", -1)
    want = [i.tolist() for _, i in seq]
    used = []
    orig = batched.BatchedEvaluator.__init__

    def spy(self, predictor, K, *a, **k):
        used.append((K, k.get("as_prompt_type")))
        orig(self, predictor, K, *a, **k)
    monkeypatch.setattr(batched.BatchedEvaluator, "__init__", spy)
    monkeypatch.setenv("VPU_EVAL_PROMPTS", "1,0")
    series, _ = evaluate_dataset(Dataset(), _predictor(), batch_objects=3, batch_box_prompts=True, **KW)
    assert used == [(3, (1, 0))] and [s.tolist() for s in series] == want
    # a schedule that can yield 1 needs the box opt-in: without it the run stays sequential, with the same series
    series, _ = evaluate_dataset(Dataset(), _predictor(), batch_objects=3, **KW)
    assert len(used) == 1 and [s.tolist() for s in series] == want
    # an explicit argument wins over the environment
    ds = Dataset(sizes=((40, 56),), per_image=(2,))
    evaluate_dataset(ds, _predictor(), batch_objects=3, as_prompt_type=0, max_iou_thr=0.8, max_clicks=2)
    assert used[1:] == [(3, 0)]
    monkeypatch.setenv("VPU_EVAL_PROMPTS", "1,x")
    with pytest.raises(ValueError, match="VPU_EVAL_PROMPTS"):
        evaluate_dataset(ds, _predictor(), max_iou_thr=0.8)
    monkeypatch.delenv("VPU_EVAL_PROMPTS")
    del used[:]
    assert batched.batchable(_predictor(), None, (1, 0)) and batched.batchable(_predictor(), None, lambda k, iou: 0)
    assert not batched.batchable(_predictor(), None, (0, 2))
    # a callable may return 1: it needs the opt-in too
    evaluate_dataset(ds, _predictor(), batch_objects=3, as_prompt_type=lambda k, iou: 0, max_iou_thr=0.8, max_clicks=2)
    assert used == []
    # a callable that returns 2 inside the batched loop
    with pytest.raises(ValueError, match="sequential"):
        evaluate_dataset(ds, _predictor(), batch_objects=3, batch_box_prompts=True, as_prompt_type=lambda k, iou: 2 * (k > 0),
                         max_iou_thr=2.0, max_clicks=3)
    assert len(used) == 1
    # a sequence that holds a 2 is dispatched to the sequential loop
    calls = []
    monkeypatch.setattr(vpu_evaluation, "evaluate_sample",
                        lambda image, gt_mask, predictor, **kw: calls.append(kw) or ([], np.zeros(1, np.float32), None))
    evaluate_dataset(ds, _predictor(), batch_objects=3, batch_box_prompts=True, as_prompt_type=(2, 0), max_iou_thr=0.8)
    assert len(used) == 1 and len(calls) == 2 and all(kw["as_prompt_type"] == (2, 0) for kw in calls)
    with pytest.raises(AssertionError):
        batched.BatchedEvaluator(_predictor(), 4, 0.8, as_prompt_type=(2, 0))


# ---------------------------------------------------------------------------------------------- 7. scribbles, sequential
def test_sequential_scribble_prompt_is_cal_scribble_on_the_flipped_cropped_ground_truth(host_transforms):
    ds = Dataset(sizes=((60, 80),), per_image=(2,))
    image, gt = ds.get_sample(0).image, ds.get_sample(0).gt_mask(1)
    net = StubNet()
    pred = _predictor(-1, net)
    pred.set_input_image(image)
    clicker, mask = Clicker(gt_mask=gt), np.zeros(gt.shape, bool)
    for k, seed in enumerate((3, 11)):
        clicker.make_next_click(mask)
        random.seed(seed); np.random.seed(seed)
        probs, prompts = pred.get_vqu_prediction(clicker, gt_mask=gt, as_prompt_type=2, click_indx=k)
        rows = torch.from_numpy(gt.astype(np.float32))[None, None]
        rows = torch.cat([rows, torch.flip(rows, dims=[3])], 0)
        assert pred.zoom_in._object_roi is not None
        rows = crop_resize(rows, pred.zoom_in._object_roi, pred.zoom_in.target_size)
        random.seed(seed); np.random.seed(seed)
        want = cal_scribble(rows.numpy()[:, 0] > 0.5)
        assert tuple(prompts[1].shape) == (2, 5)
        for got_a, want_a in zip(prompts[2], want):
            assert got_a.dtype == want_a.dtype and np.array_equal(got_a, want_a)
        assert want[1].any() and not np.array_equal(want[0][0], want[0][1])       # a stroke per row; the flip row has its own
        assert net.calls[-1]["type"] == 2 and net.calls[-1]["prompts"][2] is prompts[2]
        mask = probs > 0.49
    # types 0 and 1 return what they returned before: no scribble
    for ptype in (0, 1):
        clicker.make_next_click(mask)
        probs, prompts = pred.get_vqu_prediction(clicker, gt_mask=gt, as_prompt_type=ptype, click_indx=2)
        assert prompts[2] is None and (prompts[1] is None) == (ptype == 0)
        mask = probs > 0.49
    # and through evaluate_sample: scribble first, then clicks
    net = StubNet()
    random.seed(5); np.random.seed(5)
    _, ious, _ = evaluate_sample(image, gt, _predictor(-1, net), as_prompt_type=(2, 0), max_iou_thr=2.0, max_clicks=3)
    assert [c["type"] for c in net.calls] == [2, 0, 0] and np.isfinite(ious).all()
