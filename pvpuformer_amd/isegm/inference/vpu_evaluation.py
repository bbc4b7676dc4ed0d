"""NoBRS evaluation protocol, call-compatible with isegm/inference/vpu_evaluation.py:18-98: ``evaluate_dataset(dataset,
predictor, **kwargs)`` -> (list of per-object IoU series, elapsed seconds), ``evaluate_sample(image, gt_mask, predictor,
max_iou_thr, pred_thr=0.49, min_clicks=1, max_clicks=20, sample_id=None, callback=None)`` -> (clicks, IoU series,
last probability map).  Per click: the Clicker puts the next oracle click at the deepest point of the larger error
region, the predictor runs the network on (image, previous prediction, clicks [+ box prompt]) through its transform
pipeline, the IoU at ``pred_thr`` is recorded, and the loop stops once ``max_iou_thr`` is reached after ``min_clicks``.
As shipped the reference always evaluates with click prompts (``as_prompt_type = 0``, vpu_evaluation.py:51); the
alternatives its authors kept as comments there (vpu_evaluation.py:49-76: a box on the first click then clicks, a random
mix, a choice by the last IoU) are per-click schedules, which ``as_prompt_type`` expresses here (``prompt_schedule``)."""
import numbers
import os
import time

import numpy as np
import torch

from . import batched, utils
from .clicker import Clicker


class PromptSchedule:
    """The prompt type of every click, ``schedule(click_indx, last_iou) -> 0 (click) | 1 (box) | 2 (scribble)``, from an
    ``as_prompt_type`` given as

    * an int: that type on every click (``constant`` holds it);
    * a sequence of ints: element k for click k, the last one repeats -- ``(1, 0)`` is a box first, then clicks;
    * a callable ``f(click_indx, last_iou) -> int``; ``last_iou`` is 0 before the first click (vpu_evaluation.py:44).

    ``values``: the types it can yield, None for a callable (not known before it is asked).  The evaluation loops ask it
    exactly once per (object, click): a click that is re-run keeps the type it was given."""

    def __init__(self, spec):
        self.constant, self.values, self._seq, self._fn = None, None, None, None
        if isinstance(spec, numbers.Integral) and not isinstance(spec, bool):
            self.constant = self._checked(spec)
            self._seq = (self.constant,)
        elif callable(spec):
            self._fn = spec
        elif isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__") or not hasattr(spec, "__getitem__") or len(spec) == 0:
            raise ValueError(f"as_prompt_type must be an int, a non-empty sequence of ints or a callable, got {spec!r}")
        else:
            self._seq = tuple(self._checked(v) for v in spec)
        if self._seq is not None:
            self.values = frozenset(self._seq)

    @staticmethod
    def _checked(v):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) not in (0, 1, 2):
            raise ValueError(f"prompt type must be 0 (clicks), 1 (box) or 2 (scribble), got {v!r}")
        return int(v)

    def __call__(self, click_indx, last_iou=0):
        if self._fn is not None:
            return self._checked(self._fn(click_indx, last_iou))
        return self._seq[min(click_indx, len(self._seq) - 1)]


def prompt_schedule(as_prompt_type):
    """``as_prompt_type`` (int, sequence or callable; see ``PromptSchedule``) as a ``PromptSchedule``; ``ValueError`` for
    anything else and for types outside {0, 1, 2}."""
    return as_prompt_type if isinstance(as_prompt_type, PromptSchedule) else PromptSchedule(as_prompt_type)


def click_series(image, gt_mask, predictor, pred_thr=0.49, max_clicks=20, as_prompt_type=0):
    """Generator over the clicks of one object: yields (click index, probability map, IoU, clicker, prompts, prompt type of
    this click)."""
    schedule = prompt_schedule(as_prompt_type)
    clicker = Clicker(gt_mask=gt_mask)
    mask = np.zeros(gt_mask.shape, dtype=bool)
    predictor.set_input_image(image)
    iou = 0
    for k in range(max_clicks):
        clicker.make_next_click(mask)
        ptype = schedule(k, iou)        # asked once: a ZoomIn recalculation re-runs the click inside the predictor
        probs, prompts = predictor.get_vqu_prediction(clicker, gt_mask=gt_mask, as_prompt_type=ptype, click_indx=k,
                                                      as_multi_prompts=True)
        mask = probs > pred_thr
        iou = utils.get_iou(gt_mask, mask)
        yield k, probs, iou, clicker, prompts, ptype


def evaluate_sample(image, gt_mask, predictor, max_iou_thr, pred_thr=0.49, min_clicks=1, max_clicks=20, sample_id=None,
                    callback=None, as_prompt_type=0):
    ious, probs, clicker = [], None, None
    # the callback (the reference's visualisation hook, vpu_evaluation.py:84-97) is the one consumer of ``prompts`` in this
    # protocol: with one attached the predictor derives the box prompt on every click as the reference does (base.py:176)
    keep = getattr(predictor, "always_simulate_prompts", None)
    if callback is not None and keep is not None:
        predictor.always_simulate_prompts = True
    try:
        return _evaluate_sample(image, gt_mask, predictor, max_iou_thr, pred_thr, min_clicks, max_clicks, sample_id, callback,
                                as_prompt_type)
    finally:
        if keep is not None:
            predictor.always_simulate_prompts = keep


def _evaluate_sample(image, gt_mask, predictor, max_iou_thr, pred_thr, min_clicks, max_clicks, sample_id, callback, as_prompt_type):
    ious, probs, clicker = [], None, None
    with torch.no_grad():
        for k, probs, iou, clicker, prompts, ptype in click_series(image, gt_mask, predictor, pred_thr, max_clicks,
                                                                   as_prompt_type):
            ious.append(iou)
            reached = iou >= max_iou_thr and k + 1 >= min_clicks
            if callback is not None:
                callback(image, gt_mask, probs, iou, sample_id, k, clicker.clicks_list, reached, predictor.zoom_in, prompts,
                         ptype)
            if reached:
                break
    return (clicker.clicks_list if clicker is not None else []), np.array(ious, dtype=np.float32), probs


def evaluate_dataset(dataset, predictor, batch_objects=None, batch_box_prompts=None, **kwargs):
    """``dataset``: anything with ``len()`` and ``get_sample(i)`` returning an object with ``image``, ``objects_ids``
    and ``gt_mask(object_id)`` (the contract of the reference's isegm.data datasets).

    ``batch_objects`` (not in the reference; default: environment ``VPU_EVAL_BATCH``, else 1): K > 1 evaluates up to K
    objects at once, in lock-step through one batched forward per click (``batched.BatchedEvaluator``), and returns the
    same per-object IoU series in the same order.  That path applies only to a ``BasePredictor`` whose transforms are
    [ZoomIn with a (height, width) target_size] [SigmoidForPred] [AddHorizontalFlip], without ``callback`` and with
    click prompts (``as_prompt_type == 0``) or, when asked for, box prompts or a schedule of the two; in every other case
    the objects are silently evaluated one at a time, as with K = 1.

    ``batch_box_prompts`` (default: environment ``VPU_EVAL_BATCH_BOX`` = 1, else off): box prompts (``as_prompt_type == 1``,
    or a schedule that can yield 1) take the batched path too, with the boxes derived on the device.  It is an opt-in
    because callers and tests rely on box-prompt evaluation staying on the sequential loop by default.

    ``as_prompt_type`` (int, sequence or callable: ``PromptSchedule``; not passed: environment ``VPU_EVAL_PROMPTS``,
    comma-separated ints such as ``1,0``, else 0): the prompt type of every click."""
    if batch_objects is None:
        batch_objects = int(os.environ.get("VPU_EVAL_BATCH", "1") or 1)
    if batch_box_prompts is None:
        batch_box_prompts = os.environ.get("VPU_EVAL_BATCH_BOX", "0") == "1"
    if "as_prompt_type" not in kwargs and os.environ.get("VPU_EVAL_PROMPTS", "").strip():
        try:
            types = tuple(int(v) for v in os.environ["VPU_EVAL_PROMPTS"].split(","))
        except ValueError:
            raise ValueError(f"VPU_EVAL_PROMPTS must be comma-separated ints, got {os.environ['VPU_EVAL_PROMPTS']!r}") from None
        kwargs["as_prompt_type"] = types[0] if len(types) == 1 else types
    ptype = kwargs.get("as_prompt_type", 0)
    schedule = prompt_schedule(ptype)
    may_box = schedule.values is None or 1 in schedule.values
    if batch_objects > 1 and kwargs.get("max_clicks", 20) >= 1 and (not may_box or batch_box_prompts) and \
            batched.batchable(predictor, kwargs.get("callback"), ptype):
        return _evaluate_dataset_batched(dataset, predictor, batch_objects, **kwargs)
    started = time.time()
    series = []
    for index in range(len(dataset)):
        sample = dataset.get_sample(index)
        series += [evaluate_sample(sample.image, sample.gt_mask(oid), predictor, sample_id=index, **kwargs)[1]
                   for oid in sample.objects_ids]
    return series, time.time() - started


def dataset_objects(dataset):
    """(image, ground truth) of every object, in dataset order, then ``objects_ids`` order."""
    for index in range(len(dataset)):
        sample = dataset.get_sample(index)
        for oid in sample.objects_ids:
            yield sample.image, sample.gt_mask(oid)


def _evaluate_dataset_batched(dataset, predictor, batch_objects, max_iou_thr, pred_thr=0.49, min_clicks=1, max_clicks=20,
                              callback=None, as_prompt_type=0):
    started = time.time()
    runner = batched.BatchedEvaluator(predictor, batch_objects, max_iou_thr, pred_thr, min_clicks, max_clicks,
                                      as_prompt_type=as_prompt_type)
    series = [ious for _, ious in runner.run(dataset_objects(dataset))]
    return series, time.time() - started
