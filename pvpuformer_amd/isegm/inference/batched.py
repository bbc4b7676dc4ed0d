"""Batched NoBRS evaluation: K objects step through the click loop of ``evaluate_sample`` in lock-step, each step one
network forward at batch 2K (K with no flip) instead of K forwards at batch 2, and ONE device-to-host copy.

Each of the K slots holds one object's state: image, ground truth, previous-prediction canvas, the Clicker bookkeeping
(click list, not-clicked map) and the ZoomIn state (object roi, box of the last prediction).  Per step:

1. host: the next click of every slot from the click keys read back last step, the ZoomIn transform (``Roi`` does the
   integer work, as in ``ZoomIn.transform``), the click tokens of all 2K click lists packed by ``get_points_nd``;
2. device: ``vpu_roi_resize_batched`` builds the network input (crop, resize, mirror), the network runs, the flip average
   and the sigmoid are the predictor's own transforms on the whole batch, ``vpu_roi_paste_batched`` pastes every map into
   its canvas and counts the IoU and the ZoomIn box, ``vpu_click_keys_batched`` finds the next oracle clicks;
3. one read-back of 48 bytes per object (two click keys, IoU counts, box); a slot whose object stops takes the next one.

The results equal the sequential loop's object by object: every per-object operation is the sequential one (same
interpolation formula, same counts, same keys); what the batch shares is only the network, whose click tokens are padded
to a common count with not-a-point rows that the network ignores.  ``evaluate_dataset`` dispatches here; see
``batchable`` for when it may.  The same scheduler runs on the host with torch / scipy stand-ins of the three kernels
(``_HostOps``), which is what the CPU tests check it with.

Box prompts (``as_prompt_type=1``).  ``BasePredictor.get_vqu_prediction`` derives the box of every click from the previous
prediction and the ground truth (``prompt_sim.get_next_promts``: several read-backs, a host scan over the connected
components, and a simulated next click that is thrown away).  Here ``vpu_box_prompts_batched`` derives the boxes of all
rows of a size group on the device, between the resize and the forward, and hands the ``int32 [rows, 5]`` tensor to the
network: the step keeps its one read-back.  Reproduced as the sequential path has them:

* the flip copy's box is NOT the mirror image of the straight one: the sequential code flips ground truth and previous
  prediction first and crops both with the same, un-mirrored ZoomIn roi, so that row reads source column ``W - 1 - c``
  inside the un-mirrored roi;
* ``max_connected_regions``' merge rule (every component above 10 % of the foreground joins the largest so far);
* the slot: computed in the object's own click layout (``n_obj = max(#positive, #negative, 1)`` rows per polarity) and
  moved into the batch's padded layout (``_padded_slot``); in the false-negative case it is the object's last positive
  row, which may hold a real click that the box then replaces, as in the reference;
* the ground truth is resized as the float values 1 / 0 / -1 (ignore), which is what the sequential path uploads;
* a click whose ZoomIn recalculation fires is re-run by ``get_prediction``, which is click-only: an object with ``recalc``
  set re-runs as prompt type 0, so the groups of a step are keyed by (size, prompt type).

More components in a group than the kernel's table holds (salt-and-pepper masks; 1024 per row) raise a flag that comes
back with the read-back; the forward of that group is discarded and its objects repeat the click with boxes from the host
code (``_host_boxes``: ``crop_resize`` + ``prompt_sim.cal_box``, also ``_HostOps``' stand-in).  The sequential path also
runs ``prompt_sim.next_click`` on every box-prompt click and so advances the global numpy generator for a click it
discards; the batched path does not.  No result depends on it (the evaluation clicks come from the Clicker).

Prompt schedules (``as_prompt_type`` a sequence or a callable, ``vpu_evaluation.PromptSchedule``).  Every object carries
the type of its current click (asked once, when the click is made; a repeated click keeps it).  With a constant type the
groups are the ones above.  With a schedule the objects of a step that share a network input size go through ONE forward,
whatever their types: the box rows are still derived in sub-batches keyed by (mask size, host fallback) and scattered on the
device into an ``int32 [rows, 5]`` tensor pre-filled with (0, 0, 0, 0, -1); a negative slot tells the model that the row
carries no box, and it computes that row exactly as under ``as_prompt_type=0`` (``is_vpu_model.forward``).  The forward is
``as_prompt_type=1`` when at least one row has a box and a plain type-0 call when none has.  An overflow flag repeats the
click of the objects of its sub-batch only; the other rows of the same forward keep their results."""
import ctypes as C
import struct

import numpy as np
import torch

from ._batchcore import ZoomHost, host_count_box, host_roi_paste, host_roi_resize, upload_structs
from .clicker import Click
from .transforms import AddHorizontalFlip, Roi, SigmoidForPred, ZoomIn, crop_resize

_STATS = 2           # int64 offset of the int32 statistics in an object's 6-int64 output slot
_MASK64 = 0xFFFFFFFFFFFFFFFF
_BOX_PRED_THRESH = 0.49    # get_next_promts' default pred_thresh (get_vqu_prediction does not pass one)
_FLAGS_PER_ROW = 12        # int32 flags in one 48-byte row appended to the read-back


def batchable(predictor, callback=None, as_prompt_type=0):
    """True when ``evaluate_dataset`` may run ``predictor`` batched: a ``BasePredictor`` whose transforms are only
    [ZoomIn with a (height, width) target_size] [SigmoidForPred] [AddHorizontalFlip] (in that order, each optional), no
    callback and click or box prompts: ``as_prompt_type`` 0 or 1, a sequence of those, or a callable (scribbles are not
    batched, so type 2 and every sequence that holds a 2 stay sequential; a callable is only known to return 2 when it
    does: ``BatchedEvaluator`` raises then)."""
    from .predictors.base import BasePredictor
    from .vpu_evaluation import prompt_schedule
    values = prompt_schedule(as_prompt_type).values
    if not isinstance(predictor, BasePredictor) or callback is not None or (values is not None and 2 in values):
        return False
    ts, i = list(predictor.transforms), 0
    if i < len(ts) and type(ts[i]) is ZoomIn:
        if ts[i] is not predictor.zoom_in or not isinstance(ts[i].target_size, tuple) or len(ts[i].target_size) != 2:
            return False
        i += 1
    elif predictor.zoom_in is not None:
        return False
    for kind in (SigmoidForPred, AddHorizontalFlip):
        if i < len(ts) and type(ts[i]) is kind:
            i += 1
    return i == len(ts)


def decode_key(key, width):
    """(value, (row, col)) of a packed click key (vpu_masked_argmax): Clicker._deepest_errors_device's decoding."""
    key = int(key) & _MASK64
    value = struct.unpack("<f", struct.pack("<I", key >> 32))[0]
    return value, divmod(0xFFFFFFFF - (key & 0xFFFFFFFF), width)


def _load_image(image, device):
    """``BasePredictor.set_input_image``'s conversion -> fp32 [3, H, W] on ``device``."""
    if isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float()
        image = t / 255.0 if image.dtype == np.uint8 else t
    image = image.to(device)
    if image.dim() == 4:
        image = image[0]
    return image.float().contiguous()


def _padded_slot(loc, n_obj, n_batch):
    """Slot ``loc`` of an object's own click layout (``n_obj`` rows per polarity) in the layout padded to ``n_batch`` rows."""
    return loc if loc < n_obj else n_batch + (loc - n_obj)


def _host_boxes(rows, points_nd, n_batch, size, target_size, pred_thresh=_BOX_PRED_THRESH):
    """Box prompts int32 [len(rows), 5] by the sequential recipe (base.py:114-121 + cal_box) for ``rows`` = (object, roi or
    None, mirror, n_obj), one per row of ``points_nd`` [rows, 2 * n_batch, 3].  Each row is computed alone, as the
    sequential call does its two."""
    from ..engine.prompt_sim import cal_box
    out = np.zeros((len(rows), 5), np.int32)
    pts = points_nd.detach().float().cpu().numpy()
    for i, (o, roi, mirror, n_obj) in enumerate(rows):
        gt = torch.where(o.gt != 0, 1.0, torch.where(o.valid != 0, 0.0, -1.0)).float()[None, None]
        prev = o.canvas[o.prev][None, None]
        if mirror:
            gt, prev = torch.flip(gt, dims=[3]), torch.flip(prev, dims=[3])
        if roi is not None:
            gt, prev = crop_resize(gt, roi, target_size), crop_resize(prev, roi, target_size)
        assert tuple(gt.shape[2:]) == tuple(size)
        g = gt.cpu().numpy()[:, 0] > 0.5
        p = prev.float().cpu().numpy()[:, 0]
        fn, fp = np.logical_and(g, p < pred_thresh), np.logical_and(np.logical_not(g), p > pred_thresh)
        own = np.concatenate([pts[i, :n_obj], pts[i, n_batch:n_batch + n_obj]], 0)[None]
        box = cal_box(g, fn, fp, own, as_allmask=False, jitter_box=False)[0]
        if box.any():
            box[4] = _padded_slot(int(box[4]), n_obj, n_batch)
        out[i] = box
    return out


class _Object:
    """One object's evaluation state (a slot of the batch)."""

    def __init__(self, order, image, gt_mask, device):
        self.order = order
        self.image = image
        self.H, self.W = int(gt_mask.shape[0]), int(gt_mask.shape[1])
        assert tuple(image.shape[1:]) == (self.H, self.W), "image and ground truth sizes differ"
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device)
        self.gt, self.valid = up(gt_mask == 1), up(gt_mask != -1)           # Clicker: gt_mask == 1, != ignore_label
        self.keep = torch.ones(self.H, self.W, device=device, dtype=torch.uint8)
        self.mask = torch.zeros(self.H, self.W, device=device, dtype=torch.uint8)
        self.canvas = [torch.zeros(self.H, self.W, device=device, dtype=torch.float32) for _ in range(2)]
        self.prev = 0                  # canvas[prev] is the predictor's prev_prediction
        self.clicks, self.ious = [], []
        self.roi = None                # ZoomIn._object_roi
        self.box = None                # (count, r0, r1, c0, c1) of ZoomIn._probs > prob_thresh (no clicks); None: no _probs
        self.keys = None               # click keys of the current mask
        self.clear_at = -1             # pixel of the click made this step (cleared in the not-clicked map)
        self.recalc = False            # re-run the current click (ZoomIn.check_possible_recalculation fired)
        self.host_box = False          # re-run the current click with boxes from the host (component table overflow)
        self.ptype = 0                 # prompt type of the current click (asked of the schedule when the click is made)
        self.box_key = None            # (mask size, host fallback) of its box row in the current step; None: no box
        self.done = False
        self.plan = None


class _DeviceOps:
    """The three batched HIP kernels; per step the descriptors go up in one copy and the outputs come back in one."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self.ops, self.device = _lib, ops, torch.device(device)
        self._desc = []

    def begin(self, n_out, n_flags=0):
        self._desc, self._box, self.n_out = [], [], max(n_out, 1)
        self.out = torch.empty(self.n_out + (n_flags + _FLAGS_PER_ROW - 1) // _FLAGS_PER_ROW, 6, device=self.device,
                               dtype=torch.int64)

    def add(self, o, roi, src, out_row, prev=True):
        """Appends one descriptor; returns its index."""
        for t, align in ((o.canvas[0], 16), (o.canvas[1], 16), (o.mask, 4), (o.gt, 4), (o.valid, 4), (o.keep, 4)):
            assert t.data_ptr() % align == 0 and t.is_contiguous()
        r0, r1, c0, c1 = roi
        assert 0 <= r0 <= r1 < o.H and 0 <= c0 <= c1 < o.W and -1 <= o.clear_at < o.H * o.W, (roi, o.H, o.W, o.clear_at)
        d = self._lib.EvalObj()
        d.image, d.prev = o.image.data_ptr(), o.canvas[o.prev].data_ptr() if prev else None
        d.canvas, d.mask = o.canvas[1 - o.prev].data_ptr(), o.mask.data_ptr()
        d.gt, d.valid, d.keep = o.gt.data_ptr(), o.valid.data_ptr(), o.keep.data_ptr()
        d.out = self.out.data_ptr() + out_row * 48
        d.H, d.W = o.H, o.W
        d.r0, d.r1, d.c0, d.c1 = roi
        d.src, d.clear_at = src, o.clear_at
        self._desc.append(d)
        return len(self._desc) - 1

    def add_box(self, o, roi, mirror, n_obj):
        """Appends one row of the box-prompt kernel (``roi`` None: the whole image); returns its index."""
        r0, r1, c0, c1 = roi if roi is not None else Roi.whole(o.H, o.W)
        assert 0 <= r0 <= r1 < o.H and 0 <= c0 <= c1 < o.W and n_obj >= 1, (roi, o.H, o.W, n_obj)
        d = self._lib.BoxRow()
        d.prev, d.gt, d.valid = o.canvas[o.prev].data_ptr(), o.gt.data_ptr(), o.valid.data_ptr()
        d.H, d.W = o.H, o.W
        d.r0, d.r1, d.c0, d.c1 = r0, r1, c0, c1
        d.mirror, d.n_obj = int(mirror), int(n_obj)
        self._box.append(d)
        return len(self._box) - 1

    def upload(self):
        # the box rows ride behind the descriptors in the same copy; _host stays alive until the step's read-back
        self._host, self.desc, (_, self._box_at0) = upload_structs(
            self.device, (self._lib.EvalObj * len(self._desc))(*self._desc), (self._lib.BoxRow * len(self._box))(*self._box))

    def _at(self, i):
        return (self.desc, i * C.sizeof(self._lib.EvalObj))

    def resize(self, objs, first, n, size, flip, channels):
        out = torch.empty((2 if flip else 1) * n, channels, size[0], size[1], device=self.device, dtype=torch.float32)
        self.ops.roi_resize_batched(self._at(first), n, out, size[0], size[1], flip, channels)
        return out

    def paste(self, objs, first, n, probs, pred_thr, box_thr):
        probs = probs.contiguous().float()
        max_hw = max(o.H * o.W for o in objs)
        self.ops.roi_paste_batched(self._at(first), n, probs, probs.shape[-2], probs.shape[-1], pred_thr, box_thr, max_hw)

    def keys(self, objs, first, n):
        Hm = max(o.H for o in objs)
        Wm = (max(o.W for o in objs) + 3) // 4 * 4
        self.ops.click_keys_batched(self._at(first), n, Hm, Wm, max(o.H * o.W for o in objs), self.device)

    def boxes(self, rows, first, points_nd, n_batch, size, target_size, flag):
        """Box prompts int32 [len(rows), 5] of the box rows from ``first`` on, on the device; ``flag``: index of the int32
        behind the read-back records that reports a component table overflow."""
        assert points_nd.shape[0] == len(rows) and all(n_obj <= n_batch for _, _, _, n_obj in rows)
        flags = self.out[self.n_out:].view(torch.int32)
        return self.ops.box_prompts_batched((self.desc, self._box_at0 + first * C.sizeof(self._lib.BoxRow)), len(rows),
                                            points_nd.contiguous(), n_batch, size[0], size[1], _BOX_PRED_THRESH,
                                            (flags, flag))

    def readback(self):
        out = self.out.cpu().numpy()        # the step's one synchronisation
        self.flags = out[self.n_out:].view(np.int32).reshape(-1)      # (the box groups' overflow flags ride behind the records)
        return out[:self.n_out]


class _HostOps:
    """Host stand-ins of the three kernels (torch / scipy, as the Clicker's host path): the scheduler's CPU test bed."""

    def __init__(self, device):
        self.device = device

    def begin(self, n_out, n_flags=0):
        self._desc, self._box = [], []
        self.out = np.zeros((max(n_out, 1), 6), dtype=np.int64)
        self.flags = np.zeros(n_flags, np.int32)

    def add(self, o, roi, src, out_row, prev=True):
        self._desc.append((o, tuple(roi), src, out_row, prev, o.clear_at))
        return len(self._desc) - 1

    def add_box(self, o, roi, mirror, n_obj):
        self._box.append((o, roi, mirror, n_obj))
        return len(self._box) - 1

    def upload(self):
        pass

    def boxes(self, rows, first, points_nd, n_batch, size, target_size, flag):
        assert self._box[first:first + len(rows)] == list(rows)
        return torch.from_numpy(_host_boxes(rows, points_nd, n_batch, size, target_size))

    def resize(self, objs, first, n, size, flip, channels):
        rows = []
        for o, roi, src, _, prev, _ in self._desc[first:first + n]:
            rows.append((src, host_roi_resize(o.image, o.canvas[o.prev] if prev else None, roi, size)))
        batch = torch.cat([r for _, r in sorted(rows, key=lambda t: t[0])], 0)
        return torch.cat([batch, batch.flip(3)], 0) if flip else batch

    def paste(self, objs, first, n, probs, pred_thr, box_thr):
        for o, roi, src, row, _, _ in self._desc[first:first + n]:
            full = host_roi_paste(probs[src, 0], o.H, o.W, roi)
            o.canvas[1 - o.prev].copy_(full)
            m = full.numpy() > np.float32(pred_thr)
            o.mask.copy_(torch.from_numpy(m.astype(np.uint8)))
            g, v = o.gt.numpy() != 0, o.valid.numpy() != 0
            stats = [int((m & g & v).sum()), int(((m | g) & v).sum())] + host_count_box(full.numpy() > np.float32(box_thr), o.H, o.W)
            self.out[row, _STATS:] = np.array(stats + [0], dtype=np.int32).view(np.int64)

    def keys(self, objs, first, n):
        from scipy import ndimage
        for o, _, _, row, _, clear_at in self._desc[first:first + n]:
            if clear_at >= 0:
                o.keep.view(-1)[clear_at] = 0
            m, g, v = o.mask.numpy() != 0, o.gt.numpy() != 0, o.valid.numpy() != 0
            keep = o.keep.numpy().astype(np.float32)
            for e, err in enumerate((g & ~m & v, ~g & m & v)):
                dist = ndimage.distance_transform_edt(np.pad(err, 1)).astype(np.float32)[1:-1, 1:-1] * keep
                at = int(np.argmax(dist))
                bits = int(np.float32(dist.flat[at]).view(np.uint32))
                self.out[row, e] = np.int64(np.uint64((bits << 32) | (0xFFFFFFFF - at)).view(np.int64))

    def readback(self):
        return self.out.copy()


class BatchedEvaluator(ZoomHost):
    """Runs ``evaluate_sample``'s loop (``evaluate_dataset``'s kwargs) over a stream of objects, ``batch_objects`` at a time."""

    def __init__(self, predictor, batch_objects, max_iou_thr, pred_thr=0.49, min_clicks=1, max_clicks=20, as_prompt_type=0):
        assert batchable(predictor, None, as_prompt_type), \
            "the predictor's transforms or the prompt type are not the batched path's (see batchable)"
        from .vpu_evaluation import prompt_schedule
        super().__init__(predictor)
        self.K, self.schedule = int(batch_objects), prompt_schedule(as_prompt_type)
        self.max_iou_thr, self.pred_thr, self.min_clicks, self.max_clicks = max_iou_thr, pred_thr, min_clicks, max_clicks
        self.ops = _DeviceOps(self.device) if self.device.type == "cuda" else _HostOps(self.device)
        self.keep_probs, self.final_probs = False, {}     # keep_probs: each object's last probability map (tests)

    # ---------------------------------------------------------------------------------------------- the loop
    def run(self, objects):
        """``objects``: iterable of (image, gt_mask) in evaluation order -> list of (clicks, IoU series) in that order."""
        it, results, order, images = iter(objects), {}, [0], {}

        def load():
            try:
                image, gt = next(it)
            except StopIteration:
                return None
            key = id(image)
            if key not in images:           # (objects of one sample share its image tensor)
                images.clear()
                images[key] = (image, _load_image(image, self.device))
            o = _Object(order[0], images[key][1], np.asarray(gt), self.device)
            order[0] += 1
            return o

        active, pending = [], []
        while len(active) < self.K:
            o = load()
            if o is None:
                break
            active.append(o)
        with torch.no_grad():
            while active:
                self._step(active, pending, load)
                for o in active:
                    if o.done:
                        results[o.order] = (o.clicks, np.array(o.ious, dtype=np.float32))
                        if self.keep_probs:
                            self.final_probs[o.order] = o.canvas[o.prev].clone()
                active = [o for o in active if not o.done]
                while len(active) < self.K and pending:       # refill: the batch shrinks only at the tail
                    active.append(pending.pop(0))
        return [results[i] for i in range(len(results))]

    def _step(self, active, pending, load):
        """One batched click of every object of ``active`` that has its click keys (on the first call none has: that step
        only computes them), plus the first click keys of the objects loaded into ``pending``."""
        stepping = [o for o in active if o.keys is not None]
        for o in stepping:
            if not o.recalc and not o.host_box:         # Clicker.make_next_click
                (fn_max, fn_at), (fp_max, fp_at) = (decode_key(k, o.W) for k in o.keys)
                positive = fn_max > fp_max
                at = fn_at if positive else fp_at
                o.clicks.append(Click(is_positive=bool(positive), coords=at, indx=len(o.clicks)))
                o.clear_at = at[0] * o.W + at[1]
                o.ptype = self.schedule(len(o.clicks) - 1, o.ious[-1] if o.ious else 0)
                if o.ptype == 2:
                    raise ValueError("the prompt schedule returned 2 (scribble) inside the batched loop, which has no scribble "
                                     "prompts: evaluate this schedule on the sequential path (evaluate_sample, or "
                                     "evaluate_dataset with batch_objects=1)")
            o.plan = self._plan(o)
        # the refill queue: as many prepared objects (first keys known) as slots could free up
        new = []
        while len(pending) + len(new) < self.K:
            o = load()
            if o is None:
                break
            new.append(o)
        key_objs = stepping + [o for o in active if o.keys is None] + new
        ops = self.ops
        row = {id(o): i for i, o in enumerate(key_objs)}
        # A click that ZoomIn re-runs goes through get_prediction, i.e. as clicks only (kind 0).  The box masks have the
        # network's size except when a held roi meets an un-zoomed step (no prediction to zoom on): the sequential path then
        # still crops them to target_size, so that size is part of a box sub-batch's key.  Constant type: one forward per
        # (size, kind, box size, host fallback), as ever.  Schedule: one forward per size, its box rows in sub-batches
        mixed = self.schedule.constant is None
        groups = {}
        for o in stepping:
            kind = 0 if o.recalc else o.ptype
            box_key = None
            if kind == 1:
                box_key = (tuple(self.zoom.target_size) if o.roi is not None else (o.H, o.W), o.host_box)
            o.box_key = box_key
            groups.setdefault((o.plan[1],) if mixed else (o.plan[1], kind) + (box_key or (None, o.host_box)), []).append(o)
        spans, n_flags = [], 0
        for key, members in groups.items():
            subs = {}
            for j, o in enumerate(members):
                if o.box_key is not None:
                    subs.setdefault(o.box_key, []).append(j)
            n_flags += len(subs)
            spans.append([key[0], members, subs])
        ops.begin(len(key_objs), n_flags)
        for span in spans:
            size, members, subs = span
            box_batches = []
            for (box_size, host_box), js in subs.items():
                bfirst, brows = None, []
                for mirror in ((False, True) if self.flip else (False,)):
                    for j in js:
                        o = members[j]
                        brows.append((o, o.roi, mirror, self._own_rows(o.clicks)))
                        i = ops.add_box(*brows[-1])
                        bfirst = i if bfirst is None else bfirst
                box_batches.append((box_size, host_box, js, bfirst, brows))
            first = None
            for j, o in enumerate(members):
                i = ops.add(o, o.plan[0], j, row[id(o)], prev=self.prev_channel)
                first = i if first is None else first
            pfirst = None
            for j, o in enumerate(members):
                i = ops.add(o, o.plan[3], j, row[id(o)])
                pfirst = i if pfirst is None else pfirst
            span[2:] = [first, pfirst, box_batches]
        kfirst = None
        for o in key_objs:
            i = ops.add(o, Roi.whole(o.H, o.W), 0, row[id(o)])
            kfirst = i if kfirst is None else kfirst
        ops.upload()
        flag_of, n_box = {}, 0
        for size, members, first, pfirst, box_batches in spans:
            image_nd = ops.resize(members, first, len(members), size, self.flip, 4 if self.prev_channel else 3)
            points_nd = self.pred.get_points_nd(self.flipped_click_lists([o.plan[2] for o in members], size[1])).float()
            boxes, kind = None, 0
            for box_size, host_box, js, bfirst, brows in box_batches:
                n_batch, target = points_nd.shape[1] // 2, (self.zoom.target_size if self.zoom else None)
                whole = len(js) == len(members)
                at = None            # rows of this sub-batch in the forward: its objects, then their flip copies
                if not whole:
                    at = torch.tensor(js + ([len(members) + j for j in js] if self.flip else []), device=self.device)
                pts = points_nd if whole else points_nd[at]
                if host_box:
                    got = torch.from_numpy(_host_boxes(brows, pts, n_batch, box_size, target)).to(self.device)
                else:
                    got = ops.boxes(brows, bfirst, pts, n_batch, box_size, target, n_box)
                    flag_of.update((id(members[j]), n_box) for j in js)
                n_box += 1
                if whole:
                    boxes = got
                else:
                    if boxes is None:        # a row without a box: slot -1 (is_vpu_model.forward)
                        boxes = torch.zeros(points_nd.shape[0], 5, dtype=torch.int32, device=self.device)
                        boxes[:, 4] = -1
                    boxes[at] = got.to(self.device)
                kind = 1
            probs = self._forward(image_nd, points_nd, (points_nd, boxes, None), kind)
            ops.paste(members, pfirst, len(members), probs, self.pred_thr, self.zoom.prob_thresh if self.zoom else 0.5)
        if key_objs:
            ops.keys(key_objs, kfirst, len(key_objs))
        out = ops.readback()
        flags = ops.flags
        for o in key_objs:
            o.keys = (out[row[id(o)], 0], out[row[id(o)], 1])
            o.clear_at = -1
        for o in stepping:
            if id(o) in flag_of and flags[flag_of[id(o)]]:
                o.host_box = True                        # the component table overflowed: this forward is discarded and
                continue                                 # the click repeated with boxes from the host code
            o.host_box = False
            stats = out[row[id(o)], _STATS:].view(np.int32)
            o.box = tuple(int(v) for v in stats[2:7])       # ZoomIn._probs is the new prediction either way
            if self._wants_recalc(o):
                o.recalc = True                          # re-run this click, zoomed (BasePredictor.get_prediction)
                continue
            o.recalc = False
            o.prev = 1 - o.prev                           # prev_prediction = the new canvas
            iou = np.int64(stats[0]) / np.int64(stats[1])     # utils.get_iou: numpy's integer division
            o.ious.append(iou)
            k = len(o.clicks) - 1
            o.done = (iou >= self.max_iou_thr and k + 1 >= self.min_clicks) or k + 1 >= self.max_clicks
        pending.extend(new)
