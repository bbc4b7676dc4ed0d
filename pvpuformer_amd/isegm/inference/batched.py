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
(``_HostOps``), which is what the CPU tests check it with."""
import ctypes as C
import struct

import numpy as np
import torch

from .clicker import Click
from .transforms import AddHorizontalFlip, Roi, SigmoidForPred, ZoomIn

_STATS = 2           # int64 offset of the int32 statistics in an object's 6-int64 output slot
_MASK64 = 0xFFFFFFFFFFFFFFFF


def batchable(predictor, callback=None, as_prompt_type=0):
    """True when ``evaluate_dataset`` may run ``predictor`` batched: a ``BasePredictor`` whose transforms are only
    [ZoomIn with a (height, width) target_size] [SigmoidForPred] [AddHorizontalFlip] (in that order, each optional), no
    callback and click prompts (``as_prompt_type == 0``)."""
    from .predictors.base import BasePredictor
    if not isinstance(predictor, BasePredictor) or callback is not None or as_prompt_type != 0:
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
        self.done = False
        self.plan = None


class _DeviceOps:
    """The three batched HIP kernels; per step the descriptors go up in one copy and the outputs come back in one."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self.ops, self.device = _lib, ops, torch.device(device)
        self._desc = []

    def begin(self, n_out):
        self._desc = []
        self.out = torch.empty(max(n_out, 1), 6, device=self.device, dtype=torch.int64)

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

    def upload(self):
        n = len(self._desc)
        arr = (self._lib.EvalObj * n)(*self._desc)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory()
        self._host = host                   # (kept alive until the step's read-back has synchronised)
        self.desc = host.to(self.device, non_blocking=True)

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

    def readback(self):
        return self.out.cpu().numpy()       # the step's one synchronisation


class _HostOps:
    """Host stand-ins of the three kernels (torch / scipy, as the Clicker's host path): the scheduler's CPU test bed."""

    def __init__(self, device):
        self.device = device

    def begin(self, n_out):
        self._desc = []
        self.out = np.zeros((max(n_out, 1), 6), dtype=np.int64)

    def add(self, o, roi, src, out_row, prev=True):
        self._desc.append((o, tuple(roi), src, out_row, prev, o.clear_at))
        return len(self._desc) - 1

    def upload(self):
        pass

    @staticmethod
    def _resize(x, size):
        if tuple(x.shape[2:]) == tuple(size):
            return x.clone()
        return torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)

    def resize(self, objs, first, n, size, flip, channels):
        rows = []
        for o, (r0, r1, c0, c1), src, _, prev, _ in self._desc[first:first + n]:
            x = torch.cat((o.image[None], o.canvas[o.prev][None, None]), 1) if prev else o.image[None]
            rows.append((src, self._resize(x[:, :, r0:r1 + 1, c0:c1 + 1], size)))
        batch = torch.cat([r for _, r in sorted(rows, key=lambda t: t[0])], 0)
        return torch.cat([batch, batch.flip(3)], 0) if flip else batch

    def paste(self, objs, first, n, probs, pred_thr, box_thr):
        for o, (r0, r1, c0, c1), src, row, _, _ in self._desc[first:first + n]:
            patch = self._resize(probs[src:src + 1].float(), (r1 - r0 + 1, c1 - c0 + 1))
            full = torch.zeros(o.H, o.W, dtype=torch.float32)
            full[r0:r1 + 1, c0:c1 + 1] = patch[0, 0]
            o.canvas[1 - o.prev].copy_(full)
            m = full.numpy() > np.float32(pred_thr)
            o.mask.copy_(torch.from_numpy(m.astype(np.uint8)))
            g, v = o.gt.numpy() != 0, o.valid.numpy() != 0
            stats = [int((m & g & v).sum()), int(((m | g) & v).sum())]
            on = np.argwhere(full.numpy() > np.float32(box_thr))
            if len(on):
                stats += [len(on), int(on[:, 0].min()), int(on[:, 0].max()), int(on[:, 1].min()), int(on[:, 1].max())]
            else:
                stats += [0, o.H, -1, o.W, -1]
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


class BatchedEvaluator:
    """Runs ``evaluate_sample``'s loop (``evaluate_dataset``'s kwargs) over a stream of objects, ``batch_objects`` at a time."""

    def __init__(self, predictor, batch_objects, max_iou_thr, pred_thr=0.49, min_clicks=1, max_clicks=20):
        assert batchable(predictor), "the predictor's transforms are not the batched path's (see batchable)"
        self.pred, self.K = predictor, int(batch_objects)
        self.max_iou_thr, self.pred_thr, self.min_clicks, self.max_clicks = max_iou_thr, pred_thr, min_clicks, max_clicks
        self.zoom = predictor.zoom_in
        self.flip = any(type(t) is AddHorizontalFlip for t in predictor.transforms)
        self.inv = [t for t in reversed(predictor.transforms) if type(t) is not ZoomIn]   # flip average, then sigmoid
        self.prev_channel = bool(getattr(predictor.net, "with_prev_mask", True))
        self.device = torch.device(predictor.device)
        self.ops = _DeviceOps(self.device) if self.device.type == "cuda" else _HostOps(self.device)
        self.keep_probs, self.final_probs = False, {}     # keep_probs: each object's last probability map (tests)

    # ---------------------------------------------------------------------------------------------- ZoomIn on the host
    def _predicted_box(self, o, clicks=()):
        """ZoomIn._predicted_box from the read-back box of the last prediction, joined here with the positive clicks."""
        if o.box is None:
            return None
        count, r0, r1, c0, c1 = o.box
        for c in clicks:
            if c.is_positive:
                r, k = int(c.coords[0]), int(c.coords[1])
                r0, r1, c0, c1 = min(r0, r), max(r1, r), min(c0, k), max(c1, k)
        if count == 0:
            return None
        return Roi(r0, r1, c0, c1).grown(self.zoom.expansion_ratio, self.zoom.min_crop_size).clipped(o.H, o.W)

    def _plan(self, o):
        """ZoomIn.transform of this click: (input roi, network input size, clicks in network coordinates, paste roi)."""
        whole, clicks, zi = Roi.whole(o.H, o.W), o.clicks, self.zoom
        crop = False
        if zi is not None and len(clicks) > zi.skip_clicks:
            box = self._predicted_box(o, clicks)
            if box is None and zi.skip_clicks < 0:
                box = whole                             # zoom from the very first click on
            if box is not None:
                held = o.roi
                if held is None or not Roi(*held).encloses(clicks) or box.overlap(held) < zi.recompute_thresh_iou:
                    o.roi = box
                crop = True
        if crop:
            roi = Roi(*o.roi)
            size = tuple(int(s) for s in roi.output_size(zi.target_size))
            net_clicks = [c.copy(coords=roi.to_crop(c.coords, size)) for c in clicks]
            return roi, size, net_clicks, roi
        return whole, (o.H, o.W), list(clicks), (Roi(*o.roi) if o.roi is not None else whole)

    def _wants_recalc(self, o):
        """ZoomIn.check_possible_recalculation after this step's prediction (o.box is its box)."""
        zi = self.zoom
        if zi is None or o.roi is not None or zi.skip_clicks > 0:
            return False
        box = self._predicted_box(o)
        return box is not None and box.overlap(Roi.whole(o.H, o.W)) < 0.50

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
            if not o.recalc:                            # Clicker.make_next_click
                (fn_max, fn_at), (fp_max, fp_at) = (decode_key(k, o.W) for k in o.keys)
                positive = fn_max > fp_max
                at = fn_at if positive else fp_at
                o.clicks.append(Click(is_positive=bool(positive), coords=at, indx=len(o.clicks)))
                o.clear_at = at[0] * o.W + at[1]
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
        ops.begin(len(key_objs))
        row = {id(o): i for i, o in enumerate(key_objs)}
        groups = {}
        for o in stepping:
            groups.setdefault(o.plan[1], []).append(o)
        spans = []
        for size, members in groups.items():
            first = None
            for j, o in enumerate(members):
                i = ops.add(o, o.plan[0], j, row[id(o)], prev=self.prev_channel)
                first = i if first is None else first
            pfirst = None
            for j, o in enumerate(members):
                i = ops.add(o, o.plan[3], j, row[id(o)])
                pfirst = i if pfirst is None else pfirst
            spans.append((size, members, first, pfirst))
        kfirst = None
        for o in key_objs:
            i = ops.add(o, Roi.whole(o.H, o.W), 0, row[id(o)])
            kfirst = i if kfirst is None else kfirst
        ops.upload()
        for size, members, first, pfirst in spans:
            image_nd = ops.resize(members, first, len(members), size, self.flip, 4 if self.prev_channel else 3)
            lists = [o.plan[2] for o in members]
            if self.flip:
                lists = lists + [[c.copy(coords=(c.coords[0], size[1] - c.coords[1] - 1)) for c in cl] for cl in lists]
            points_nd = self.pred.get_points_nd(lists).float()
            logits = self.pred.net(image_nd, points_nd, (points_nd, None, None), 0)['instances']
            if tuple(logits.shape[2:]) != tuple(image_nd.shape[2:]):
                from .transforms import resize_align_corners
                logits = resize_align_corners(logits, image_nd.shape[2:])
            probs = logits
            for t in self.inv:
                probs = t.inv_transform(probs)
            ops.paste(members, pfirst, len(members), probs, self.pred_thr, self.zoom.prob_thresh if self.zoom else 0.5)
        if key_objs:
            ops.keys(key_objs, kfirst, len(key_objs))
        out = ops.readback()
        for o in key_objs:
            o.keys = (out[row[id(o)], 0], out[row[id(o)], 1])
            o.clear_at = -1
        for o in stepping:
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
