"""Several interactive sessions served through one batched forward.

``BasePredictor.get_prediction(clicker, prev_mask)`` is one session per forward and hands back the full fp32 map
(``4 * H * W`` bytes device-to-host per click), which the caller then thresholds.  ``SessionPool`` holds up to
``max_sessions`` sessions (image, previous prediction, ZoomIn state, each of its own size); ``predict`` takes the pending
click lists of any subset of them and runs them through ONE forward per network input size, then one launch of
``vpu_session_paste_batched`` that writes every session's probability canvas, its mask ``> pred_thr`` at one bit per pixel
and the ZoomIn box, and ONE device-to-host copy of the records and packed masks of all sessions (about ``H * W / 8`` bytes
per session).  The probability maps stay on the device (``probs``).

Per session the results are those of a private copy of the predictor: every per-session operation is the sequential one
(``ZoomIn.transform`` on the host by ``ZoomHost``, which ``BatchedEvaluator`` runs on too, the crop / resize / mirror of
``vpu_roi_resize_batched``, the predictor's own flip average and sigmoid on the whole batch, the paste with
``vpu_roi_paste_batched``'s per-pixel function); what the batch shares is the network, whose click rows are padded to a
common count by ``get_points_nd`` with not-a-point rows that it ignores.  In the ``f32`` engine mode the maps are the
sequential ones bit for bit.  ``check_possible_recalculation`` is honoured inside the call: the sessions it fires for run a
second forward of their own, as ``get_prediction`` re-runs itself.

Drawn prompts.  Besides its clicks a session may hand ``predict`` a box or a stroke that the annotator drew (no ground
truth is involved: deriving prompts from one is ``BatchedEvaluator``'s job).  The drawn coordinates are image pixels; the
host maps them into the network's frame with the map ``ZoomIn.transform`` applies to that session's clicks (``map_drawn``),
truncates them to integers and mirrors the columns for the flip row, then states the box row (``box_row``: ``cal_box``'s
un-jittered arithmetic) or the stroke's curve, rectangle and profiles (``stroke_row``).  A forward whose rows are all clicks
is the plain call, one with clicks and boxes is ``as_prompt_type=1`` with the no-box row (0, 0, 0, 0, -1), one that holds a
stroke is ``as_prompt_type=3`` (a prompt kind per row, ``is_vpu_model.forward``): still one forward per network input size.
The new kernels run inside the network, so the pool needs no further device operation of its own.

On a CPU device the same scheduler runs with torch / numpy stand-ins of the two kernels (``_HostOps``), which is what the
CPU tests check it with."""
import ctypes as C
import random

import numpy as np
import torch

from ..model.scribble import scribble_profiles
from ._batchcore import (PackedLayout, ZoomHost, host_count_box, host_roi_paste, host_roi_resize, n_words, pack_mask,  # noqa: F401
                         unpack_mask, upload_structs)
from .batched import _load_image, _padded_slot, batchable
from .regions import DeviceRegionOps, HostRegionOps, TidyItem, check_tidy_args, click_seeds
from .outlines import DeviceOutlineOps, HostOutlineOps
from .polygons import quantise
from .runs import KIND_PROB, DeviceRunOps, HostRunOps, RunMap, as_run_map


def host_session_paste(prob_map, H, W, roi, pred_thr, box_thr):
    """Stand-in of vpu_session_paste_batched for one session: ``prob_map`` fp32 [S_h, S_w] (cpu) resized to the roi and pasted
    into zeros -> (canvas fp32 [H, W], packed mask uint64, record int32 [8]: area, count, rmin, rmax, cmin, cmax, 0, 0)."""
    canvas = host_roi_paste(prob_map, H, W, roi)
    values = canvas.numpy()
    mask = values > np.float32(pred_thr)
    box = host_count_box(values > np.float32(box_thr), H, W)
    return canvas, pack_mask(mask), np.array([int(mask.sum())] + box + [0, 0], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------ drawn prompts
def map_drawn(points, roi, size, mirror):
    """Image pixels ``points`` [P, 2] of (row, col) -> int64 [P, 2] of (x, y) in the network input of ``size`` cropped from
    ``roi``: ``Roi.to_crop``'s expression (the map of the session's clicks; the identity on integer pixels when the whole image
    goes in unscaled), truncation toward zero as ``scribble_curves`` / ``cal_box`` truncate, then for the flip row the mirror
    ``size_w - 1 - col`` of the click lists.  Points outside the roi map outside the input; the kernels clip."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    r0, r1, c0, c1 = roi
    rows = (size[0] * (p[:, 0] - r0) / (r1 - r0 + 1)).astype(np.int64)
    cols = (size[1] * (p[:, 1] - c0) / (c1 - c0 + 1)).astype(np.int64)
    if mirror:
        cols = size[1] - 1 - cols
    return np.stack([cols, rows], 1)


def own_slot(n_own):
    """The PuE row of a drawn box in the session's own click layout (``n_own`` rows per polarity): ``cal_box``'s
    ``as_allmask=False`` rule with the box as the missing region -- the annotator outlines the object, there is no
    false-positive region -- which is always the LAST positive row, ``n_own - 1`` (trainer.py:1088).  A click in that row is
    replaced by the box in the encoder (its disk is still drawn), as in the reference."""
    return n_own - 1


def box_row(xy, slot):
    """``cal_box``'s un-jittered row (x_center, y_center, width, height, slot) of the mapped corners ``xy`` [2, 2] in any
    order; a box it calls degenerate (a centre below 1 or an extent below 1) is its all-zero row."""
    x0, x1, y0, y1 = int(xy[:, 0].min()), int(xy[:, 0].max()), int(xy[:, 1].min()), int(xy[:, 1].max())
    xc, yc, bw, bh = int(0.5 * (x0 + x1)), int(0.5 * (y0 + y1)), x1 - x0, y1 - y0
    if xc >= 1 and yc >= 1 and bw >= 1 and bh >= 1:
        return (xc, yc, bw, bh, slot)
    return (0, 0, 0, 0, 0)


def stroke_row(xy, img, rng):
    """(curve int32 [P, 2], profiles float64 [2 * img]) of the mapped stroke ``xy``: the curve is the points as they are, the
    rectangle their bounding box in ``cal_scribble``'s form, the profiles ``scribble_profiles``' drawn from ``rng``."""
    curve = np.ascontiguousarray(xy, dtype=np.int32)
    c0, c1, r0, r1 = int(xy[:, 0].min()), int(xy[:, 0].max()), int(xy[:, 1].min()), int(xy[:, 1].max())
    rect = np.array([[[int(0.5 * (c0 + c1)), int(0.5 * (r0 + r1)), c1 - c0, r1 - r0]]], dtype=np.int64)
    return curve, scribble_profiles(curve[None, None], rect, img, rng=rng)[0]


class _Session:
    """One session's state (a slot of the pool, as ``ZoomHost`` reads one)."""

    def __init__(self, sid, image, seed=None):
        self.sid, self.image = sid, image
        self.H, self.W = int(image.shape[1]), int(image.shape[2])
        self.canvas = [torch.zeros(self.H, self.W, device=image.device, dtype=torch.float32) for _ in range(2)]
        self.prev = 0                  # canvas[prev] is the predictor's prev_prediction
        self.clicks = []               # the click list of the call in progress
        self.roi = None                # ZoomIn._object_roi
        self.box = None                # (count, r0, r1, c0, c1) of ZoomIn._probs > prob_thresh (no clicks); None: no _probs
        self.plan = None
        self.rng = random.Random(seed)  # the stroke profiles' draws: the session's own generator
        self.drawn = None              # the drawn prompt of the call in progress: ("box", [2, 2]) / ("stroke", [P, 2]) of (row, col)


class _Round(PackedLayout):
    """Layout of a forward round's read-back, keyed by session id: ``row[sid]`` is the session's row, ``at[sid]`` the int64
    offset of its packed words."""

    def __init__(self, sessions):
        super().__init__([(s.H, s.W) for s in sessions])
        self.row = {s.sid: i for i, s in enumerate(sessions)}
        self.at = {s.sid: self.bits_at(i) for i, s in enumerate(sessions)}


class _DeviceOps:
    """The two HIP kernels; per round the descriptors go up in one copy and the results come back in one."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self.ops, self.device = _lib, ops, torch.device(device)

    def begin(self, layout):
        self.layout, self._inp, self._out = layout, [], []
        self.out = torch.empty(layout.size, device=self.device, dtype=torch.int64)

    def add_input(self, s, roi, src, prev):
        """One row of vpu_roi_resize_batched (a vpu_eval_obj that carries only what that kernel reads); returns its index."""
        r0, r1, c0, c1 = roi
        assert 0 <= r0 <= r1 < s.H and 0 <= c0 <= c1 < s.W, (roi, s.H, s.W)
        assert s.image.is_contiguous() and (prev is None or (prev.is_contiguous() and tuple(prev.shape) == (s.H, s.W)))
        d = self._lib.EvalObj()
        d.image, d.prev = s.image.data_ptr(), prev.data_ptr() if prev is not None else None
        d.H, d.W = s.H, s.W
        d.r0, d.r1, d.c0, d.c1 = r0, r1, c0, c1
        d.src, d.clear_at = src, -1
        self._inp.append(d)
        return len(self._inp) - 1

    def add_paste(self, s, roi, src):
        """One row of vpu_session_paste_batched; returns its index."""
        r0, r1, c0, c1 = roi
        assert 0 <= r0 <= r1 < s.H and 0 <= c0 <= c1 < s.W, (roi, s.H, s.W)
        canvas = s.canvas[1 - s.prev]
        assert canvas.is_contiguous() and canvas.data_ptr() % 16 == 0 and self.out.data_ptr() % 8 == 0
        d = self._lib.SessionObj()
        d.canvas = canvas.data_ptr()
        d.bits = self.out.data_ptr() + 8 * self.layout.at[s.sid]
        d.rec = self.out.data_ptr() + 8 * self.layout.rec_at(self.layout.row[s.sid])
        d.H, d.W = s.H, s.W
        d.r0, d.r1, d.c0, d.c1 = r0, r1, c0, c1
        d.src = src
        self._out.append(d)
        return len(self._out) - 1

    def upload(self):
        # the paste rows ride behind the input rows in the same copy; _host stays alive until the read-back
        self._host, self.desc, (_, self._out_at0) = upload_structs(
            self.device, (self._lib.EvalObj * len(self._inp))(*self._inp), (self._lib.SessionObj * len(self._out))(*self._out))

    def resize(self, sessions, first, size, flip, channels):
        n = len(sessions)
        out = torch.empty((2 if flip else 1) * n, channels, size[0], size[1], device=self.device, dtype=torch.float32)
        self.ops.roi_resize_batched((self.desc, first * C.sizeof(self._lib.EvalObj)), n, out, size[0], size[1], flip, channels)
        return out

    def paste(self, sessions, first, probs, pred_thr, box_thr):
        probs = probs.contiguous().float()
        at = (self.desc, self._out_at0 + first * C.sizeof(self._lib.SessionObj))
        self.ops.session_paste_batched(at, len(sessions), probs, probs.shape[-2], probs.shape[-1], pred_thr, box_thr,
                                       max(s.H * s.W for s in sessions))

    def readback(self):
        return self.out.cpu().numpy()        # the round's one synchronisation


class _HostOps:
    """Host stand-ins of the two kernels (torch / numpy): the scheduler's CPU test bed."""

    def __init__(self, device):
        self.device = device

    def begin(self, layout):
        self.layout, self._inp, self._out = layout, [], []
        self.out = np.zeros(layout.size, dtype=np.int64)

    def add_input(self, s, roi, src, prev):
        self._inp.append((s, tuple(roi), src, prev))
        return len(self._inp) - 1

    def add_paste(self, s, roi, src):
        self._out.append((s, tuple(roi), src))
        return len(self._out) - 1

    def upload(self):
        pass

    def resize(self, sessions, first, size, flip, channels):
        rows = []
        for s, roi, src, prev in self._inp[first:first + len(sessions)]:
            rows.append((src, host_roi_resize(s.image, prev if channels == 4 else None, roi, size)))
        batch = torch.cat([r for _, r in sorted(rows, key=lambda t: t[0])], 0)
        return torch.cat([batch, batch.flip(3)], 0) if flip else batch

    def paste(self, sessions, first, probs, pred_thr, box_thr):
        for s, roi, src in self._out[first:first + len(sessions)]:
            canvas, words, rec = host_session_paste(probs[src, 0], s.H, s.W, roi, pred_thr, box_thr)
            s.canvas[1 - s.prev].copy_(canvas)
            self.layout.put(self.out, self.layout.row[s.sid], rec, words)

    def readback(self):
        return self.out.copy()


class SessionPool(ZoomHost):
    """``pool = SessionPool(predictor, max_sessions=8, pred_thr=0.49)``; ``predictor``: a ``BasePredictor`` for which
    ``batched.batchable(predictor)`` holds (ValueError otherwise).  It lends the pool its network, its transforms' parameters,
    ``get_points_nd`` / ``net_clicks_limit`` and the cascade rule for ``prev_masks``; its own image and state are not touched.

    ``sid = pool.open(image, seed=None)``; ``pool.predict({sid: clicks, ...}, prev_masks=None, boxes=None, strokes=None) ->
    {sid: bool ndarray [H, W]}``; ``pool.probs(sid)``; ``pool.get_states(sid)`` / ``pool.set_states(sid, st)``;
    ``pool.close(sid)``; ``pool.mask_runs(sids=None) -> {sid: RunMap}``, the masks as run-length maps (runs.py);
    ``pool.mask_outlines(sids=None) -> {sid: Outline}``, the masks as polygon loops (outlines.py).
    ``max_batch``: sessions per forward (default ``max_sessions``); a size group with more runs in chunks.
    ``max_stroke_points``: the longest stroke ``predict`` takes.
    ``pool.tidy(sids=None, min_area=0, max_hole=0, keep="all", seeds=None) -> {sid: mask}``: small islands dropped and small
    holes filled on the device (regions.py).
    ``readbacks`` counts the device-to-host synchronisations (one per forward round, two per ``mask_runs``, one per
    ``tidy``, two per ``mask_outlines``).  ``ops_runs`` holds the run-length encoder and decoder and may be replaced by
    ``HostRunOps()``; ``ops_regions`` holds the region clean-up and may be replaced by ``HostRegionOps()``; ``ops_outlines`` holds
    the outline tracer and may be replaced by ``HostOutlineOps()``."""

    def __init__(self, predictor, max_sessions=8, pred_thr=0.49, max_batch=None, max_stroke_points=1024):
        if not batchable(predictor):
            raise ValueError("SessionPool: the predictor's transforms are not the batched path's (batched.batchable): only "
                             "[ZoomIn with a (height, width) target_size] [SigmoidForPred] [AddHorizontalFlip]")
        if int(max_sessions) < 1 or (max_batch is not None and int(max_batch) < 1):
            raise ValueError("SessionPool: max_sessions and max_batch must be at least 1")
        super().__init__(predictor)
        self.max_sessions, self.pred_thr = int(max_sessions), float(pred_thr)
        self.max_batch = int(max_batch) if max_batch is not None else self.max_sessions
        self.max_stroke_points = int(max_stroke_points)
        size = getattr(predictor.net, "image_size", None)     # the length of the stroke profiles (the model's own image size)
        self.prompt_img = int(size[0]) if size is not None else None
        self.ops = _DeviceOps(self.device) if self.device.type == "cuda" else _HostOps(self.device)
        self.ops_runs = DeviceRunOps(self.device) if self.device.type == "cuda" else HostRunOps(self.device)
        self.ops_regions = DeviceRegionOps(self.device) if self.device.type == "cuda" else HostRegionOps(self.device)
        self.ops_outlines = DeviceOutlineOps(self.device) if self.device.type == "cuda" else HostOutlineOps(self.device)
        self._slots = [None] * self.max_sessions
        self.readbacks = self.forwards = 0

    # ---------------------------------------------------------------------------------------------- sessions
    def open(self, image, seed=None):
        """A new session on ``image`` (``set_input_image``'s conversions) -> its id; ids of closed sessions are reused.
        ``seed`` seeds the session's own ``random.Random``, from which the profiles of its strokes are drawn."""
        for sid, held in enumerate(self._slots):
            if held is None:
                self._slots[sid] = _Session(sid, _load_image(image, self.device), seed)
                return sid
        raise ValueError(f"SessionPool: all {self.max_sessions} sessions are open")

    def close(self, sid):
        self._session(sid)
        self._slots[sid] = None

    def _session(self, sid):
        if not isinstance(sid, (int, np.integer)) or not 0 <= sid < self.max_sessions or self._slots[sid] is None:
            raise KeyError(f"SessionPool: no open session {sid!r}")
        return self._slots[sid]

    def probs(self, sid):
        """The session's ``prev_prediction``: fp32 [1, 1, H, W] on the device.  A view of the session's canvas: it holds
        until the second ``predict`` of that session from now (clone it to keep it longer)."""
        s = self._session(sid)
        return s.canvas[s.prev][None, None]

    def mask_runs(self, sids=None):
        """{sid: RunMap} of the mask ``probs(sid) > pred_thr`` of the named sessions (default: all open ones), values 0 / 1, so
        ``rm.to_coco()`` is the session's mask in COCO's uncompressed run-length form.  One encode for all of them: two
        read-backs (the offsets, then 8 bytes per run).  A session without a prediction yet gives the single run (0, 0)."""
        if sids is None:
            sids = [sid for sid, held in enumerate(self._slots) if held is not None]
        held = [self._session(sid) for sid in sids]
        if not held:
            return {}
        maps = self.ops_runs.encode([(s.canvas[s.prev], KIND_PROB, self.pred_thr) for s in held])
        self.readbacks += 2
        return {s.sid: rm for s, rm in zip(held, maps)}

    def mask_outlines(self, sids=None, tolerance=None):
        """{sid: Outline} (outlines.py) of the mask ``probs(sid) > pred_thr`` of the named sessions (default: all open ones):
        its polygon loops on the pixel lattice, so ``outline.to_coco()`` is the mask in COCO's polygon form.  One trace for all
        of them: two read-backs (the offsets, then 8 bytes per corner).  A session without a prediction yet gives an outline
        without loops; no session's state is touched.  With a ``tolerance`` in pixels (0 .. 1024; sides up to 8191, else
        ValueError before any launch) {sid: Polygons} (polygons.py): the loops simplified on the device, three read-backs, and
        only the kept corners cross to the host."""
        if tolerance is not None:
            quantise(tolerance)
        if sids is None:
            sids = [sid for sid, held in enumerate(self._slots) if held is not None]
        held = [self._session(sid) for sid in sids]
        if not held:
            return {}
        items = [(s.canvas[s.prev], KIND_PROB, self.pred_thr, 0) for s in held]
        got = self.ops_outlines.trace(items) if tolerance is None else self.ops_outlines.trace(items, tolerance)
        self.readbacks += 2 if tolerance is None else 3
        return {s.sid: outline for s, outline in zip(held, got)}

    def tidy(self, sids=None, min_area=0, max_hole=0, keep="all", seeds=None):
        """Region clean-up (regions.py, rules T1-T8) of the mask ``probs(sid) > pred_thr`` of the named sessions (default: all
        open ones) -> {sid: bool ndarray [H, W]}: components below ``min_area`` pixels dropped, holes of at most ``max_hole``
        pixels filled (None: every hole); ``keep``: "all", "seeded" (only components that hold a positive seed: empty
        without one) or "largest".  The seeds are the clicks of the session's last ``predict`` -- a component with a positive
        click is always kept, a hole with a negative click never filled -- or ``seeds[sid]``, a list of ``Click`` or of
        (is_positive, (row, col)).  The session's previous prediction becomes the edited map (0.0 on dropped pixels, 1.0 on
        filled ones), so the next click's network input sees the cleaned mask; the ZoomIn state and the generator are not
        touched.  One call for all of them, one read-back.  A session without a prediction yet gives an all-False mask."""
        min_area, max_hole = check_tidy_args("SessionPool.tidy", min_area, max_hole, keep)
        if not 0.0 <= self.pred_thr < 1.0:      # the edits 0.0 and 1.0 must fall on the clear and the set side of it
            raise ValueError(f"SessionPool.tidy: pred_thr {self.pred_thr} is outside [0, 1)")
        if sids is None:
            sids = [sid for sid, held in enumerate(self._slots) if held is not None]
        held = [self._session(sid) for sid in sids]
        for sid in (seeds or {}):
            if sid not in sids:
                raise ValueError(f"SessionPool.tidy: seeds names session {sid!r}, which is not among the sessions of this call")
        if not held:
            return {}
        items = []
        for s in held:
            prev = s.canvas[s.prev]
            items.append(TidyItem(s.H, s.W, add=prev, add_out=prev, min_area=min_area, max_hole=max_hole, keep=keep,
                                  seeds=click_seeds(seeds[s.sid] if seeds and s.sid in seeds else s.clicks)))
        got = self.ops_regions.tidy(items, self.pred_thr, "masks")
        self.readbacks += 1
        return {s.sid: mask for s, (_, mask) in zip(held, got)}

    def get_states(self, sid):
        s = self._session(sid)
        return {"roi": s.roi, "box": s.box, "prev_prediction": s.canvas[s.prev].clone(), "rng": s.rng.getstate()}

    def set_states(self, sid, states):
        s = self._session(sid)
        prev = states["prev_prediction"]
        assert tuple(prev.shape[-2:]) == (s.H, s.W), "the state is of another image size"
        s.roi, s.box = states["roi"], states["box"]
        if "rng" in states:
            s.rng.setstate(states["rng"])
        s.canvas[s.prev].copy_(prev.reshape(s.H, s.W))

    # ---------------------------------------------------------------------------------------------- prediction
    def _as_map(self, value, s):
        if isinstance(value, (RunMap, dict)):       # run-length form: v == 1, decoded on the device from 8 bytes per run
            rm = as_run_map(value)
            assert rm.size == (s.H, s.W), "prev_masks: a map of another size than the session's image"
            out = torch.empty(s.H, s.W, device=self.device, dtype=torch.float32)
            self.ops_runs.decode([(rm, out, KIND_PROB, 1)])
            return out
        if not torch.is_tensor(value):
            value = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32))
        assert value.numel() == s.H * s.W, "prev_masks: a map of another size than the session's image"
        return value.to(self.device).float().reshape(s.H, s.W).contiguous()

    def _drawn(self, clicks, boxes, strokes):
        """{sid: ("box", float64 [2, 2]) or ("stroke", float64 [P, 2])} of (row, col) after every check of ``predict``."""
        boxes, strokes, drawn = boxes or {}, strokes or {}, {}
        for name, given in (("boxes", boxes), ("strokes", strokes)):
            for sid in given:
                if sid not in clicks:
                    raise ValueError(f"SessionPool.predict: {name} names session {sid!r}, which is not in clicks in this call")
                if name == "strokes" and sid in boxes:
                    raise ValueError(f"SessionPool.predict: session {sid!r} has a box and a stroke in one call; the encoder has "
                                     "one row to give")
        for sid, box in boxes.items():
            pts = np.asarray(box, dtype=np.float64)
            if pts.shape != (4,):
                raise ValueError(f"SessionPool.predict: the box of session {sid!r} is not (r0, c0, r1, c1)")
            drawn[sid] = ("box", pts.reshape(2, 2))
        for sid, stroke in strokes.items():
            pts = np.asarray(stroke, dtype=np.float64)
            if pts.ndim != 2 or pts.shape[1] != 2 or not 2 <= len(pts) <= self.max_stroke_points:
                raise ValueError(f"SessionPool.predict: the stroke of session {sid!r} must be [P, 2] of (row, col) with "
                                 f"2 <= P <= {self.max_stroke_points}")
            cl = clicks[sid]
            if len(cl.get_clicks() if hasattr(cl, "get_clicks") else cl) == 0:
                raise ValueError(f"SessionPool.predict: the stroke of session {sid!r} comes without a click (only a box may)")
            if self.prompt_img is None:
                raise ValueError("SessionPool.predict: the network does not state its image_size, which the stroke profiles need")
            drawn[sid] = ("stroke", pts)
        for sid, (_, pts) in drawn.items():
            s = self._session(sid)
            if not (np.isfinite(pts).all() and (pts >= 0).all() and (pts[:, 0] <= s.H - 1).all() and (pts[:, 1] <= s.W - 1).all()):
                raise ValueError(f"SessionPool.predict: the drawn prompt of session {sid!r} leaves its {s.H} x {s.W} image")
        return drawn

    @torch.no_grad()
    def predict(self, clicks, prev_masks=None, boxes=None, strokes=None):
        """``clicks``: {sid: list of Click, or a Clicker}; ``prev_masks``: {sid: map} replaces that session's previous
        prediction for this call (dropped under ``_net_input``'s cascade rule; a ``RunMap`` or a COCO ``dict(size, counts)``
        stands for its pixels ``v == 1`` and is decoded through ``ops_runs``) -> {sid: bool ndarray [H, W]}, the mask
        ``probs(sid) > pred_thr``.  Sessions that are not named are untouched.

        ``boxes``: {sid: (r0, c0, r1, c1)}, a drawn box in image pixels, inclusive corners in any order.  ``strokes``: {sid:
        array-like [P, 2] of (row, col)}, a drawn stroke as the tool sampled it, 2 <= P <= ``max_stroke_points``: the points
        are used as they are, they are neither resampled nor smoothed (the poly-line through them is drawn, and each point
        is a candidate of the profile walk).  A session named in either must be in ``clicks`` too; one named in both, or a
        coordinate outside the image, raises ValueError.  A drawn prompt holds for this call only: the next call of the
        session is its clicks alone unless it draws again.

        A box may come with an empty click list (a stroke may not: its encoder row replaces the last positive click's).  The
        points of a box-only call are all padding: one not-a-point row per polarity, nothing in the click maps but the
        outline, and by the slot rule (``own_slot``) the box takes row 0.

        When ZoomIn's recalculation fires, the second round maps the SAME drawn prompt under the new crop and draws the
        stroke profiles anew from the session's generator, which goes on from where it was.  ``get_prediction`` re-runs with
        clicks only; here the annotator's box or stroke is still the prompt, on purpose."""
        drawn = self._drawn(clicks, boxes, strokes)
        todo, prev_of = [], {}
        for sid, cl in clicks.items():
            s = self._session(sid)
            s.clicks = list(cl.get_clicks() if hasattr(cl, "get_clicks") else cl)
            s.drawn = drawn.get(sid)
            todo.append(s)
        for sid, value in (prev_masks or {}).items():
            if sid not in clicks:
                raise ValueError(f"SessionPool.predict: prev_masks names session {sid!r}, which has no clicks in this call")
            s = self._session(sid)
            if self.pred.cascade_step and len(s.clicks) <= self.pred.cascade_clicks:
                continue                    # base.py:62-64: the caller's mask is dropped during the first clicks
            prev_of[sid] = self._as_map(value, s)
        out = {}
        if not todo:
            return out
        again = self._round(todo, prev_of, out)
        if again:                           # get_prediction re-runs itself, on the predictor's own previous prediction
            left = self._round(again, {}, out)
            assert not left                 # (the crop is chosen now, so the recalculation cannot fire twice)
        for s in todo:
            s.drawn = None
        return out

    def _prompts(self, members, size, points_nd):
        """(prompts, as_prompt_type) of a forward over ``members`` (then their flip copies): None and 0 when nobody drew, the
        box tensor with no-box rows and 1 when only boxes were drawn, the per-row operands and 3 when a stroke was.
        A session's profile draws happen for its row and then for its flip row, from its own generator: its result does
        not depend on who shares the forward."""
        kinds = [0 if s.drawn is None else 1 if s.drawn[0] == "box" else 2 for s in members]
        if not any(kinds):
            return None, 0
        n, n_batch, mirrors = len(members), points_nd.shape[1] // 2, ((False, True) if self.flip else (False,))
        rows = n * len(mirrors)
        boxes = np.zeros((rows, 5), dtype=np.int32)
        boxes[:, 4] = -1
        strokes = 2 in kinds
        if strokes:
            pmax = max(len(s.drawn[1]) for s in members if s.drawn is not None and s.drawn[0] == "stroke")
            curve, counts = np.zeros((rows, pmax, 2), dtype=np.int32), np.zeros(rows, dtype=np.int32)
            profiles = np.zeros((rows, 2 * self.prompt_img), dtype=np.float64)
        for j, (s, kind) in enumerate(zip(members, kinds)):
            for m, mirror in enumerate(mirrors):
                if kind == 0:
                    continue
                row, xy = m * n + j, map_drawn(s.drawn[1], s.plan[0], size, mirror)
                if kind == 1:
                    n_own = self._own_rows(s.clicks)
                    boxes[row] = box_row(xy, _padded_slot(own_slot(n_own), n_own, n_batch))
                else:
                    curve[row, :len(xy)], profiles[row] = stroke_row(xy, self.prompt_img, s.rng)
                    counts[row] = len(xy)
        boxes = torch.from_numpy(boxes)
        if not strokes:
            return (points_nd, boxes, None), 1
        kinds = torch.tensor(kinds * len(mirrors), dtype=torch.int32)
        return (points_nd, boxes, (torch.from_numpy(curve), torch.from_numpy(counts), torch.from_numpy(profiles)), kinds), 3

    def _round(self, todo, prev_of, out):
        """One forward round of ``todo`` (one forward per network input size and chunk, one read-back); fills ``out`` for
        the sessions it finishes and returns those whose ZoomIn recalculation fired."""
        ops = self.ops
        groups = {}
        for s in todo:
            s.plan = self._plan(s)
            groups.setdefault(s.plan[1], []).append(s)
        ops.begin(_Round(todo))
        spans = []
        for size, group in groups.items():
            for at in range(0, len(group), self.max_batch):
                members = group[at:at + self.max_batch]
                first = pfirst = None
                for j, s in enumerate(members):
                    prev = prev_of.get(s.sid, s.canvas[s.prev]) if self.prev_channel else None
                    i = ops.add_input(s, s.plan[0], j, prev)
                    first = i if first is None else first
                for j, s in enumerate(members):
                    i = ops.add_paste(s, s.plan[3], j)
                    pfirst = i if pfirst is None else pfirst
                spans.append((size, members, first, pfirst))
        ops.upload()
        for size, members, first, pfirst in spans:
            image_nd = ops.resize(members, first, size, self.flip, 4 if self.prev_channel else 3)
            points_nd = self.pred.get_points_nd(self.flipped_click_lists([s.plan[2] for s in members], size[1])).float()
            probs = self._forward(image_nd, points_nd, *self._prompts(members, size, points_nd))
            self.forwards += 1
            ops.paste(members, pfirst, probs, self.pred_thr, self.zoom.prob_thresh if self.zoom else 0.5)
        got = ops.readback()
        self.readbacks += 1
        again = []
        for s in todo:
            rec, mask = ops.layout.decode(got, ops.layout.row[s.sid])
            if self.zoom is not None:
                s.box = tuple(int(v) for v in rec[1:6])       # ZoomIn._probs is the new prediction either way
            if self._wants_recalc(s):
                again.append(s)             # prev_prediction stays; the click runs again, zoomed
                continue
            s.prev = 1 - s.prev             # prev_prediction = the new canvas
            out[s.sid] = mask
        return again
