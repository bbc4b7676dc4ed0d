"""Several interactive sessions served through one batched forward.

``BasePredictor.get_prediction(clicker, prev_mask)`` is one session per forward and hands back the full fp32 map
(``4 * H * W`` bytes device-to-host per click), which the caller then thresholds.  ``SessionPool`` holds up to
``max_sessions`` sessions (image, previous prediction, ZoomIn state, each of its own size); ``predict`` takes the pending
click lists of any subset of them and runs them through ONE forward per network input size, then one launch of
``vpu_session_paste_batched`` that writes every session's probability canvas, its mask ``> pred_thr`` at one bit per pixel
and the ZoomIn box, and ONE device-to-host copy of the records and packed masks of all sessions (about ``H * W / 8`` bytes
per session).  The probability maps stay on the device (``probs``).

Per session the results are those of a private copy of the predictor: every per-session operation is the sequential one
(``ZoomIn.transform`` restated on the host exactly as ``BatchedEvaluator._plan`` does, the crop / resize / mirror of
``vpu_roi_resize_batched``, the predictor's own flip average and sigmoid on the whole batch, the paste with
``vpu_roi_paste_batched``'s per-pixel expression); what the batch shares is the network, whose click rows are padded to a
common count by ``get_points_nd`` with not-a-point rows that it ignores.  In the ``f32`` engine mode the maps are the
sequential ones bit for bit.  ``check_possible_recalculation`` is honoured inside the call: the sessions it fires for run a
second forward of their own, as ``get_prediction`` re-runs itself.

Click prompts only (there is no ground truth to derive boxes from).  On a CPU device the same scheduler runs with torch /
numpy stand-ins of the two kernels (``_HostOps``), which is what the CPU tests check it with."""
import ctypes as C

import numpy as np
import torch

from .batched import BatchedEvaluator, _load_image, batchable
from .transforms import AddHorizontalFlip, Roi, ZoomIn

_REC = 4             # int64 per session record (int32 [8]: area, count, rmin, rmax, cmin, cmax, 0, 0)


# ------------------------------------------------------------------------------------------------------ the bit codec
def n_words(hw):
    return (int(hw) + 63) // 64


def pack_mask(mask):
    """bool [H, W] -> uint64 [ceil(H * W / 64)]: pixel i = r * W + c is bit i & 63 of little-endian word i >> 6; the bits at or
    beyond H * W are zero."""
    flat = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
    padded = np.zeros(n_words(flat.size) * 64, dtype=bool)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def unpack_mask(words, H, W):
    """The inverse of ``pack_mask``: 64-bit words (uint64 or the int64 of a read-back) -> bool [H, W]."""
    raw = np.ascontiguousarray(words).view(np.uint64).astype("<u8").view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[:H * W].astype(bool).reshape(H, W)


def host_session_paste(prob_map, H, W, roi, pred_thr, box_thr):
    """Stand-in of vpu_session_paste_batched for one session: ``prob_map`` fp32 [S_h, S_w] (cpu) resized to the roi and pasted
    into zeros -> (canvas fp32 [H, W], packed mask uint64, record int32 [8])."""
    r0, r1, c0, c1 = roi
    h, w = r1 - r0 + 1, c1 - c0 + 1
    patch = prob_map.float()[None, None]
    if tuple(patch.shape[2:]) != (h, w):
        patch = torch.nn.functional.interpolate(patch, size=(h, w), mode="bilinear", align_corners=True)
    canvas = torch.zeros(H, W, dtype=torch.float32)
    canvas[r0:r1 + 1, c0:c1 + 1] = patch[0, 0]
    values = canvas.numpy()
    mask = values > np.float32(pred_thr)
    on = np.argwhere(values > np.float32(box_thr))
    if len(on):
        box = [len(on), int(on[:, 0].min()), int(on[:, 0].max()), int(on[:, 1].min()), int(on[:, 1].max())]
    else:
        box = [0, H, -1, W, -1]
    return canvas, pack_mask(mask), np.array([int(mask.sum())] + box + [0, 0], dtype=np.int32)


class _Session:
    """One session's state (a slot of the pool); the attribute names are the ones ``BatchedEvaluator._plan`` reads."""

    def __init__(self, sid, image):
        self.sid, self.image = sid, image
        self.H, self.W = int(image.shape[1]), int(image.shape[2])
        self.canvas = [torch.zeros(self.H, self.W, device=image.device, dtype=torch.float32) for _ in range(2)]
        self.prev = 0                  # canvas[prev] is the predictor's prev_prediction
        self.clicks = []               # the click list of the call in progress
        self.roi = None                # ZoomIn._object_roi
        self.box = None                # (count, r0, r1, c0, c1) of ZoomIn._probs > prob_thresh (no clicks); None: no _probs
        self.plan = None


class _Round:
    """Layout of a forward round's read-back: ``_REC`` int64 per session, then every session's packed words."""

    def __init__(self, sessions):
        self.row = {s.sid: i for i, s in enumerate(sessions)}
        self.at, at = {}, _REC * len(sessions)
        for s in sessions:
            self.at[s.sid] = at
            at += n_words(s.H * s.W)
        self.size = at

    def decode(self, out, s):
        """(record int32 [8], mask bool [H, W]) of session ``s`` from the read-back ``out`` (int64)."""
        i = self.row[s.sid]
        rec = out[_REC * i:_REC * (i + 1)].view(np.int32)
        return rec, unpack_mask(out[self.at[s.sid]:self.at[s.sid] + n_words(s.H * s.W)], s.H, s.W)


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
        d.rec = self.out.data_ptr() + 8 * _REC * self.layout.row[s.sid]
        d.H, d.W = s.H, s.W
        d.r0, d.r1, d.c0, d.c1 = r0, r1, c0, c1
        d.src = src
        self._out.append(d)
        return len(self._out) - 1

    def upload(self):
        inp = (self._lib.EvalObj * len(self._inp))(*self._inp)
        self._out_at0 = C.sizeof(inp)                 # the paste rows ride behind the input rows in the same copy
        raw = bytes(inp) + bytes((self._lib.SessionObj * len(self._out))(*self._out))
        self._host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()   # (alive until the read-back)
        self.desc = self._host.to(self.device, non_blocking=True)

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
        for s, (r0, r1, c0, c1), src, prev in self._inp[first:first + len(sessions)]:
            x = torch.cat((s.image[None], prev[None, None]), 1) if channels == 4 else s.image[None]
            x = x[:, :, r0:r1 + 1, c0:c1 + 1]
            if tuple(x.shape[2:]) != tuple(size):
                x = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)
            rows.append((src, x.clone()))
        batch = torch.cat([r for _, r in sorted(rows, key=lambda t: t[0])], 0)
        return torch.cat([batch, batch.flip(3)], 0) if flip else batch

    def paste(self, sessions, first, probs, pred_thr, box_thr):
        for s, roi, src in self._out[first:first + len(sessions)]:
            canvas, words, rec = host_session_paste(probs[src, 0], s.H, s.W, roi, pred_thr, box_thr)
            s.canvas[1 - s.prev].copy_(canvas)
            i, at = self.layout.row[s.sid], self.layout.at[s.sid]
            self.out[_REC * i:_REC * (i + 1)] = rec.view(np.int64)
            self.out[at:at + len(words)] = words.view(np.int64)

    def readback(self):
        return self.out.copy()


class SessionPool:
    """``pool = SessionPool(predictor, max_sessions=8, pred_thr=0.49)``; ``predictor``: a ``BasePredictor`` for which
    ``batched.batchable(predictor)`` holds (ValueError otherwise).  It lends the pool its network, its transforms' parameters,
    ``get_points_nd`` / ``net_clicks_limit`` and the cascade rule for ``prev_masks``; its own image and state are not touched.

    ``sid = pool.open(image)``; ``pool.predict({sid: clicks, ...}, prev_masks=None) -> {sid: bool ndarray [H, W]}``;
    ``pool.probs(sid)``; ``pool.get_states(sid)`` / ``pool.set_states(sid, st)``; ``pool.close(sid)``.
    ``max_batch``: sessions per forward (default ``max_sessions``); a size group with more runs in chunks.
    ``readbacks`` counts the device-to-host synchronisations (one per forward round)."""

    # ZoomIn on the host, from the box read back with the last prediction: BatchedEvaluator's restatement of ZoomIn.transform /
    # _predicted_box / check_possible_recalculation, used as it stands (they read .zoom and a slot's clicks / roi / box / H / W)
    _predicted_box = BatchedEvaluator._predicted_box
    _plan = BatchedEvaluator._plan
    _wants_recalc = BatchedEvaluator._wants_recalc

    def __init__(self, predictor, max_sessions=8, pred_thr=0.49, max_batch=None):
        if not batchable(predictor):
            raise ValueError("SessionPool: the predictor's transforms are not the batched path's (batched.batchable): only "
                             "[ZoomIn with a (height, width) target_size] [SigmoidForPred] [AddHorizontalFlip]")
        if int(max_sessions) < 1 or (max_batch is not None and int(max_batch) < 1):
            raise ValueError("SessionPool: max_sessions and max_batch must be at least 1")
        self.pred, self.max_sessions, self.pred_thr = predictor, int(max_sessions), float(pred_thr)
        self.max_batch = int(max_batch) if max_batch is not None else self.max_sessions
        self.zoom = predictor.zoom_in
        self.flip = any(type(t) is AddHorizontalFlip for t in predictor.transforms)
        self.inv = [t for t in reversed(predictor.transforms) if type(t) is not ZoomIn]   # flip average, then sigmoid
        self.prev_channel = bool(getattr(predictor.net, "with_prev_mask", True))
        self.device = torch.device(predictor.device)
        self.ops = _DeviceOps(self.device) if self.device.type == "cuda" else _HostOps(self.device)
        self._slots = [None] * self.max_sessions
        self.readbacks = self.forwards = 0

    # ---------------------------------------------------------------------------------------------- sessions
    def open(self, image):
        """A new session on ``image`` (``set_input_image``'s conversions) -> its id; ids of closed sessions are reused."""
        for sid, held in enumerate(self._slots):
            if held is None:
                self._slots[sid] = _Session(sid, _load_image(image, self.device))
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

    def get_states(self, sid):
        s = self._session(sid)
        return {"roi": s.roi, "box": s.box, "prev_prediction": s.canvas[s.prev].clone()}

    def set_states(self, sid, states):
        s = self._session(sid)
        prev = states["prev_prediction"]
        assert tuple(prev.shape[-2:]) == (s.H, s.W), "the state is of another image size"
        s.roi, s.box = states["roi"], states["box"]
        s.canvas[s.prev].copy_(prev.reshape(s.H, s.W))

    # ---------------------------------------------------------------------------------------------- prediction
    def _as_map(self, value, s):
        if not torch.is_tensor(value):
            value = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32))
        assert value.numel() == s.H * s.W, "prev_masks: a map of another size than the session's image"
        return value.to(self.device).float().reshape(s.H, s.W).contiguous()

    @torch.no_grad()
    def predict(self, clicks, prev_masks=None):
        """``clicks``: {sid: list of Click, or a Clicker}; ``prev_masks``: {sid: map} replaces that session's previous
        prediction for this call (dropped under ``_net_input``'s cascade rule) -> {sid: bool ndarray [H, W]}, the mask
        ``probs(sid) > pred_thr``.  Sessions that are not named are untouched."""
        todo, prev_of = [], {}
        for sid, cl in clicks.items():
            s = self._session(sid)
            s.clicks = list(cl.get_clicks() if hasattr(cl, "get_clicks") else cl)
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
        return out

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
            lists = [s.plan[2] for s in members]
            if self.flip:
                lists = lists + [[c.copy(coords=(c.coords[0], size[1] - c.coords[1] - 1)) for c in cl] for cl in lists]
            logits = self.pred.net(image_nd, self.pred.get_points_nd(lists).float())['instances']
            self.forwards += 1
            if tuple(logits.shape[2:]) != tuple(image_nd.shape[2:]):
                from .transforms import resize_align_corners
                logits = resize_align_corners(logits, image_nd.shape[2:])
            probs = logits
            for t in self.inv:
                probs = t.inv_transform(probs)
            ops.paste(members, pfirst, probs, self.pred_thr, self.zoom.prob_thresh if self.zoom else 0.5)
        got = ops.readback()
        self.readbacks += 1
        again = []
        for s in todo:
            rec, mask = ops.layout.decode(got, s)
            if self.zoom is not None:
                s.box = tuple(int(v) for v in rec[1:6])       # ZoomIn._probs is the new prediction either way
            if self._wants_recalc(s):
                again.append(s)             # prev_prediction stays; the click runs again, zoomed
                continue
            s.prev = 1 - s.prev             # prev_prediction = the new canvas
            out[s.sid] = mask
        return again
