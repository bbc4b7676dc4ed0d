"""Multi-object annotation over ``SessionPool``: several objects per image, objects built from parts, initial masks, undo
and reopening, with every map on the device.

A ``SessionPool`` session is one object: one probability canvas, one bit-packed mask per click.  ``AnnotationPool`` keeps,
per image, a 16-bit label map of the committed objects and the object being edited -- its click list, the parts finished
so far (``parts``), an optional initial mask and an undo stack -- and drives one pool session per image through the pool's
public methods only (``open / close / predict / probs / get_states / set_states``).  The rules:

  R1  current = max(parts, additive), the mask is current > prob_thresh (strict); additive is the session's previous
      prediction, zeros while the object has no clicks.
  R2  the preview label map is ``labels`` with object_count + 1 under the current mask; ``labels`` is not modified.
  R3  a click is appended and predicted through the pool; an initial mask is that session's ``prev_masks`` entry on every
      click, and the first click of such an object is predicted twice.
  R4  partial finish: parts = current, the click list emptied, the session reset, the initial mask cleared.
  R5  finish: labels = object_count + 1 under the current mask (earlier objects are overwritten there), the count goes up,
      the record is appended, the object starts anew.
  R6  undo restores the object as it was before its last click or partial finish (a stack of at most ``max_undo``).
  R7  an initial mask stands in for ``parts`` until a partial finish or finish clears it.
  R8  reopen removes a committed label from ``labels`` and makes its pixels the initial mask.
  R9  tidy drops small islands of R1's mask and fills its small holes (regions.py, rules T1-T8; the seeds are the object's
      clicks): an undo snapshot first, then additive and parts / initial mask both take the edits 0.0 / 1.0, so R1's mask
      is the cleaned one from then on.

All of this is max, a strict compare and integer writes, done by ``vpu_annot_compose_batched`` / ``vpu_label_extract``
(csrc/evalbatch.hip, section 7): what crosses to the host is the packed mask (``H * W / 8`` bytes) or the 32-byte record,
never an fp32 map.  On a CPU predictor the numpy stand-ins ``host_annot_compose`` / ``host_label_extract`` run instead
(``HostAnnotOps``); ``pool.ops`` may be replaced by them on a device pool, which is how the GPU tests build their twin."""
import numpy as np
import torch

from .clicker import Click, Clicker
from .outlines import DeviceOutlineOps, HostOutlineOps
from .polygons import check_request
from .regions import DeviceRegionOps, HostRegionOps, TidyItem, check_tidy_args, click_seeds
from .runs import KIND_LABELS, KIND_PROB, DeviceRunOps, HostRunOps, RunMap, as_run_map, stack_objects
from ._batchcore import PackedLayout, host_count_box, pack_mask, unpack_mask, upload_structs
from .sessions import SessionPool

MAX_LABEL = 65535


# ------------------------------------------------------------------------------------------------------ host stand-ins
def _record(mask, overwritten):
    """int32 [8]: area, overwritten, rmin, rmax, cmin, cmax, 0, 0."""
    area, *box = host_count_box(mask, *mask.shape)
    return np.array([area, overwritten] + box + [0, 0], dtype=np.int32)


def host_annot_compose(add, total, labels, H, W, label, mode, thr):
    """Stand-in of vpu_annot_compose_batched for one annotation.  ``add`` / ``total``: fp32 [H, W] or None (zeros), ``labels``:
    uint16 [H, W] or None; ``total`` and ``labels`` are written in place as ``mode`` says -> (packed mask uint64, record
    int32 [8])."""
    zeros = np.zeros((H, W), dtype=np.float32)
    cur = np.maximum(zeros if total is None else total, zeros if add is None else add)
    mask = cur > np.float32(thr)
    over = 0 if labels is None else int((mask & (labels != 0) & (labels != np.uint16(label))).sum())
    if mode & 1 and total is not None:
        total[...] = cur
    if mode & 2 and labels is not None:
        labels[mask] = np.uint16(label)
    return pack_mask(mask), _record(mask, over)


def host_label_extract(labels, label):
    """Stand-in of vpu_label_extract: ``labels`` uint16 [H, W], its ``label`` pixels set to 0 in place -> (fp32 [H, W] of
    1 / 0, record int32 [8])."""
    mask = labels == np.uint16(label)
    labels[mask] = 0
    return mask.astype(np.float32), _record(mask, 0)


# ------------------------------------------------------------------------------------------------------ the two kernels
class _Item:
    """One row of a compose call; ``add`` / ``total`` fp32 [H, W] tensors or None, ``labels`` int16 [H, W] tensor or None."""

    def __init__(self, H, W, add=None, total=None, labels=None, label=0, mode=0):
        self.H, self.W, self.add, self.total, self.labels, self.label, self.mode = H, W, add, total, labels, int(label), int(mode)


class DeviceAnnotOps:
    """The HIP kernels: the descriptors of a call go up in one copy, its records and packed masks come back in one."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self._ops, self.device = _lib, ops, torch.device(device)

    def compose(self, items, thr, read):
        """``read``: "masks" -> [(record, mask bool [H, W])], "records" -> [(record, None)] (one read-back each), None ->
        nothing is read back and nothing waited for."""
        n, layout = len(items), PackedLayout([(it.H, it.W) for it in items])
        out = torch.empty(layout.size, device=self.device, dtype=torch.int64)
        assert out.data_ptr() % 8 == 0
        rows = []
        for i, it in enumerate(items):
            assert it.H >= 1 and it.W >= 1 and it.H * it.W < 2 ** 31 and 0 <= it.label <= MAX_LABEL and 0 <= it.mode <= 3
            for t in (it.add, it.total):
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == it.H * it.W
                                     and t.device == out.device and t.data_ptr() % 16 == 0)
            assert it.labels is None or (it.labels.dtype == torch.int16 and it.labels.is_contiguous() and it.labels.numel() == it.H * it.W
                                         and it.labels.device == out.device and it.labels.data_ptr() % 8 == 0)
            d = self._lib.AnnotObj()
            d.add = it.add.data_ptr() if it.add is not None else None
            d.total = it.total.data_ptr() if it.total is not None else None
            d.labels = it.labels.data_ptr() if it.labels is not None else None
            d.bits = out.data_ptr() + 8 * layout.bits_at(i)
            d.rec = out.data_ptr() + 8 * layout.rec_at(i)
            d.H, d.W, d.label, d.mode = it.H, it.W, it.label, it.mode
            rows.append(d)
        host, desc, _ = upload_structs(self.device, (self._lib.AnnotObj * n)(*rows))    # (host: alive until the read-back)
        self._ops.annot_compose_batched(desc, n, thr, max(it.H * it.W for it in items))
        if read is None:
            return None
        got = (out if read == "masks" else out[:layout.rec_at(n)]).cpu().numpy()        # the call's one synchronisation
        return [layout.decode(got, i, read == "masks") for i in range(n)]

    def extract(self, labels, label):
        """-> (fp32 [H, W] on the device, record); one read-back (32 bytes)."""
        out = torch.empty(labels.shape, device=self.device, dtype=torch.float32)
        rec = torch.empty(8, device=self.device, dtype=torch.int32)
        self._ops.label_extract(labels, label, out, rec)
        return out, rec.cpu().numpy()


class HostAnnotOps:
    """The numpy stand-ins behind the same two calls; maps on a device are copied to the host and back."""

    def __init__(self, device=None):
        self.device = device

    @staticmethod
    def _host(t, kind):
        return None if t is None else t.detach().cpu().numpy().view(kind)

    def compose(self, items, thr, read):
        got = []
        for it in items:
            add, total, labels = self._host(it.add, np.float32), self._host(it.total, np.float32), self._host(it.labels, np.uint16)
            words, rec = host_annot_compose(add, total, labels, it.H, it.W, it.label, it.mode, thr)
            if it.mode & 1 and total is not None and it.total.device.type != "cpu":
                it.total.copy_(torch.from_numpy(total))
            if it.mode & 2 and labels is not None and it.labels.device.type != "cpu":
                it.labels.copy_(torch.from_numpy(labels.view(np.int16)))
            got.append((rec, unpack_mask(words, it.H, it.W) if read == "masks" else None))
        return None if read is None else got

    def extract(self, labels, label):
        host = self._host(labels, np.uint16)
        out, rec = host_label_extract(host, label)
        if labels.device.type != "cpu":
            labels.copy_(torch.from_numpy(host.view(np.int16)))
        return torch.from_numpy(out).to(labels.device), rec


# ------------------------------------------------------------------------------------------------------ the pool
class _Annotation:
    """One image: the committed labels and the object being edited."""

    def __init__(self, aid, H, W, device):
        self.aid, self.H, self.W = aid, H, W
        self.labels = torch.zeros(H, W, device=device, dtype=torch.int16)      # uint16 values in 16-bit storage
        self.zeros = torch.zeros(H, W, device=device, dtype=torch.float32)     # (never written)
        self.object_count, self.records = 0, []
        self.start()

    def start(self):
        """A new object.  ``parts`` and ``mask`` are None for zeros / no mask; a tensor that an undo snapshot may hold is
        never written again (a partial finish makes a new one)."""
        self.clicker, self.parts, self.mask, self.undo = Clicker(device=None), None, None, []

    @property
    def total(self):
        return self.mask if self.mask is not None else self.parts      # R7: the initial mask stands in for the parts

    @property
    def empty(self):
        return len(self.clicker) == 0 and self.parts is None and self.mask is None


class AnnotationPool:
    """``ann = AnnotationPool(predictor, max_images=8, prob_thresh=0.5, max_undo=32, **session_pool_kwargs)``; ``predictor``:
    any predictor ``SessionPool`` accepts.  ``aid = ann.open(image, seed=None)``; ``ann.click({aid: click, ...}, boxes=None,
    strokes=None) -> {aid: bool ndarray [H, W]}``; ``undo / partially_finish / finish / set_mask / load / reopen / label_map /
    label_runs / label_outlines / export / objects / object_count / current_prob / close`` take an ``aid``.

    ``readbacks`` counts the device-to-host synchronisations, the pool's included: a click on objects without parts and
    initial mask costs the pool's, otherwise one compose launch and one more read-back for those annotations together;
    ``finish`` one launch and one read-back (32 bytes), ``label_map`` one copy, ``reopen`` one read-back (32 bytes), ``undo``
    one (the mask), ``tidy`` one for all named annotations (``ops_regions``, replaceable by ``HostRegionOps()``),
    ``partially_finish`` and ``current_prob`` none; ``label_runs`` two (the offsets, then 8 bytes per run) and
    ``export`` two, none when no object is finished; ``label_outlines`` two (``ops_outlines``, replaceable by
    ``HostOutlineOps()``) and ``export(aid, polygons=True)`` two more.  ``ops`` holds the two device operations and may be replaced by
    ``HostAnnotOps()``; ``ops_runs`` holds the run-length encoder and decoder and may be replaced by ``HostRunOps()``.
    ``load(aid, objects)`` and ``set_mask(aid, RunMap or COCO dict)`` bring run-length objects onto the device through
    ``ops_runs.decode``: one copy up, one launch, no read-back."""

    def __init__(self, predictor, max_images=8, prob_thresh=0.5, max_undo=32, **session_pool_kwargs):
        if int(max_undo) < 0:
            raise ValueError("AnnotationPool: max_undo must not be negative")
        if "max_sessions" in session_pool_kwargs or "pred_thr" in session_pool_kwargs:
            raise ValueError("AnnotationPool: max_sessions and pred_thr are max_images and prob_thresh here")
        self.prob_thresh, self.max_images, self.max_undo = float(prob_thresh), int(max_images), int(max_undo)
        # the pool's own mask is then R1's whenever the object has neither parts nor an initial mask
        self.pool = SessionPool(predictor, max_sessions=self.max_images, pred_thr=self.prob_thresh, **session_pool_kwargs)
        self.device = self.pool.device
        self.ops = DeviceAnnotOps(self.device) if self.device.type == "cuda" else HostAnnotOps(self.device)
        self.ops_runs = DeviceRunOps(self.device) if self.device.type == "cuda" else HostRunOps(self.device)
        self.ops_regions = DeviceRegionOps(self.device) if self.device.type == "cuda" else HostRegionOps(self.device)
        self.ops_outlines = DeviceOutlineOps(self.device) if self.device.type == "cuda" else HostOutlineOps(self.device)
        self._held = {}
        self._own_readbacks = 0

    readbacks = property(lambda self: self.pool.readbacks + self._own_readbacks)
    forwards = property(lambda self: self.pool.forwards)

    # ---------------------------------------------------------------------------------------------- images
    def open(self, image, seed=None):
        """A new annotation of ``image`` -> its id (the id of its pool session; ids of closed ones are reused)."""
        try:
            aid = self.pool.open(image, seed)
        except ValueError:
            raise ValueError(f"AnnotationPool: all {self.max_images} images are open") from None
        H, W = (int(v) for v in self.pool.probs(aid).shape[-2:])
        self._held[aid] = _Annotation(aid, H, W, self.device)
        return aid

    def close(self, aid):
        self._ann(aid)
        self.pool.close(aid)
        del self._held[aid]

    def _ann(self, aid):
        if not isinstance(aid, (int, np.integer)) or aid not in self._held:
            raise KeyError(f"AnnotationPool: no open annotation {aid!r}")
        return self._held[aid]

    # ---------------------------------------------------------------------------------------------- the object in progress
    def _additive(self, a):
        return self.pool.probs(a.aid)[0, 0] if len(a.clicker) else None     # zeros while the object has no clicks

    def _reset_session(self, a):
        self.pool.set_states(a.aid, {"roi": None, "box": None, "prev_prediction": a.zeros})

    def _snapshot(self, a):
        a.undo.append((a.clicker.get_state(), self.pool.get_states(a.aid), a.parts, a.mask))
        if len(a.undo) > self.max_undo:
            del a.undo[0]

    def _item(self, a, **more):
        return _Item(a.H, a.W, add=self._additive(a), total=a.total, **more)

    def _next_label(self, a):
        if a.object_count + 1 > MAX_LABEL:
            raise ValueError(f"AnnotationPool: label {a.object_count + 1} does not fit the 16-bit label map")
        return a.object_count + 1

    def _masks(self, anns):
        """R1's masks of ``anns`` by one compose launch and one read-back."""
        got = self.ops.compose([self._item(a) for a in anns], self.prob_thresh, "masks")
        self._own_readbacks += 1
        return {a.aid: mask for a, (_, mask) in zip(anns, got)}

    @torch.no_grad()
    def click(self, clicks, boxes=None, strokes=None):
        """``clicks``: {aid: Click or (is_positive, (row, col))}, one click per named annotation; ``boxes`` / ``strokes`` are
        ``SessionPool.predict``'s, keyed by ``aid`` -> {aid: the current object's mask}."""
        anns = [self._ann(aid) for aid in clicks]
        new = {}
        for aid, c in clicks.items():
            new[aid] = c.copy() if isinstance(c, Click) else Click(bool(c[0]), (int(c[1][0]), int(c[1][1])))
        for a in anns:
            self._snapshot(a)
            a.clicker.add_click(new[a.aid])
        try:
            out = self.pool.predict({a.aid: a.clicker for a in anns}, prev_masks={a.aid: a.mask for a in anns if a.mask is not None},
                                    boxes=boxes, strokes=strokes)
        except Exception:
            for a in anns:                   # the pool refuses a call before it changes a session: take the click back
                a.clicker._remove_last_click()
                a.undo.pop()
            raise
        twice = [a for a in anns if a.mask is not None and len(a.clicker) == 1]
        if twice:                           # the first click on an initial mask runs again, on the ZoomIn state the first pass left
            named = {a.aid for a in twice}
            out.update(self.pool.predict({a.aid: a.clicker for a in twice}, prev_masks={a.aid: a.mask for a in twice},
                                         boxes={k: v for k, v in (boxes or {}).items() if k in named},
                                         strokes={k: v for k, v in (strokes or {}).items() if k in named}))
        composed = [a for a in anns if a.total is not None]
        if composed:
            out.update(self._masks(composed))
        return {a.aid: out[a.aid] for a in anns}

    def undo(self, aid):
        """Back to before the object's last click or partial finish -> its mask then, or None when there is nothing to undo."""
        a = self._ann(aid)
        if not a.undo:
            return None
        clicks, states, a.parts, a.mask = a.undo.pop()
        a.clicker.click_indx_offset = 1 if a.mask is not None else 0
        a.clicker.set_state(clicks)
        self.pool.set_states(aid, states)
        if a.empty:
            return np.zeros((a.H, a.W), dtype=bool)
        return self._masks([a])[aid]

    def tidy(self, aids, min_area=0, max_hole=0, keep="all"):
        """R9: the region clean-up of regions.py (rules T1-T8) on R1's mask of the named annotations' objects -> {aid: mask}.
        Components below ``min_area`` pixels are dropped, holes of at most ``max_hole`` pixels filled (None: every hole);
        ``keep``: "all", "seeded" or "largest".  The seeds are the object's clicks.  An undo snapshot is pushed first; then both
        maps take the edits (0.0 on dropped pixels, 1.0 on filled ones): the session's previous prediction when the object has
        clicks, and a NEW tensor in place of the parts or the initial mask when there is one (a snapshot may hold the old one,
        which is never written).  The click list, ``click_indx_offset`` and the ZoomIn state stay.  One launch group and one
        read-back for all of them; an empty object gives an all-False mask and pushes nothing."""
        min_area, max_hole = check_tidy_args("AnnotationPool.tidy", min_area, max_hole, keep)
        if not 0.0 <= self.prob_thresh < 1.0:   # the edits 0.0 and 1.0 must fall on the clear and the set side of it
            raise ValueError(f"AnnotationPool.tidy: prob_thresh {self.prob_thresh} is outside [0, 1)")
        anns = [self._ann(aid) for aid in aids]
        out = {a.aid: np.zeros((a.H, a.W), dtype=bool) for a in anns if a.empty}
        live, items = [a for a in anns if not a.empty], []
        for a in live:
            self._snapshot(a)
            add, total = self._additive(a), a.total
            items.append(TidyItem(a.H, a.W, add=add, total=total, add_out=None if add is None else torch.empty_like(add),
                                  total_out=None if total is None else torch.empty_like(total),
                                  seeds=click_seeds(a.clicker.get_clicks()), min_area=min_area, max_hole=max_hole, keep=keep))
        if not live:
            return out
        got = self.ops_regions.tidy(items, self.prob_thresh, "masks")
        self._own_readbacks += 1
        for a, it, (_, mask) in zip(live, items, got):
            if it.add_out is not None:
                self.pool.set_states(a.aid, dict(self.pool.get_states(a.aid), prev_prediction=it.add_out))
            if a.mask is not None:
                a.mask = it.total_out
            elif a.parts is not None:
                a.parts = it.total_out
            out[a.aid] = mask
        return {a.aid: out[a.aid] for a in anns}

    def partially_finish(self, aid):
        """R4.  No synchronisation: one launch that writes the new parts."""
        a = self._ann(aid)
        if a.empty:
            return
        self._snapshot(a)
        parts = a.total.clone() if a.total is not None else torch.zeros_like(a.zeros)
        if len(a.clicker):
            self.ops.compose([_Item(a.H, a.W, add=self._additive(a), total=parts, mode=1)], self.prob_thresh, None)
        a.parts, a.mask = parts, None
        a.clicker.reset_clicks()
        a.clicker.click_indx_offset = 0
        self._reset_session(a)

    def finish(self, aid):
        """R5 -> the object's record ``dict(label, area, box=(rmin, rmax, cmin, cmax), overwritten)``, None for an empty
        object.  The box of an object without a pixel is (H, -1, W, -1)."""
        a = self._ann(aid)
        if a.empty:
            return None
        label = self._next_label(a)
        (rec, _), = self.ops.compose([self._item(a, labels=a.labels, label=label, mode=2)], self.prob_thresh, "records")
        self._own_readbacks += 1
        record = dict(label=label, area=int(rec[0]), box=tuple(int(v) for v in rec[2:6]), overwritten=int(rec[1]))
        a.object_count = label
        a.records.append(record)
        a.start()
        self._reset_session(a)
        return dict(record)

    def _as_mask(self, a, mask):
        if torch.is_tensor(mask):
            mask = mask.detach()
        else:
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        if tuple(mask.shape) != (a.H, a.W):
            raise ValueError(f"AnnotationPool: a mask of {tuple(mask.shape)} for an image of {(a.H, a.W)}")
        return mask.to(self.device).float().contiguous().clone()

    def _run_map(self, a, value, label=1):
        """``value`` (a RunMap or a COCO ``dict(size, counts)``) as a checked RunMap of the image's size."""
        rm = as_run_map(value, label)
        if rm.size != (a.H, a.W):
            raise ValueError(f"AnnotationPool: a map of {rm.size} for an image of {(a.H, a.W)}")
        return rm

    def set_mask(self, aid, mask, label=1):
        """R7: the object in progress is discarded; ``mask`` (bool or float [H, W]) is the new object's initial mask.  A
        ``RunMap`` or a COCO ``dict(size, counts)`` is taken as well: the initial mask is then ``v == label``, decoded on the
        device from 8 bytes per run -- no raster is uploaded, nothing is read back -- and is bit for bit what
        ``set_mask(aid, rm.decode() == label)`` gives.  ``label`` is not read for arrays and tensors."""
        a = self._ann(aid)
        if isinstance(mask, (RunMap, dict)):
            if not (isinstance(label, (int, np.integer)) and 0 <= label <= MAX_LABEL):
                raise ValueError(f"AnnotationPool: label {label!r} is not an integer in 0 .. {MAX_LABEL}")
            rm = self._run_map(a, mask, label)
            mask = torch.empty(a.H, a.W, device=self.device, dtype=torch.float32)
            self.ops_runs.decode([(rm, mask, KIND_PROB, int(label))])
        else:
            mask = self._as_mask(a, mask)
        a.start()
        self._reset_session(a)
        a.mask = mask
        a.clicker.click_indx_offset = 1

    def reopen(self, aid, label):
        """R8.  The record of ``label`` leaves ``objects``; finishing the reopened object appends a new one."""
        a = self._ann(aid)
        if not isinstance(label, (int, np.integer)) or not any(r["label"] == label for r in a.records):
            raise KeyError(f"AnnotationPool: annotation {aid!r} has no object {label!r}")
        out, rec = self.ops.extract(a.labels, int(label))
        self._own_readbacks += 1
        if int(rec[0]) == 0:                # later objects have overwritten all of it: nothing was changed
            raise KeyError(f"AnnotationPool: no pixel of annotation {aid!r} holds label {label!r} any more")
        a.records = [r for r in a.records if r["label"] != label]
        a.start()
        self._reset_session(a)
        a.mask = out
        a.clicker.click_indx_offset = 1

    # ---------------------------------------------------------------------------------------------- results
    def label_map(self, aid, preview=True):
        """uint16 [H, W]: the committed labels, with ``preview`` R2's (the object in progress drawn with its future label)."""
        a = self._ann(aid)
        labels = a.labels
        if preview and not a.empty:
            labels = a.labels.clone()
            self.ops.compose([self._item(a, labels=labels, label=self._next_label(a), mode=2)], self.prob_thresh, None)
        self._own_readbacks += 1
        host = labels.cpu().numpy().view(np.uint16)
        return host.copy() if labels is a.labels and self.device.type == "cpu" else host

    def label_runs(self, aid, preview=True):
        """The ``RunMap`` (runs.py) of exactly the array ``label_map(aid, preview)`` returns, built as that method builds it
        and encoded on the device: two read-backs, the offsets and 8 bytes per run, in place of the 16-bit map."""
        a = self._ann(aid)
        labels = a.labels
        if preview and not a.empty:
            labels = a.labels.clone()
            self.ops.compose([self._item(a, labels=labels, label=self._next_label(a), mode=2)], self.prob_thresh, None)
        rm, = self.ops_runs.encode([(labels, KIND_LABELS, 0.0)])
        self._own_readbacks += 2
        return rm

    def label_outlines(self, aid, labels=None, preview=True, tolerance=None):
        """{label: Outline} (outlines.py): the polygon loops of ``label_map(aid, preview) == label`` for every label of
        ``labels`` (integers in 0 .. 65535; default: every committed object's label and, with ``preview``, that of the object
        in progress), traced on the device from the map built as ``label_map`` builds it.  One item per label, all in ONE trace:
        two read-backs.  A label no pixel holds gives an outline without loops; without a label to trace the result is {} and
        the device is not touched.  With a ``tolerance`` in pixels (0 .. 1024; sides up to 8191, else ValueError before any
        launch) {label: Polygons} (polygons.py): the loops simplified on the device, three read-backs."""
        a = self._ann(aid)
        if tolerance is not None:
            check_request(tolerance, [tuple(a.labels.shape)])
        drawn = preview and not a.empty
        if labels is None:
            labels = [r["label"] for r in a.records] + ([self._next_label(a)] if drawn else [])
        labels = list(labels)
        for label in labels:
            if not (isinstance(label, (int, np.integer)) and 0 <= label <= MAX_LABEL):
                raise ValueError(f"AnnotationPool: label {label!r} is not an integer in 0 .. {MAX_LABEL}")
        if not labels:
            return {}
        source = a.labels
        if drawn:
            source = a.labels.clone()
            self.ops.compose([self._item(a, labels=source, label=self._next_label(a), mode=2)], self.prob_thresh, None)
        items = [(source, KIND_LABELS, 0.0, int(label)) for label in labels]
        got = self.ops_outlines.trace(items) if tolerance is None else self.ops_outlines.trace(items, tolerance)
        self._own_readbacks += 2 if tolerance is None else 3
        return {int(label): outline for label, outline in zip(labels, got)}

    def export(self, aid, polygons=False, tolerance=None):
        """The finished objects in COCO's form: the records of ``objects(aid)``, each with ``segmentation = dict(size=[H, W],
        counts=[...])``, the uncompressed run-length encoding of the pixels that hold its label now (an object that later
        ones have covered keeps its record; its counts are then ``[H * W]``).  ONE encode of the committed label map, without
        the object in progress: two read-backs.  With ``polygons`` each record also carries ``polygons``, the outer loops of
        those pixels in COCO's polygon form (``Outline.to_coco()``), and ``polygon_holes``, the number of hole loops that form
        leaves out, from ONE trace of the committed label map: two more read-backs.  With ``polygons`` and a ``tolerance`` in
        pixels the loops are simplified on the device (``Polygons.to_coco()``; three more read-backs instead of two),
        ``polygon_holes`` counts the hole loops that survive, and each record also carries ``polygon_tolerance``, the quantised
        tolerance, and ``polygon_dropped``, the loops that collapsed.  [] without touching the device when no object is
        finished."""
        a = self._ann(aid)
        if tolerance is not None:
            check_request(tolerance, [tuple(a.labels.shape)])
        if not a.records:
            return []
        rm, = self.ops_runs.encode([(a.labels, KIND_LABELS, 0.0)])
        self._own_readbacks += 2
        out = [dict(r, segmentation=rm.to_coco(r["label"])) for r in a.records]
        if polygons:
            outlines = self.label_outlines(aid, [r["label"] for r in a.records], preview=False, tolerance=tolerance)
            for e in out:
                e["polygons"] = outlines[e["label"]].to_coco()
                e["polygon_holes"] = int(outlines[e["label"]].holes().sum())
                if tolerance is not None:
                    e["polygon_tolerance"] = outlines[e["label"]].tolerance
                    e["polygon_dropped"] = outlines[e["label"]].dropped
        return out

    def load(self, aid, objects, keep_labels=False):
        """Finished objects into a fresh annotation -> their records.  ``objects``: a list of ``RunMap``s (a pixel set where
        ``v != 0``), COCO ``dict(size, counts)``s, or record dicts that carry ``segmentation`` (what ``export`` returns).  Labels
        are 1 .. K in list order; with ``keep_labels`` each record's own ``label`` (distinct, in 1 .. 65535), and
        ``object_count`` is then the largest.  Allowed only on an annotation as ``open`` left it.  For 0 <= prob_thresh < 1 the
        annotation is left exactly as by ``set_mask(aid, raster_k)``, ``finish(aid)`` for each object in turn: later objects
        overwrite earlier ones, an empty one still takes its label.  The objects are merged on the host from their runs
        (``runs.stack_objects``), 40 + 8 bytes per run of the merged map go up in one copy and ONE launch decodes them into the
        label map; nothing is read back.  Every ValueError is raised before anything is changed."""
        a = self._ann(aid)
        if a.records or a.object_count or not a.empty:
            raise ValueError(f"AnnotationPool.load: annotation {aid!r} already has objects or an object in progress")
        objects = list(objects)
        if len(objects) > MAX_LABEL:
            raise ValueError(f"AnnotationPool.load: {len(objects)} objects do not fit the 16-bit label map")
        maps, labels = [], []
        for k, obj in enumerate(objects):
            record = obj if isinstance(obj, dict) and "segmentation" in obj else None
            maps.append(self._run_map(a, record["segmentation"] if record is not None else obj))
            if not keep_labels:
                labels.append(k + 1)
                continue
            label = record.get("label") if record is not None else None
            if not (isinstance(label, (int, np.integer)) and 1 <= label <= MAX_LABEL) or int(label) in labels:
                raise ValueError(f"AnnotationPool.load: object {k} has no label of its own in 1 .. {MAX_LABEL}, or repeats one")
            labels.append(int(label))
        rm, records = stack_objects((a.H, a.W), maps, labels)
        self.ops_runs.decode([(rm, a.labels, KIND_LABELS, 0)])
        a.records, a.object_count = records, max(labels, default=0)
        a.start()
        self._reset_session(a)
        return [dict(r) for r in records]

    def objects(self, aid):
        return [dict(r) for r in self._ann(aid).records]

    def object_count(self, aid):
        return self._ann(aid).object_count

    def current_prob(self, aid):
        """R1's ``current``: fp32 [1, 1, H, W] on the device, a map of its own."""
        a = self._ann(aid)
        cur = a.total.clone() if a.total is not None else torch.zeros_like(a.zeros)
        if len(a.clicker):
            self.ops.compose([_Item(a.H, a.W, add=self._additive(a), total=cur, mode=1)], self.prob_thresh, None)
        return cur[None, None]
