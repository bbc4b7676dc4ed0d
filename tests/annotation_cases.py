"""Shared by test_annotation_cpu.py and test_annotation_gpu.py: the annotation rules R1-R8 restated over
one private ``BasePredictor`` + ``Clicker`` per image with numpy arrays (``TwinPool``, which has ``AnnotationPool``'s
methods), the script both files drive, and the comparison of two pools after every call."""
import numpy as np
import torch

from pvpuformer_amd.isegm.inference.clicker import Click, Clicker


THR = 0.5


def compose_case(H, W, seed, empty=False):
    """(add, total fp32 [H, W], labels uint16 [H, W]): values on both sides of THR and some exactly at it; labels 0, 7 and 65535."""
    rs = np.random.RandomState(seed)
    add, total = rs.rand(H, W).astype(np.float32), rs.rand(H, W).astype(np.float32)
    if empty:
        add, total = add * np.float32(0.5), total * np.float32(0.5)         # all <= THR
    at = rs.rand(H, W) < 0.2
    add[at] = np.float32(THR)
    total[at] = np.minimum(total[at], np.float32(THR))                      # max == THR exactly: not in the mask
    labels = rs.choice(np.array([0, 7, 65535], dtype=np.uint16), size=(H, W))
    return add, total, labels


def rect_mask(H, W):
    """A bool mask in the top-left corner of the image, away from the blob in its centre."""
    mask = np.zeros((H, W), dtype=bool)
    mask[2:max(4, H // 4), 1:max(4, W // 3)] = True
    return mask


def box_of(mask):
    rows, cols = np.nonzero(mask)
    if len(rows) == 0:
        return (mask.shape[0], -1, mask.shape[1], -1)
    return (int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max()))


class TwinAnnotation:
    """One image by the rules, in host numpy."""

    def __init__(self, make, image, thr, max_undo):
        self.make, self.image, self.thr, self.max_undo = make, image, np.float32(thr), max_undo
        self.H, self.W = image.shape[:2]
        self.labels = np.zeros((self.H, self.W), dtype=np.uint16)
        self.count, self.records = 0, []
        self.start()

    def start(self):
        self.pred = self.make()
        self.pred.set_input_image(self.image)
        self.clicker = Clicker(device=None)
        self.parts, self.has_parts, self.mask, self.stack = np.zeros((self.H, self.W), dtype=np.float32), False, None, []

    def reset_predictor(self):
        self.pred = self.make()
        self.pred.set_input_image(self.image)

    @property
    def empty(self):
        return len(self.clicker) == 0 and not self.has_parts and self.mask is None

    def current(self):                                                          # R1 (and R7: the mask stands in for the parts)
        total = self.mask if self.mask is not None else self.parts
        add = self.pred.prev_prediction[0, 0].cpu().numpy() if len(self.clicker) else np.zeros_like(total)
        return np.maximum(total, add)

    def snapshot(self):
        self.stack.append((self.clicker.get_state(), self.pred.get_states(), self.parts.copy(), self.has_parts, self.mask))
        del self.stack[:max(0, len(self.stack) - self.max_undo)]

    def click(self, positive, coords):                                          # R3
        self.snapshot()
        self.clicker.add_click(Click(bool(positive), (int(coords[0]), int(coords[1]))))
        prev = None if self.mask is None else torch.from_numpy(self.mask)[None, None].to(self.pred.device)
        self.pred.get_prediction(self.clicker, prev_mask=prev)
        if self.mask is not None and len(self.clicker) == 1:
            self.pred.get_prediction(self.clicker, prev_mask=prev)
        return self.current() > self.thr

    def undo(self):                                                             # R6
        if not self.stack:
            return None
        clicks, states, self.parts, self.has_parts, self.mask = self.stack.pop()
        self.clicker.click_indx_offset = 1 if self.mask is not None else 0
        self.clicker.set_state(clicks)
        self.pred.set_states(states)
        return self.current() > self.thr

    def partially_finish(self):                                                 # R4
        if self.empty:
            return
        self.snapshot()
        self.parts, self.has_parts, self.mask = self.current(), True, None
        self.clicker.reset_clicks()
        self.clicker.click_indx_offset = 0
        self.reset_predictor()

    def finish(self):                                                           # R5
        if self.empty:
            return None
        label = self.count + 1
        if label > 65535:
            raise ValueError("label")
        m = self.current() > self.thr
        record = dict(label=label, area=int(m.sum()), box=box_of(m),
                      overwritten=int((m & (self.labels != 0) & (self.labels != label)).sum()))
        self.labels[m] = label
        self.count = label
        self.records.append(record)
        self.start()
        return dict(record)

    def set_mask(self, mask):                                                   # R7
        if tuple(np.shape(mask)) != (self.H, self.W):
            raise ValueError("size")
        self.start()
        self.mask = np.asarray(mask).astype(np.float32)
        self.clicker.click_indx_offset = 1

    def reopen(self, label):                                                    # R8
        at = self.labels == label
        if not any(r["label"] == label for r in self.records) or not at.any():
            raise KeyError(label)
        self.labels[at] = 0
        self.records = [r for r in self.records if r["label"] != label]
        self.start()
        self.mask = at.astype(np.float32)
        self.clicker.click_indx_offset = 1

    def label_map(self, preview):                                               # R2
        out = self.labels.copy()
        if preview and not self.empty:
            out[self.current() > self.thr] = self.count + 1
        return out


class TwinPool:
    """``AnnotationPool``'s methods over ``TwinAnnotation``s; ``make`` builds a private predictor."""

    def __init__(self, make, prob_thresh=0.5, max_undo=32):
        self.make, self.thr, self.max_undo, self.held = make, prob_thresh, max_undo, []

    def open(self, image):
        self.held.append(TwinAnnotation(self.make, image, self.thr, self.max_undo))
        return len(self.held) - 1

    def click(self, clicks):
        return {aid: self.held[aid].click(*c) for aid, c in clicks.items()}

    def undo(self, aid):
        return self.held[aid].undo()

    def partially_finish(self, aid):
        self.held[aid].partially_finish()

    def finish(self, aid):
        return self.held[aid].finish()

    def set_mask(self, aid, mask):
        self.held[aid].set_mask(mask)

    def reopen(self, aid, label):
        self.held[aid].reopen(label)

    def label_map(self, aid, preview=True):
        return self.held[aid].label_map(preview)

    def objects(self, aid):
        return [dict(r) for r in self.held[aid].records]

    def object_count(self, aid):
        return self.held[aid].count

    def current_prob(self, aid):
        return torch.from_numpy(self.held[aid].current())[None, None]


def assert_same(a, b, aids, where):
    """Everything two pools show of ``aids``, bit for bit."""
    for aid in aids:
        pa, pb = a.current_prob(aid), b.current_prob(aid)
        assert pa.dtype == torch.float32 and tuple(pa.shape) == tuple(pb.shape) and pa.dim() == 4, (where, aid)
        assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy()), (where, aid, "current_prob")
        for preview in (True, False):
            la, lb = a.label_map(aid, preview=preview), b.label_map(aid, preview=preview)
            assert la.dtype == np.uint16 and la.shape == lb.shape and np.array_equal(la, lb), (where, aid, "label_map", preview)
        assert a.objects(aid) == b.objects(aid), (where, aid, a.objects(aid), b.objects(aid))
        assert a.object_count(aid) == b.object_count(aid), (where, aid)


def run_script(a, b, images, finite=False):
    """The script of the tests on every image at once, on pools ``a`` and ``b`` side by side (``b`` None: ``a`` alone); after
    every call the two are compared.  ``images``: [(image, (row, col) of its object)].  -> the log [(where, {aid: mask})] of
    ``a``'s returned masks."""
    pools = [p for p in (a, b) if p is not None]
    aids = None
    for p in pools:
        got = [p.open(image) for image, _ in images]
        assert aids is None or got == aids
        aids = got
    shape = {aid: image.shape[:2] for aid, (image, _) in zip(aids, images)}
    centre = {aid: c for aid, (_, c) in zip(aids, images)}
    log = []

    def at(aid, dr, dc):
        H, W = shape[aid]
        return (int(np.clip(centre[aid][0] + dr, 0, H - 1)), int(np.clip(centre[aid][1] + dc, 0, W - 1)))

    def check(where, results):
        if results is not None:
            ra = results[0]
            for aid in aids:
                if isinstance(ra, dict) and ra.get(aid) is not None and isinstance(ra[aid], np.ndarray):
                    assert ra[aid].dtype == np.bool_ and ra[aid].shape == tuple(shape[aid]), (where, aid)
            if len(results) == 2:
                rb = results[1]
                assert sorted(ra) == sorted(rb), where
                for aid in ra:
                    if isinstance(ra[aid], np.ndarray):
                        assert np.array_equal(ra[aid], rb[aid]), (where, aid, "returned mask")
                    else:
                        assert ra[aid] == rb[aid], (where, aid, ra[aid], rb[aid])
            log.append((where, ra))
        if len(pools) == 2:
            assert_same(a, b, aids, where)
        if finite:
            for aid in aids:
                assert torch.isfinite(a.current_prob(aid)).all(), (where, aid)

    def click(where, positive, dr, dc, absolute=False):
        clicks = {aid: (positive, (dr, dc) if absolute else at(aid, dr, dc)) for aid in aids}
        check(where, [p.click(clicks) for p in pools])

    def each(where, name, *args):
        held = None
        if finite and name == "finish":     # R5 on a's own maps: the labels written are those of its current_prob > prob_thresh
            held = {aid: (a.current_prob(aid)[0, 0].cpu().numpy() > np.float32(a.prob_thresh), a.label_map(aid, preview=False),
                          a.label_map(aid, preview=True), a.object_count(aid)) for aid in aids}
        check(where, [{aid: getattr(p, name)(aid, *args) for aid in aids} for p in pools])
        for aid, (mask, before, preview, count) in (held or {}).items():
            want = np.where(mask, np.uint16(count + 1), before)
            assert np.array_equal(preview, want) and np.array_equal(a.label_map(aid, preview=False), want), (where, aid)
            assert a.objects(aid)[-1]["area"] == int(mask.sum()) and a.object_count(aid) == count + 1, (where, aid)

    check("open", None)
    click("click 1", True, 0, 0)
    click("click 2 (background)", True, -int(0.4 * min(s[0] for s in shape.values())), 3)
    each("partial finish", "partially_finish")
    click("click 3 (negative)", False, 3, 5, absolute=True)
    click("click 4", True, 8, 6)
    each("undo", "undo")
    click("click 4 again", True, -6, 7)
    each("finish 1", "finish")
    click("second object", True, 3, 2)
    each("finish 2", "finish")
    for p in pools:
        for aid in aids:
            p.set_mask(aid, rect_mask(*shape[aid]))
    check("set_mask", None)
    click("click on the mask (predicted twice)", True, 1, -2)
    each("finish 3", "finish")
    # reopen label 1; where object 2 has covered all of it, both pools refuse alike and label 3 (the newest, whole) is reopened
    reopened = {}
    for aid in aids:
        outcome = []
        for p in pools:
            try:
                p.reopen(aid, 1)
                outcome.append(1)
            except KeyError:
                p.reopen(aid, 3)
                outcome.append(3)
        assert len(set(outcome)) == 1, (aid, outcome)
        reopened[aid] = outcome[0]
    check("reopen", None)
    click("click on the reopened object", True, 10, -9)
    each("finish 4", "finish")
    return log, reopened
