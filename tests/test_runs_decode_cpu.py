"""CPU: run-length maps back into maps (isegm/inference/runs.py).  ``host_runs_decode``, ``RunMap.from_coco /
check / box`` and ``stack_objects`` against per-pixel loops at the shapes and patterns of runs_cases.py, and ``AnnotationPool.load``,
``set_mask`` and ``prev_masks`` in run-length form on the stub network with the host ops against twins driven with rasters.
Everything is integer or 0 / 1: equality is exact."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd import _lib
from pvpuformer_amd.isegm.inference import HostRunOps, RunMap, host_runs_decode, host_runs_encode, stack_objects
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import MAX_LABEL, AnnotationPool, _record
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool

from annotation_cases import box_of
from runs_cases import LABELS, PATTERNS, SHAPES, THR, case, decode_counts, pattern, shape_id, values_of
from sessions_cases import PRED_THR, StubNet, blob_image

SIZES = [(60, 80), (48, 48), (50, 70)]


@pytest.fixture(autouse=True)
def host_transforms(monkeypatch):
    """ZoomIn's two device calls on the host, as in test_annotation_cpu.py."""
    def mask_box(prob, thr, positive_clicks=()):
        m = (prob[0, 0] > thr).numpy().copy()
        count = int(m.sum())
        for r, c in positive_clicks:
            m[int(r), int(c)] = True
        rows, cols = np.nonzero(m)
        if len(rows) == 0:
            return 0, m.shape[0], -1, m.shape[1], -1
        return count, int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())

    monkeypatch.setattr(T._device, "resize_align_corners",
                        lambda x, size: F.interpolate(x.float(), size=tuple(int(s) for s in size), mode="bilinear",
                                                      align_corners=True))
    monkeypatch.setattr(T._device, "mask_box", mask_box)


def ellipse(H, W, cy, cx, ry, rx):
    rr, cc = np.mgrid[0:H, 0:W]
    return ((rr - cy) / ry) ** 2 + ((cc - cx) / rx) ** 2 <= 1.0


def runs_of(mask):
    """The binary RunMap of a bool raster."""
    return host_runs_encode(np.ascontiguousarray(mask).astype(np.uint16), 1)


# ------------------------------------------------------------------------------------------------------------- the type
@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_decode_inverts_encode(shape, kind):
    H, W = shape
    for name in PATTERNS:
        src = case(kind, name, H, W)
        v = values_of(src, kind)
        rm = host_runs_encode(src, kind, THR)
        assert rm.check() is rm
        labels = host_runs_decode(rm, 1)
        assert labels.dtype == np.uint16 and labels.shape == (H, W) and np.array_equal(labels, v), (shape, kind, name)
        for label in (1, 0, 2, 65535, 7):                                   # 7 never occurs
            got = host_runs_decode(rm, 0, label)
            assert got.dtype == np.float32 and got.shape == (H, W), (shape, kind, name)
            assert np.array_equal(got, (v == label).astype(np.float32)), (shape, kind, name, label)
            assert rm.box(label) == box_of(v == label), (shape, kind, name, label)
        assert not host_runs_decode(rm, 0, 7).any()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_from_coco_inverts_to_coco(shape):
    H, W = shape
    for name in PATTERNS:
        v = LABELS[pattern(name, H, W)]
        rm = host_runs_encode(v, 1)
        for label in (1, 2, 65535, 7):
            seg = rm.to_coco(label)
            back = RunMap.from_coco(seg, label)
            back.check()
            assert back.size == (H, W) and back.starts.dtype == np.int32 and back.values.dtype == np.int32
            assert np.array_equal(back.decode() == label, decode_counts(seg)), (shape, name, label)
            assert set(back.values.tolist()) <= {0, label} and (np.diff(back.values) != 0).all(), (shape, name, label)
            assert back.counts(label) == seg["counts"], (shape, name, label)
        assert RunMap.from_coco(rm.to_coco(7), 7).values.tolist() == [0]    # absent: counts == [H * W]


def test_from_coco_first_pixel_set_interior_zero_and_absent():
    rm = RunMap.from_coco(dict(size=[3, 4], counts=[0, 5, 7]))             # the first stream pixel is set
    assert rm.starts.tolist() == [0, 5] and rm.values.tolist() == [1, 0]
    assert np.array_equal(rm.decode() == 1, decode_counts(dict(size=[3, 4], counts=[0, 5, 7])))
    seg = dict(size=[3, 4], counts=[2, 3, 0, 4, 0, 0, 3])                  # interior zero counts: 2 clear, 3 + 4 set, 3 clear
    rm = RunMap.from_coco(seg, label=9)
    assert rm.starts.tolist() == [0, 2, 9] and rm.values.tolist() == [0, 9, 0]  # the set runs of 3 and 4 are one run of 7
    assert np.array_equal(rm.decode() == 9, decode_counts(seg))
    seg = dict(size=[3, 4], counts=[2, 0, 3, 7])                           # a zero SET count: the clear runs around it merge
    rm = RunMap.from_coco(seg)
    assert rm.starts.tolist() == [0, 5] and rm.values.tolist() == [0, 1]
    assert np.array_equal(rm.decode() == 1, decode_counts(seg))
    rm = RunMap.from_coco(dict(size=[3, 4], counts=[12]))
    assert rm.starts.tolist() == [0] and rm.values.tolist() == [0] and rm.box() == (3, -1, 4, -1)
    rm = RunMap.from_coco(dict(size=[3, 4], counts=[0, 12]), label=65535)
    assert rm.starts.tolist() == [0] and rm.values.tolist() == [65535]
    assert RunMap.from_coco(dict(size=(3, 4), counts=np.array([5, 7]))).starts.tolist() == [0, 5]


def test_from_coco_refuses_bad_counts():
    for counts in ([5, 6], [5, 8], [], [13, -1], [-1, 13], [5.0, 7.0], [5, 7.5], [[5, 7]]):
        with pytest.raises(ValueError):
            RunMap.from_coco(dict(size=[3, 4], counts=counts))
    for counts in ("52203", b"52203"):
        with pytest.raises(TypeError):
            RunMap.from_coco(dict(size=[3, 4], counts=counts))
    for label in (0, 65536, -1, 1.0):
        with pytest.raises(ValueError):
            RunMap.from_coco(dict(size=[3, 4], counts=[5, 7]), label=label)
    with pytest.raises(ValueError):
        RunMap.from_coco(dict(size=[0, 4], counts=[]))


def test_check_refuses_malformed_streams():
    good = lambda: RunMap((3, 4), [0, 5, 9], [0, 1, 65535])    # noqa: E731
    assert good().check().starts.tolist() == [0, 5, 9]
    bad = []
    rm = good(); rm.starts[0] = 1; bad.append(rm)                          # noqa: E702  does not begin at 0
    rm = good(); rm.starts[2] = 5; bad.append(rm)                          # noqa: E702  a repeated start
    rm = good(); rm.starts[1] = 10; bad.append(rm)                         # noqa: E702  a decreasing start
    rm = good(); rm.starts[2] = 12; bad.append(rm)                         # noqa: E702  the last start at H * W
    rm = good(); rm.values[1] = -1; bad.append(rm)                         # noqa: E702
    rm = good(); rm.values[2] = 65536; bad.append(rm)                      # noqa: E702
    rm = good(); rm.size = (0, 4); bad.append(rm)                          # noqa: E702
    rm = good(); rm.values = rm.values[:2]; bad.append(rm)                 # noqa: E702
    for rm in bad:
        with pytest.raises(ValueError):
            rm.check()
        dst = torch.zeros(3, 4, dtype=torch.int16)
        with pytest.raises(ValueError):                                     # every decode entry point checks
            HostRunOps().decode([(rm, dst, 1, 0)])
        assert not dst.any()


def test_box_of_a_run_across_a_column_boundary():
    H, W = 5, 4
    v = np.zeros((H, W), dtype=np.uint16)
    v[3:, 1] = 2
    v[:2, 2] = 2                                                            # ONE run: rows 3, 4 of column 1, rows 0, 1 of column 2
    rm = host_runs_encode(v, 1)
    assert len(rm) == 3 and rm.box(2) == (0, 4, 1, 2) == box_of(v == 2)
    assert rm.box(0) == (0, 4, 0, 3) and rm.box(1) == (H, -1, W, -1)
    v[2, 3] = 1
    rm = host_runs_encode(v, 1)
    assert rm.box(1) == (2, 2, 3, 3)
    want = [H, -1, W, -1]
    for i in range(H * W):                                                  # the per-pixel loop
        r, c = i % H, i // H
        if v[r, c] == 2:
            want = [min(want[0], r), max(want[1], r), min(want[2], c), max(want[3], c)]
    assert rm.box(2) == tuple(want)


# ------------------------------------------------------------------------------------------------------------- the merge
def paint(size, masks, labels):
    """The per-pixel paint loop: (label map uint16, records by annotation._record)."""
    H, W = size
    out = np.zeros((H, W), dtype=np.uint16)
    records = []
    for mask, label in zip(masks, labels):
        over = 0
        for r in range(H):
            for c in range(W):
                if mask[r, c]:
                    over += int(out[r, c] != 0 and out[r, c] != label)
                    out[r, c] = label
        rec = _record(mask, over)
        records.append(dict(label=label, area=int(rec[0]), box=tuple(int(x) for x in rec[2:6]), overwritten=int(rec[1])))
    return out, records


def object_masks(H, W):
    """Overlapping ellipses, an object that a later one covers fully, an empty one, one that touches the first and last pixel."""
    corners = np.zeros((H, W), dtype=bool)
    corners[0, 0] = corners[H - 1, W - 1] = True
    corners[H - 1, 0] = W > 1
    return [ellipse(H, W, 0.4 * H, 0.4 * W, 0.3 * H, 0.25 * W), ellipse(H, W, 0.55 * H, 0.6 * W, 0.3 * H, 0.3 * W),
            ellipse(H, W, 0.3 * H, 0.3 * W, 0.1 * H, 0.1 * W),               # inside the next
            ellipse(H, W, 0.3 * H, 0.3 * W, 0.2 * H, 0.2 * W), np.zeros((H, W), dtype=bool), corners]


@pytest.mark.parametrize("shape", [(40, 52), (33, 130), (70, 1), (1, 70), (1, 1), (7, 5)], ids=shape_id)
def test_stack_objects_equals_the_paint_loop(shape):
    H, W = shape
    masks = object_masks(H, W)
    for labels in (None, [7, 65535, 3, 1, 2, 40000]):
        want, records = paint(shape, masks, labels or list(range(1, len(masks) + 1)))
        given = [runs_of(m) if k % 2 == 0 else runs_of(m).to_coco() for k, m in enumerate(masks)]
        rm, got = stack_objects(shape, given, labels)
        rm.check()
        assert rm.size == shape and np.array_equal(rm.decode(), want), (shape, labels)
        assert (np.diff(rm.values) != 0).all(), (shape, labels)            # neighbouring runs differ: the form the encoder gives
        assert got == records, (shape, labels)
        assert host_runs_encode(want, 1).starts.tolist() == rm.starts.tolist()
    if min(H, W) >= 30:                                                     # (the last turn: the custom labels)
        assert records[2]["area"] > 0 and records[4] == dict(label=2, area=0, box=(H, -1, W, -1), overwritten=0)


def test_stack_objects_edges():
    rm, records = stack_objects((5, 7), [])
    assert rm.size == (5, 7) and rm.starts.tolist() == [0] and rm.values.tolist() == [0] and records == []
    # a map counts where v != 0, whatever the value
    v = np.zeros((5, 7), dtype=np.uint16)
    v[1:3, 2:5] = 9
    rm, records = stack_objects((5, 7), [host_runs_encode(v, 1)], [4])
    assert np.array_equal(rm.decode(), np.where(v != 0, 4, 0)) and records[0]["area"] == 6 and records[0]["box"] == (1, 2, 2, 4)
    one = runs_of(np.ones((5, 7), dtype=bool))
    with pytest.raises(ValueError):
        stack_objects((5, 8), [one])
    with pytest.raises(ValueError):
        stack_objects((5, 7), [one], [1, 2])
    for label in (0, 65536, 1.5):
        with pytest.raises(ValueError):
            stack_objects((5, 7), [one], [label])
    with pytest.raises(TypeError):
        stack_objects((5, 7), [dict(size=[5, 7], counts="abc")])


def test_unrun_descriptor_is_40_bytes():
    assert ctypes.sizeof(_lib.UnrunObj) == 40
    assert [name for name, _ in _lib.UnrunObj._fields_] == ["dst", "entries", "H", "W", "n_runs", "kind", "label", "pad"]
    assert _lib.UnrunObj.entries.offset == 8 and _lib.UnrunObj.H.offset == 16 and _lib.UnrunObj.label.offset == 32
    assert _lib.SIGNATURES["vpu_runs_decode_batched"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]


def test_host_ops_decode_in_place():
    labels = case(1, "random", 33, 130)
    rm = host_runs_encode(labels, 1)
    a, b = torch.full((33, 130), 5, dtype=torch.int16), torch.full((33, 130), 5.0)
    assert HostRunOps().decode([(rm, a, 1, 0), (rm, b, 0, 65535)]) is None
    assert np.array_equal(a.numpy().view(np.uint16), labels) and np.array_equal(b.numpy(), (labels == 65535).astype(np.float32))
    HostRunOps().decode([])


# ------------------------------------------------------------------------------------------------------------- the pools
def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


def _images():
    return [blob_image(H, W, seed=j) for j, (H, W) in enumerate(SIZES)]


def same_annotation(a, b, aid, where):
    for preview in (True, False):
        assert np.array_equal(a.label_map(aid, preview), b.label_map(aid, preview)), (where, aid, preview)
    assert a.objects(aid) == b.objects(aid) and a.object_count(aid) == b.object_count(aid), (where, aid)
    assert np.array_equal(a.current_prob(aid).numpy(), b.current_prob(aid).numpy()), (where, aid)


def go_on(pools, aid, centre, where):
    """reopen, click and finish on both pools after a load: the two stay alike."""
    a, b = pools
    label = a.objects(aid)[-1]["label"]
    for p in pools:
        p.reopen(aid, label)
    same_annotation(a, b, aid, where + ": reopen")
    masks = [p.click({aid: (True, centre)})[aid] for p in pools]
    assert np.array_equal(masks[0], masks[1]), where
    same_annotation(a, b, aid, where + ": click")
    records = [p.finish(aid) for p in pools]
    assert records[0] == records[1] and records[0]["label"] == a.object_count(aid), where
    same_annotation(a, b, aid, where + ": finish")
    assert a.export(aid) == b.export(aid), where


@pytest.mark.parametrize("thr", [0.5, 0.0, 0.99])
@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_load_equals_set_mask_and_finish(zoom, thr):
    a, b = (AnnotationPool(_make(zoom)(), max_images=3, prob_thresh=thr) for _ in range(2))
    for image, centre in _images():
        H, W = image.shape[:2]
        masks = object_masks(H, W)
        aid = a.open(image)
        assert b.open(image) == aid
        for m in masks:
            b.set_mask(aid, m)
            assert b.finish(aid) is not None
        given = [runs_of(m) if k % 3 == 0 else runs_of(m).to_coco() if k % 3 == 1 else dict(label=99, segmentation=runs_of(m).to_coco())
                 for k, m in enumerate(masks)]
        before = a.readbacks
        got = a.load(aid, given)
        assert a.readbacks == before                                       # nothing comes back
        assert got == a.objects(aid) == b.objects(aid) and [r["label"] for r in got] == list(range(1, len(masks) + 1))
        assert got[4] == dict(label=5, area=0, box=(H, -1, W, -1), overwritten=0)      # the empty one took its label
        got[0]["area"] = -1
        assert a.objects(aid)[0]["area"] >= 0                               # the returned records are copies
        same_annotation(a, b, aid, "load")
        with pytest.raises(ValueError):
            a.load(aid, given)                                              # not as open left it
        same_annotation(a, b, aid, "second load refused")
        go_on((a, b), aid, centre, "after load")


def test_export_then_load_round_trip():
    """A script with an overlap, a fully covered object and a reopen; then export -> load on fresh annotations."""
    src = AnnotationPool(_make(False)(), max_images=3)
    kept, fresh = (AnnotationPool(_make(False)(), max_images=3) for _ in range(2))
    for image, centre in _images():
        H, W = image.shape[:2]
        masks = object_masks(H, W)
        aid = src.open(image)
        for m in masks[:4]:                                                 # 1 and 2 overlap, 3 is covered by 4
            src.set_mask(aid, m)
            src.finish(aid)
        src.reopen(aid, 2)
        src.click({aid: (True, centre)})
        src.finish(aid)                                                     # label 5; label 2 is gone
        out = src.export(aid)
        assert [e["label"] for e in out] == [1, 3, 4, 5] and out[1]["segmentation"]["counts"] == [H * W]
        committed = src.label_map(aid, False)

        k = kept.open(image)
        before = kept.readbacks
        records = kept.load(k, out, keep_labels=True)
        assert kept.readbacks == before
        assert np.array_equal(kept.label_map(k, False), committed) and np.array_equal(kept.label_map(k, True), committed)
        assert [r["label"] for r in records] == [1, 3, 4, 5] and kept.object_count(k) == 5
        # what is exported is what is visible now: areas are the visible pixels, nothing is overwritten among them
        assert [r["area"] for r in records] == [int((committed == e["label"]).sum()) for e in out]
        assert all(r["overwritten"] == 0 for r in records)
        assert [e["segmentation"] for e in kept.export(k)] == [e["segmentation"] for e in out]

        f = fresh.open(image)
        records = fresh.load(f, out)
        renumbered = np.zeros_like(committed)
        for new, e in enumerate(out, start=1):
            renumbered[committed == e["label"]] = new
        assert np.array_equal(fresh.label_map(f, False), renumbered) and fresh.object_count(f) == 4
        assert [r["label"] for r in records] == [1, 2, 3, 4]

        # both go on working: the next label follows object_count, reopen finds the loaded labels
        for pool, i, last in ((kept, k, 5), (fresh, f, 4)):
            pool.reopen(i, last)
            assert not (pool.label_map(i, False) == last).any()
            pool.click({i: (True, centre)})
            assert pool.finish(i)["label"] == last + 1
            with pytest.raises(KeyError):
                pool.reopen(i, last)


def test_load_refusals_change_nothing():
    ann = AnnotationPool(_make(False)(), max_images=2)
    image, centre = blob_image(48, 56, seed=0)
    H, W = image.shape[:2]
    aid = ann.open(image)
    good = runs_of(ellipse(H, W, 20, 20, 8, 9))
    rec = lambda label: dict(label=label, segmentation=good.to_coco())      # noqa: E731
    broken = RunMap((H, W), [0, 9, 9], [0, 1, 0])

    def untouched():
        assert not ann.label_map(aid).any() and ann.objects(aid) == [] and ann.object_count(aid) == 0

    for objects, kw in (([runs_of(np.ones((H, W + 1), dtype=bool))], {}), ([good, dict(size=[H + 1, W], counts=[(H + 1) * W])], {}),
                        ([good, dict(size=[H, W], counts=[5])], {}), ([good, dict(size=[H, W], counts=[-1, H * W + 1])], {}),
                        ([good, broken], {}), ([good] * (MAX_LABEL + 1), {}),
                        ([good], dict(keep_labels=True)),                   # a bare map has no label of its own
                        ([rec(3), rec(3)], dict(keep_labels=True)), ([rec(0)], dict(keep_labels=True)),
                        ([rec(65536)], dict(keep_labels=True)), ([rec(2.0)], dict(keep_labels=True))):
        with pytest.raises(ValueError):
            ann.load(aid, objects, **kw)
        untouched()
    with pytest.raises(TypeError):
        ann.load(aid, [good, dict(size=[H, W], counts="abc")])
    untouched()
    with pytest.raises(KeyError):
        ann.load(aid + 1, [good])
    assert ann.load(aid, []) == [] and ann.object_count(aid) == 0           # nothing loaded: still as open left it
    ann.click({aid: (True, centre)})
    with pytest.raises(ValueError):
        ann.load(aid, [good])                                               # an object in progress
    assert ann.objects(aid) == [] and not ann.label_map(aid, False).any() and ann.label_map(aid, True).any()
    ann.finish(aid)
    before = ann.label_map(aid)
    with pytest.raises(ValueError):
        ann.load(aid, [good])
    assert np.array_equal(ann.label_map(aid), before) and len(ann.objects(aid)) == 1
    # keep_labels: object_count is the largest label, 65535 fits and leaves no room for a further object
    other = ann.open(image)
    assert [r["label"] for r in ann.load(other, [rec(65535), rec(7)], keep_labels=True)] == [65535, 7]
    assert ann.object_count(other) == 65535 and set(np.unique(ann.label_map(other))) == {0, 7}
    ann.set_mask(other, good)
    with pytest.raises(ValueError):
        ann.finish(other)


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_set_mask_in_run_length_form_equals_the_raster(zoom):
    a, b = (AnnotationPool(_make(zoom)(), max_images=3) for _ in range(2))
    for image, centre in _images():
        H, W = image.shape[:2]
        v = np.zeros((H, W), dtype=np.uint16)
        v[ellipse(H, W, 0.3 * H, 0.3 * W, 0.15 * H, 0.2 * W)] = 1
        v[ellipse(H, W, 0.7 * H, 0.6 * W, 0.15 * H, 0.2 * W)] = 65535
        rm = host_runs_encode(v, 1)
        aid = a.open(image)
        assert b.open(image) == aid
        for given, label, kw in ((rm, 65535, dict(label=65535)), (rm, 1, {}), (rm.to_coco(65535), 65535, dict(label=65535)),
                                 (rm.to_coco(1), 1, {}), (rm, 7, dict(label=7)), (rm, 0, dict(label=0))):
            before = a.readbacks
            a.set_mask(aid, given, **kw)
            assert a.readbacks == before
            b.set_mask(aid, v == label)
            same_annotation(a, b, aid, ("set_mask", label))
            masks = [p.click({aid: (True, centre)})[aid] for p in (a, b)]   # the mask is the network's previous mask
            assert np.array_equal(masks[0], masks[1]), label
            same_annotation(a, b, aid, ("click", label))
        for p in (a, b):
            p.finish(aid)
        same_annotation(a, b, aid, "finish")
        before = a.label_map(aid)
        for bad, kw in ((runs_of(np.ones((H, W + 1), dtype=bool)), {}), (dict(size=[H + 1, W], counts=[(H + 1) * W]), {}),
                        (dict(size=[H, W], counts=[3]), {}), (rm, dict(label=-1)), (rm, dict(label=65536)),
                        (rm.to_coco(1), dict(label=0)), (RunMap((H, W), [0, 9, 9], [0, 1, 0]), {})):
            a.click({aid: (True, centre)})
            held = a.label_map(aid)
            with pytest.raises(ValueError):
                a.set_mask(aid, bad, **kw)
            assert np.array_equal(a.label_map(aid), held) and held.any()    # the object in progress is still there
            a.undo(aid)
        assert np.array_equal(a.label_map(aid), before)
        a.set_mask(aid, v == 1, 5)                                           # arrays as before: the label is not read
        b.set_mask(aid, v == 1)
        same_annotation(a, b, aid, "array")


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_prev_masks_in_run_length_form_equal_the_raster(zoom):
    a, b = (SessionPool(_make(zoom)(), max_sessions=3, pred_thr=PRED_THR) for _ in range(2))
    images = _images()
    sids = [a.open(image) for image, _ in images]
    assert [b.open(image) for image, _ in images] == sids
    clicks, rasters, given = {}, {}, {}
    for j, (sid, (image, (r, c))) in enumerate(zip(sids, images)):
        H, W = image.shape[:2]
        clicks[sid] = Clicker(device=None)
        clicks[sid].add_click(Click(True, (r, c)))
        v = np.zeros((H, W), dtype=np.uint16)
        v[ellipse(H, W, r, c, 0.2 * H, 0.15 * W)] = 1
        v[:3] = 2                                                           # other values are not the mask
        rasters[sid] = (v == 1).astype(np.float32)
        rm = host_runs_encode(v, 1)
        given[sid] = rm if j % 2 == 0 else rm.to_coco(1)
    for step in range(2):
        before = a.readbacks, b.readbacks
        got, want = a.predict(clicks, prev_masks=given), b.predict(clicks, prev_masks=rasters)
        assert a.readbacks - before[0] == b.readbacks - before[1]
        for sid in sids:
            assert np.array_equal(got[sid], want[sid]), (step, sid)
            assert np.array_equal(a.probs(sid).numpy(), b.probs(sid).numpy()), (step, sid)
            clicks[sid].add_click(Click(False, (2, 3)))
    with pytest.raises(AssertionError, match="another size"):
        a.predict({sids[0]: clicks[sids[0]]}, prev_masks={sids[0]: given[sids[1]]})
    with pytest.raises(AssertionError, match="another size"):
        b.predict({sids[0]: clicks[sids[0]]}, prev_masks={sids[0]: rasters[sids[1]]})
