"""CPU: ``AnnotationPool`` (isegm/inference/annotation.py) with the stub network and the host stand-ins of its two kernels.
The stand-ins against the rules written out per pixel, the pool against a twin of private predictors and numpy arrays
(annotation_cases.TwinPool) after every call of the script, its synchronisation counts, its errors, and the isolation of
the annotations from one another.  Everything is max, a strict compare and integer writes: equality is bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import (AnnotationPool, HostAnnotOps, host_annot_compose,
                                                       host_label_extract)
from pvpuformer_amd.isegm.inference.clicker import Click
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import n_words

from annotation_cases import THR, TwinPool, assert_same, compose_case, rect_mask, run_script
from sessions_cases import StubNet, blob_image

SHAPES = [(1, 1), (3, 5), (8, 8), (5, 13), (17, 15), (16, 16), (47, 70)]


def _host_mask_box(prob, thr, positive_clicks=()):
    m = (prob[0, 0] > thr).numpy().copy()
    count = int(m.sum())
    for r, c in positive_clicks:
        m[int(r), int(c)] = True
    rows, cols = np.nonzero(m)
    if len(rows) == 0:
        return 0, m.shape[0], -1, m.shape[1], -1
    return count, int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())


@pytest.fixture(autouse=True)
def host_transforms(monkeypatch):
    """The private predictors' ZoomIn on the host (its two device calls replaced by torch / numpy)."""
    monkeypatch.setattr(T._device, "resize_align_corners",
                        lambda x, size: F.interpolate(x.float(), size=tuple(int(s) for s in size), mode="bilinear",
                                                      align_corners=True))
    monkeypatch.setattr(T._device, "mask_box", _host_mask_box)


# ------------------------------------------------------------------------------------------------------------- stand-ins
def rules(add, total, labels, H, W, label, mode, thr):
    """The compose rules per pixel in plain Python -> (cur, mask, words, rec, new total, new labels)."""
    cur, mask = np.zeros((H, W), np.float32), np.zeros((H, W), bool)
    words = [0] * n_words(H * W)
    area = over = 0
    box = [H, -1, W, -1]
    new_total = None if total is None else total.copy()
    new_labels = None if labels is None else labels.copy()
    for r in range(H):
        for c in range(W):
            t = np.float32(0) if total is None else total[r, c]
            a = np.float32(0) if add is None else add[r, c]
            cur[r, c] = t if t >= a else a
            if mode & 1 and total is not None:
                new_total[r, c] = cur[r, c]
            if not cur[r, c] > np.float32(thr):
                continue
            mask[r, c] = True
            i = r * W + c
            words[i >> 6] |= 1 << (i & 63)
            area += 1
            box = [min(box[0], r), max(box[1], r), min(box[2], c), max(box[3], c)]
            if labels is not None and labels[r, c] != 0 and labels[r, c] != label:
                over += 1
            if mode & 2 and labels is not None:
                new_labels[r, c] = label
    return cur, mask, np.array(words, dtype=np.uint64), np.array([area, over] + box + [0, 0], np.int32), new_total, new_labels


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stand_ins_follow_the_rules(shape):
    H, W = shape
    variants = [("both", False, False, False), ("no add", True, False, False), ("no total", False, True, False),
                ("no labels", False, False, True), ("empty", False, False, False)]
    for mode in range(4):
        for name, no_add, no_total, no_labels in variants:
            for label in (3, 65535):
                add, total, labels = compose_case(H, W, seed=H * 100 + W + mode, empty=name == "empty")
                add, total, labels = (None if no_add else add), (None if no_total else total), (None if no_labels else labels)
                want = rules(add, total, labels, H, W, label, mode, THR)
                words, rec = host_annot_compose(add, total, labels, H, W, label, mode, THR)
                where = (shape, mode, name, label)
                assert words.dtype == np.uint64 and np.array_equal(words, want[2]), where
                assert rec.dtype == np.int32 and np.array_equal(rec, want[3]), where
                assert total is None or np.array_equal(total, want[4]), where
                assert labels is None or np.array_equal(labels, want[5]), where
                if name == "empty":
                    assert rec.tolist() == [0, 0, H, -1, W, -1, 0, 0] and not words.any(), where
                elif name == "both":
                    at_thr = np.maximum(*compose_case(H, W, seed=H * 100 + W + mode)[:2]) == np.float32(THR)
                    assert not (want[1] & at_thr).any(), where             # the compare is strict
    # extract
    for label in (7, 65535, 9):
        labels = compose_case(H, W, seed=H + W)[2]
        before = labels.copy()
        out, rec = host_label_extract(labels, label)
        at = before == label
        assert out.dtype == np.float32 and np.array_equal(out, at.astype(np.float32)), (shape, label)
        assert np.array_equal(labels, np.where(at, 0, before)) and labels.dtype == np.uint16, (shape, label)
        rows, cols = np.nonzero(at)
        box = [rows.min(), rows.max(), cols.min(), cols.max()] if len(rows) else [H, -1, W, -1]
        assert rec.tolist() == [int(at.sum()), 0] + [int(v) for v in box] + [0, 0], (shape, label)


# ------------------------------------------------------------------------------------------------------------- the pool
SIZES = [(60, 80), (48, 48), (50, 70)]


def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


def _images(sizes=SIZES):
    return [blob_image(H, W, seed=j) for j, (H, W) in enumerate(sizes)]


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_pool_equals_the_twin_after_every_call(zoom):
    make = _make(zoom)
    ann = AnnotationPool(make(), max_images=3)
    assert isinstance(ann.ops, HostAnnotOps) and ann.prob_thresh == 0.5
    twin = TwinPool(make)
    log, reopened = run_script(ann, twin, _images())
    assert [w for w, _ in log].count("finish 4") == 1
    for aid in range(3):
        records = ann.objects(aid)
        assert ann.object_count(aid) == 4 and reopened[aid] == 1
        assert [r["label"] for r in records] == [2, 3, 4]                  # label 1 was reopened and became label 4
        assert records[0]["overwritten"] > 0                               # the second object lies over the first
        assert all(r["area"] > 0 and r["box"][0] <= r["box"][1] for r in records)
        final = ann.label_map(aid, preview=False)
        assert set(np.unique(final).tolist()) <= {0, 2, 3, 4} and (final == 4).any() and not (final == 1).any()
        assert np.array_equal(ann.label_map(aid, preview=True), final)      # no object in progress
        assert ann.undo(aid) is None and ann.finish(aid) is None            # an empty object
    masks = dict(log)
    for aid in range(3):
        before, after = masks["partial finish"], masks["click 4"][aid]
        assert before[aid] is None and after.any()
        assert not np.array_equal(masks["click 2 (background)"][aid], masks["click 1"][aid])


def test_initial_mask_shows_and_is_merged():
    """R7: the mask is in the preview before the first click, stays after it, and is part of the finished object."""
    make = _make(False)
    ann, twin = AnnotationPool(make(), max_images=1), TwinPool(make)
    image, centre = blob_image(48, 48, seed=1)
    aid = ann.open(image)
    assert twin.open(image) == aid
    mask = rect_mask(48, 48)
    ann.set_mask(aid, mask.astype(np.float32))
    twin.set_mask(aid, mask)
    assert_same(ann, twin, [aid], "set_mask")
    assert np.array_equal(ann.label_map(aid) == 1, mask) and not ann.label_map(aid, preview=False).any()
    forwards = ann.forwards
    got = ann.click({aid: Click(True, centre)})
    assert ann.forwards == forwards + 2                                     # the first click on a mask is predicted twice
    assert np.array_equal(got[aid], twin.click({aid: (True, centre)})[aid])
    assert (got[aid] & mask).sum() == mask.sum() and got[aid].sum() > mask.sum()
    got = ann.click({aid: (False, (40, 40))})
    assert ann.forwards == forwards + 3
    assert np.array_equal(got[aid], twin.click({aid: (False, (40, 40))})[aid])
    assert_same(ann, twin, [aid], "clicks on the mask")
    record = ann.finish(aid)
    assert record == twin.finish(aid) and record["label"] == 1 and record["area"] == int(got[aid].sum())
    assert (ann.label_map(aid)[mask] == 1).all()


def test_undo_stack_is_bounded():
    make = _make(False)
    ann, twin = AnnotationPool(make(), max_images=1, max_undo=2), TwinPool(make, max_undo=2)
    image, (r, c) = blob_image(48, 48, seed=2)
    aid = ann.open(image)
    twin.open(image)
    for k, where in enumerate([(r, c), (5, 6), (40, 9)]):
        for p in (ann, twin):
            p.click({aid: (k != 1, where)})
    for p in (ann, twin):
        p.partially_finish(aid)
    assert_same(ann, twin, [aid], "three clicks and a partial finish")
    for step in range(2):
        assert np.array_equal(ann.undo(aid), twin.undo(aid))
        assert_same(ann, twin, [aid], f"undo {step}")
    assert ann.undo(aid) is None and twin.undo(aid) is None                 # the oldest two snapshots were dropped
    assert ann.current_prob(aid).any()


def test_counters():
    ann = AnnotationPool(_make(False)(), max_images=2)
    (img_a, ca), (img_b, cb) = _images([(60, 80), (48, 48)])
    a, b = ann.open(img_a), ann.open(img_b)
    assert (ann.readbacks, ann.forwards) == (0, 0)
    ann.click({a: (True, ca), b: (True, cb)})
    assert (ann.readbacks, ann.pool.readbacks, ann.forwards) == (1, 1, 2)    # the pool's: one round, a forward per image size
    ann.partially_finish(a)
    assert (ann.readbacks, ann.forwards) == (1, 2)                          # no synchronisation
    ann.click({b: (True, (cb[0] + 3, cb[1]))})
    assert (ann.readbacks, ann.pool.readbacks) == (2, 2)                    # b has neither parts nor a mask
    ann.click({a: (True, (5, 5)), b: (False, (2, 2))})
    assert (ann.readbacks, ann.pool.readbacks, ann.forwards) == (4, 3, 5)    # one compose and read-back more, for a
    ann.partially_finish(b)
    ann.click({a: (True, (9, 70)), b: (True, (40, 40))})
    assert (ann.readbacks, ann.pool.readbacks) == (6, 4)                    # one for a and b together
    ann.current_prob(a)
    assert ann.readbacks == 6
    ann.label_map(a)
    ann.label_map(a, preview=False)
    assert ann.readbacks == 8                                               # one copy each
    assert ann.finish(a)["label"] == 1
    assert (ann.readbacks, ann.pool.readbacks, ann.forwards) == (9, 4, 7)
    ann.set_mask(a, rect_mask(60, 80))
    assert ann.readbacks == 9
    ann.click({a: (True, ca)})
    assert (ann.readbacks, ann.pool.readbacks, ann.forwards) == (12, 6, 9)   # predicted twice, composed once


def test_errors():
    ann = AnnotationPool(_make(False)(), max_images=2)
    (img_a, ca), (img_b, _) = _images([(60, 80), (48, 48)])
    a, b = ann.open(img_a), ann.open(img_b)
    with pytest.raises(ValueError):
        ann.open(img_a)                                                     # more images than max_images
    for call in (lambda: ann.click({7: (True, (1, 1))}), lambda: ann.finish(7), lambda: ann.undo("a"), lambda: ann.label_map(2),
                 lambda: ann.set_mask(5, np.zeros((4, 4))), lambda: ann.reopen(9, 1), lambda: ann.close(3)):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(ValueError):
        ann.set_mask(a, np.zeros((48, 48), dtype=bool))                     # b's size
    with pytest.raises(KeyError):
        ann.reopen(a, 1)                                                    # nothing committed yet
    ann.click({a: (True, ca)})
    before = ann.label_map(a)
    assert ann.finish(a)["label"] == 1
    for label in (0, 2, -1, 1.0):
        with pytest.raises(KeyError):
            ann.reopen(a, label)
    ann.click({a: (True, ca)})
    assert ann.finish(a)["overwritten"] > 0                                 # the same clicks: label 2 covers all of label 1
    assert np.array_equal(ann.label_map(a) == 2, before == 1)
    with pytest.raises(KeyError):
        ann.reopen(a, 1)                                                    # committed, but no pixel holds it any more
    assert [r["label"] for r in ann.objects(a)] == [1, 2] and ann.object_count(a) == 2
    # a label above 65535 is refused before anything is written
    ann.click({a: (True, ca)})
    ann._held[a].object_count = 65535
    labels, prob = ann.label_map(a, preview=False), ann.current_prob(a).clone()
    with pytest.raises(ValueError):
        ann.finish(a)
    with pytest.raises(ValueError):
        ann.label_map(a)
    assert np.array_equal(ann.label_map(a, preview=False), labels) and torch.equal(ann.current_prob(a), prob)
    assert ann.object_count(a) == 65535 and len(ann.objects(a)) == 2
    ann._held[a].object_count = 65534
    assert ann.finish(a)["label"] == 65535 and (ann.label_map(a) == 65535).any()
    # a call the pool refuses leaves the annotation as it was
    ann.click({b: (True, (20, 20))})
    prob = ann.current_prob(b).clone()
    with pytest.raises(ValueError):
        ann.click({b: (True, (24, 24))}, boxes={b: (0, 0, 99, 99)})         # the box leaves the image
    assert torch.equal(ann.current_prob(b), prob) and len(ann._held[b].clicker) == 1 and len(ann._held[b].undo) == 1
    ann.close(b)
    with pytest.raises(KeyError):
        ann.finish(b)
    assert ann.open(img_b) == b and not ann.current_prob(b).any()


def test_annotations_do_not_touch_one_another():
    ann = AnnotationPool(_make(True)(), max_images=3)
    images = _images()
    aids = [ann.open(image) for image, _ in images]
    ann.click({aid: (True, c) for aid, (_, c) in zip(aids, images)})
    for aid in aids[1:]:
        ann.partially_finish(aid)
    ann.click({aid: (True, (c[0] + 4, c[1] - 3)) for aid, (_, c) in zip(aids, images)})

    def seen(aid):
        return (ann.current_prob(aid).clone(), ann.label_map(aid), ann.label_map(aid, preview=False), ann.objects(aid),
                ann.pool.probs(aid).clone())

    def unchanged(aid, held):
        now = seen(aid)
        return (torch.equal(now[0], held[0]) and np.array_equal(now[1], held[1]) and np.array_equal(now[2], held[2])
                and now[3] == held[3] and torch.equal(now[4], held[4]))

    held = {aid: seen(aid) for aid in aids}
    assert ann.finish(aids[0])["label"] == 1
    assert not unchanged(aids[0], held[aids[0]]) and unchanged(aids[1], held[aids[1]]) and unchanged(aids[2], held[aids[2]])
    held = {aid: seen(aid) for aid in aids}
    assert ann.undo(aids[1]) is not None
    assert unchanged(aids[0], held[aids[0]]) and not unchanged(aids[1], held[aids[1]]) and unchanged(aids[2], held[aids[2]])
    held = {aid: seen(aid) for aid in aids}
    ann.set_mask(aids[2], rect_mask(*SIZES[2]))
    ann.reopen(aids[0], 1)
    assert unchanged(aids[1], held[aids[1]]) and ann.object_count(aids[1]) == 0
