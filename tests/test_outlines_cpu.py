"""CPU: outlines (isegm/inference/outlines.py).  The numpy stand-in, which never walks, against the sequential tracer of
outline_ref.py at every shape and pattern of outline_cases.py; rules O4-O6 against scipy's component counts; the constants
against the header; the pools' outline calls on the stub network with the host ops after every step of a script.  Everything
is integer: equality is exact."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage

from pvpuformer_amd import ops
from pvpuformer_amd.isegm.inference import HostOutlineOps, Outline, host_outline
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool

from outline_cases import PATTERNS, SHAPES, THR, case, pattern, run_pool_script, shape_id
from runs_cases import decode_counts
from sessions_cases import PRED_THR, StubNet, blob_image


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


def _items(kind, src, thr, label):
    return [(torch.from_numpy(src.view(np.int16) if kind == 1 else src), kind, thr, label)]


def assert_rules(o, m, where):
    """O4, O5 and O6 on an outline ``o`` of the map ``m``."""
    H, W = m.shape
    assert o.size == (H, W) and o.points.dtype == np.int32 and o.offsets.dtype == np.int32, where
    o.check()
    got = o.decode()
    assert got.dtype == bool and np.array_equal(got, m), where                                       # O6
    areas = o.areas()
    assert areas.dtype == np.int64 and int(areas.sum()) == o.area() == int(m.sum()), where           # O5
    outer = ndimage.label(m, structure=np.ones((3, 3), dtype=int))[1]
    enclosed = ndimage.label(np.pad(~m, 1, constant_values=True))[1] - 1                             # all but the outside
    holes = o.holes()
    assert holes.dtype == bool and int((~holes).sum()) == outer and int(holes.sum()) == enclosed, where
    loops = o.loops()
    assert len(loops) == len(o) == outer + enclosed, where
    starts = [(int(loop[0][1]), int(loop[0][0])) for loop in loops]
    assert all(a < b for a, b in zip(starts, starts[1:])), where                                     # O4
    for loop, hole in zip(loops, holes):
        keys = [(int(y), int(x)) for x, y in loop]
        assert keys.count(min(keys)) == 1 and keys[0] == min(keys), where
        step = (int(loop[1][0] - loop[0][0]), int(loop[1][1] - loop[0][1]))
        assert (step[0] == 0 and step[1] > 0) if hole else (step[0] > 0 and step[1] == 0), where
    rows, cols = np.nonzero(m)
    assert o.box() == ((int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())) if len(rows) else (H, -1, W, -1)), where


# ------------------------------------------------------------------------------------------------------------- the type
@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_stand_in_equals_the_sequential_tracer(shape, kind):
    H, W = shape
    for name in PATTERNS:
        src, thr, label, m, (points, offsets) = case(kind, name, shape)
        where = (shape, kind, name)
        o, = HostOutlineOps().trace(_items(kind, src, thr, label))
        assert isinstance(o, Outline), where
        assert o.points.tolist() == points.tolist() and o.offsets.tolist() == offsets.tolist(), where
        assert_rules(o, m, where)
        if name in ("zero", "absent"):
            assert len(o) == 0 and o.points.shape == (0, 2) and o.offsets.tolist() == [0] and o.to_coco() == [], where
        if name == "set":
            assert o.points.tolist() == [[0, 0], [W, 0], [W, H], [0, H]] and o.offsets.tolist() == [0, 4], where
        if name == "two_diagonal" and H >= 2 and W >= 2:
            assert o.offsets.tolist() == [0, 8], where
        if name in ("diagonal", "antidiagonal"):
            assert len(o) == 1 and len(o.points) == 4 * min(H, W), where                 # one loop through every saddle twice


def test_a_label_that_is_present_and_one_that_is_absent():
    labels = np.array([[0, 1, 1], [2, 65535, 1], [2, 2, 0]], dtype=np.uint16)
    for label in (0, 1, 2, 65535, 7):
        o, = HostOutlineOps().trace(_items(1, labels, 0.0, label))
        assert np.array_equal(o.decode(), labels == label) and (len(o) == 0) == (label == 7)
    assert len(host_outline(labels == 0)) == 2                                            # two pixels that do not touch


def test_threshold_is_strict_and_in_fp32():
    above = np.nextafter(np.float32(THR), np.float32(1))
    src = np.array([[THR, above], [above, THR]], dtype=np.float32)
    o, = HostOutlineOps().trace(_items(0, src, THR, 0))
    assert o.offsets.tolist() == [0, 8] and np.array_equal(o.decode(), [[False, True], [True, False]])
    src0 = case(0, "random50", (47, 70))[0]
    assert src0.dtype == np.float32 and (src0 == np.float32(THR)).any() and (src0 == above).any()


def test_saddles_turn_left_foreground_8_connected_holes_4_connected():
    ring = pattern("corner_ring", 4, 4)
    o = host_outline(ring)
    assert o.holes().tolist() == [False, True] and o.areas().tolist() == [12, -4]
    assert o.loops()[1].tolist() == [[1, 1], [1, 3], [3, 3], [3, 1]]                       # the hole: South first
    inverse = host_outline(~ring)                                                         # the four corner pixels touch the centre
    assert inverse.holes().tolist() == [False] and inverse.areas().tolist() == [8]
    diamond = pattern("diamond", 3, 3)
    o = host_outline(diamond)
    assert [loop[0].tolist() for loop in o.loops()] == [[1, 0], [1, 1]] and o.holes().tolist() == [False, True]


def test_to_coco_with_and_without_holes():
    m = pattern("rings", 7, 9)
    o = host_outline(m)
    assert o.holes().tolist() == [False, True, False, True]
    outer, every = o.to_coco(), o.to_coco(holes=True)
    assert len(outer) == 2 and len(every) == 4 and outer == [every[0], every[2]]
    assert outer[0] == [0.0, 0.0, 9.0, 0.0, 9.0, 7.0, 0.0, 7.0] and all(type(v) is float for poly in every for v in poly)
    assert every[1] == [1.0, 1.0, 1.0, 6.0, 8.0, 6.0, 8.0, 1.0]
    assert host_outline(np.zeros((3, 4), dtype=bool)).to_coco(holes=True) == []


def test_check_rejects_a_broken_outline():
    good = host_outline(pattern("rings", 7, 9))
    good.check()
    size, pts, off = good.size, good.points, good.offsets

    def broken(points=pts, offsets=off, size=size):
        with pytest.raises(ValueError):
            Outline(size, points, offsets).check()

    broken(offsets=off[:-1])                                                              # does not end at V
    broken(offsets=np.concatenate(([1], off[1:])))                                        # does not begin at 0
    broken(offsets=np.array([0, 2, 4, 8, 12, 16]))                                        # a loop of two corners
    broken(points=np.roll(pts[:4], 1, axis=0), offsets=[0, 4])                            # starts elsewhere
    broken(points=pts[:4][::-1], offsets=[0, 4])                                          # runs the other way
    broken(points=np.concatenate((pts[4:8], pts[:4])), offsets=[0, 4, 8])                 # loops in the wrong order
    broken(points=pts + 1)                                                                # leaves the lattice
    broken(points=np.array([[0, 0], [2, 1], [2, 2], [0, 2]]), offsets=[0, 4])             # a diagonal step
    broken(points=np.array([[0, 0], [1, 0], [2, 0], [2, 2], [1, 2], [0, 2]]), offsets=[0, 6])     # two horizontal steps in a row
    broken(size=(0, 9))


def test_header_defines_equal_the_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vpu_hip.h")).read()
    assert f"#define VPU_OUTLINE_BAND_ROWS {ops.OUTLINE_BAND_ROWS}\n" in header
    assert f"#define VPU_OUTLINE_COLS {ops.OUTLINE_COLS}\n" in header
    assert "#define VPU_OUTLINE_WORK_INTS(v) (16 * (int64_t)(v) + 2)\n" in header and ops.outline_work_len(10) == 162
    B, C = ops.OUTLINE_BAND_ROWS, ops.OUTLINE_COLS
    # lattices of (B + 1) x C and 4 x (C + 1) vertices: rows x groups = max(B + 1, 4 * 2), columns x bands = max(C * 2, C + 1)
    assert ops.outline_scratch_len([(B, C - 1), (3, C)]) == 2 * (max(B + 1, 8) + 2 * C)


def test_host_ops_trace_tensors():
    a, b = case(1, "random30", (33, 130)), case(0, "rings", (47, 70))
    got = HostOutlineOps().trace(_items(1, *a[:3]) + _items(0, *b[:3]))
    assert np.array_equal(got[0].decode(), a[3]) and np.array_equal(got[1].decode(), b[3])
    assert HostOutlineOps().trace([]) == []


# ------------------------------------------------------------------------------------------------------------- the pools
def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


IMAGES = [(60, 80), (48, 48), (50, 70)]


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_session_pool_mask_outlines(zoom):
    pool = SessionPool(_make(zoom)(), max_sessions=3, pred_thr=PRED_THR)
    assert isinstance(pool.ops_outlines, HostOutlineOps)
    images = [blob_image(H, W, seed=j) for j, (H, W) in enumerate(IMAGES)]
    sids = [pool.open(image) for image, _ in images]
    before = pool.readbacks
    fresh = pool.mask_outlines()
    assert pool.readbacks == before + 2 and sorted(fresh) == sids
    for sid, (image, _) in zip(sids, images):                                 # no prediction yet: no loops
        assert fresh[sid].size == image.shape[:2] and len(fresh[sid]) == 0 and fresh[sid].offsets.tolist() == [0]
        assert not pool.probs(sid).any()
    clicks = {sid: Clicker(device=None) for sid in sids}
    for sid, (_, centre) in zip(sids, images):
        clicks[sid].add_click(Click(True, centre))
    for step in range(3):
        masks = pool.predict({sid: clicks[sid] for sid in sids[:2]} if step == 1 else clicks)
        before = pool.readbacks
        outlines = pool.mask_outlines(list(masks))
        assert pool.readbacks == before + 2 and sorted(outlines) == sorted(masks)
        for sid, mask in masks.items():
            assert_rules(outlines[sid], mask, (step, sid))
            assert mask.any() and not mask.all()
        for sid, (_, (r, c)) in zip(sids, images):
            clicks[sid].add_click(Click(step == 0, (r // 2 + 3 * step, c // 2 + 5)))
    assert list(pool.mask_outlines([sids[2]])) == [sids[2]]
    before = pool.readbacks
    assert pool.mask_outlines([]) == {} and pool.readbacks == before
    pool.close(sids[1])
    assert sorted(pool.mask_outlines()) == [sids[0], sids[2]]
    for bad in (sids[1], 7, "0"):
        with pytest.raises(KeyError):
            pool.mask_outlines([bad])


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_annotation_pool_label_outlines_and_export(zoom):
    ann = AnnotationPool(_make(zoom)(), max_images=3)
    assert isinstance(ann.ops_outlines, HostOutlineOps) and isinstance(ann.pool.ops_outlines, HostOutlineOps)
    images = [blob_image(H, W, seed=j) for j, (H, W) in enumerate(IMAGES)]
    seen = []

    def check(where, aids, masks):
        seen.append(where)
        if masks is not None and where in ("click 1", "click 2"):            # no parts yet: the pool's mask is the object's
            before = ann.readbacks
            outlines = ann.pool.mask_outlines(aids)
            assert ann.readbacks == before + 2, where
            for aid in aids:
                assert_rules(outlines[aid], masks[aid], (where, aid))
        for aid in aids:
            for preview in (True, False):
                want = ann.label_map(aid, preview)
                committed = [r["label"] for r in ann.objects(aid)]
                labels = committed + ([ann.object_count(aid) + 1] if preview and where not in ("open", "finish 1", "finish 2", "finish 3") else [])
                before = ann.readbacks
                outlines = ann.label_outlines(aid, preview=preview)
                assert ann.readbacks == before + (2 if labels else 0), (where, aid, preview)
                assert list(outlines) == labels, (where, aid, preview)
                for label, o in outlines.items():
                    assert_rules(o, want == label, (where, aid, preview, label))
                if masks is not None and preview and where in ("click 1", "tidy"):
                    assert np.array_equal(outlines[labels[-1]].decode(), masks[aid]), (where, aid)
                named = ann.label_outlines(aid, [0, 40000], preview)                # the background, and a label no pixel holds
                assert np.array_equal(named[0].decode(), want == 0) and len(named[40000]) == 0, (where, aid, preview)
            committed, records = ann.label_map(aid, False), ann.objects(aid)
            plain = ann.export(aid)
            before = ann.readbacks
            out = ann.export(aid, polygons=True)
            assert ann.readbacks == before + (4 if records else 0), (where, aid)
            assert [{k: v for k, v in e.items() if k not in ("polygons", "polygon_holes")} for e in out] == plain, (where, aid)
            assert [{k: v for k, v in e.items() if k != "segmentation"} for e in plain] == records, (where, aid)
            for e in out:
                on = committed == e["label"]
                assert np.array_equal(decode_counts(e["segmentation"]), on), (where, aid, e["label"])
                o = host_outline(on)
                assert e["polygons"] == o.to_coco() and e["polygon_holes"] == int(o.holes().sum()), (where, aid, e["label"])
                assert all(type(v) is float for poly in e["polygons"] for v in poly), (where, aid)

    aids = run_pool_script(ann, images, check)
    assert "reopen" in seen and "tidy" in seen and len(seen) == 14
    assert all(len(ann.export(aid, True)) == 2 for aid in aids)


def test_fresh_annotation_and_counters():
    ann = AnnotationPool(_make(False)(), max_images=1)
    image, (r, c) = blob_image(60, 80, seed=0)
    aid = ann.open(image)
    before = ann.readbacks
    assert ann.label_outlines(aid) == {} and ann.label_outlines(aid, preview=False) == {}      # nothing to trace:
    assert ann.export(aid, polygons=True) == [] and ann.readbacks == before                    # the device is not touched
    empty = ann.label_outlines(aid, [1])
    assert ann.readbacks == before + 2 and list(empty) == [1] and len(empty[1]) == 0 and empty[1].size == (60, 80)
    mask = ann.click({aid: (True, (r, c))})[aid]
    drawn = ann.label_outlines(aid)
    assert list(drawn) == [1] and np.array_equal(drawn[1].decode(), mask)
    assert ann.label_outlines(aid, preview=False) == {} and ann.export(aid, polygons=True) == []
    first = ann.finish(aid)
    before = ann.readbacks
    out = ann.export(aid)
    assert ann.readbacks == before + 2 and "polygons" not in out[0]                            # as before this call existed
    out = ann.export(aid, polygons=True)
    assert ann.readbacks == before + 6 and first["area"] == host_outline(mask).area()
    assert out[0]["polygons"] == host_outline(mask).to_coco()
    for bad in (-1, 65536, 1.0, "1"):
        with pytest.raises(ValueError):
            ann.label_outlines(aid, [bad])


def test_unknown_ids_raise_key_error():
    ann = AnnotationPool(_make(False)(), max_images=2)
    aid = ann.open(blob_image(48, 48, seed=0)[0])
    for bad in (aid + 1, -1, "0", None):
        with pytest.raises(KeyError):
            ann.label_outlines(bad)
        with pytest.raises(KeyError):
            ann.export(bad, polygons=True)
        with pytest.raises(KeyError):
            ann.pool.mask_outlines([bad])
    ann.close(aid)
    with pytest.raises(KeyError):
        ann.label_outlines(aid)
