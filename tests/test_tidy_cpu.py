"""CPU: the region clean-up (isegm/inference/regions.py).  The numpy + scipy stand-in against the rules
written per pixel (tidy_ref.py) on every case of tidy_cases.py, idempotence, the component count, the diamond and the
``largest`` tie; then ``SessionPool.tidy`` and ``AnnotationPool.tidy`` with the stub network against twins driven by the
per-pixel rules, their read-back counts, their errors and the isolation of what is not named.  Every comparison is exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage

from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.clicker import Click
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.regions import HostRegionOps, host_regions_tidy
from pvpuformer_amd.isegm.inference.sessions import SessionPool

from sessions_cases import PRED_THR, StubNet, blob_image
from tidy_cases import (DIAMOND, PARAMS, SHAPES, THR, SessionTwin, TidyTwinPool, bits_equal, call_args, cases, maps_of,
                        run_annotation_script, run_session_script, shape_id)
from tidy_ref import count_components, tidy_ref


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


# ------------------------------------------------------------------------------------------------------------- the stand-in
def _same(got, want, where):
    add, total, words, rec = got
    assert words.dtype == np.uint64 and np.array_equal(words, want["words"]), where
    assert rec.dtype == np.int32 and np.array_equal(rec, want["rec"]), (where, rec, want["rec"])
    for out, ref in ((add, want["add_out"]), (total, want["total_out"])):
        assert (out is None) == (ref is None) and (out is None or bits_equal(out, ref)), where


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_stand_in_follows_the_rules(shape):
    H, W = shape
    for k, case in enumerate(cases(shape)):
        where = (shape, case["name"], case["seeds"], case["min_area"], case["max_hole"], case["keep"])
        before = case["add"].copy(), case["total"].copy()
        want = tidy_ref(*call_args(case))
        got = host_regions_tidy(*call_args(case))
        _same(got, want, where)
        assert bits_equal(case["add"], before[0]) and bits_equal(case["total"], before[1]), where     # the inputs are not written
        rec = got[3]
        M = np.maximum(case["add"], case["total"]) > np.float32(THR)
        M2 = want["mask"]
        assert rec[0] == M2.sum() and rec[1] == (M & ~M2).sum() and rec[2] == (M2 & ~M).sum(), where
        assert np.array_equal(np.maximum(got[0], got[1]) > np.float32(THR), M2), where                 # the edits land on M2
        if not M2.any():
            assert rec[3:7].tolist() == [H, -1, W, -1], where
        # rec[7] counts the kept components as they stand in M2; filling adds none to those of M1
        assert count_components(M2) == rec[7] <= count_components(want["kept"]), where
        # idempotence: the cleaned maps are a fixed point
        again = host_regions_tidy(got[0], got[1], H, W, case["seeds"], case["min_area"], case["max_hole"], case["keep"], THR)
        assert np.array_equal(again[2], got[2]) and again[3][1] == 0 and again[3][2] == 0, where
        assert np.array_equal(again[3], [rec[0], 0, 0, *rec[3:8]]), where
        assert bits_equal(again[0], got[0]) and bits_equal(again[1], got[1]), where
        # one map absent: M is the other map's
        if k % 3 == 0:
            for kw in (dict(add=False), dict(total=False)):
                _same(host_regions_tidy(*call_args(case, **kw)), tidy_ref(*call_args(case, **kw)), (where, kw))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_component_count_of_the_result_equals_the_kept_components(shape):
    """The 8-connected component count of M2 equals rec[7], on every case, counted here by the flood fill of tidy_ref.py and
    in the stand-in by scipy.  rec[7] counts the kept components as they stand in M2.  That is the number of components of M1
    except where a kept island lies inside a hole that is filled -- the hole is the 4-connected background between the ring
    and the island, and filling it makes one component of the two.  Five of the 846 cases have such a hole, all with
    max_hole None (components of M2 against those of M1): 17 x 13 nested rings 1 / 3, 47 x 70 nested rings with a seeded
    inner ring 1 / 2 and "at thr" 16 / 20, 33 x 130 random 0.5 11 / 14, 64 x 64 random 0.5 15 / 20."""
    H, W = shape
    joined = 0
    for case in cases(shape):
        add, total, _, rec = host_regions_tidy(*call_args(case))
        M2 = np.maximum(add, total) > np.float32(THR)
        assert count_components(M2) == rec[7], (shape, case["name"], case["seeds"], case["min_area"], case["max_hole"], case["keep"])
        joined += count_components(tidy_ref(*call_args(case))["kept"]) > rec[7]
    assert joined == {(17, 13): 1, (47, 70): 2, (33, 130): 1, (64, 64): 1}.get(shape, 0)


def test_the_cases_cover_every_parameter():
    seen = set()
    for shape in SHAPES:
        for case in cases(shape):
            above = case["min_area"] == shape[0] * shape[1] + 1
            seen.add(("above" if above else case["min_area"], case["max_hole"], case["keep"]))
    assert seen == set(PARAMS)


def test_the_diamond_is_one_component_with_a_one_pixel_hole():
    rs = np.random.RandomState(0)
    add, total = maps_of(DIAMOND, rs)
    for run in (host_regions_tidy, lambda *a: (lambda d: (d["add_out"], d["total_out"], d["words"], d["rec"]))(tidy_ref(*a))):
        rec = run(add, total, 3, 3, [], 4, 0, "all", THR)[3]
        assert rec.tolist() == [4, 0, 0, 0, 2, 0, 2, 1]                         # one component of area 4: min_area 4 keeps it
        rec = run(add, total, 3, 3, [], 5, 0, "all", THR)[3]
        assert rec.tolist() == [0, 4, 0, 3, -1, 3, -1, 0]
        a, t, _, rec = run(add, total, 3, 3, [], 0, 1, "all", THR)
        assert rec.tolist() == [5, 0, 1, 0, 2, 0, 2, 1] and a[1, 1] == 1.0 and t[1, 1] == 1.0       # the hole is one pixel
        rec = run(add, total, 3, 3, [(1, 1, False)], 0, None, "all", THR)[3]
        assert rec.tolist() == [4, 0, 0, 0, 2, 0, 2, 1]                         # a negative seed keeps the hole open


def test_largest_tie_goes_to_the_first_component_in_raster_order():
    M = np.zeros((5, 5), dtype=bool)
    M[0, 3:5] = True                        # two components of two pixels; this one comes first
    M[2:4, 0] = True
    M[4, 4] = True
    add, total = maps_of(M, np.random.RandomState(1))
    want = np.zeros((5, 5), dtype=bool)
    want[0, 3:5] = True
    for seeds, keep_also in (([], None), ([(4, 4, True)], (4, 4))):
        ref = tidy_ref(add, total, 5, 5, seeds, 99, 0, "largest", THR)
        got = host_regions_tidy(add, total, 5, 5, seeds, 99, 0, "largest", THR)
        expect = want.copy()
        if keep_also:
            expect[keep_also] = True        # a protected component is kept beside the largest
        assert np.array_equal(ref["mask"], expect) and np.array_equal(got[2], ref["words"]) and np.array_equal(got[3], ref["rec"])
        assert got[3][7] == 1 + (keep_also is not None)
    empty = host_regions_tidy(add, total, 5, 5, [(1, 1, True)], 0, 0, "seeded", THR)       # no positive seed on the foreground
    assert empty[3].tolist() == [0, 5, 0, 5, -1, 5, -1, 0]


def test_stand_in_errors():
    z = np.zeros((2, 2), dtype=np.float32)
    for bad in (dict(keep="biggest"), dict(min_area=-1), dict(max_hole=-1), dict(min_area=1.5)):
        kw = dict(min_area=0, max_hole=0, keep="all")
        kw.update(bad)
        with pytest.raises(ValueError):
            host_regions_tidy(z, None, 2, 2, [], kw["min_area"], kw["max_hole"], kw["keep"], THR)


# ------------------------------------------------------------------------------------------------------------- the pools
SIZES = [(60, 80), (48, 48), (50, 70)]


def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


def _images(sizes=SIZES):
    return [blob_image(H, W, seed=j) for j, (H, W) in enumerate(sizes)]


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_session_pool_tidy_equals_the_twin(zoom):
    make = _make(zoom)
    pool = SessionPool(make(), max_sessions=5, pred_thr=PRED_THR)
    assert isinstance(pool.ops_regions, HostRegionOps)
    twins = [SessionTwin(pool, make, image) for image, _ in _images()]
    bystander = pool.open(_images([(40, 44)])[0][0])
    pool.predict({bystander: [Click(True, (20, 22), indx=0)]})
    held = pool.probs(bystander).clone(), pool.readbacks
    kept, cleaned = run_session_script(pool, twins)
    for t in twins:                         # the island of click 2 is kept by its click, and goes without it; so do the holes
        assert count_components(kept[t.sid]) >= 2 and count_components(cleaned[t.sid]) == 1, t.sid
        assert np.array_equal(ndimage.binary_fill_holes(cleaned[t.sid]), cleaned[t.sid]), t.sid
    assert torch.equal(pool.probs(bystander), held[0])                          # a session that is not named is untouched
    # defaults: every open session, and a session without a prediction yet gives an all-False mask
    fresh = pool.open(_images([(9, 11)])[0][0]) if None in pool._slots else None
    reads = pool.readbacks
    got = pool.tidy(min_area=3)
    assert pool.readbacks == reads + 1 and sorted(got) == sorted(sid for sid, s in enumerate(pool._slots) if s is not None)
    assert fresh is None or (got[fresh].shape == (9, 11) and not got[fresh].any())


def test_session_pool_tidy_errors():
    pool = SessionPool(_make(False)(), max_sessions=2, pred_thr=PRED_THR)
    sid = pool.open(_images([(20, 24)])[0][0])
    reads = pool.readbacks
    for kw in (dict(keep="biggest"), dict(min_area=-1), dict(max_hole=-2)):
        with pytest.raises(ValueError):
            pool.tidy([sid], **kw)
    with pytest.raises(KeyError):
        pool.tidy([1])
    with pytest.raises(ValueError):
        pool.tidy([sid], seeds={1: []})
    assert pool.readbacks == reads and pool.tidy([]) == {}
    with pytest.raises(ValueError):
        SessionPool(_make(False)(), max_sessions=1, pred_thr=1.0).tidy()


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_annotation_pool_tidy_equals_the_twin_after_every_call(zoom):
    make = _make(zoom)
    ann = AnnotationPool(make(), max_images=3)
    assert isinstance(ann.ops_regions, HostRegionOps)
    seen = []

    def on_tidy(where, aid, before, mask, kw):
        a = ann._ann(aid)
        ref = tidy_ref(before, None, a.H, a.W, [(c.coords[0], c.coords[1], c.is_positive) for c in a.clicker.get_clicks()],
                       kw.get("min_area", 0), kw.get("max_hole", 0), kw.get("keep", "all"), ann.prob_thresh)
        assert np.array_equal(mask, ref["mask"]), (where, aid)
        seen.append((where, int(ref["rec"][1]), int(ref["rec"][2])))
        if where == "tidy with the clicks as seeds":                            # T2 and T5: the clicks protect what they made
            for c in a.clicker.get_clicks():
                assert mask[c.coords] == bool(before[c.coords] > np.float32(ann.prob_thresh)), (where, aid, c.coords)

    log = run_annotation_script(ann, TidyTwinPool(make), _images(), on_tidy=on_tidy)
    assert [w for w, _ in log].count("tidy on the reopened object") == 1
    changed = {w for w, removed, added in seen if removed or added}
    assert {"tidy on the parts", "tidy on the initial mask"} <= changed, changed
    for aid in range(3):
        assert ann.object_count(aid) == 3 and [r["label"] for r in ann.objects(aid)] == [2, 3]


def test_annotation_pool_tidy_counts_errors_and_isolation():
    ann = AnnotationPool(_make(False)(), max_images=3, max_undo=2)
    (img0, c0), (img1, c1), (img2, _) = _images()
    a0, a1, a2 = ann.open(img0), ann.open(img1), ann.open(img2)
    ann.click({a0: (True, c0), a1: (True, c1)})
    ann.partially_finish(a1)
    ann.click({a1: (True, (3, 3))})
    other = ann.current_prob(a0).clone(), ann.label_map(a0).copy()
    parts_before, offset = ann._ann(a1).parts, ann._ann(a1).clicker.click_indx_offset
    snapshot = parts_before.clone()
    reads, forwards = ann.readbacks, ann.forwards
    got = ann.tidy([a1, a2], min_area=30, max_hole=None)                        # a2 is empty: all False, nothing pushed
    assert ann.readbacks == reads + 1 and ann.forwards == forwards
    assert not got[a2].any() and got[a2].shape == img2.shape[:2] and ann._ann(a2).undo == []
    assert ann._ann(a1).parts is not parts_before and torch.equal(parts_before, snapshot)       # a new tensor; the old one unwritten
    assert len(ann._ann(a1).clicker) == 1 and ann._ann(a1).clicker.click_indx_offset == offset
    assert np.array_equal(got[a1], ann.current_prob(a1)[0, 0].numpy() > np.float32(0.5))
    assert torch.equal(ann.current_prob(a0), other[0]) and np.array_equal(ann.label_map(a0), other[1])
    reads = ann.readbacks
    assert not ann.tidy([a2])[a2].any() and ann.readbacks == reads              # only empty objects: no launch, no read-back
    for kw in (dict(keep="biggest"), dict(min_area=-1), dict(max_hole=-1)):
        with pytest.raises(ValueError):
            ann.tidy([a1], **kw)
    with pytest.raises(KeyError):
        ann.tidy([a1, 7])
    assert ann.readbacks == reads and len(ann._ann(a1).undo) == 2               # refused before anything changed
