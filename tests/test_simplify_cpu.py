"""CPU: the numpy stand-in ``host_simplify`` (polygons.py, rules S1-S6) against the sequential Douglas-Peucker of simplify_ref.py
on every case of simplify_cases.py, the ``Polygons`` class, the refusals, the mirrored header constants, and the pools' new
arguments on the stub network with host ops.  Everything is integers: equality is element for element."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd import ops
from pvpuformer_amd.isegm.inference import HostOutlineOps, Outline, Polygons, host_outline, host_simplify
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.polygons import quantise, same_polygons, simplify_loops
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool

from outline_cases import run_pool_script, same_outline
from sessions_cases import PRED_THR, StubNet, blob_image
from simplify_cases import ALL_CASES, OUTLINE_CASES, SYNTHETIC_CASES, TOLERANCES, assert_s6, reference, source, synthetic_case
from simplify_ref import quantise_ref


@pytest.fixture(autouse=True)
def host_transforms(monkeypatch):
    """ZoomIn's two device calls on the host, as in test_outlines_cpu.py."""
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


_GOT = {}


def _got(case, tolerance):
    key = (case, tolerance)
    if key not in _GOT:
        _GOT[key] = host_simplify(source(case), tolerance)
    return _GOT[key]


def is_subsequence(short, long):
    it = iter(long)
    return all(any(s == v for v in it) for s in short)


# -------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("tolerance", TOLERANCES, ids=str)
def test_stand_in_equals_the_sequential_reference(tolerance):
    t = quantise_ref(tolerance)
    for case in ALL_CASES:
        o, got = source(case), _got(case, tolerance)
        points, offsets, hole, dropped, kept_of = reference(case, tolerance)
        where = (case, tolerance)
        assert got.points.dtype == np.int32 and got.offsets.dtype == np.int32 and got.hole.dtype == bool, where
        assert np.array_equal(got.points, points) and np.array_equal(got.offsets, offsets), where
        assert np.array_equal(got.hole, hole) and got.dropped == dropped, where
        assert got.size == o.size and got.tolerance == t / 4 and got.source == (len(o.points), len(o)), where
        assert len(got) + got.dropped == len(o), where
        assert_s6(o, kept_of, t, where)
        alive = [l for l, k in enumerate(kept_of) if k is not None]
        assert len(alive) == len(got), where
        exact_loops = o.loops()
        for loop, l in zip(got.loops(), alive):                # a subsequence of the exact loop from the same start
            exact = exact_loops[l]
            assert len(loop) >= 3 and tuple(loop[0]) == tuple(exact[0]), where
            assert is_subsequence(loop.tolist(), exact.tolist()), where
        if case[0] == "outline":
            got.check()
            assert np.array_equal(got.hole, o.holes()[alive]), where                # S5: the exact loop's sign (O5)


def test_tolerance_zero_keeps_every_corner_of_an_outline():
    for case in OUTLINE_CASES:
        o, got = source(case), _got(case, 0)
        assert got.dropped == 0 and np.array_equal(got.points, o.points) and np.array_equal(got.offsets, o.offsets), case
        assert np.array_equal(got.hole, o.holes()) and np.array_equal(got.areas(), o.areas().astype(np.float64)), case


def test_synthetic_loops_do_what_they_are_for():
    kept = {(name, n, tol): len(_got(("synthetic", name, n), tol).points) for _, name, n in SYNTHETIC_CASES for tol in TOLERANCES}
    for _, name, n in SYNTHETIC_CASES:
        o = synthetic_case(name, n)
        assert len(o.points) == n and o.points.min() >= 0 and o.points.max() <= 8191
    assert synthetic_case("square", 65).points.max() == 8191 and synthetic_case("square", 65).points.min() == 0
    for n in (63, 64, 65, 1025):
        for tol in TOLERANCES:
            assert kept[("revisit", n, tol)] == 0 and _got(("synthetic", "revisit", n), tol).dropped == 1     # zero area
            assert kept[("pinned", n, tol)] == 0                                                              # A == B, never split
        assert kept[("sliver", n, 0)] == n and kept[("sliver", n, 3)] == 0                                    # two vertices left
        assert kept[("zigzag", n, 0)] == n
        # depth 1 is AT tolerance 1 and depth 3 AT tolerance 3 (16 num == t^2 den: not kept); depth 2 and 4 are a step beyond
        assert kept[("threshold", n, 0.5)] > kept[("threshold", n, 1)] > kept[("threshold", n, 3)] > kept[("threshold", n, 1024)] == 4
        top = [tuple(p) for p in _got(("synthetic", "threshold", n), 1).points.tolist()]
        assert not any(y == 1 for _, y in top) and any(y == 2 for _, y in top)
        right = [tuple(p) for p in _got(("synthetic", "threshold", n), 3).points.tolist()]
        assert not any(x == 3997 for x, _ in right) and any(x == 3996 for x, _ in right)
    for n in (65, 257):                                                       # the comb needs a round per tooth, and more
        o = synthetic_case("comb", n)
        teeth = min(64, (n - 2) // 2)
        assert simplify_loops(o.points, o.offsets, 4)[3] >= teeth
    o = synthetic_case("zigzag", 65)                                          # level chain, equal heights: ties in every chain
    assert simplify_loops(o.points, o.offsets, 0)[3] >= 60


# ------------------------------------------------------------------------------------------------------------- the class
def _two_loops():
    m = np.zeros((12, 14), dtype=bool)
    m[1:9, 1:10] = True
    m[3:6, 3:7] = False                                                       # a hole
    m[10, 12] = True                                                          # a speck that collapses at a tolerance
    return host_outline(m)


def test_to_coco_loops_and_holes():
    o = _two_loops()
    assert len(o) == 3 and o.holes().tolist() == [False, True, False]
    exact = o.simplify(0)
    assert isinstance(exact, Polygons) and exact.to_coco() == o.to_coco() and exact.to_coco(holes=True) == o.to_coco(holes=True)
    p = o.simplify(1)
    assert p.dropped == 1 and len(p) == 2 and p.holes().tolist() == [False, True] and p.source == (12, 3)
    assert p.to_coco() == [[1.0, 1.0, 10.0, 1.0, 10.0, 9.0, 1.0, 9.0]]
    assert p.to_coco(holes=True) == [[1.0, 1.0, 10.0, 1.0, 10.0, 9.0, 1.0, 9.0], [3.0, 3.0, 3.0, 6.0, 7.0, 6.0, 7.0, 3.0]]
    assert all(type(v) is float for poly in p.to_coco(True) for v in poly)
    assert p.areas().tolist() == [72.0, -12.0] and [loop.tolist() for loop in p.loops()][1][0] == [3, 3]
    p.holes()[0] = True
    assert p.holes().tolist() == [False, True]                                # a copy
    gone = o.simplify(1024)
    assert len(gone) == 0 and gone.dropped == 3 and gone.to_coco(True) == [] and gone.offsets.tolist() == [0] and gone.check() is gone
    none = host_simplify(host_outline(np.zeros((3, 4), dtype=bool)), 2)
    assert len(none) == 0 and none.dropped == 0 and none.source == (0, 0) and none.size == (3, 4) and none.tolerance == 2.0


def test_check_rejects_a_broken_object():
    p = _two_loops().simplify(0.5)
    assert p.check() is p and len(p) == 3

    def broken(**changes):
        kw = dict(size=p.size, points=p.points, offsets=p.offsets, hole=p.hole, tolerance=p.tolerance, source=p.source, dropped=p.dropped)
        kw.update(changes)
        with pytest.raises(ValueError):
            Polygons(**kw).check()

    broken(offsets=p.offsets[:-1])                                            # does not end at V'
    broken(offsets=np.concatenate(([1], p.offsets[1:])))
    broken(offsets=np.array([0, 2, 4, len(p.points)]))                        # a loop of two vertices
    broken(hole=p.hole[:-1])
    broken(points=p.points + np.array([20, 0]))                               # off the lattice
    broken(points=-p.points)
    broken(points=np.roll(p.points[:4], 1, axis=0), offsets=[0, 4], hole=[False])      # does not start at its smallest (y, x)
    broken(points=np.concatenate((p.points[4:], p.points[:4])), offsets=np.concatenate(([0], (p.offsets[2:] - 4), [len(p.points)])),
           hole=np.roll(p.hole, -1))                                          # the starts do not ascend
    broken(size=(0, 5))
    broken(tolerance=0.3)
    broken(tolerance=2000)
    broken(dropped=-1)


def test_the_tolerance_is_quantised_to_quarter_pixels():
    for tol in TOLERANCES + [0.1, 0.12, 0.13, 0.3, 0.37, 0.38, 0.6, 2.9, 1023.9, 1024.0, 7]:
        assert quantise(tol) == round(4 * tol) == quantise_ref(tol), tol
    assert quantise(0.125) == 0 and quantise(0.375) == 2 and quantise(1024) == 4096 and quantise(np.float32(1.5)) == 6
    o = _two_loops()
    assert o.simplify(0.3).tolerance == 0.25 and o.simplify(0.4).tolerance == 0.5 and o.simplify(3).tolerance == 3.0
    case = ("outline", "random50", (47, 70))
    assert same_polygons(host_simplify(source(case), 0.3), _got(case, 0.25))
    assert not same_polygons(host_simplify(source(case), 0.4), _got(case, 0.25))


def test_refusals():
    o = _two_loops()
    for bad in (-0.25, -1, float("nan"), 1024.25, 5000, float("inf"), "wide", None):
        with pytest.raises(ValueError):
            host_simplify(o, bad)
        with pytest.raises(ValueError):
            quantise(bad)
    for bad in (-0.25, float("nan"), 1024.25):
        with pytest.raises(ValueError):
            o.simplify(bad)
        with pytest.raises(ValueError):
            HostOutlineOps().trace([(torch.zeros(4, 4), 0, 0.5, 0)], bad)
    square = Outline((3, 8192), [[0, 0], [8192, 0], [8192, 3], [0, 3]], [0, 4])
    with pytest.raises(ValueError):
        square.simplify(1)
    with pytest.raises(ValueError):
        HostOutlineOps().trace([(torch.zeros(1, 8192), 0, 0.5, 0)], 1)
    assert len(HostOutlineOps().trace([(torch.ones(1, 8191), 0, 0.5, 0)], 0.5)[0]) == 1
    assert len(HostOutlineOps().trace([(torch.zeros(1, 8192), 0, 0.5, 0)])[0]) == 0           # no tolerance: as before


def test_header_defines_equal_the_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vpu_hip.h")).read()
    assert f"#define VPU_SIMPLIFY_THREADS {ops.SIMPLIFY_THREADS}\n" in header
    assert f"#define VPU_SIMPLIFY_SHORT {ops.SIMPLIFY_SHORT}\n" in header and ops.SIMPLIFY_SHORT == 64
    assert "#define VPU_SIMPLIFY_WORK_INTS(v, l) (10 * (int64_t)(v) + 5 * (int64_t)(l) + 8)\n" in header
    assert ops.outline_simplify_work_len(10, 3) == 123
    assert ops.SIMPLIFY_SHORT_FORM in (ops.SIMPLIFY_FORM_A, ops.SIMPLIFY_FORM_B) and (ops.SIMPLIFY_FORM_A, ops.SIMPLIFY_FORM_B) == (0, 1)
    assert "int vpu_outline_simplify_batched(" in header


# ------------------------------------------------------------------------------------------------------------- the pools
def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


IMAGES = [(60, 80), (48, 48), (50, 70)]
TOL = 1.0


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_pools_with_and_without_a_tolerance(zoom):
    ann = AnnotationPool(_make(zoom)(), max_images=3)
    assert isinstance(ann.ops_outlines, HostOutlineOps) and isinstance(ann.pool.ops_outlines, HostOutlineOps)
    images = [blob_image(H, W, seed=j) for j, (H, W) in enumerate(IMAGES)]
    seen, simplified = [], [0]

    def check(where, aids, masks):
        seen.append(where)
        before = ann.readbacks
        exact = ann.pool.mask_outlines(aids, tolerance=None)
        assert ann.readbacks == before + 2, where
        today = ann.pool.mask_outlines(aids)
        polys = ann.pool.mask_outlines(aids, tolerance=TOL)
        assert ann.readbacks == before + 2 + 2 + 3, where
        for aid in aids:
            thr = np.float32(ann.pool.pred_thr)
            want = host_outline(ann.pool.probs(aid)[0, 0].numpy() > thr)
            assert type(exact[aid]) is Outline and same_outline(exact[aid], want) and same_outline(today[aid], want), (where, aid)
            assert type(polys[aid]) is Polygons and same_polygons(polys[aid], want.simplify(TOL)), (where, aid)
            simplified[0] += len(want.points) - len(polys[aid].points)
            for preview in (True, False):
                before = ann.readbacks
                exact_l = ann.label_outlines(aid, preview=preview, tolerance=None)
                assert ann.readbacks == before + (2 if exact_l else 0), (where, aid)
                before = ann.readbacks
                polys_l = ann.label_outlines(aid, preview=preview, tolerance=TOL)
                assert ann.readbacks == before + (3 if exact_l else 0) and list(polys_l) == list(exact_l), (where, aid)
                label_map = ann.label_map(aid, preview)
                for label, o in exact_l.items():
                    assert type(o) is Outline and same_outline(o, host_outline(label_map == label)), (where, aid, label)
                    assert same_polygons(polys_l[label].check(), o.simplify(TOL)), (where, aid, label)
            records = ann.objects(aid)
            plain = ann.export(aid, polygons=True)
            before = ann.readbacks
            out = ann.export(aid, polygons=True, tolerance=TOL)
            assert ann.readbacks == before + (5 if records else 0), (where, aid)
            assert ann.export(aid, tolerance=TOL) == ann.export(aid), (where, aid)              # without polygons: no trace
            assert ann.export(aid, True, None) == plain, (where, aid)
            committed = ann.label_map(aid, False)
            assert len(out) == len(plain) == len(records), (where, aid)
            for e, was in zip(out, plain):
                assert set(e) == set(was) | {"polygon_tolerance", "polygon_dropped"} and "polygon_tolerance" not in was, (where, aid)
                assert e["segmentation"] == was["segmentation"], (where, aid)
                p = host_outline(committed == e["label"]).simplify(TOL)
                assert e["polygons"] == p.to_coco() and e["polygon_holes"] == int(p.holes().sum()), (where, aid)
                assert e["polygon_tolerance"] == TOL and e["polygon_dropped"] == p.dropped, (where, aid)
                assert {k: v for k, v in e.items() if not k.startswith("polygon")} == \
                       {k: v for k, v in was.items() if not k.startswith("polygon")}, (where, aid)

    run_pool_script(ann, images, check)
    assert len(seen) == 14 and simplified[0] > 100
    for bad in (-1, float("nan"), 1025):
        before = ann.readbacks
        for call in (lambda: ann.pool.mask_outlines(None, tolerance=bad), lambda: ann.label_outlines(0, tolerance=bad),
                     lambda: ann.export(0, True, tolerance=bad), lambda: ann.label_outlines(0, preview=True, tolerance=bad)):
            with pytest.raises(ValueError):
                call()
        assert ann.readbacks == before


def test_session_pool_counters_and_empty_calls():
    pool = SessionPool(_make(False)(), max_sessions=2, pred_thr=PRED_THR)
    image, _ = blob_image(60, 80, seed=0)
    sid = pool.open(image)
    before = pool.readbacks
    fresh = pool.mask_outlines(tolerance=2)
    assert pool.readbacks == before + 3 and type(fresh[sid]) is Polygons and len(fresh[sid]) == 0 and fresh[sid].tolerance == 2.0
    assert pool.mask_outlines([], tolerance=2) == {} and pool.readbacks == before + 3
    with pytest.raises(ValueError):
        pool.mask_outlines([], tolerance=-2)
    assert math.isclose(pool.mask_outlines(tolerance=0.3)[sid].tolerance, 0.25)
