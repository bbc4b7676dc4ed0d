"""GPU: ``vpu_outline_simplify_batched`` (csrc/outline.hip) against the numpy stand-in ``host_simplify`` on every case of
simplify_cases.py, both split forms, and the pools' tolerance arguments on the device model against a twin pool on host ops.
Everything is integers: equality is element for element."""
import numpy as np
import pytest
import torch

from pvpuformer_amd import ops
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.outlines import DeviceOutlineOps, HostOutlineOps, Outline
from pvpuformer_amd.isegm.inference.polygons import Polygons, host_simplify, same_polygons, simplify_loops
from pvpuformer_amd.isegm.inference.predictors import get_predictor

from outline_cases import PATTERNS, SHAPES, THR, case, run_pool_script, same_outline
from sessions_cases import blob_image
from simplify_cases import OUTLINE_CASES, SYNTHETIC_CASES, TOLERANCES, assert_s6, source
from simplify_ref import quantise_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GARBAGE = -0x12345679
SPARE = 16
IMG = 224
A, B = ops.SIMPLIFY_FORM_A, ops.SIMPLIFY_FORM_B


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_WANT = {}


def _want(c, tolerance):
    """The stand-in's Polygons of a case at a tolerance, computed once."""
    if (c, tolerance) not in _WANT:
        _WANT[(c, tolerance)] = host_simplify(source(c), tolerance)
    return _WANT[(c, tolerance)]


_ROUNDS = {}


def _rounds(o, t):
    if (id(o), t) not in _ROUNDS:
        _ROUNDS[(id(o), t)] = simplify_loops(o.points, o.offsets, t)[3]
    return _ROUNDS[(id(o), t)]


def _launch(items, t, form, cap=None, loop_cap=None, loop_max=None):
    """``items``: [Outline], each one item of ONE call, its loops as a trace would have left them on the device -> (out_points of
    cap + SPARE rows, out_offsets and out_hole of loop_cap + SPARE entries, firsts of 2 (n + 1) + 4 + SPARE entries).  Every output
    is pre-filled with a sentinel and the work array with garbage; the inputs must come back unchanged."""
    n = len(items)
    V, L = sum(len(o.points) for o in items), sum(len(o) for o in items)
    starts = np.concatenate(([0], np.cumsum([len(o.points) for o in items])))
    points = np.concatenate([o.points for o in items] + [np.zeros((0, 2), dtype=np.int32)]).astype(np.int32)
    offsets = np.concatenate([o.offsets[:-1] + s for o, s in zip(items, starts)] + [[V]]).astype(np.int32)
    item_loops = np.concatenate(([0], np.cumsum([len(o) for o in items]))).astype(np.int32)
    loop_max = L if loop_max is None else loop_max
    cap = V if cap is None else cap
    loop_cap = L + 1 if loop_cap is None else loop_cap
    d_points = torch.from_numpy(points).cuda() if V else torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    d_offsets = torch.from_numpy(np.concatenate((offsets, np.full(max(loop_max - L, 0), SENTINEL, dtype=np.int32)))).cuda()
    d_loops = torch.from_numpy(item_loops).cuda()
    before = (d_points.clone(), d_offsets.clone(), d_loops.clone())
    work = torch.full((ops.outline_simplify_work_len(V, loop_max),), GARBAGE, device="cuda", dtype=torch.int32)
    out_points = torch.full((cap + SPARE, 2), SENTINEL, device="cuda", dtype=torch.int32)
    out_offsets = torch.full((loop_cap + SPARE,), SENTINEL, device="cuda", dtype=torch.int32)
    out_hole = torch.full((loop_cap + SPARE,), 0x5A, device="cuda", dtype=torch.uint8)
    firsts = torch.full((2 * (n + 1) + 4 + SPARE,), SENTINEL, device="cuda", dtype=torch.int32)
    ops.outline_simplify_batched(d_points, d_offsets, d_loops, n, V, loop_max, t, work, out_points, out_offsets, out_hole, firsts,
                                 cap=cap, loop_cap=loop_cap, short_form=form)
    torch.cuda.synchronize()
    for now, was in zip((d_points, d_offsets, d_loops), before):
        assert torch.equal(now, was)                                         # the inputs are as they were
    return out_points.cpu().numpy(), out_offsets.cpu().numpy(), out_hole.cpu().numpy(), firsts.cpu().numpy()


def _check(items, want, t, form, cap=None, loop_cap=None, loop_max=None):
    """One launch against the stand-in's Polygons ``want`` of the items -> the raw bytes of all four outputs."""
    n = len(items)
    V, L = sum(len(o.points) for o in items), sum(len(o) for o in items)
    points, offsets, hole, firsts = _launch(items, t, form, cap, loop_cap, loop_max)
    raw = points.tobytes() + offsets.tobytes() + hole.tobytes() + firsts.tobytes()
    cap = V if cap is None else cap
    loop_cap = L + 1 if loop_cap is None else loop_cap
    assert (points[cap:] == SENTINEL).all() and (offsets[loop_cap:] == SENTINEL).all() and (hole[loop_cap:] == 0x5A).all()
    assert (firsts[2 * (n + 1) + 4:] == SENTINEL).all()                      # nothing at or beyond a cap or an end
    if V == 0 or (L if loop_max is None else loop_max) == 0:                 # nothing was launched
        assert (points == SENTINEL).all() and (offsets == SENTINEL).all() and (hole == 0x5A).all() and (firsts == SENTINEL).all()
        return raw
    kept = np.concatenate(([0], np.cumsum([len(w.points) for w in want])))
    alive = np.concatenate(([0], np.cumsum([len(w) for w in want])))
    Vs, Ls = int(kept[-1]), int(alive[-1])
    all_points = np.concatenate([w.points for w in want] + [np.zeros((0, 2), dtype=np.int32)])
    all_offsets = np.concatenate([w.offsets[:-1] + s for w, s in zip(want, kept)] + [[Vs]])
    all_hole = np.concatenate([w.hole for w in want] + [np.zeros(0, dtype=bool)])
    assert firsts[:n + 1].tolist() == alive.tolist() and firsts[n + 1:2 * n + 2].tolist() == kept.tolist()
    assert firsts[2 * n + 2:2 * n + 5].tolist() == [Vs, Ls, sum(w.dropped for w in want)]      # the true totals whatever the caps
    rounds = max(_rounds(o, t) for o in items if len(o))
    assert firsts[2 * n + 5] == rounds                                       # the most rounds of one loop
    assert np.array_equal(points[:min(cap, Vs)], all_points[:cap]) and (points[min(cap, Vs):] == SENTINEL).all()
    assert np.array_equal(offsets[:min(loop_cap, Ls + 1)], all_offsets[:loop_cap]) and (offsets[min(loop_cap, Ls + 1):] == SENTINEL).all()
    assert np.array_equal(hole[:min(loop_cap, Ls)], all_hole[:loop_cap].astype(np.uint8)) and (hole[min(loop_cap, Ls):] == 0x5A).all()
    return raw


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("tolerance", TOLERANCES, ids=str)
def test_alone_equals_the_stand_in(tolerance):
    _need_gpu()
    t = quantise_ref(tolerance)
    for c in OUTLINE_CASES + SYNTHETIC_CASES:
        _check([source(c)], [_want(c, tolerance)], t, None)                  # the default form; both forms alone: below


@pytest.mark.parametrize("tolerance", TOLERANCES, ids=str)
def test_all_loops_of_a_kind_in_one_launch_and_both_forms_write_the_same_bytes(tolerance):
    _need_gpu()
    t = quantise_ref(tolerance)
    for cases in (OUTLINE_CASES, SYNTHETIC_CASES, SYNTHETIC_CASES[::-1] + OUTLINE_CASES[::7]):
        items, want = [source(c) for c in cases], [_want(c, tolerance) for c in cases]
        assert _check(items, want, t, A) == _check(items, want, t, B), (tolerance, len(cases))
    short = [c for c in SYNTHETIC_CASES if c[2] <= ops.SIMPLIFY_SHORT]       # every short synthetic loop alone, in both forms
    for c in short:
        assert _check([source(c)], [_want(c, tolerance)], t, A) == _check([source(c)], [_want(c, tolerance)], t, B), c


def test_caps_below_the_totals_keep_the_counts_and_the_rest_of_the_buffers():
    _need_gpu()
    cases = OUTLINE_CASES[5::11] + SYNTHETIC_CASES[::5]
    items, want = [source(c) for c in cases], [_want(c, 1) for c in cases]
    Vs, Ls = sum(len(w.points) for w in want), sum(len(w) for w in want)
    L = sum(len(o) for o in items)
    assert Vs > 64 and Ls > 8 and sum(w.dropped for w in want) > 8
    for form in (A, B):
        _check(items, want, 4, form)
        _check(items, want, 4, form, cap=Vs // 2, loop_cap=(Ls + 1) // 2)
        _check(items, want, 4, form, cap=0, loop_cap=0)
        _check(items, want, 4, form, cap=Vs, loop_cap=Ls)                    # all loops, not the closing offset
        _check(items, want, 4, form, loop_max=L + 5)                         # a bound above the loops, as after a trace
    empty = Outline((5, 7), np.zeros((0, 2), dtype=np.int32), [0])
    _check([empty, empty], [host_simplify(empty, 1)] * 2, 4, B)              # no corner anywhere: nothing is launched
    _check([empty, items[0], empty], [host_simplify(empty, 1), want[0], host_simplify(empty, 1)], 4, B)


def test_device_ops_equal_the_host_ops():
    _need_gpu()
    items = []
    for i, shape in enumerate(SHAPES):
        kind, name = i % 2, PATTERNS[(i + 6) % len(PATTERNS)]
        src, thr, label = case(kind, name, shape)[:3]
        items.append((torch.from_numpy(src.view(np.int16) if kind == 1 else src).cuda(), kind, thr, label))
    exact = HostOutlineOps().trace(items)
    for tolerance in (0, 0.5, 1, 3):
        got = DeviceOutlineOps("cuda").trace(items, tolerance)
        host = HostOutlineOps().trace(items, tolerance)
        assert len(got) == len(host) == len(items)
        for g, h, o in zip(got, host, exact):
            assert type(g) is Polygons and same_polygons(g, h) and same_polygons(g, o.simplify(tolerance)), tolerance
            g.check()
    for g, o in zip(DeviceOutlineOps("cuda").trace(items, None), exact):     # None: today's path and today's values
        assert type(g) is Outline and same_outline(g, o)
    assert DeviceOutlineOps("cuda").trace([], 1) == []
    empty = DeviceOutlineOps("cuda").trace([(torch.zeros(5, 7, device="cuda"), 0, THR, 0)], 1.5)
    assert len(empty) == 1 and len(empty[0]) == 0 and empty[0].size == (5, 7) and empty[0].tolerance == 1.5
    for bad in (-1, float("nan"), 1024.5):
        with pytest.raises(ValueError):
            DeviceOutlineOps("cuda").trace(items, bad)
    with pytest.raises(ValueError):                                          # a side above 8191: refused before any launch
        DeviceOutlineOps("cuda").trace([(torch.zeros(1, 8192, device="cuda"), 0, THR, 0)], 1)


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    buf = torch.full((4096,), 1, device="cuda", dtype=torch.int32)          # a launch on this buffer would write the totals {0, 0, 1, 0}
    p = buf.data_ptr()
    assert p % 16 == 0

    def call(points=p, offsets=p + 256, item_loops=p + 512, n=1, V=8, loop_max=2, t=4, form=1, work=p + 1024, work_len=2048,
             out_points=p + 10240, cap=8, out_offsets=p + 11264, loop_cap=3, out_hole=p + 11776, firsts=p + 12288):
        with pytest.raises(_lib.VpuError, match="outline_simplify_batched"):
            _lib.call("vpu_outline_simplify_batched", points, offsets, item_loops, n, V, loop_max, t, form, work, work_len, out_points,
                      cap, out_offsets, loop_cap, out_hole, firsts, None)

    call(points=None)
    call(offsets=None)
    call(item_loops=None)
    call(firsts=None)
    call(out_points=None)
    call(out_offsets=None)
    call(out_hole=None)
    call(work=None)
    call(n=0)
    call(n=-1)
    call(V=-1)
    call(loop_max=-1)
    call(cap=-1)
    call(loop_cap=-1)
    call(t=-1)
    call(t=4097)
    call(form=2)
    call(form=-1)
    call(work_len=ops.outline_simplify_work_len(8, 2) - 1)
    call(work=p + 1024 + 8)
    call(points=p + 4)
    call(out_points=p + 10240 + 4)
    call(offsets=p + 256 + 4)
    call(out_offsets=p + 11264 + 4)
    call(item_loops=p + 512 + 2)
    call(firsts=p + 12288 + 2)
    torch.cuda.synchronize()
    assert bool((buf == 1).all())                                            # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the pools
TOL = 1.0


def _pool(dtype):
    from test_crops_gpu import _tiny
    model = _tiny(dtype)
    zoom = dict(skip_clicks=-1, target_size=(IMG, IMG))
    ann = AnnotationPool(get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), max_images=2)
    assert isinstance(ann.ops_outlines, DeviceOutlineOps) and isinstance(ann.pool.ops_outlines, DeviceOutlineOps)
    assert ann.pool.flip and ann.pool.zoom is not None
    return ann


IMAGES = [(240, 300, 3), (IMG, IMG, 4)]


class _Pair:
    """The device pool and its twin driven together: every call goes to both, the device pool's result is returned."""

    def __init__(self, pools):
        self.pools = pools

    def __getattr__(self, name):
        def call(*args, **kwargs):
            got, refused = [], None
            for p in self.pools:
                try:
                    got.append(getattr(p, name)(*args, **kwargs))
                except KeyError as e:           # (reopen of a label that is covered: both refuse alike)
                    refused = e
            if refused is not None:
                assert not got
                raise refused
            return got[0]
        return call


def _s6(polygons, outline, where):
    """S6 of a device result against the exact outline of the same call: the kept points are the exact ones at the stand-in's
    kept positions, and every exact vertex lies within the tolerance of the segment over its position."""
    t = int(polygons.tolerance * 4)
    kept, alive, _, _ = simplify_loops(outline.points, outline.offsets, t) if len(outline) else (np.zeros(0, dtype=bool),) * 4
    assert np.array_equal(polygons.points, outline.points[kept]) and len(polygons) == int(np.sum(alive)), where
    assert polygons.source == (len(outline.points), len(outline)) and polygons.dropped == len(outline) - len(polygons), where
    kept_of = [np.flatnonzero(kept[a:b]).tolist() if ok else None for a, b, ok in zip(outline.offsets[:-1], outline.offsets[1:], alive)]
    assert_s6(outline, kept_of, t, where)
    polygons.check()


def _script(ann, twin):
    """The script on ``ann`` and, side by side, on ``twin`` (None: ``ann`` alone); after every call the tolerance calls of the
    two against each other, and ``ann``'s against its own exact outlines."""
    steps = []

    def check(where, aids, masks):
        steps.append(where)
        before = ann.readbacks
        exact = ann.pool.mask_outlines(aids)
        polys = ann.pool.mask_outlines(aids, tolerance=TOL)
        assert ann.readbacks == before + 2 + 3, where
        host = twin.pool.mask_outlines(aids, tolerance=TOL) if twin else None
        for aid in aids:
            assert host is None or same_polygons(polys[aid], host[aid]), (where, aid)
            _s6(polys[aid], exact[aid], (where, aid))
            before = ann.readbacks
            exact_l = ann.label_outlines(aid, tolerance=None)
            got = ann.label_outlines(aid, tolerance=TOL)
            assert ann.readbacks == before + (5 if got else 0) and list(got) == list(exact_l), (where, aid)
            other = twin.label_outlines(aid, tolerance=TOL) if twin else None
            for label, p in got.items():
                assert other is None or same_polygons(p, other[label]), (where, aid, label)
                _s6(p, exact_l[label], (where, aid, label))
            before = ann.readbacks
            out = ann.export(aid, True, tolerance=TOL)
            assert ann.readbacks == before + (5 if out else 0), (where, aid)
            assert twin is None or out == twin.export(aid, True, tolerance=TOL), (where, aid)
            committed = ann.label_outlines(aid, preview=False) if out else {}
            for e in out:
                p = committed[e["label"]].simplify(TOL)
                assert e["polygons"] == p.to_coco() and e["polygon_holes"] == int(p.holes().sum()), (where, aid, e["label"])
                assert e["polygon_tolerance"] == TOL and e["polygon_dropped"] == p.dropped, (where, aid, e["label"])

    run_pool_script(_Pair([ann, twin] if twin else [ann]), [blob_image(H, W, seed=s) for H, W, s in IMAGES], check)
    assert len(steps) == 14 and all(ann.object_count(aid) == 3 for aid in range(2))


def _host_twin(dtype):
    twin = _pool(dtype)
    twin.ops_outlines = twin.pool.ops_outlines = HostOutlineOps()
    return twin


def test_pools_fp32_equal_the_host_ops_after_every_call():
    _need_gpu()
    _script(_pool("f32"), _host_twin("f32"))


def test_pools_bf16_satisfy_s6_against_their_own_outlines():
    _need_gpu()
    _script(_pool("bf16"), None)
