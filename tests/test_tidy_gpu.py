"""GPU: ``vpu_regions_tidy_batched`` (csrc/evalbatch.hip, section 9) against the numpy + scipy stand-in on every case of
tidy_cases.py, each alone and all of them in one launch, with sentinels around the outputs; its bad-argument returns; and
``SessionPool.tidy`` / ``AnnotationPool.tidy`` on the device model against twin pools whose ``ops_regions`` is the stand-in.
Union-find, integer atomics and two constant edits: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.regions import (INT32_MAX, KEEP_MODES, DeviceRegionOps, HostRegionOps, TidyItem,
                                                    host_regions_tidy)
from pvpuformer_amd.isegm.inference.sessions import SessionPool, n_words

from sessions_cases import blob_image
from tidy_cases import (SHAPES, THR, SessionTwin, bits_equal, call_args, cases, maps_of, run_annotation_script, run_session_script,
                        shape_id)
from tidy_ref import tidy_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
MAP_SENTINEL = -7.0
IMG = 224
ERR_ARG, ERR_ALIGN = -1, -2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _launch(todo, outputs=(True, True), inputs=(True, True)):
    """``todo``: cases of tidy_cases in ONE launch; records, packed words and one word more per item pre-filled with a sentinel,
    the output maps too, the scratch with garbage -> per case (add_out, total_out, words, rec) as the stand-in returns them."""
    from pvpuformer_amd import _lib, ops
    n, at, size = len(todo), [], 4 * len(todo)
    for case in todo:
        at.append(size)
        size += n_words(case["H"] * case["W"]) + 1
    out = torch.full((size,), SENTINEL, device="cuda", dtype=torch.int64)
    scratch_at, ints = [], 0
    for case in todo:
        scratch_at.append(ints)
        ints += (ops.tidy_scratch_ints(case["H"] * case["W"]) + 3) // 4 * 4
    scratch = torch.full((ints,), 0x5A5A5A5A, device="cuda", dtype=torch.int32)
    rows, held = [], []
    for i, case in enumerate(todo):
        src = [torch.from_numpy(case[name]).cuda() if use else None for name, use in zip(("add", "total"), inputs)]
        dst = [torch.full_like(t, MAP_SENTINEL) if t is not None and want else None for t, want in zip(src, outputs)]
        seeds = torch.tensor(case["seeds"], dtype=torch.int64).reshape(-1, 3).to(torch.int32).cuda() if case["seeds"] else None
        d = _lib.TidyObj()
        d.add, d.total, d.add_out, d.total_out = (None if t is None else t.data_ptr() for t in src + dst)
        d.bits, d.rec = out.data_ptr() + 8 * at[i], out.data_ptr() + 32 * i
        d.seeds, d.n_seeds = (None if seeds is None else seeds.data_ptr()), len(case["seeds"])
        d.scratch = scratch.data_ptr() + 4 * scratch_at[i]
        d.H, d.W, d.min_area, d.keep = case["H"], case["W"], case["min_area"], KEEP_MODES[case["keep"]]
        d.max_hole = INT32_MAX if case["max_hole"] is None else case["max_hole"]
        rows.append(d)
        held.append((src, dst, seeds))
    host = torch.frombuffer(bytearray(bytes((_lib.TidyObj * n)(*rows))), dtype=torch.uint8)
    ops.regions_tidy_batched(host.cuda(), host, n, THR)
    got = out.cpu().numpy()
    results = []
    for i, case in enumerate(todo):
        src, dst, _ = held[i]
        nw = n_words(case["H"] * case["W"])
        assert got[at[i] + nw] == SENTINEL, (i, case["name"], "the word past the item's packed words")
        for t, name, use in zip(src, ("add", "total"), inputs):
            assert not use or bits_equal(t.cpu().numpy(), case[name]), (i, case["name"], "an input map was written")
        results.append((*(None if t is None else t.cpu().numpy() for t in dst), got[at[i]:at[i] + nw].view(np.uint64),
                        got[4 * i:4 * i + 4].view(np.int32)))
    return results


def _check(todo, outputs=(True, True), inputs=(True, True)):
    for case, got in zip(todo, _launch(todo, outputs, inputs)):
        where = (case["H"], case["W"], case["name"], case["seeds"], case["min_area"], case["max_hole"], case["keep"], outputs, inputs)
        want = host_regions_tidy(*call_args(case, add=inputs[0], total=inputs[1]))
        assert np.array_equal(got[2], want[2]), where
        assert np.array_equal(got[3], want[3]), (where, got[3], want[3])
        for k in range(2):
            if outputs[k] and inputs[k]:
                assert bits_equal(got[k], want[k]), where
            else:
                assert got[k] is None


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_kernel_alone_equals_the_stand_in(shape):
    _need_gpu()
    for case in cases(shape):
        _check([case])


def test_kernel_on_all_shapes_in_one_launch_equals_the_stand_in():
    _need_gpu()
    _check([case for shape in SHAPES for case in cases(shape)])


def test_largest_tie_goes_to_the_first_component_in_raster_order():
    _need_gpu()
    M = np.zeros((5, 5), dtype=bool)
    M[0, 3:5] = True                        # two components of two pixels; this one comes first
    M[2:4, 0] = True
    M[4, 4] = True
    add, total = maps_of(M, np.random.RandomState(1))
    todo = [dict(name=f"tie {seeds}", H=5, W=5, add=add, total=total, seeds=seeds, min_area=99, max_hole=0, keep="largest")
            for seeds in ([], [(4, 4, True)], [(3, 0, True), (0, 0, False)])]
    _check(todo)
    got = _launch(todo)
    assert [int(g[3][7]) for g in got] == [1, 2, 2] and [int(g[3][0]) for g in got] == [2, 3, 4]
    assert got[0][2][0] == (1 << 3) | (1 << 4)


def test_absent_maps():
    """A NULL add_out / total_out is not written, a NULL add / total reads as zeros."""
    _need_gpu()
    todo = [cases(shape)[k] for shape in SHAPES for k in (3, 11)]
    for outputs in ((True, False), (False, True), (False, False)):
        _check(todo, outputs=outputs)
    _check(todo, inputs=(True, False))
    _check(todo, inputs=(False, True))


def test_region_ops_equal_the_stand_in():
    """``DeviceRegionOps.tidy`` and ``HostRegionOps.tidy`` side by side, an output in place included."""
    _need_gpu()
    todo = [cases(shape)[k] for shape in SHAPES for k in (0, 5, 9)]
    results = []
    for ops in (DeviceRegionOps("cuda"), HostRegionOps()):
        items = []
        for case in todo:
            add, total = torch.from_numpy(case["add"]).cuda(), torch.from_numpy(case["total"]).cuda()
            items.append(TidyItem(case["H"], case["W"], add=add, total=total, add_out=add, total_out=torch.empty_like(total),
                                  seeds=case["seeds"], min_area=case["min_area"], max_hole=case["max_hole"], keep=case["keep"]))
        results.append((items, ops.tidy(items, THR, "masks")))
    (dev_items, dev), (host_items, host) = results
    for case, a, b, (rec_a, mask_a), (rec_b, mask_b) in zip(todo, dev_items, host_items, dev, host):
        assert np.array_equal(rec_a, rec_b) and np.array_equal(mask_a, mask_b), case["name"]
        assert torch.equal(a.add_out, b.add_out) and torch.equal(a.total_out, b.total_out), case["name"]
        assert bits_equal(a.total.cpu().numpy(), case["total"]), case["name"]


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(256, device="cuda", dtype=torch.int32)
    p = buf.data_ptr()

    def call(n=1, thr=THR, **fields):
        d = _lib.TidyObj()
        d.add, d.add_out, d.bits, d.rec, d.scratch = p, p + 256, p + 512, p + 640, p + 768
        d.H, d.W, d.keep = 2, 2, 0
        for name, value in fields.items():
            setattr(d, name, value)
        rows = (_lib.TidyObj * max(n, 1))(*([d] * max(n, 1)))
        return lib.vpu_regions_tidy_batched(p, ctypes.addressof(rows), n, ctypes.c_float(thr), None)

    for bad in (dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(add=None), dict(min_area=-1),
                dict(max_hole=-1), dict(keep=3), dict(keep=-1), dict(thr=1.0), dict(thr=-0.25), dict(thr=float("nan")),
                dict(n_seeds=-1), dict(n_seeds=1), dict(bits=None), dict(rec=None), dict(scratch=None)):
        assert call(**bad) == ERR_ARG, bad
        assert b"regions_tidy_batched" in lib.vpu_last_error(), bad
    for bad in (dict(add=p + 4), dict(total=p + 8), dict(add_out=p + 260), dict(total_out=p + 12), dict(bits=p + 516),
                dict(rec=p + 642), dict(scratch=p + 776), dict(seeds=p + 2, n_seeds=1)):
        assert call(**bad) == ERR_ALIGN, bad
    torch.cuda.synchronize()
    assert not buf.any()                    # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- the pools
IMAGES = [(120, 150, 3), (100, 96, 4)]


def _predictor(dtype):
    from test_crops_gpu import _tiny
    return get_predictor(_tiny(dtype), "NoBRS", "cuda", with_flip=True, zoom_in_params=dict(skip_clicks=-1, target_size=(IMG, IMG)))


def _annotation_pools(dtype, twin):
    dev = AnnotationPool(_predictor(dtype), max_images=2)
    assert isinstance(dev.ops_regions, DeviceRegionOps) and dev.pool.flip and dev.pool.zoom is not None
    host = None
    if twin:
        host = AnnotationPool(_predictor(dtype), max_images=2)
        host.ops_regions = HostRegionOps()
    return dev, host


def test_annotation_pool_fp32_equals_the_stand_in_twin_after_every_call():
    _need_gpu()
    dev, host = _annotation_pools("f32", twin=True)
    log = run_annotation_script(dev, host, [blob_image(H, W, seed=s) for H, W, s in IMAGES], finite=True)
    assert len([w for w, _ in log if w.startswith("tidy")]) == 8 and all(dev.object_count(aid) == 3 for aid in range(2))
    assert dev.forwards == host.forwards and dev.readbacks == host.readbacks


def test_session_pool_fp32_equals_the_stand_in_twin():
    _need_gpu()
    pools = [SessionPool(_predictor("f32"), max_sessions=2) for _ in range(2)]
    pools[1].ops_regions = HostRegionOps()
    assert isinstance(pools[0].ops_regions, DeviceRegionOps)
    images = [blob_image(H, W, seed=s)[0] for H, W, s in IMAGES]
    results = [_drive_sessions(pool, images) for pool in pools]
    for (masks_a, probs_a), (masks_b, probs_b) in zip(*results):
        for sid in masks_a:
            assert np.array_equal(masks_a[sid], masks_b[sid]) and torch.equal(probs_a[sid], probs_b[sid]), sid


class _Bare:
    """A SessionTwin without a private predictor: the pool alone."""

    def __init__(self, pool, image):
        from pvpuformer_amd.isegm.inference.clicker import Clicker
        self.pool, self.sid, self.clicker = pool, pool.open(image), Clicker(device=None)
        self.H, self.W = image.shape[:2]

    click = SessionTwin.click


def _drive_sessions(pool, images):
    """run_session_script on the pool alone -> [(masks, probs)] after every ``tidy`` and at the end."""
    twins, seen = [_Bare(pool, image) for image in images], []
    tidy = pool.tidy

    def recorded(*args, **kw):
        got = tidy(*args, **kw)
        seen.append((got, {t.sid: pool.probs(t.sid).clone() for t in twins}))
        return got

    pool.tidy = recorded
    run_session_script(pool, twins, exact=False)
    seen.append(({}, {t.sid: pool.probs(t.sid).clone() for t in twins}))
    assert len(seen) == 4 and all(torch.isfinite(p).all() for _, probs in seen for p in probs.values())
    return seen


def test_pools_bf16_run():
    """No twin: the scripts run, every map is finite, and every mask ``tidy`` returns is tidy_ref applied to the pool's own
    ``current_prob > prob_thresh`` from before the call."""
    _need_gpu()
    dev, _ = _annotation_pools("bf16", twin=False)
    checked = []

    def on_tidy(where, aid, before, mask, kw):
        a = dev._ann(aid)
        seeds = [(c.coords[0], c.coords[1], c.is_positive) for c in a.clicker.get_clicks()]
        ref = tidy_ref(before, None, a.H, a.W, seeds, kw.get("min_area", 0), kw.get("max_hole", 0), kw.get("keep", "all"), dev.prob_thresh)
        assert np.array_equal(mask, ref["mask"]), (where, aid)
        assert np.array_equal(mask, dev.current_prob(aid)[0, 0].cpu().numpy() > np.float32(dev.prob_thresh)), (where, aid)
        checked.append(where)

    run_annotation_script(dev, None, [blob_image(H, W, seed=s) for H, W, s in IMAGES], finite=True, on_tidy=on_tidy)
    assert len(checked) == 16
    _drive_sessions(SessionPool(_predictor("bf16"), max_sessions=2), [blob_image(H, W, seed=s)[0] for H, W, s in IMAGES])
