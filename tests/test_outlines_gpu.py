"""GPU: ``vpu_outline_count_batched`` / ``vpu_outline_trace_batched`` (csrc/outline.hip) against the numpy stand-in, and the
pools' outline calls on the device model against a twin pool whose outline ops are the stand-in.  Everything is a strict
compare and integers: equality is element for element."""
import ctypes

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.outlines import DeviceOutlineOps, HostOutlineOps, host_outline
from pvpuformer_amd.isegm.inference.predictors import get_predictor

from outline_cases import PATTERNS, SHAPES, THR, case, run_pool_script, same_outline, shape_id
from sessions_cases import blob_image

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GARBAGE = -0x12345679
SPARE = 16
IMG = 224


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_WANT = {}


def _want(kind, name, shape):
    """The stand-in's Outline of a case, computed once per pattern and shape."""
    key = (name, tuple(shape))
    if key not in _WANT:
        _WANT[key] = host_outline(case(kind, name, shape)[3])
    return _WANT[key]


def _launch(cases, cap=None, loop_cap=None):
    """``cases``: [(kind, pattern, shape)] in ONE count call and ONE trace call -> (header, points of cap + SPARE rows, offsets of
    loop_cap + SPARE entries, item_loops of n + 2 entries).  Every output is pre-filled with a sentinel and both scratch arrays
    with garbage; ``cap`` / ``loop_cap`` None: the true totals."""
    from pvpuformer_amd import _lib, ops
    n = len(cases)
    held, rows = [], []
    for kind, name, shape in cases:
        src, thr, label = case(kind, name, shape)[:3]
        # four elements past an allocation: exactly the 8-byte (labels) and 16-byte (fp32) alignment the pools guarantee
        flat = torch.from_numpy(src.view(np.int16) if kind == 1 else src).reshape(-1)
        room = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda")
        room[4:].copy_(flat)
        dev = room[4:].view(shape)
        assert room.data_ptr() % 32 == 0 and dev.data_ptr() % (8 if kind == 1 else 16) == 0 and dev.data_ptr() % 32 != 0
        d = _lib.OutlineObj()
        d.src, d.H, d.W, d.kind, d.thr, d.label, d.pad = dev.data_ptr(), shape[0], shape[1], kind, thr, label, 0
        held.append((room, room.clone()))
        rows.append(d)
    host = torch.frombuffer(bytearray(bytes((_lib.OutlineObj * n)(*rows))), dtype=torch.uint8)
    desc = host.cuda()
    scratch = torch.full((ops.outline_scratch_len([shape for _, _, shape in cases]),), GARBAGE, device="cuda", dtype=torch.int32)
    header = torch.full((n + 2,), SENTINEL, device="cuda", dtype=torch.int32)
    ops.outline_count_batched(desc, host, n, scratch, header)
    head = header.cpu()
    assert int(head[n + 1]) == SENTINEL
    V = int(head[n])
    loops = sum(len(_want(*c)) for c in cases)
    cap = V if cap is None else cap
    loop_cap = loops + 1 if loop_cap is None else loop_cap
    work = torch.full((ops.outline_work_len(V),), GARBAGE, device="cuda", dtype=torch.int32)
    points = torch.full((cap + SPARE, 2), SENTINEL, device="cuda", dtype=torch.int32)
    offsets = torch.full((loop_cap + SPARE,), SENTINEL, device="cuda", dtype=torch.int32)
    item_loops = torch.full((n + 2,), SENTINEL, device="cuda", dtype=torch.int32)
    ops.outline_trace_batched(desc, host, n, scratch, header, head[:n + 1].contiguous(), work, points, offsets, item_loops, cap, loop_cap)
    torch.cuda.synchronize()
    for room, before in held:
        assert torch.equal(room, before)                                     # the sources are as they were
    return head.numpy()[:n + 1], points.cpu().numpy(), offsets.cpu().numpy(), item_loops.cpu().numpy()


def _check(cases, cap=None, loop_cap=None):
    head, points, offsets, item_loops = _launch(cases, cap, loop_cap)
    want = [_want(*c) for c in cases]
    n = len(cases)
    sums = np.concatenate(([0], np.cumsum([len(w.points) for w in want])))
    assert head.tolist() == sums.tolist(), (cases, head, sums)              # the header holds the true counts whatever the caps
    V, L = int(sums[-1]), sum(len(w) for w in want)
    cap = V if cap is None else cap
    loop_cap = L + 1 if loop_cap is None else loop_cap
    assert (points[cap:] == SENTINEL).all() and (offsets[loop_cap:] == SENTINEL).all(), cases    # nothing at or beyond a cap
    assert item_loops[n + 1] == SENTINEL, cases
    if V == 0:                                                               # no corner anywhere: nothing was launched
        assert (points == SENTINEL).all() and (offsets == SENTINEL).all() and (item_loops == SENTINEL).all(), cases
        return V, L
    all_points = np.concatenate([w.points for w in want])
    all_offsets = np.concatenate([w.offsets[:-1] + s for w, s in zip(want, sums)] + [[V]])
    first = np.concatenate(([0], np.cumsum([len(w) for w in want])))
    assert np.array_equal(points[:cap], all_points[:cap]), cases
    assert np.array_equal(offsets[:loop_cap], all_offsets[:loop_cap]), cases
    assert item_loops[:n + 1].tolist() == first.tolist(), cases
    return V, L


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_alone_equals_the_stand_in(shape, kind):
    _need_gpu()
    for name in PATTERNS:
        _check([(kind, name, shape)])


@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
def test_all_cases_of_a_kind_in_one_launch(kind):
    _need_gpu()
    for turn in range(len(PATTERNS)):                                        # every pattern at every shape, SHAPES items a launch
        _check([(kind, PATTERNS[(i + turn) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)])
    _check([(kind, name, shape) for shape in SHAPES for name in PATTERNS])          # and all 270 cases in one


def test_both_kinds_mixed_in_one_launch():
    _need_gpu()
    for turn in range(4):
        _check([((i + turn) % 2, PATTERNS[(3 * i + turn) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)])
    _check([(0, "zero", (3, 65)), (1, "absent", (33, 5)), (1, "zero", (1, 1))])     # no corner in any item


def test_caps_below_the_totals_keep_the_counts_and_the_rest_of_the_buffers():
    _need_gpu()
    cases = [((i + 1) % 2, PATTERNS[(i + 2) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)]
    V, L = _check(cases)
    assert V > 64 and L > 8
    assert _check(cases, cap=V // 2, loop_cap=(L + 1) // 2) == (V, L)
    assert _check(cases, cap=0, loop_cap=0) == (V, L)
    assert _check(cases, cap=V, loop_cap=L) == (V, L)                        # all loops, not the closing offset
    assert _check([(1, "checkerboard0", (33, 130))], cap=1000, loop_cap=3)[0] > 4000


def test_device_ops_equal_the_host_ops():
    _need_gpu()
    items, want = [], []
    for i, shape in enumerate(SHAPES):
        kind, name = i % 2, PATTERNS[(i + 6) % len(PATTERNS)]
        src, thr, label = case(kind, name, shape)[:3]
        items.append((torch.from_numpy(src.view(np.int16) if kind == 1 else src).cuda(), kind, thr, label))
        want.append(_want(kind, name, shape))
    got = DeviceOutlineOps("cuda").trace(items)
    host = HostOutlineOps().trace(items)
    assert len(got) == len(want) == len(host)
    for g, h, w in zip(got, host, want):
        assert same_outline(g, w) and same_outline(h, w)
        g.check()
    assert DeviceOutlineOps("cuda").trace([]) == []
    empty = DeviceOutlineOps("cuda").trace([(torch.zeros(5, 7, device="cuda"), 0, THR, 0)])
    assert len(empty) == 1 and len(empty[0]) == 0 and empty[0].size == (5, 7)


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    ONE = 0x3F800000                         # 1.0f: a launch on this buffer would find corners and write other words
    buf = torch.full((4096,), ONE, device="cuda", dtype=torch.int32)
    p = buf.data_ptr()
    assert p % 16 == 0

    def descs(*rows):
        made = []
        for src, H, W, kind, thr, label in rows:
            d = _lib.OutlineObj()
            d.src, d.H, d.W, d.kind, d.thr, d.label, d.pad = src, H, W, kind, thr, label, 0
            made.append(d)
        arr = (_lib.OutlineObj * len(made))(*made)
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    def count(host, n=1, objs=p, scratch=p, scratch_len=4096, header=p):
        with pytest.raises(_lib.VpuError, match="outline_count_batched"):
            _lib.call("vpu_outline_count_batched", objs, host, n, scratch, scratch_len, header, None)

    head1 = (ctypes.c_int32 * 2)(0, 4)
    head2 = (ctypes.c_int32 * 3)(0, 4, 8)

    def trace(host, n=1, objs=p, scratch=p, scratch_len=4096, header=p, host_header=head1, work=p, work_len=2048, points=p,
              cap=8, offsets=p, loop_cap=8, item_loops=p):
        hh = None if host_header is None else ctypes.cast(host_header, ctypes.c_void_p)
        with pytest.raises(_lib.VpuError, match="outline_trace_batched"):
            _lib.call("vpu_outline_trace_batched", objs, host, n, scratch, scratch_len, header, hh, work, work_len, points, cap,
                      offsets, loop_cap, item_loops, None)

    good = (p, 4, 4, 0, THR, 0)
    bad_rows = [(None, 4, 4, 0, THR, 0), (p, 0, 4, 0, THR, 0), (p, 4, 0, 1, THR, 1), (p, 32767, 32767, 1, THR, 1),
                (p, 4, 4, 2, THR, 1), (p, 4, 4, -1, THR, 1), (p, 4, 4, 1, THR, -1), (p, 4, 4, 1, THR, 65536),
                (p, 4, 4, 0, -0.1, 0), (p, 4, 4, 0, 1.0, 0), (p, 4, 4, 0, float("nan"), 0),
                (p + 8, 4, 4, 0, THR, 0), (p + 4, 4, 4, 1, THR, 1), (p + 2, 4, 4, 1, THR, 1)]   # the last three: misaligned
    for row in bad_rows:
        for rows in ((row,), (good, row)):
            keep, host = descs(*rows)
            count(host, len(rows))
            trace(host, len(rows), host_header=head1 if len(rows) == 1 else head2)
    keep, host = descs((p, 23170, 23170, 1, THR, 1), (p, 23170, 23170, 1, THR, 1))   # each below 2^31 lattice slots, not both
    count(host, 2)
    trace(host, 2, host_header=head2)
    keep, host = descs(good)
    for n in (0, -1, 65536):
        count(host, n)
        trace(host, n)
    count(host, objs=None)
    count(None)
    count(host, scratch_len=9)                                               # 5 x 1 row slots and 5 x 1 column slots
    count(host, scratch=None)
    count(host, header=None)
    trace(host, objs=None)
    trace(None)
    trace(host, scratch_len=9)
    trace(host, scratch=None)
    trace(host, header=None)
    trace(host, host_header=None)
    trace(host, host_header=(ctypes.c_int32 * 2)(0, 51))                     # more corners than 2 x 5 x 5
    trace(host, host_header=(ctypes.c_int32 * 2)(1, 4))
    trace(host, host_header=(ctypes.c_int32 * 2)(0, -4))
    trace(host, work=None)
    trace(host, work_len=16 * 4 + 1)
    trace(host, work=p + 8)
    trace(host, cap=-1)
    trace(host, loop_cap=-1)
    trace(host, points=None)
    trace(host, points=p + 4)
    trace(host, offsets=None)
    trace(host, offsets=p + 4)
    trace(host, item_loops=None)
    torch.cuda.synchronize()
    assert bool((buf == ONE).all())                                          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the pools
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


def _script(ann, twin):
    """The script on ``ann`` and, side by side, on ``twin`` (None: ``ann`` alone); after every call the outline methods of the
    two against each other, and ``ann``'s against its own masks and label maps."""
    steps = []

    def check(where, aids, masks):
        steps.append(where)
        before = ann.readbacks
        outlines = ann.pool.mask_outlines(aids)
        assert ann.readbacks == before + 2, where
        host = twin.pool.mask_outlines(aids) if twin else None
        for aid in aids:
            assert host is None or same_outline(outlines[aid], host[aid]), (where, aid)
            thr = np.float32(ann.pool.pred_thr)
            assert np.array_equal(outlines[aid].decode(), ann.pool.probs(aid)[0, 0].cpu().numpy() > thr), (where, aid)
            if masks is not None and where in ("click 1", "click 2"):          # no parts yet: the pool's mask is the object's
                assert np.array_equal(outlines[aid].decode(), masks[aid]), (where, aid)
            for preview in (True, False):
                before = ann.readbacks
                got = ann.label_outlines(aid, preview=preview)
                assert ann.readbacks == before + (2 if got else 0), (where, aid)
                want = ann.label_map(aid, preview)
                assert (set(np.unique(want).tolist()) - {0}) | {r["label"] for r in ann.objects(aid)} <= set(got), (where, aid)
                other = twin.label_outlines(aid, preview=preview) if twin else None
                for label, o in got.items():
                    assert other is None or same_outline(o, other[label]), (where, aid, preview, label)
                    assert np.array_equal(o.check().decode(), want == label), (where, aid, preview, label)
            out = ann.export(aid, True)
            assert twin is None or out == twin.export(aid, True), (where, aid)
            committed = ann.label_map(aid, False)
            assert [e["label"] for e in out] == [r["label"] for r in ann.objects(aid)], (where, aid)
            for e in out:
                o = host_outline(committed == e["label"])
                assert e["polygons"] == o.to_coco() and e["polygon_holes"] == int(o.holes().sum()), (where, aid, e["label"])

    run_pool_script(_Pair([ann, twin] if twin else [ann]), [blob_image(H, W, seed=s) for H, W, s in IMAGES], check)
    assert len(steps) == 14 and all(ann.object_count(aid) == 3 for aid in range(2))


def _host_twin(dtype):
    twin = _pool(dtype)
    twin.ops_outlines = twin.pool.ops_outlines = HostOutlineOps()
    return twin


def test_pools_fp32_equal_the_host_ops_after_every_call():
    _need_gpu()
    _script(_pool("f32"), _host_twin("f32"))


def test_pools_bf16_decode_to_their_own_maps():
    _need_gpu()
    _script(_pool("bf16"), None)
