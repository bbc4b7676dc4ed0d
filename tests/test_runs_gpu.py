"""GPU: ``vpu_runs_count_batched`` / ``vpu_runs_write_batched`` (csrc/evalbatch.hip, section 8) against the numpy stand-in, and
the pools' three run-length calls on the device model against a twin pool whose run ops are the stand-in.  Everything is a
strict compare and integers: equality is element for element."""
import ctypes

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.runs import DeviceRunOps, HostRunOps, host_runs_encode

from runs_cases import PATTERNS, SHAPES, THR, case, run_pool_script, same_runs, shape_id
from sessions_cases import blob_image

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SPARE = 16
IMG = 224


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_WANT = {}


def _want(kind, name, shape):
    """(source array, the stand-in's RunMap), computed once."""
    key = (kind, name, shape)
    if key not in _WANT:
        src = case(kind, name, *shape)
        _WANT[key] = (src, host_runs_encode(src, kind, THR))
    return _WANT[key]


def _launch(cases, cap=None):
    """``cases``: [(kind, pattern, shape)] in ONE count call and ONE write call -> (header, entries of cap + SPARE rows, the
    true total).  The entry buffer is pre-filled with a sentinel; ``cap`` None: the true total."""
    from pvpuformer_amd import _lib, ops
    n = len(cases)
    held, rows = [], []
    for kind, name, shape in cases:
        src = _want(kind, name, shape)[0]
        # four elements past an allocation: exactly the 8-byte (labels) and 16-byte (fp32) alignment the pools guarantee
        flat = torch.from_numpy(src.view(np.int16) if kind == 1 else src).reshape(-1)
        room = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda")
        room[4:].copy_(flat)
        dev = room[4:].view(shape)
        assert room.data_ptr() % 32 == 0 and dev.data_ptr() % (8 if kind == 1 else 16) == 0 and dev.data_ptr() % 32 != 0
        d = _lib.RunsObj()
        d.src, d.H, d.W, d.kind, d.thr = dev.data_ptr(), shape[0], shape[1], kind, THR
        held.append(dev)
        rows.append(d)
    host = torch.frombuffer(bytearray(bytes((_lib.RunsObj * n)(*rows))), dtype=torch.uint8)
    desc = host.cuda()
    scratch = torch.empty(ops.runs_scratch_len([shape for _, _, shape in cases]), device="cuda", dtype=torch.int32)
    header = torch.full((n + 2,), SENTINEL, device="cuda", dtype=torch.int32)
    ops.runs_count_batched(desc, host, n, scratch, header)
    head = header.cpu().numpy()
    assert head[n + 1] == SENTINEL
    total = int(head[n])
    cap = total if cap is None else cap
    entries = torch.full((cap + SPARE, 2), SENTINEL, device="cuda", dtype=torch.int32)
    ops.runs_write_batched(desc, host, n, scratch, entries, cap)
    return head[:n + 1], entries.cpu().numpy(), total


def _check(cases, cap=None):
    head, entries, total = _launch(cases, cap)
    want = [_want(*c)[1] for c in cases]
    sums = np.concatenate(([0], np.cumsum([len(w) for w in want])))
    assert head.tolist() == sums.tolist(), (cases, head, sums)
    cap = total if cap is None else cap
    assert (entries[cap:] == SENTINEL).all(), cases                         # nothing at or beyond cap is touched
    for k, (c, w) in enumerate(zip(cases, want)):
        lo, hi = int(head[k]), min(int(head[k + 1]), cap)
        if lo >= hi:
            continue
        assert np.array_equal(entries[lo:hi, 0], w.starts[:hi - lo]), c
        assert np.array_equal(entries[lo:hi, 1], w.values[:hi - lo]), c
    return total


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_alone_equals_the_stand_in(shape, kind):
    _need_gpu()
    for name in PATTERNS:
        _check([(kind, name, shape)])


@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
def test_all_shapes_of_a_kind_in_one_launch(kind):
    _need_gpu()
    for turn in range(3):
        _check([(kind, PATTERNS[(i + 3 * turn + 5) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)])


def test_both_kinds_mixed_in_one_launch():
    _need_gpu()
    for turn in range(2):
        _check([((i + turn) % 2, PATTERNS[(i + turn + 2) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)])


def test_cap_below_the_total_keeps_the_counts_and_the_rest_of_the_buffer():
    _need_gpu()
    cases = [((i + 1) % 2, PATTERNS[(i + 2) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)]
    total = _check(cases)
    assert total > 64
    assert _check(cases, cap=total // 2) == total
    assert _check(cases, cap=0) == total
    assert _check([(1, "checkerboard", (33, 130))], cap=1000) == 33 * 130


def test_device_ops_equal_the_host_ops():
    _need_gpu()
    items, want = [], []
    for i, shape in enumerate(SHAPES):
        kind = i % 2
        src, rm = _want(kind, PATTERNS[(i + 6) % len(PATTERNS)], shape)
        items.append((torch.from_numpy(src.view(np.int16) if kind == 1 else src).cuda(), kind, THR))
        want.append(rm)
    got = DeviceRunOps("cuda").encode(items)
    host = HostRunOps().encode(items)
    assert len(got) == len(want) == len(host)
    for g, h, w in zip(got, host, want):
        assert same_runs(g, w) and same_runs(h, w)
    assert DeviceRunOps("cuda").encode([]) == []


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    buf = torch.zeros(4096, device="cuda", dtype=torch.int32)
    p = buf.data_ptr()
    assert p % 16 == 0

    def descs(*rows):
        made = []
        for src, H, W, kind in rows:
            d = _lib.RunsObj()
            d.src, d.H, d.W, d.kind, d.thr = src, H, W, kind, THR
            made.append(d)
        arr = (_lib.RunsObj * len(made))(*made)
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    good = (p, 4, 4, 0)
    bad_rows = [(None, 4, 4, 0), (p, 0, 4, 0), (p, 4, 0, 1), (p, 65536, 32768, 1), (p, 4, 4, 2), (p, 4, 4, -1),
                (p + 8, 4, 4, 0), (p + 4, 4, 4, 1), (p + 2, 4, 4, 1)]      # the last three: fp32 / labels misaligned
    for row in bad_rows:
        for rows in ((row,), (good, row)):
            keep, host = descs(*rows)
            with pytest.raises(_lib.VpuError, match="runs_count_batched"):
                _lib.call("vpu_runs_count_batched", p, host, len(rows), p, 4096, p, None)
            with pytest.raises(_lib.VpuError, match="runs_write_batched"):
                _lib.call("vpu_runs_write_batched", p, host, len(rows), p, 4096, p, 8, None)
    keep, host = descs(good)
    for n in (0, -1, 65536):
        with pytest.raises(_lib.VpuError, match="runs_count_batched"):
            _lib.call("vpu_runs_count_batched", p, host, n, p, 4096, p, None)
    with pytest.raises(_lib.VpuError, match="runs_count_batched"):
        _lib.call("vpu_runs_count_batched", None, host, 1, p, 4096, p, None)
    with pytest.raises(_lib.VpuError, match="runs_count_batched"):
        _lib.call("vpu_runs_count_batched", p, None, 1, p, 4096, p, None)
    with pytest.raises(_lib.VpuError, match="runs_count_batched"):
        _lib.call("vpu_runs_count_batched", p, host, 1, p, 3, p, None)             # scratch shorter than W * bands
    with pytest.raises(_lib.VpuError, match="runs_count_batched"):
        _lib.call("vpu_runs_count_batched", p, host, 1, p, 4096, None, None)
    with pytest.raises(_lib.VpuError, match="runs_write_batched"):
        _lib.call("vpu_runs_write_batched", p, host, 1, p, 4096, p, -1, None)       # cap < 0
    with pytest.raises(_lib.VpuError, match="runs_write_batched"):
        _lib.call("vpu_runs_write_batched", p, host, 1, p, 4096, p + 4, 8, None)    # entries misaligned
    with pytest.raises(_lib.VpuError, match="runs_write_batched"):
        _lib.call("vpu_runs_write_batched", p, host, 1, p, 4096, None, 8, None)
    torch.cuda.synchronize()
    assert not buf.any()                                                     # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the pools
def _pool(dtype):
    from test_crops_gpu import _tiny
    model = _tiny(dtype)
    zoom = dict(skip_clicks=-1, target_size=(IMG, IMG))
    ann = AnnotationPool(get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), max_images=2)
    assert isinstance(ann.ops_runs, DeviceRunOps) and isinstance(ann.pool.ops_runs, DeviceRunOps)
    assert ann.pool.flip and ann.pool.zoom is not None
    return ann


IMAGES = [(240, 300, 3), (IMG, IMG, 4)]


class _Pair:
    """The device pool and its twin driven together: every call goes to both, the device pool's result is returned."""

    def __init__(self, pools):
        self.pools = pools

    def __getattr__(self, name):
        def call(*args):
            got, refused = [], None
            for p in self.pools:
                try:
                    got.append(getattr(p, name)(*args))
                except KeyError as e:           # (reopen of a label that is covered: both refuse alike)
                    refused = e
            if refused is not None:
                assert not got
                raise refused
            return got[0]
        return call


def _script(ann, twin):
    """The script on ``ann`` and, side by side, on ``twin`` (None: ``ann`` alone); after every call the three run-length methods
    of the two against each other, and ``ann``'s against its own masks and label maps."""
    steps = []

    def check(where, aids, masks):
        steps.append(where)
        before = ann.readbacks
        runs = ann.pool.mask_runs(aids)
        assert ann.readbacks == before + 2, where
        host = twin.pool.mask_runs(aids) if twin else None
        for aid in aids:
            assert host is None or same_runs(runs[aid], host[aid]), (where, aid)
            thr = np.float32(ann.pool.pred_thr)
            assert np.array_equal(runs[aid].decode(), ann.pool.probs(aid)[0, 0].cpu().numpy() > thr), (where, aid)
            if masks is not None and where in ("click 1", "click 2"):          # no parts yet: the pool's mask is the object's
                assert np.array_equal(runs[aid].decode(), masks[aid]), (where, aid)
            for preview in (True, False):
                before = ann.readbacks
                rm = ann.label_runs(aid, preview)
                assert ann.readbacks == before + 2, (where, aid)
                assert twin is None or same_runs(rm, twin.label_runs(aid, preview)), (where, aid, preview)
                assert np.array_equal(rm.decode(), ann.label_map(aid, preview)), (where, aid, preview)
            out = ann.export(aid)
            assert twin is None or out == twin.export(aid), (where, aid)
            committed = ann.label_map(aid, False)
            assert [e["label"] for e in out] == [r["label"] for r in ann.objects(aid)], (where, aid)
            for e in out:
                assert e["segmentation"]["size"] == list(committed.shape), (where, aid)
                assert sum(e["segmentation"]["counts"][1::2]) == int((committed == e["label"]).sum()), (where, aid)

    run_pool_script(_Pair([ann, twin] if twin else [ann]), [blob_image(H, W, seed=s) for H, W, s in IMAGES], check)
    assert len(steps) == 13 and all(ann.object_count(aid) == 3 for aid in range(2))


def _host_twin(dtype):
    twin = _pool(dtype)
    twin.ops_runs = twin.pool.ops_runs = HostRunOps()
    return twin


def test_pools_fp32_equal_the_host_ops_after_every_call():
    _need_gpu()
    _script(_pool("f32"), _host_twin("f32"))


def test_pools_bf16_decode_to_their_own_maps():
    _need_gpu()
    _script(_pool("bf16"), None)
