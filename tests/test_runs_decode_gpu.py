"""GPU: ``vpu_runs_decode_batched`` (csrc/evalbatch.hip, section 9) against the numpy stand-in at the launcher's edges, the way
round through the encoder without the host in between, and ``AnnotationPool.load`` / ``set_mask`` / ``prev_masks`` in run-length
form on the device model against a twin pool whose run ops are the stand-in.  The values are integers and 0 / 1: equality is
element for element.  Only valid streams reach the kernel; that a malformed one stays inside its buffers is read from the code."""
import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.runs import DeviceRunOps, HostRunOps, RunMap, host_runs_decode, host_runs_encode

from runs_cases import B, C, PATTERNS, SHAPES, THR, case, shape_id, values_of
from sessions_cases import blob_image

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL_16 = 0x5A5A
SENTINEL_F = -7.0
SPARE = 16
IMG = 224


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_RUNS = {}


def _runs(name, shape):
    """(label values uint16 [H, W] from {0, 1, 2, 65535}, their RunMap), computed once."""
    key = (name, shape)
    if key not in _RUNS:
        v = case(1, name, *shape)
        _RUNS[key] = (v, host_runs_encode(v, 1).check())
    return _RUNS[key]


def _room(shape, kind):
    """A sentinel-filled ``dst`` four elements into its allocation -- exactly the 16-byte (fp32) / 8-byte (labels) alignment the
    contract asks for -- with SPARE elements behind it -> (the whole allocation, dst)."""
    n = shape[0] * shape[1]
    room = (torch.full((4 + n + SPARE,), SENTINEL_F, dtype=torch.float32, device="cuda") if kind == 0 else
            torch.full((4 + n + SPARE,), SENTINEL_16, dtype=torch.int16, device="cuda"))
    dst = room[4:4 + n].view(shape)
    assert room.data_ptr() % 32 == 0 and dst.data_ptr() % (16 if kind == 0 else 8) == 0 and dst.data_ptr() % 32 != 0
    return room, dst


def _margins_intact(room, shape, kind):
    n = shape[0] * shape[1]
    edge = torch.cat((room[:4], room[4 + n:])).cpu().numpy()
    return bool((edge == (np.float32(SENTINEL_F) if kind == 0 else np.int16(SENTINEL_16))).all())


def _descs(rows):
    """[(dst pointer, entries pointer, H, W, n_runs, kind, label)] -> (host tensor of the descriptors, its device copy)."""
    from pvpuformer_amd import _lib
    made = []
    for dst, entries, H, W, n_runs, kind, label in rows:
        d = _lib.UnrunObj()
        d.dst, d.entries, d.H, d.W, d.n_runs, d.kind, d.label, d.pad = dst, entries, H, W, n_runs, kind, label, 0
        made.append(d)
    host = torch.frombuffer(bytearray(bytes((_lib.UnrunObj * len(made))(*made))), dtype=torch.uint8)
    return host, host.cuda()


def _check(cases):
    """``cases``: [(kind, pattern, shape, label)] decoded in ONE launch; every dst against the stand-in, its margins and the
    entries buffer (with a spare tail) intact."""
    from pvpuformer_amd import ops
    maps = [_runs(name, shape)[1] for _, name, shape, _ in cases]
    at = np.concatenate(([0], np.cumsum([len(rm) for rm in maps])))
    flat = np.full((int(at[-1]) + SPARE, 2), SENTINEL, dtype=np.int32)
    for rm, lo in zip(maps, at):
        flat[lo:lo + len(rm), 0], flat[lo:lo + len(rm), 1] = rm.starts, rm.values
    entries = torch.from_numpy(flat).cuda()
    rooms, rows = [], []
    for (kind, name, shape, label), rm, lo in zip(cases, maps, at):
        room, dst = _room(shape, kind)
        rooms.append((room, dst))
        rows.append((dst.data_ptr(), entries.data_ptr() + 8 * int(lo), shape[0], shape[1], len(rm), kind, label))
    host, desc = _descs(rows)
    ops.runs_decode_batched(desc, host, len(cases))
    for (kind, name, shape, label), rm, (room, dst) in zip(cases, maps, rooms):
        want = host_runs_decode(rm, kind, label)
        got = dst.cpu().numpy()
        assert np.array_equal(got.view(np.uint16) if kind == 1 else got, want), (kind, name, shape, label)
        assert _margins_intact(room, shape, kind), (kind, name, shape, label)
    assert np.array_equal(entries.cpu().numpy(), flat), cases                # the decoder writes nothing but dst


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", [0, 1], ids=["mask", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_alone_equals_the_stand_in(shape, kind):
    _need_gpu()
    for name in PATTERNS:
        # kind 1 does not read the label: any value passes the wrapper
        _check([(kind, name, shape, 1 if kind == 0 else -5)])


@pytest.mark.parametrize("shape", [(47, 70), (127, 129), (2 * B + 1, 3), (3, 2 * C + 1), (1, 1)], ids=shape_id)
def test_mask_of_an_absent_label_of_65535_and_of_the_background(shape):
    _need_gpu()
    for name in ("random", "boundary", "zero"):
        v = _runs(name, shape)[0]
        assert not (v == 7).any() and (name == "zero" or shape == (1, 1) or (v == 65535).any())
        _check([(0, name, shape, 7), (0, name, shape, 65535), (0, name, shape, 0), (0, name, shape, 2)])


@pytest.mark.parametrize("kind", [0, 1], ids=["mask", "labels"])
def test_all_shapes_of_a_kind_in_one_launch(kind):
    _need_gpu()
    for turn in range(3):
        _check([(kind, PATTERNS[(i + 3 * turn + 5) % len(PATTERNS)], shape, (1, 2, 65535)[turn]) for i, shape in enumerate(SHAPES)])


def test_both_kinds_mixed_in_one_launch():
    _need_gpu()
    for turn in range(2):
        _check([((i + turn) % 2, PATTERNS[(i + turn + 2) % len(PATTERNS)], shape, 1 + i % 2) for i, shape in enumerate(SHAPES)])


def test_encode_then_decode_on_the_device():
    """``vpu_runs_write_batched``'s entries go straight into the decoder: only the 4 (n + 1) offsets visit the host."""
    _need_gpu()
    from pvpuformer_amd import _lib, ops
    cases = [(i % 2, PATTERNS[(i + 1) % len(PATTERNS)], shape) for i, shape in enumerate(SHAPES)]
    n = len(cases)
    srcs, made = [], []
    for kind, name, shape in cases:
        src = case(kind, name, *shape)
        dev = torch.from_numpy(src.view(np.int16) if kind == 1 else src).cuda()
        d = _lib.RunsObj()
        d.src, d.H, d.W, d.kind, d.thr = dev.data_ptr(), shape[0], shape[1], kind, THR
        srcs.append((src, dev))
        made.append(d)
    host = torch.frombuffer(bytearray(bytes((_lib.RunsObj * n)(*made))), dtype=torch.uint8)
    desc = host.cuda()
    scratch = torch.empty(ops.runs_scratch_len([shape for _, _, shape in cases]), device="cuda", dtype=torch.int32)
    header = torch.empty(n + 1, device="cuda", dtype=torch.int32)
    ops.runs_count_batched(desc, host, n, scratch, header)
    at = header.cpu().numpy()
    entries = torch.empty(int(at[n]), 2, device="cuda", dtype=torch.int32)
    ops.runs_write_batched(desc, host, n, scratch, entries)
    rooms, rows = [], []
    for k, (kind, name, shape) in enumerate(cases):
        room, dst = _room(shape, kind)
        rooms.append((room, dst))
        rows.append((dst.data_ptr(), entries.data_ptr() + 8 * int(at[k]), shape[0], shape[1], int(at[k + 1] - at[k]), kind, 1))
    uhost, udesc = _descs(rows)
    ops.runs_decode_batched(udesc, uhost, n)
    for (kind, name, shape), (src, _), (room, dst) in zip(cases, srcs, rooms):
        v = values_of(src, kind)
        got = dst.cpu().numpy()
        if kind == 1:
            assert np.array_equal(got.view(np.uint16), v), (name, shape)
        else:
            assert np.array_equal(got, v.astype(np.float32)), (name, shape)
        assert _margins_intact(room, shape, kind), (name, shape)


def test_device_ops_equal_the_host_ops():
    _need_gpu()
    items, twins = [], []
    for i, shape in enumerate(SHAPES):
        kind = i % 2
        rm = _runs(PATTERNS[(i + 6) % len(PATTERNS)], shape)[1]
        dtype = torch.float32 if kind == 0 else torch.int16
        label = (1, 65535, 2, 7)[i % 4]
        items.append((rm, torch.full(shape, 3, dtype=dtype, device="cuda"), kind, label))
        twins.append((rm, torch.full(shape, 3, dtype=dtype), kind, label))
    assert DeviceRunOps("cuda").decode(items) is None
    HostRunOps().decode(twins)
    for (rm, got, kind, label), (_, want, _, _) in zip(items, twins):
        assert np.array_equal(got.cpu().numpy(), want.numpy()), (rm.size, kind, label)
        assert np.array_equal(want.numpy().view(np.uint16) if kind == 1 else want.numpy(), host_runs_decode(rm, kind, label))
    onto = torch.full((47, 70), 3, dtype=torch.int16, device="cuda")        # the host ops write a device map as well
    HostRunOps().decode([(_runs("random", (47, 70))[1], onto, 1, 0)])
    assert np.array_equal(onto.cpu().numpy().view(np.uint16), _runs("random", (47, 70))[0])
    assert DeviceRunOps("cuda").decode([]) is None
    bad = RunMap((3, 4), [0, 5, 5], [0, 1, 2])
    dst = torch.full((3, 4), 3, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):                                          # a malformed stream never reaches the kernel
        DeviceRunOps("cuda").decode([(bad, dst, 1, 0)])
    assert (dst == 3).all()


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    buf = torch.full((4096,), SENTINEL, device="cuda", dtype=torch.int32)
    ent = torch.tensor([[0, 1], [5, 0]], device="cuda", dtype=torch.int32)
    p, e = buf.data_ptr(), ent.data_ptr()
    assert p % 16 == 0 and e % 8 == 0

    def refused(rows, n=None, objs=p, null_host=False):
        host, _ = _descs(rows)
        with pytest.raises(_lib.VpuError, match="runs_decode_batched"):
            _lib.call("vpu_runs_decode_batched", objs, None if null_host else host.data_ptr(), len(rows) if n is None else n, None)

    good = (p, e, 4, 4, 2, 0, 1)
    bad_rows = [(None, e, 4, 4, 2, 0, 1), (p, None, 4, 4, 2, 0, 1), (p, e, 0, 4, 2, 0, 1), (p, e, 4, 0, 2, 1, 1),
                (p, e, 65536, 32768, 1, 1, 0),                              # H * W == 2^31
                (p, e, 4, 4, 0, 0, 1), (p, e, 4, 4, -1, 1, 1), (p, e, 4, 4, 17, 1, 1),      # n_runs outside 1 .. H * W
                (p, e, 4, 4, 2, 2, 1), (p, e, 4, 4, 2, -1, 1),              # the kind
                (p, e, 4, 4, 2, 0, -1), (p, e, 4, 4, 2, 0, 65536),          # kind 0: the label
                (p + 8, e, 4, 4, 2, 0, 1), (p + 4, e, 4, 4, 2, 1, 1), (p + 2, e, 4, 4, 2, 1, 1),   # dst: fp32 / labels misaligned
                (p, e + 4, 4, 4, 2, 0, 1), (p, e + 4, 4, 4, 1, 1, 1)]       # entries misaligned
    for row in bad_rows:
        refused([row])
        refused([good, row])
    for n in (0, -1, 65536):
        refused([good], n=n)
    refused([good], objs=None)
    refused([good], null_host=True)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                           # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the pools
IMAGES = [(240, 300, 3), (IMG, IMG, 4)]


def _pool(dtype, host_runs=False):
    from test_crops_gpu import _tiny
    model = _tiny(dtype)
    zoom = dict(skip_clicks=-1, target_size=(IMG, IMG))
    ann = AnnotationPool(get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), max_images=2)
    assert isinstance(ann.ops_runs, DeviceRunOps) and isinstance(ann.pool.ops_runs, DeviceRunOps)
    assert ann.pool.flip and ann.pool.zoom is not None
    if host_runs:
        ann.ops_runs = ann.pool.ops_runs = HostRunOps()
    return ann


def _ellipse(H, W, cy, cx, ry, rx):
    rr, cc = np.mgrid[0:H, 0:W]
    return ((rr - cy) / ry) ** 2 + ((cc - cx) / rx) ** 2 <= 1.0


def _objects(H, W):
    """Binary RunMaps: two overlapping ellipses, one that the next covers, an empty one."""
    masks = [_ellipse(H, W, 0.4 * H, 0.4 * W, 0.3 * H, 0.25 * W), _ellipse(H, W, 0.55 * H, 0.6 * W, 0.3 * H, 0.3 * W),
             _ellipse(H, W, 0.3 * H, 0.3 * W, 0.1 * H, 0.1 * W), _ellipse(H, W, 0.3 * H, 0.3 * W, 0.2 * H, 0.2 * W),
             np.zeros((H, W), dtype=bool)]
    return masks, [host_runs_encode(m.astype(np.uint16), 1) for m in masks]


def _paint(masks):
    out = np.zeros(masks[0].shape, dtype=np.uint16)
    for k, m in enumerate(masks):
        out[m] = k + 1
    return out


def _same(ann, twin, aids, where):
    for aid in aids:
        for preview in (True, False):
            assert np.array_equal(ann.label_map(aid, preview), twin.label_map(aid, preview)), (where, aid, preview)
        assert ann.objects(aid) == twin.objects(aid) and ann.object_count(aid) == twin.object_count(aid), (where, aid)
        assert np.array_equal(ann.current_prob(aid).cpu().numpy(), twin.current_prob(aid).cpu().numpy()), (where, aid)


def _script(ann, twin):
    """load, set_mask in run-length form, a click with ``prev_masks`` in run-length form and an export -> load round trip on
    ``ann`` and, side by side, on ``twin`` (None: ``ann`` alone)."""
    pools = [p for p in (ann, twin) if p is not None]
    images = [blob_image(H, W, seed=s) for H, W, s in IMAGES]
    aids = [ann.open(image) for image, _ in images]
    assert twin is None or [twin.open(image) for image, _ in images] == aids
    committed = {}
    for aid, (image, centre) in zip(aids, images):
        H, W = image.shape[:2]
        masks, maps = _objects(H, W)
        given = [rm if k % 2 == 0 else dict(label=40 + k, segmentation=rm.to_coco()) for k, rm in enumerate(maps)]
        before = ann.readbacks
        records = [p.load(aid, given) for p in pools][0]
        assert ann.readbacks == before and [r["label"] for r in records] == [1, 2, 3, 4, 5]
        assert [r["area"] for r in records] == [int(m.sum()) for m in masks] and ann.object_count(aid) == 5
        assert np.array_equal(ann.label_map(aid), _paint(masks)), aid
        assert np.array_equal(ann.label_runs(aid).decode(), ann.label_map(aid)), aid
    if twin:
        _same(ann, twin, aids, "load")
    for aid, (image, centre) in zip(aids, images):
        H, W = image.shape[:2]
        v = np.zeros((H, W), dtype=np.uint16)
        v[_ellipse(H, W, 0.7 * H, 0.3 * W, 0.15 * H, 0.2 * W)] = 65535
        v[:5] = 1
        rm = host_runs_encode(v, 1)
        before = ann.readbacks
        for p in pools:
            p.set_mask(aid, rm if aid == aids[0] else rm.to_coco(65535), label=65535)
        assert ann.readbacks == before
        assert np.array_equal(ann.current_prob(aid)[0, 0].cpu().numpy(), (v == 65535).astype(np.float32)), aid
    if twin:
        _same(ann, twin, aids, "set_mask")
    clicks = {aid: (True, (int(0.7 * image.shape[0]), int(0.3 * image.shape[1]))) for aid, (image, _) in zip(aids, images)}
    got = [p.click(clicks) for p in pools]
    for aid in aids:
        assert got[0][aid].any() and (twin is None or np.array_equal(got[0][aid], got[1][aid])), aid
    for p in pools:
        for aid in aids:
            assert p.finish(aid)["label"] == 6
    if twin:
        _same(ann, twin, aids, "click and finish on the mask")
    # prev_masks in run-length form, on the pools' sessions directly
    clickers, prev = {}, {}
    for aid, (image, centre) in zip(aids, images):
        H, W = image.shape[:2]
        clickers[aid] = Clicker(device=None)
        clickers[aid].add_click(Click(True, centre))
        rm = host_runs_encode(_ellipse(H, W, centre[0], centre[1], 0.2 * H, 0.2 * W).astype(np.uint16), 1)
        prev[aid] = rm if aid == aids[1] else rm.to_coco()
    got = [p.pool.predict(clickers, prev_masks=prev) for p in pools]
    for aid in aids:
        assert twin is None or np.array_equal(got[0][aid], got[1][aid]), aid
        assert twin is None or np.array_equal(ann.pool.probs(aid).cpu().numpy(), twin.pool.probs(aid).cpu().numpy()), aid
    # export -> load on a fresh annotation of the same image
    for aid, (image, centre) in zip(aids, images):
        out = ann.export(aid)
        assert twin is None or out == twin.export(aid)
        committed = ann.label_map(aid, False)
        for p in pools:
            p.close(aid)
            assert p.open(image) == aid
            before = p.readbacks
            records = p.load(aid, out, keep_labels=True)
            assert p.readbacks == before
        assert [r["label"] for r in records] == [e["label"] for e in out] == [1, 2, 3, 4, 5, 6] and ann.object_count(aid) == 6
        assert np.array_equal(ann.label_map(aid), committed), aid
        assert np.array_equal(ann.label_runs(aid).decode(), committed), aid
        assert [e["segmentation"] for e in ann.export(aid)] == [e["segmentation"] for e in out], aid
    if twin:
        _same(ann, twin, aids, "export -> load")


def test_pools_fp32_equal_the_host_ops():
    _need_gpu()
    _script(_pool("f32"), _pool("f32", host_runs=True))


def test_pools_bf16_decode_to_their_own_maps():
    _need_gpu()
    _script(_pool("bf16"), None)
