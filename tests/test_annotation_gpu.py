"""GPU: ``vpu_annot_compose_batched`` / ``vpu_label_extract`` (csrc/evalbatch.hip, section 7) against the numpy stand-ins, and
``AnnotationPool`` on the device model against a twin pool whose compose and extract are the stand-ins.  Everything is max,
a strict compare and integer writes: equality is bit for bit."""
import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.annotation import (AnnotationPool, DeviceAnnotOps, HostAnnotOps, host_annot_compose,
                                                       host_label_extract)
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import n_words

from annotation_cases import THR, compose_case, run_script
from sessions_cases import blob_image

pytestmark = pytest.mark.gpu

# fewer pixels than a quad; H * W % 4 != 0; whole words; fewer than a wave's turn; H * W % 64 != 0; one turn; several blocks
SHAPES = [(1, 1), (3, 5), (8, 8), (5, 13), (17, 15), (16, 16), (47, 70), (33, 130), (127, 129)]
VARIANTS = ["both", "no add", "no total", "no labels"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
IMG = 224


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _launch(cases):
    """``cases``: [(H, W, mode, variant, label, seed)] in ONE launch, outputs pre-filled with a sentinel (one word more than each
    annotation owns) -> per case (words, rec, word past the end, total, labels, and the host's inputs)."""
    from pvpuformer_amd import _lib, ops
    n, at, size = len(cases), [], 4 * len(cases)
    for H, W, *_ in cases:
        at.append(size)
        size += n_words(H * W) + 1
    out = torch.full((size,), SENTINEL, device="cuda", dtype=torch.int64)
    rows, held = [], []
    for i, (H, W, mode, variant, label, seed) in enumerate(cases):
        add, total, labels = compose_case(H, W, seed)
        add, total, labels = (None if variant == "no add" else add, None if variant == "no total" else total,
                              None if variant == "no labels" else labels)
        dev = [None if v is None else torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for v in (add, total, labels)]
        d = _lib.AnnotObj()
        d.add, d.total, d.labels = (None if t is None else t.data_ptr() for t in dev)
        d.bits, d.rec = out.data_ptr() + 8 * at[i], out.data_ptr() + 32 * i
        d.H, d.W, d.label, d.mode = H, W, label, mode
        rows.append(d)
        held.append((dev, (add, total, labels)))
    desc = torch.frombuffer(bytearray(bytes((_lib.AnnotObj * n)(*rows))), dtype=torch.uint8).cuda()
    ops.annot_compose_batched(desc, n, THR, max(H * W for H, W, *_ in cases))
    got = out.cpu().numpy()
    results = []
    for i, (H, W, *_) in enumerate(cases):
        dev, host = held[i]
        words = got[at[i]:at[i] + n_words(H * W)].view(np.uint64)
        results.append((words, got[4 * i:4 * i + 4].view(np.int32), got[at[i] + n_words(H * W)],
                        None if dev[1] is None else dev[1].cpu().numpy(),
                        None if dev[2] is None else dev[2].cpu().numpy().view(np.uint16), host))
    return results


def _check(cases):
    for case, (words, rec, past, total, labels, (add, h_total, h_labels)) in zip(cases, _launch(cases)):
        H, W, mode, variant, label, seed = case
        before = None if h_labels is None else h_labels.copy()
        h_words, h_rec = host_annot_compose(add, h_total, h_labels, H, W, label, mode, THR)
        assert np.array_equal(words, h_words), case                         # (the bits past H * W are zero in both)
        assert np.array_equal(rec, h_rec), (case, rec, h_rec)
        assert past == SENTINEL, case
        assert total is None or np.array_equal(total, h_total), case
        if labels is not None:
            assert np.array_equal(labels, h_labels), case
            mask = np.maximum(add if add is not None else 0, h_total if h_total is not None else 0) > np.float32(THR)
            assert np.array_equal(labels[~mask], before[~mask]), case        # the pattern survives where the mask is clear
            assert mode & 2 or np.array_equal(labels, before), case


def _case(i, shape, mode):
    return (shape[0], shape[1], mode, VARIANTS[(i + mode) % 4], 65535 if (i + mode) % 3 == 0 else 3 + i, 100 * i + mode)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("at", range(len(SHAPES)), ids=[f"{h}x{w}" for h, w in SHAPES])
def test_compose_alone_equals_the_stand_in(at):
    _need_gpu()
    for mode in range(4):
        _check([_case(at, SHAPES[at], mode)])
        _check([(SHAPES[at][0], SHAPES[at][1], mode, "both", 65535, 7 * at + mode)])


def test_compose_of_nine_in_one_launch_equals_the_stand_in():
    _need_gpu()
    for turn in range(4):
        _check([_case(i, shape, (i + turn) % 4) for i, shape in enumerate(SHAPES)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extract_equals_the_stand_in(shape):
    _need_gpu()
    from pvpuformer_amd import ops
    H, W = shape
    for label in (7, 65535, 9):                                             # 9 is absent
        host = compose_case(H, W, seed=H + W)[2]
        labels = torch.from_numpy(host.view(np.int16).copy()).cuda()
        out = torch.full((H, W), -7.0, device="cuda")
        rec = torch.full((9,), -5, device="cuda", dtype=torch.int32)
        ops.label_extract(labels, label, out, rec)
        want, h_rec = host_label_extract(host, label)
        assert np.array_equal(out.cpu().numpy(), want), (shape, label)      # every pixel is written
        assert np.array_equal(labels.cpu().numpy().view(np.uint16), host), (shape, label)
        assert rec.cpu().numpy().tolist() == h_rec.tolist() + [-5], (shape, label)


def test_bad_arguments_are_refused():
    _need_gpu()
    from pvpuformer_amd import _lib
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    for args in ((p, 0, THR, 16), (p, 65536, THR, 16), (p, 1, THR, 0), (None, 1, THR, 16), (p, 1, float("nan"), 16)):
        with pytest.raises(_lib.VpuError, match="annot_compose"):
            _lib.call("vpu_annot_compose_batched", *args, None)
    for args in ((p, p, p, 0, 4, 1), (p, p, p, 4, 4, 0), (p, p, p, 4, 4, 65536), (p, None, p, 4, 4, 1),
                 (p + 2, p, p, 4, 4, 1), (p, p + 4, p, 4, 4, 1)):         # the last two: labels / out misaligned
        with pytest.raises(_lib.VpuError, match="label_extract"):
            _lib.call("vpu_label_extract", *args, None)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------- the pool
def _pools(dtype, twin):
    from test_crops_gpu import _tiny
    model = _tiny(dtype)
    zoom = dict(skip_clicks=-1, target_size=(IMG, IMG))
    make = lambda: AnnotationPool(get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), max_images=2)
    dev = make()
    assert isinstance(dev.ops, DeviceAnnotOps) and dev.pool.flip and dev.pool.zoom is not None
    host = None
    if twin:
        host = make()
        host.ops = HostAnnotOps()
    return dev, host


IMAGES = [(240, 300, 3), (IMG, IMG, 4)]


def test_pool_fp32_equals_the_stand_in_twin_after_every_call():
    _need_gpu()
    dev, host = _pools("f32", twin=True)
    log, reopened = run_script(dev, host, [blob_image(H, W, seed=s) for H, W, s in IMAGES], finite=True)
    assert len(log) == 14 and all(dev.object_count(aid) == 4 for aid in range(2))
    assert dev.forwards == host.forwards == dev.pool.forwards


def test_pool_bf16_runs():
    """No twin: the script runs, every map is finite, and the labels are those of the pool's own current_prob > prob_thresh."""
    _need_gpu()
    dev, _ = _pools("bf16", twin=False)
    log, _ = run_script(dev, None, [blob_image(H, W, seed=s) for H, W, s in IMAGES], finite=True)
    assert len(log) == 14 and all(dev.object_count(aid) == 4 for aid in range(2))
    for aid in range(2):
        assert [r["label"] for r in dev.objects(aid)][-1] == 4 and dev.label_map(aid).max() <= 4
