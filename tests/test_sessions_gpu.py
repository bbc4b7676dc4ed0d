"""GPU: ``vpu_session_paste_batched`` (csrc/evalbatch.hip) against ``ZoomIn.inv_transform`` and the host stand-in, and
``SessionPool`` on the device path against one private predictor per session: ViT-B in the fp32 engine mode bit for bit,
bf16 within the frozen click-logit bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference import sessions
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool
from pvpuformer_amd.isegm.inference.transforms import Roi, ZoomIn

from sessions_cases import PRED_THR, StubNet, Twin, assert_equal, blob_image, step

pytestmark = pytest.mark.gpu

BOX_THR = 0.5
SIZES = [(5, 7), (64, 64), (33, 130), (127, 129)]   # fewer pixels than a wave; whole words; H * W % 4 != 0; H * W % 64 != 0
MAP = 32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _roi(kind, H, W):
    if kind == "copy" and H >= MAP and W >= MAP:          # exactly the map's size: the copy path
        r0, c0 = min(1, H - MAP), min(3, W - MAP)
        return Roi(r0, r0 + MAP - 1, c0, c0 + MAP - 1)
    return {"whole": Roi.whole(H, W), "copy": Roi.whole(H, W), "interior": Roi(1, H - 2, 1, W - 2),
            "two corners": Roi(0, H // 2, 0, W - 1), "one row": Roi(H // 2, H // 2, 1, W - 2)}[kind]


def _maps():
    """One 32 x 32 map per size: low values, a block above both thresholds, and single pixels AT the thresholds, which the
    strict comparisons must leave out of the mask (0.49) and out of the box (0.5)."""
    g = torch.Generator().manual_seed(7)
    probs = torch.rand(len(SIZES), 1, MAP, MAP, generator=g) * 0.3
    probs[:, 0, 9:21, 12:25] = 0.6 + 0.4 * torch.rand(len(SIZES), 12, 13, generator=g)
    probs[:, 0, 2, 3:6] = PRED_THR
    probs[:, 0, 1, 28] = BOX_THR
    probs[:, 0, 30, 1] = BOX_THR
    probs[2, 0, 9:21, 12:25] = 0.2                        # one session with an empty box
    probs[2, 0, 1, 28] = probs[2, 0, 30, 1] = 0.1
    return probs


def _launch(members, rois, probs, form):
    """One launch over ``members`` (indices into SIZES) -> per member (canvas, int64 record + words as read back)."""
    from pvpuformer_amd import _lib, ops
    layout = sessions._Round([type("S", (), dict(sid=j, H=SIZES[j][0], W=SIZES[j][1])) for j in members])
    out = torch.full((layout.size,), -1, device="cuda", dtype=torch.int64)      # (stale bits everywhere)
    canvases, desc = [], []
    for k, (j, roi) in enumerate(zip(members, rois)):
        H, W = SIZES[j]
        canvases.append(torch.full((H, W), 7.0, device="cuda"))
        assert canvases[-1].data_ptr() % 16 == 0 and 0 <= roi[0] <= roi[1] < H and 0 <= roi[2] <= roi[3] < W
        d = _lib.SessionObj()
        d.canvas, d.bits, d.rec = canvases[-1].data_ptr(), out.data_ptr() + 8 * layout.at[j], out.data_ptr() + 32 * k
        d.H, d.W = H, W
        d.r0, d.r1, d.c0, d.c1 = roi
        d.src = j
        desc.append(d)
    raw = bytes((_lib.SessionObj * len(desc))(*desc))
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    ops.session_paste_batched(dev, len(desc), probs, MAP, MAP, PRED_THR, BOX_THR, max(SIZES[j][0] * SIZES[j][1] for j in members),
                              form=form)
    got = out.cpu().numpy()
    res = []
    for k, j in enumerate(members):
        H, W = SIZES[j]
        res.append((canvases[k], got[4 * k:4 * k + 4].view(np.int32), got[layout.at[j]:layout.at[j] + sessions.n_words(H * W)]))
    return res


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", [4, 1])
def test_session_paste_kernel(n, form):
    _need_gpu()
    from pvpuformer_amd import _lib
    assert C.sizeof(_lib.SessionObj) == 56                 # 3 pointers + 8 int32, as the C struct
    probs_host = _maps()
    probs = probs_host.cuda()
    launches = [list(range(len(SIZES)))] if n == 4 else [[j] for j in range(len(SIZES))]
    for kind in ("whole", "interior", "two corners", "one row", "copy"):
        for members in launches:
            rois = [_roi(kind, *SIZES[j]) for j in members]
            for j, roi, (canvas, rec, words) in zip(members, rois, _launch(members, rois, probs, form)):
                H, W = SIZES[j]
                tag = (kind, n, form, (H, W))
                # the canvas: ZoomIn.inv_transform's, bit for bit (as test_roi_paste_batched_equals_inv_transform_iou_and_box)
                z = ZoomIn(target_size=(MAP, MAP))
                z._object_roi, z._probs = roi, torch.zeros(1, 1, H, W, device="cuda")
                want = z.inv_transform(probs[j:j + 1])
                assert torch.equal(canvas, want[0, 0]), tag
                # bits, padding, area and box: exactly those of the kernel's own canvas
                values = canvas.cpu().numpy()
                mask = values > np.float32(PRED_THR)
                assert np.array_equal(words.view(np.uint64), sessions.pack_mask(mask)), tag
                if H * W % 64:
                    assert int(words.view(np.uint64)[-1]) >> (H * W % 64) == 0, tag
                assert np.array_equal(sessions.unpack_mask(words, H, W), mask), tag
                on = np.argwhere(values > np.float32(BOX_THR))
                box = [len(on), on[:, 0].min(), on[:, 0].max(), on[:, 1].min(), on[:, 1].max()] if len(on) else [0, H, -1, W, -1]
                assert rec.tolist() == [int(mask.sum())] + [int(v) for v in box] + [0, 0], tag
                # the host stand-in: the same record layout; its canvas is torch's interpolation of the same formula, whose
                # three roundings per pixel of values <= 1 stay below 1e-6; on the copy path it is the same bytes
                s_canvas, s_words, s_rec = sessions.host_session_paste(probs_host[j, 0], H, W, roi, PRED_THR, BOX_THR)
                assert np.abs(s_canvas.numpy() - values).max() < 1e-6, tag
                if (roi[1] - roi[0] + 1, roi[3] - roi[2] + 1) == (MAP, MAP):
                    assert np.array_equal(s_canvas.numpy(), values) and np.array_equal(s_words, words.view(np.uint64)), tag
                    assert s_rec.tolist() == rec.tolist(), tag
                    # the planted threshold values lie inside the roi, outside mask and box
                    r0, c0 = roi[0], roi[2]
                    assert values[r0 + 2, c0 + 4] == np.float32(PRED_THR) and not mask[r0 + 2, c0 + 4], tag
                    if j != 2:
                        assert values[r0 + 1, c0 + 28] == np.float32(BOX_THR) and mask[r0 + 1, c0 + 28], tag
                        assert rec[1:6].tolist() == [12 * 13, r0 + 9, r0 + 20, c0 + 12, c0 + 24], tag
                    else:
                        assert rec[1:6].tolist() == [0, H, -1, W, -1], tag


# ------------------------------------------------------------------------------------------------ end to end
def _vitb(dtype):
    from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model
    from pvpuformer_amd.synth import vitb_model_kwargs
    torch.manual_seed(0)
    model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
    model.set_compute_dtype(dtype)
    model.eval()
    model.weights_frozen = True
    return model


E2E_SIZES = [(448, 448), (480, 640), (333, 517)]


def _synth_image(H, W, seed):
    """(uint8 image [H, W, 3], (row, col) inside the first object) from pvpuformer_amd.synth, cropped to the size."""
    from pvpuformer_amd.synth import synth_batch
    b = synth_batch(1, max(H, W), seed=seed)
    image = (b["images"][0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    rows, cols = np.nonzero(b["instances"][0, 0, :H, :W].numpy() > 0)
    centre = (int(np.median(rows)), int(np.median(cols))) if len(rows) else (H // 2, W // 2)
    return image, centre


def _scenario(model, exact):
    """Four rounds on three sessions: all click; b idles; all click, a takes its click back and clicks elsewhere; all click.
    ``exact``: compare bit for bit after every call; else collect (pool map, private map, pool mask) per call."""
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    make = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom)
    pool = SessionPool(make(), max_sessions=4, pred_thr=PRED_THR)
    twins = []
    for j, (H, W) in enumerate(E2E_SIZES):
        image, centre = _synth_image(H, W, seed=60 + j)
        twins.append(Twin(pool, make, image))
        twins[-1].centre = centre
    a, b, c = twins
    log = []

    def run(live, where):
        res = step(live)
        if exact:
            assert_equal(live, res, where)
        for t in live:
            log.append((where, t.sid, pool.probs(t.sid)[0, 0].cpu().numpy().copy(), res[t.sid][1].copy(), res[t.sid][0]))

    for t in twins:
        t.add(True, t.centre)
    run(twins, "click 1")
    a.add(False, (5, 9))
    c.add(True, (min(c.centre[0] + 25, 332), max(c.centre[1] - 30, 0)))
    run([a, c], "click 2")
    assert torch.equal(pool.probs(b.sid), b.pred.prev_prediction) or not exact
    saved = a.save()
    a.add(True, (max(a.centre[0] - 30, 0), min(a.centre[1] + 20, 447)))
    b.add(False, (470, 630))
    c.add(False, (3, 500))
    run(twins, "click 3")
    a.restore(saved)
    a.add(False, (440, 440))
    run([a], "click 3 after undo")
    for t in twins:
        t.add(True, (max(t.centre[0] - 12, 0), max(t.centre[1] - 14, 0)))
    run(twins, "click 4")
    assert pool.readbacks == 5 and pool.forwards == 5       # every input is zoomed to 448 x 448: one forward per call
    return log


def test_end_to_end_fp32_pool_equals_private_predictors():
    _need_gpu()
    log = _scenario(_vitb("f32"), exact=True)
    assert len(log) == 12


def test_recalculation_on_the_device_path():
    """skip_clicks=0 with a stub network whose prediction is the bright blob: the small blobs' boxes cover less than half of
    the image, so those sessions run again, zoomed, inside the call (two read-backs); the large one does not.  The maps are
    the private predictors' bit for bit (the stub computes every sample alone)."""
    _need_gpu()
    make = lambda: get_predictor(StubNet(), "NoBRS", "cuda", with_flip=True,
                                 zoom_in_params=dict(skip_clicks=0, target_size=(64, 96), min_crop_size=12))
    pool = SessionPool(make(), max_sessions=3)
    twins = []
    for j, (H, W, radius) in enumerate([(120, 160, 0.12), (96, 96, 0.15), (96, 96, 0.45)]):
        image, centre = blob_image(H, W, seed=j, radius=radius)
        twins.append(Twin(pool, make, image))
        twins[-1].centre = centre
    for t in twins:
        t.add(True, t.centre)
    res = step(twins)
    assert (pool.readbacks, pool.forwards) == (2, 3)
    assert_equal(twins, res, "click 1")
    assert twins[0].pred.zoom_in._object_roi is not None and twins[2].pred.zoom_in._object_roi is None
    for t in twins:
        t.add(False, (2, 3))
    res = step(twins)
    assert pool.readbacks == 3
    assert_equal(twins, res, "click 2")


def test_end_to_end_bf16_close_to_private_predictors():
    """As test_end_to_end_bf16_close_to_sequential: bf16 is not compared bit for bit (the GEMM instantiation is chosen by row
    count, so a batch of 6 runs other kernels than a batch of 2).  Asserted: each session's first-click map stays within the
    frozen ViT-B click-logit bound of its private predictor's.  Printed: that figure for every call, and the mask IoU."""
    _need_gpu()
    from bf16_bounds import frozen_upper
    bound = frozen_upper("vitb click logits (budget test)")
    log = _scenario(_vitb("bf16"), exact=False)
    for where, sid, got, want, mask in log:
        err = np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-12)
        ref = want > PRED_THR
        iou = (mask & ref).sum() / max((mask | ref).sum(), 1)
        print(f"[bf16-bound] session {sid} {where}: map vs private predictor {err:.4g} (bound {bound:.4g}), mask IoU {iou:.4f}")
        if where == "click 1":
            assert err < bound
