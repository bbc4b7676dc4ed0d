"""GPU: the batched NoBRS evaluation (isegm/inference/batched.py, csrc/evalbatch.hip) against the sequential loop.
Each batched kernel equals the sequential chain it replaces bit for bit (resize + flip, ZoomIn paste + get_iou + box,
Clicker keys), and ViT-B in the fp32 engine mode gives the same clicks and IoU series with K objects per forward as one
at a time."""
import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference import batched, vpu_evaluation
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.transforms import AddHorizontalFlip, Roi, ZoomIn, crop_resize
from pvpuformer_amd.isegm.inference.vpu_evaluation import evaluate_dataset, evaluate_sample

pytestmark = pytest.mark.gpu

SIZES = [(448, 448), (480, 640), (375, 500), (333, 517)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _objects(n, seed):
    """n objects cycling through SIZES, random image / previous prediction / ground truth (with -1 regions)."""
    g = torch.Generator().manual_seed(seed)
    objs = []
    for j in range(n):
        H, W = SIZES[j % len(SIZES)]
        gt = (torch.rand(H, W, generator=g) < 0.3).numpy().astype(np.int32)
        gt[H // 3:H // 3 + 7, :] = -1
        image = torch.rand(3, H, W, generator=g).cuda()
        o = batched._Object(j, image, gt, "cuda")
        o.canvas[0].copy_(torch.rand(H, W, generator=g))
        objs.append(o)
    return objs


def _rois(H, W, j):
    """ROIs touching each border in turn, and the whole image."""
    return [Roi(0, H // 2, 10, W // 2 + 40), Roi(H // 3, H - 1, W // 4, W // 4 + 220), Roi(20, H - 31, 0, 190),
            Roi(5, 300, W - 250, W - 1), Roi.whole(H, W)][j % 5]


@pytest.mark.parametrize("K", [1, 3, 8])
def test_roi_resize_batched_equals_crop_resize_and_flip(K):
    _need_gpu()
    objs = _objects(K, seed=K)
    ops = batched._DeviceOps("cuda")
    ops.begin(K)
    rois = [_rois(o.H, o.W, j + K) for j, o in enumerate(objs)]
    for j, (o, roi) in enumerate(zip(objs, rois)):
        ops.add(o, roi, j, j)
    ops.upload()
    got = ops.resize(objs, 0, K, (448, 448), True, 4)
    straight = [crop_resize(torch.cat((o.image[None], o.canvas[0][None, None]), 1), roi, (448, 448))
                for o, roi in zip(objs, rois)]
    want, _ = AddHorizontalFlip().transform(torch.cat(straight, 0), [[] for _ in objs])
    assert torch.equal(got, want)
    # a crop of the output size itself is copied (the 448 x 448 whole image)
    o = _objects(1, seed=0)[0]
    ops.begin(1)
    ops.add(o, Roi.whole(448, 448), 0, 0)
    ops.upload()
    got = ops.resize([o], 0, 1, (448, 448), False, 4)
    assert torch.equal(got[0], torch.cat((o.image, o.canvas[0][None]), 0))


def test_roi_paste_batched_equals_inv_transform_iou_and_box():
    _need_gpu()
    K = 8
    objs = _objects(K, seed=11)
    rois = [_rois(o.H, o.W, j) for j, o in enumerate(objs)]
    g = torch.Generator().manual_seed(5)
    probs = torch.rand(K, 1, 448, 448, generator=g)
    probs[1, 0, 100:110, 200:300] = 0.49      # values at the thresholds
    probs[2, 0, 10:20, 30:40] = 0.5
    probs[3] = 0.0                            # an empty prediction
    probs = probs.cuda()
    ops = batched._DeviceOps("cuda")
    ops.begin(K)
    for j, (o, roi) in enumerate(zip(objs, rois)):
        ops.add(o, roi, j, j)
    ops.upload()
    ops.paste(objs, 0, K, probs, 0.49, 0.5)
    out = ops.readback()
    from pvpuformer_amd.isegm.inference import utils
    for j, (o, roi) in enumerate(zip(objs, rois)):
        z = ZoomIn(target_size=(448, 448))
        z._object_roi, z._probs = roi, torch.zeros(1, 1, o.H, o.W, device="cuda")
        want = z.inv_transform(probs[j:j + 1])
        canvas = o.canvas[1 - o.prev]
        assert torch.equal(canvas, want[0, 0]), j
        mask = want[0, 0].cpu().numpy() > 0.49
        assert torch.equal(o.mask.cpu(), torch.from_numpy(mask.astype(np.uint8)))
        gt = np.where(o.valid.cpu().numpy() != 0, o.gt.cpu().numpy().astype(np.int32), -1)
        stats = out[j, 2:].view(np.int32)
        keep, obj = gt != -1, gt == 1
        assert stats[0] == np.logical_and(np.logical_and(mask, obj), keep).sum()
        assert stats[1] == np.logical_and(np.logical_or(mask, obj), keep).sum()
        assert np.int64(stats[0]) / np.int64(stats[1]) == utils.get_iou(gt, mask)
        clicks = [(roi[0] + 3, roi[2] + 1), (roi[1], roi[3])]
        box = list(stats[2:7])
        for r, c in clicks:
            box[1:] = [min(box[1], r), max(box[2], r), min(box[3], c), max(box[4], c)]
        assert tuple(int(v) for v in box) == T._device.mask_box(want, 0.5, clicks), j


def test_click_keys_batched_equal_clicker_keys():
    """Objects of four sizes in one launch (the canvas is padded to the largest), each with its own not-clicked map."""
    _need_gpu()
    K = 6
    objs = _objects(K, seed=3)
    g = torch.Generator().manual_seed(9)
    ops = batched._DeviceOps("cuda")
    ops.begin(K)
    clickers = []
    for j, o in enumerate(objs):
        gt = np.where(o.valid.cpu().numpy() != 0, o.gt.cpu().numpy().astype(np.int32), -1)
        # blobby masks: a smoothed noise field thresholded
        noise = torch.nn.functional.avg_pool2d(torch.rand(1, 1, o.H, o.W, generator=g), 31, 1, 15)[0, 0]
        pred = (noise > noise.median()).numpy()
        gt_blob = (torch.nn.functional.avg_pool2d(torch.rand(1, 1, o.H, o.W, generator=g), 41, 1, 20)[0, 0] > 0.5).numpy()
        gt = np.where(gt == -1, -1, gt_blob.astype(np.int32))
        o.gt.copy_(torch.from_numpy((gt == 1).astype(np.uint8)))
        o.mask.copy_(torch.from_numpy(pred.astype(np.uint8)))
        clicker = Clicker(gt_mask=gt, device="cuda")
        for r, c in [(o.H // 2, o.W // 2), (7, 9), (o.H - 1, o.W - 1)][:j % 4]:
            clicker.add_click(Click(True, (r, c)))
            o.keep[r, c] = 0
        if j == 1:                              # the click of this step: cleared by the kernel itself
            r, c = 40, 50
            clicker.add_click(Click(False, (r, c)))
            o.clear_at = r * o.W + c
        clickers.append((clicker, pred))
        ops.add(o, Roi.whole(o.H, o.W), 0, j)
    ops.upload()
    ops.keys(objs, 0, K)
    out = ops.readback()
    for j, (o, (clicker, pred)) in enumerate(zip(objs, clickers)):
        want = clicker._deepest_errors_device(pred, True)
        got = [batched.decode_key(out[j, e], o.W) for e in (0, 1)]
        assert got == want, (j, got, want)
        assert torch.equal(o.keep.cpu().bool(), torch.from_numpy(clicker.not_clicked_map)), j


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


class _Sample:
    def __init__(self, image, masks):
        self.image, self._masks = image, masks
        self.objects_ids = list(range(len(masks)))

    def gt_mask(self, oid):
        return self._masks[oid]


class _Dataset:
    def __init__(self, samples):
        self.samples = samples

    def __len__(self):
        return len(self.samples)

    def get_sample(self, i):
        return self.samples[i]


def _synth_dataset(sizes, per_image=2, seed=0):
    """Images and objects from pvpuformer_amd.synth, cropped to each size; one object per image carries a -1 band."""
    from pvpuformer_amd.synth import synth_batch
    samples = []
    for i, (H, W) in enumerate(sizes):
        b = synth_batch(per_image, max(H, W), seed=seed + i)
        image = (b["images"][0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
        masks = []
        for k in range(per_image):
            gt = b["instances"][k, 0, :H, :W].numpy().astype(np.int32)
            if k == 1:
                gt[H // 2:H // 2 + 9, :] = -1
            masks.append(gt)
        samples.append(_Sample(image, masks))
    return _Dataset(samples)


def _sequential(ds, pred, **kw):
    out = []
    for i in range(len(ds)):
        s = ds.get_sample(i)
        for oid in s.objects_ids:
            clicks, ious, probs = evaluate_sample(s.image, s.gt_mask(oid), pred, **kw)
            out.append(([(c.is_positive, int(c.coords[0]), int(c.coords[1])) for c in clicks], ious, probs))
    return out


def _batched(ds, pred, K, **kw):
    runner = batched.BatchedEvaluator(pred, K, **kw)
    runner.keep_probs = True
    res = runner.run(vpu_evaluation.dataset_objects(ds))
    return [([(c.is_positive, int(c.coords[0]), int(c.coords[1])) for c in clicks], ious, runner.final_probs[i])
            for i, (clicks, ious) in enumerate(res)]


def _truncate(series, thr, min_clicks=1):
    """evaluate_sample's stopping rule applied to a series run without one."""
    for k, v in enumerate(series):
        if v >= thr and k + 1 >= min_clicks:
            return k + 1
    return len(series)


def test_end_to_end_fp32_batched_equals_sequential():
    _need_gpu()
    model = _vitb("f32")
    ds = _synth_dataset([(448, 448), (480, 640), (375, 500)])
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    max_clicks = 5
    seq = _sequential(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom),
                      max_iou_thr=2.0, max_clicks=max_clicks)
    # a threshold that some objects reach before their last click and others never reach (refill + tail shrink)
    thr = None
    for cand in sorted({float(v) for _, s, _ in seq for v in s}):
        stops = [_truncate(s, cand) for _, s, _ in seq]
        if any(n < max_clicks for n in stops) and any(float(s.max()) < cand for _, s, _ in seq):
            thr = cand
            break
    assert thr is not None, [s for _, s, _ in seq]
    want = [(c[:_truncate(s, thr)], s[:_truncate(s, thr)]) for c, s, _ in seq]
    for K in (4, 16):
        pred = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom)
        got = _batched(ds, pred, K, max_iou_thr=thr, max_clicks=max_clicks)
        assert len(got) == len(want) == 6
        for j, ((cw, sw), (cg, sg, _)) in enumerate(zip(want, got)):
            assert cg == cw, (K, j, cg, cw)
            assert np.array_equal(sg, sw), (K, j, sg, sw)
        series, _ = evaluate_dataset(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom),
                                     batch_objects=K, max_iou_thr=thr, max_clicks=max_clicks)
        assert all(np.array_equal(a, b) for a, (_, b) in zip(series, want))
    # full-budget runs end on the same probability map
    got = _batched(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), 4, max_iou_thr=2.0,
                   max_clicks=max_clicks)
    for (_, _, pw), (_, _, pg) in zip(seq, got):
        assert np.array_equal(pg.cpu().numpy(), pw)


def test_end_to_end_fp32_zoom_recalculation(monkeypatch):
    """skip_clicks=0: the first click runs on the whole 448 x 448 image and ZoomIn may re-run it zoomed in."""
    _need_gpu()
    model = _vitb("f32")
    ds = _synth_dataset([(448, 448), (448, 448)], seed=20)
    zoom = dict(skip_clicks=0, target_size=(448, 448))
    seq = _sequential(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), max_iou_thr=2.0,
                      max_clicks=3)
    fired = []
    orig = batched.BatchedEvaluator._wants_recalc
    monkeypatch.setattr(batched.BatchedEvaluator, "_wants_recalc", lambda self, o: fired.append(orig(self, o)) or fired[-1])
    got = _batched(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), 3, max_iou_thr=2.0,
                   max_clicks=3)
    print(f"[batched] zoom recalculations: {sum(fired)} of {len(fired)} steps")
    for (cw, sw, _), (cg, sg, _) in zip(seq, got):
        assert cg == cw and np.array_equal(sg, sw)


def test_padding_does_not_change_an_objects_logits():
    """get_points_nd pads every click list to the batch's common count with (-1, -1, -1) rows: one object alone and in a
    batch beside an object with more clicks gets the same logits, bit for bit in fp32."""
    _need_gpu()
    model = _vitb("f32")
    pred = get_predictor(model, "NoBRS", "cuda", with_flip=False, zoom_in_params=None)
    g = torch.Generator().manual_seed(1)
    img = torch.cat([torch.rand(2, 3, 448, 448, generator=g), torch.zeros(2, 1, 448, 448)], 1).cuda()
    a = [Click(True, (100, 120), 0)]
    b = [Click(True, (200, 220), 0), Click(False, (10, 10), 1), Click(True, (300, 40), 2), Click(False, (400, 400), 3),
         Click(True, (250, 260), 4)]
    with torch.no_grad():
        alone = model(img[:1], pred.get_points_nd([a]).float(), None, 0)["instances"].clone()
        pair = model(img, pred.get_points_nd([a, b]).float(), None, 0)["instances"].clone()
    assert pred.get_points_nd([a]).shape[1] == 2 and pred.get_points_nd([a, b]).shape[1] == 6
    assert torch.equal(alone[0], pair[0])


def test_end_to_end_bf16_close_to_sequential():
    """bf16 is not compared bit for bit: the GEMM instantiation is chosen by row count, so a batch of 2K runs other
    kernels than a batch of 2, and near-ties of the distance transform move (test_nobrs_vitb_20_clicks_config3 records
    one such tie moving with the instantiation).  Each object's first-click probability map stays within the ViT-B
    click-logit bound of its sequential counterpart, and the mean final IoU within 0.02."""
    _need_gpu()
    from bf16_bounds import frozen_upper
    model = _vitb("bf16")
    ds = _synth_dataset([(448, 448), (480, 640), (375, 500)], seed=40)
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    mk = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom)
    first_seq = _sequential(ds, mk(), max_iou_thr=2.0, max_clicks=1)
    first_bat = _batched(ds, mk(), 4, max_iou_thr=2.0, max_clicks=1)
    bound = frozen_upper("vitb click logits (budget test)")
    for (_, _, pw), (_, _, pg) in zip(first_seq, first_bat):
        err = np.abs(pg.cpu().numpy().astype(np.float64) - pw).max() / max(np.abs(pw).max(), 1e-12)
        print(f"[bf16-bound] batched first-click map vs sequential: {err:.4g} (bound {bound:.4g})")
        assert err < bound
    seq = _sequential(ds, mk(), max_iou_thr=2.0, max_clicks=5)
    bat = _batched(ds, mk(), 4, max_iou_thr=2.0, max_clicks=5)
    ms, mb = np.mean([s[-1] for _, s, _ in seq]), np.mean([s[-1] for _, s, _ in bat])
    print(f"[batched] bf16 mean final IoU: sequential {ms:.4f}, batched {mb:.4f}")
    assert abs(ms - mb) <= 0.02
