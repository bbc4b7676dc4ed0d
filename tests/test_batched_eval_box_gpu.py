"""GPU: box-prompt evaluation in the batched NoBRS loop (isegm/inference/batched.py, ``vpu_box_prompts_batched`` in
csrc/evalbatch.hip).  The kernel's boxes equal the sequential derivation (``get_next_promts`` on the flipped, cropped and
resized tensors that ``get_vqu_prediction`` builds) bit for bit, padding does not change an object's logits, and ViT-B in
the fp32 engine mode gives the same clicks and IoU series with K objects per forward as one at a time."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from pvpuformer_amd.isegm.engine.prompt_sim import get_next_promts
from pvpuformer_amd.isegm.inference import batched, vpu_evaluation
from pvpuformer_amd.isegm.inference.clicker import Click
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.predictors.base import BasePredictor
from pvpuformer_amd.isegm.inference.transforms import Roi, crop_resize
from pvpuformer_amd.isegm.inference.vpu_evaluation import evaluate_sample

pytestmark = pytest.mark.gpu

SIZES = [(448, 448), (480, 640), (375, 500), (333, 517)]
NET = (448, 448)
KMAX_PER_ROW = 1024          # ops.box_prompts_batched's default table size per row
DEV = "cuda"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _blobs(H, W, g, k, level):
    f = torch.nn.functional.avg_pool2d(torch.rand(1, 1, H, W, generator=g), k, 1, k // 2)[0, 0]
    return f > f.flatten().kthvalue(max(1, int(level * f.numel()))).values


def _clicks(j):
    """Click lists of different lengths (network coordinates; only their polarity and order matter to the slot)."""
    c = [Click(True, (100.0, 120.5), 0), Click(False, (10.0, 10.0), 1), Click(True, (300.0, 40.0), 2),
         Click(True, (250.0, 260.0), 3), Click(False, (400.0, 400.0), 4), Click(True, (17.0, 333.0), 5)]
    return c[:1 + (j * 2) % 6]


def _objects(n, seed, sizes=SIZES):
    """n objects cycling through ``sizes``: blobby ground truth with a -1 band and a previous prediction that misses parts
    of it and adds others (several components of either kind); every fourth one predicted perfectly outside the -1 band."""
    g = torch.Generator().manual_seed(seed)
    objs = []
    for j in range(n):
        H, W = sizes[j % len(sizes)]
        obj = _blobs(H, W, g, 41, 0.6)
        gt = obj.numpy().astype(np.int32)
        gt[H // 3:H // 3 + 7, :] = -1
        o = batched._Object(j, torch.zeros(3, H, W, device=DEV), gt, DEV)
        if j % 4 == 3:
            prev = obj.float() * 0.9 + 0.05
        else:
            many, few = _blobs(H, W, g, 21, 0.5), _blobs(H, W, g, 21, 0.9)
            wrong = (many & obj) | (few & ~obj) if j % 2 == 0 else (few & obj) | (many & ~obj)      # fn wins / fp wins
            prev = torch.where(wrong, 1.0 - obj.float(), obj.float()) * 0.8 + 0.2 * torch.rand(H, W, generator=g)
        o.canvas[0].copy_(prev)
        o.clicks = _clicks(j)
        objs.append(o)
    return objs


def _rois(H, W, j):
    """ROIs touching each border in turn, and the whole image."""
    return [Roi(0, H // 2, 10, W // 2 + 40), Roi(H // 3, H - 1, W // 4, W // 4 + 220), Roi(20, H - 31, 0, 190),
            Roi(5, 300, W - 250, W - 1), Roi.whole(H, W)][j % 5]


def _float_gt(o):
    return torch.where(o.gt != 0, 1.0, torch.where(o.valid != 0, 0.0, -1.0)).float()[None, None]


def _sequential_boxes(pred, o, roi, flip, size):
    """What get_vqu_prediction computes for this object (base.py:114-121): (boxes [1 or 2, 5] in the object's own click
    layout, n_obj, the host's fn / fp masks of every row)."""
    gt, prev = _float_gt(o), o.canvas[o.prev][None, None]
    lists = [o.clicks]
    if flip:
        gt = torch.cat([gt, torch.flip(gt, dims=[3])], dim=0)
        prev = torch.cat([prev, torch.flip(prev, dims=[3])], dim=0)
        lists = lists + [[c.copy(coords=(c.coords[0], size[1] - c.coords[1] - 1)) for c in o.clicks]]
    if roi is not None:
        gt, prev = crop_resize(gt, roi, size), crop_resize(prev, roi, size)
    points = pred.get_points_nd(lists).float()
    boxes = get_next_promts(prev, gt, points, None, as_allmask=False, jitter_box=False)[1].cpu().numpy()
    g, p = gt.cpu().numpy()[:, 0] > 0.5, prev.cpu().numpy()[:, 0]
    return boxes, points.shape[1] // 2, (g & (p < np.float32(0.49)), ~g & (p > np.float32(0.49)))


def _expected(pred, objs, rois, flip, size):
    """(expected boxes of the batch in the padded layout, facts about the inputs, packed points, n_batch)."""
    lists = [o.clicks for o in objs]
    if flip:
        lists = lists + [[c.copy(coords=(c.coords[0], size[1] - c.coords[1] - 1)) for c in cl] for cl in lists]
    points_nd = pred.get_points_nd(lists).float()
    n_batch, n = points_nd.shape[1] // 2, len(objs)
    want = np.zeros((len(lists), 5), np.int32)
    facts = dict(components=[], fn=0, fp=0, empty=0, equal=0, own_slots=[])
    for j, (o, roi) in enumerate(zip(objs, rois)):
        boxes, n_obj, (fn, fp) = _sequential_boxes(pred, o, roi, flip, size)
        for r in range(len(boxes)):
            chosen = fn[r] if fn[r].sum() > fp[r].sum() else fp[r]
            facts["components"].append(ndimage.label(chosen, structure=np.ones((3, 3)))[1])
            facts["fn" if fn[r].sum() > fp[r].sum() else "fp"] += 1
            facts["empty"] += int(chosen.sum() == 0)
            facts["equal"] += int(fn[r].sum() == fp[r].sum())
            facts["own_slots"].append((int(boxes[r, 4]), n_obj))
            want[r * n + j] = boxes[r]
            if boxes[r].any():
                want[r * n + j, 4] = batched._padded_slot(int(boxes[r, 4]), n_obj, n_batch)
    return want, facts, points_nd, n_batch, len(lists)


def _device_boxes(pred, objs, rois, flip, size, kmax_check=True):
    """(boxes of the batch from the kernel, flag, expected boxes in the padded layout, facts about the inputs)."""
    want, facts, points_nd, n_batch, n_rows = _expected(pred, objs, rois, flip, size)
    if kmax_check:      # inputs chosen on the host so that the kernel's component table holds them
        assert sum(facts["components"]) <= KMAX_PER_ROW * n_rows, facts["components"]
    ops = batched._DeviceOps(DEV)
    ops.begin(1, 1)
    ev = batched.BatchedEvaluator(pred, 2, 0.8, as_prompt_type=1)
    rows = [(o, roi, mirror, ev._own_rows(o.clicks)) for mirror in ((False, True) if flip else (False,))
            for o, roi in zip(objs, rois)]
    for row in rows:
        ops.add_box(*row)
    ops.upload()
    got = ops.boxes(rows, 0, points_nd, n_batch, size, size, 0)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(rows), 5)
    ops.readback()
    return got.cpu().numpy(), int(ops.flags[0]), want, facts, (rows, points_nd, n_batch)


def _host_predictor():
    return BasePredictor(None, DEV, with_flip=True)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_box_prompts_kernel_equals_sequential_derivation(K, flip):
    """Objects of four sizes, ROIs touching every border and the whole image, resized to the network size."""
    _need_gpu()
    pred = _host_predictor()
    objs = _objects(K, seed=10 + K)
    rois = [_rois(o.H, o.W, j + K) for j, o in enumerate(objs)]
    got, flag, want, facts, _ = _device_boxes(pred, objs, rois, flip, NET)
    print(f"[box] K={K} flip={flip}: components per row {facts['components']}, fn rows {facts['fn']}, fp rows {facts['fp']}, "
          f"empty {facts['empty']}")
    assert flag == 0
    assert np.array_equal(got, want), (got, want)
    if K == 8:
        assert facts["fn"] and facts["fp"] and max(facts["components"]) > 3
        assert any(slot >= n_obj for slot, n_obj in facts["own_slots"])          # a slot that moves with the padding
        if flip:    # the flip row is not the mirror image of the straight row (un-mirrored roi)
            mirrored = want[:K].copy()
            mirrored[:, 0] = np.where(want[:K, 2] > 0, NET[1] - 1 - want[:K, 0], 0)
            assert not np.array_equal(mirrored[:, :4], want[K:, :4])


def _special_objects(H, W):
    """Whole-image group (no roi: the masks are the full planes): the 10 % merge quirk, equal fn / fp counts, boxes of
    width / height 0, an empty mask, and a blobby one."""
    def make(gt, prev, j):
        o = batched._Object(j, torch.zeros(3, H, W, device=DEV), gt.astype(np.int32), DEV)
        o.canvas[0].copy_(torch.from_numpy(prev.astype(np.float32)))
        o.clicks = _clicks(j)
        return o
    z = lambda: np.zeros((H, W), np.float32)
    objs = []
    # (0) fn components in label order: A small, D above 10 % but before the largest, B largest, C above 10 % after it, E
    # small: max_connected_regions keeps B and C only
    gt = z(); gt[10:16, 10:21] = 1; gt[20:46, 300:481] = 1; gt[50:151, 50:251] = 1; gt[200:261, 300:451] = 1; gt[300:304, 5:9] = 1
    objs.append(make(gt, z(), 0))
    # (1) equal counts: 100 missed pixels, 100 extra ones -> the fp mask
    gt = z(); gt[30:40, 30:40] = 1
    prev = z(); prev[200:210, 100:110] = 0.9
    objs.append(make(gt, prev, 1))
    # (2), (3) a one-pixel wide column / row: width / height 0 -> zero box
    gt = z(); gt[100:141, 77] = 1
    objs.append(make(gt, z(), 2))
    gt = z(); gt[60, 20:90] = 1
    objs.append(make(gt, z(), 3))
    # (4) nothing wrong: empty mask; (5) a box touching row / column 0 on one side only
    gt = z(); gt[100:200, 100:200] = 1
    objs.append(make(gt, gt * 0.9, 4))
    gt = z(); gt[0:3, 0:2] = 1
    objs.append(make(gt, z(), 5))
    return objs


@pytest.mark.parametrize("flip", [True, False])
def test_box_prompts_kernel_whole_image_and_edge_cases(flip):
    _need_gpu()
    H, W = 375, 500
    pred = _host_predictor()
    objs = _special_objects(H, W) + _objects(2, seed=77, sizes=[(H, W)])
    got, flag, want, facts, (_, _, n_batch) = _device_boxes(pred, objs, [None] * len(objs), flip, (H, W))
    assert flag == 0
    assert np.array_equal(got, want), (got, want)
    # the cases are what they were built to be
    assert tuple(want[0, :4]) == ((50 + 450) >> 1, (50 + 260) >> 1, 450 - 50, 260 - 50)       # B and C, without D
    assert facts["equal"] >= 2 and tuple(want[1, :4]) == (104, 204, 9, 9) and want[1, 4] >= n_batch
    assert not want[2].any() and not want[3].any() and not want[4].any()
    assert tuple(want[5]) == (0, 0, 0, 0, 0)            # x centre (0 + 1) >> 1 = 0 fails the >= 1 test
    if flip:
        n = len(objs)
        assert tuple(want[n, :4]) == (W - 1 - 250, 155, 400, 210)     # whole image: here the flip row IS the mirror image


def test_box_prompts_kernel_overflow_raises_the_flag_and_the_host_takes_over():
    """Salt-and-pepper false positives: more components than the table holds."""
    _need_gpu()
    H, W = 448, 448
    pred = _host_predictor()
    g = torch.Generator().manual_seed(4)
    o = batched._Object(0, torch.zeros(3, H, W, device=DEV), np.zeros((H, W), np.int32), DEV)
    o.canvas[0].copy_((torch.rand(H, W, generator=g) < 0.1).float() * 0.9)
    o.clicks = _clicks(1)
    got, flag, want, facts, (rows, points_nd, n_batch) = _device_boxes(pred, [o], [Roi.whole(H, W)], True, NET, kmax_check=False)
    assert min(facts["components"]) > 2 * KMAX_PER_ROW, facts["components"]
    assert flag == 1
    host = batched._host_boxes(rows, points_nd, n_batch, NET, NET)
    assert np.array_equal(host, want) and want.any()


# ------------------------------------------------------------------------------------------------ with the network
_MODELS = {}


def _vitb(dtype):
    if dtype not in _MODELS:
        from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model
        from pvpuformer_amd.synth import vitb_model_kwargs
        torch.manual_seed(0)
        model = VitMultiGaussianVector_ed_Model(**vitb_model_kwargs()).cuda()
        model.set_compute_dtype(dtype)
        model.eval()
        model.weights_frozen = True
        _MODELS[dtype] = model
    return _MODELS[dtype]


def test_padding_does_not_change_an_objects_logits_with_a_box_prompt():
    """One object alone and the same object inside a batch of 2K = 8 padded to more click rows: with its box slot moved
    into the padded layout the logits are the same bit for bit in fp32, for a box in a positive and in a negative row."""
    _need_gpu()
    model = _vitb("f32")
    pred = get_predictor(model, "NoBRS", "cuda", with_flip=False, zoom_in_params=None)
    g = torch.Generator().manual_seed(1)
    img = torch.cat([torch.rand(8, 3, 448, 448, generator=g), torch.zeros(8, 1, 448, 448)], 1).cuda()
    a = [Click(True, (100, 120), 0), Click(False, (30, 40), 1), Click(True, (180, 90), 2)]
    others = [_clicks(j) for j in range(1, 8)]
    others[1] = others[1] + [Click(True, (50.0, 60.0), 5)]         # four positive clicks: the batch pads to four rows
    own = pred.get_points_nd([a]).float()
    padded = pred.get_points_nd([a] + others).float()
    n_obj, n_batch = own.shape[1] // 2, padded.shape[1] // 2
    assert (n_obj, n_batch) == (2, 4)
    for own_slot in (n_obj - 1, n_obj + 1):                       # fn: last positive row (a real click); fp: first free negative
        box = torch.tensor([[200, 150, 120, 80, own_slot]], dtype=torch.int32, device="cuda")
        boxes = torch.zeros(8, 5, dtype=torch.int32, device="cuda")
        boxes[:, :4] = torch.tensor([210, 140, 60, 90], dtype=torch.int32)
        boxes[:, 4] = 1
        boxes[0] = box[0]
        boxes[0, 4] = batched._padded_slot(own_slot, n_obj, n_batch)
        with torch.no_grad():
            alone = model(img[:1], own, (own, box, None), 1)["instances"].clone()
            batch = model(img, padded, (padded, boxes, None), 1)["instances"].clone()
            clicks_only = model(img[:1], own, None, 0)["instances"].clone()
        assert torch.equal(alone[0], batch[0]), own_slot
        assert not torch.equal(alone[0], clicks_only[0])            # the box is read


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
            clicks, ious, probs = evaluate_sample(s.image, s.gt_mask(oid), pred, as_prompt_type=1, **kw)
            out.append(([(c.is_positive, int(c.coords[0]), int(c.coords[1])) for c in clicks], ious, probs))
    return out


def _batched(ds, pred, K, **kw):
    runner = batched.BatchedEvaluator(pred, K, as_prompt_type=1, **kw)
    runner.keep_probs = True
    res = runner.run(vpu_evaluation.dataset_objects(ds))
    return [([(c.is_positive, int(c.coords[0]), int(c.coords[1])) for c in clicks], ious, runner.final_probs[i])
            for i, (clicks, ious) in enumerate(res)]


def test_end_to_end_fp32_box_prompts_batched_equals_sequential(monkeypatch):
    _need_gpu()
    model = _vitb("f32")
    ds = _synth_dataset([(448, 448), (480, 640), (375, 500)])
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    kw = dict(max_iou_thr=2.0, max_clicks=4)
    seq = _sequential(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), **kw)
    on_device, on_host = [], []
    dev, host = batched._DeviceOps.boxes, batched._host_boxes
    monkeypatch.setattr(batched._DeviceOps, "boxes", lambda self, *a: on_device.append(1) or dev(self, *a))
    monkeypatch.setattr(batched, "_host_boxes", lambda *a, **k: on_host.append(1) or host(*a, **k))
    got = _batched(ds, get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom), 4, **kw)
    assert len(got) == len(seq) == 6
    for j, ((cw, sw, pw), (cg, sg, pg)) in enumerate(zip(seq, got)):
        assert cg == cw, (j, cg, cw)
        assert np.array_equal(sg, sw), (j, sg, sw)
        assert np.array_equal(pg.cpu().numpy(), pw), j
    assert on_device and not on_host                 # the boxes came from the kernel; no table overflow on ordinary masks


def test_end_to_end_bf16_box_prompts_report():
    """bf16 is not compared bit for bit (the GEMM instantiation depends on the row count).  Reports the mean final IoU
    of both paths and the first-click map difference; no bound on the difference has been measured yet, so none is asserted.

    Observed on one MI355X (ViT-B, random weights, these 6 synthetic objects, 5 clicks, K = 4): first-click maps differ by
    6.7e-4 to 8.0e-4 of the map's maximum; mean final IoU 0.1778 sequential, 0.1778 batched."""
    _need_gpu()
    model = _vitb("bf16")
    ds = _synth_dataset([(448, 448), (480, 640), (375, 500)], seed=40)
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    mk = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom)
    max_clicks = 5
    first_seq = _sequential(ds, mk(), max_iou_thr=2.0, max_clicks=1)
    first_bat = _batched(ds, mk(), 4, max_iou_thr=2.0, max_clicks=1)
    for (_, _, pw), (_, _, pg) in zip(first_seq, first_bat):
        err = np.abs(pg.cpu().numpy().astype(np.float64) - pw).max() / max(np.abs(pw).max(), 1e-12)
        print(f"[bf16-report] box prompts, batched first-click map vs sequential: {err:.4g}")
    seq = _sequential(ds, mk(), max_iou_thr=2.0, max_clicks=max_clicks)
    bat = _batched(ds, mk(), 4, max_iou_thr=2.0, max_clicks=max_clicks)
    ms, mb = np.mean([s[-1] for _, s, _ in seq]), np.mean([s[-1] for _, s, _ in bat])
    print(f"[batched] box prompts, bf16 mean final IoU: sequential {ms:.4f}, batched {mb:.4f}")
    for _, s, _ in seq + bat:
        assert 1 <= len(s) <= max_clicks and np.isfinite(s).all()
