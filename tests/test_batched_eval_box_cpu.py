"""CPU: box-prompt evaluation (``as_prompt_type=1``) through the batched NoBRS scheduler against the sequential
``evaluate_sample``, with a stub network that also reads the box prompt and the host stand-ins of the batched kernels:
series equality, the translation of the box slot into the padded click layout, dispatch, and the repeat of a click whose
component table overflowed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd.isegm.engine.prompt_sim import get_next_promts
from pvpuformer_amd.isegm.inference import batched, vpu_evaluation
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.clicker import Click
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.vpu_evaluation import evaluate_dataset, evaluate_sample


class BoxStubNet:
    """Logits from the image brightness, the previous mask, Gaussian bumps at the clicks and, with box prompts, a bump
    shaped by the box (centre, size) whose sign and weight come from the slot: its polarity and its position within the
    polarity, which are the same in an object's own click layout and in a padded one.  Each sample is computed alone."""
    with_prev_mask = True

    def __init__(self):
        self.types, self.boxes = [], []

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        assert as_prompt_type in (0, 1)
        self.types.append(as_prompt_type)
        B, _, H, W = image.shape
        n = points.shape[1] // 2
        yy = torch.arange(H, dtype=torch.float32)[:, None]
        xx = torch.arange(W, dtype=torch.float32)[None, :]
        boxes = None
        if as_prompt_type == 1:
            assert prompts[0] is points and prompts[2] is None
            boxes = prompts[1]
            assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 5)
        out = []
        for b in range(B):
            x = image[b]
            logit = 8.0 * (x[:3].mean(0) - 0.5) + 2.0 * (x[3] - 0.5)
            for j in range(points.shape[1]):
                r, c, _ = (float(v) for v in points[b, j])
                if r < 0:
                    continue
                bump = torch.exp(-((yy - r) ** 2 + (xx - c) ** 2) / 18.0)
                logit = logit + (6.0 if j < n else -6.0) * bump
            if boxes is not None:
                xc, yc, bw, bh, slot = (int(v) for v in boxes[b])
                pol, within = (0, slot) if slot < n else (1, slot - n)
                self.boxes.append((xc, yc, bw, bh, pol, within))
                bump = torch.exp(-((yy - yc) ** 2 / (bh * bh + 4.0) + (xx - xc) ** 2 / (bw * bw + 4.0)))
                logit = logit + (1.5 if pol == 0 else -1.5) * (1.0 + 0.5 * within) * bump
            out.append(logit[None, None])
        return {"instances": torch.cat(out, 0)}


def _host_mask_box(prob, thr, positive_clicks=()):
    m = (prob[0, 0] > thr).numpy().copy()
    count = int(m.sum())
    for r, c in positive_clicks:
        m[int(r), int(c)] = True
    rows, cols = np.nonzero(m)
    if len(rows) == 0:
        return 0, m.shape[0], -1, m.shape[1], -1
    return count, int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())


@pytest.fixture
def host_transforms(monkeypatch):
    monkeypatch.setattr(T._device, "resize_align_corners",
                        lambda x, size: F.interpolate(x.float(), size=tuple(int(s) for s in size), mode="bilinear",
                                                      align_corners=True))
    monkeypatch.setattr(T._device, "mask_box", _host_mask_box)


class Sample:
    def __init__(self, image, masks):
        self.image, self._masks = image, masks
        self.objects_ids = list(range(len(masks)))

    def gt_mask(self, oid):
        return self._masks[oid]


class Dataset:
    """Images of different sizes; objects are noisy bright ellipses / boxes, some in two parts, some with an ignore band."""

    def __init__(self, sizes=((60, 80), (48, 48), (50, 70), (64, 64)), per_image=(2, 1, 3, 2), seed=0):
        rs = np.random.RandomState(seed)
        self.samples = []
        for (H, W), k in zip(sizes, per_image):
            yy, xx = np.mgrid[0:H, 0:W]
            img = rs.rand(H, W, 3) * 0.35
            masks = []
            for j in range(k):
                cy, cx = rs.randint(H // 4, 3 * H // 4), rs.randint(W // 4, 3 * W // 4)
                ry, rx = rs.randint(4, H // 4), rs.randint(4, W // 4)
                m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
                if j == 1:
                    m |= (yy >= 2) & (yy < 2 + H // 5) & (xx >= W // 2) & (xx < W // 2 + W // 6)
                img[m] += rs.rand() * 0.5 + 0.1 * j
                g = m.astype(np.int32)
                if j == 2:
                    g[:, :3] = -1
                    g[cy - 1:cy + 1, :] = -1         # an ignore band through the object: the resized float ground truth sees -1
                masks.append(g)
            self.samples.append(Sample((np.clip(img, 0, 1) * 255).astype(np.uint8), masks))

    def __len__(self):
        return len(self.samples)

    def get_sample(self, i):
        return self.samples[i]


def _predictor(skip_clicks=-1, net=None, **kw):
    return get_predictor(net or BoxStubNet(), "NoBRS", "cpu", with_flip=True,
                         zoom_in_params=dict(skip_clicks=skip_clicks, target_size=(32, 32), min_crop_size=12), **kw)


def _sequential(ds, pred, **kw):
    out = []
    for i in range(len(ds)):
        s = ds.get_sample(i)
        for oid in s.objects_ids:
            clicks, ious, _ = evaluate_sample(s.image, s.gt_mask(oid), pred, as_prompt_type=1, **kw)
            out.append(([(c.is_positive, int(c.coords[0]), int(c.coords[1]), c.indx) for c in clicks], ious))
    return out


def _batched(ds, pred, K, **kw):
    runner = batched.BatchedEvaluator(pred, K, as_prompt_type=1, **kw)
    return [([(c.is_positive, int(c.coords[0]), int(c.coords[1]), c.indx) for c in clicks], ious)
            for clicks, ious in runner.run(vpu_evaluation.dataset_objects(ds))]


KW = dict(max_iou_thr=0.8, pred_thr=0.49, min_clicks=1, max_clicks=6)
_SEQ = {}


def _seq_reference(skip_clicks):
    """The sequential series, computed once per zoom setting and shared by the K cases."""
    if skip_clicks not in _SEQ:
        net = BoxStubNet()
        _SEQ[skip_clicks] = (_sequential(Dataset(), _predictor(skip_clicks, net), **KW), net)
    return _SEQ[skip_clicks]


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("skip_clicks", [-1, 0])
def test_batched_box_prompts_equal_sequential(host_transforms, K, skip_clicks):
    seq, seq_net = _seq_reference(skip_clicks)
    lens = [len(i) for _, i in seq]
    assert min(lens) < 6 and max(lens) == 6, lens            # early stops and full budgets: refill and tail shrink
    # the sequential run saw fn and fp boxes, slots beyond the first of a polarity, and (skip_clicks = 0) re-ran clicks as
    # click prompts: the comparison below covers those paths
    assert {b[4] for b in seq_net.boxes} == {0, 1} and max(b[5] for b in seq_net.boxes) >= 1
    assert (0 in seq_net.types) == (skip_clicks == 0)
    net = BoxStubNet()
    got = _batched(Dataset(), _predictor(skip_clicks, net), K, **KW)
    assert len(got) == len(seq) == 8
    for (cs, i_s), (cb, i_b) in zip(seq, got):
        assert cs == cb
        assert i_s.dtype == i_b.dtype and np.array_equal(i_s, i_b)
    assert (0 in net.types) == (skip_clicks == 0)
    # the same boxes reached the network (as a multiset: the batch interleaves the objects)
    assert sorted(net.boxes) == sorted(seq_net.boxes)
    series, secs = evaluate_dataset(Dataset(), _predictor(skip_clicks), batch_objects=K, as_prompt_type=1,
                                    batch_box_prompts=True, **KW)
    assert [s.tolist() for s in series] == [i.tolist() for _, i in seq] and secs >= 0


def _object(H, W, gt, prev, clicks):
    o = batched._Object(0, torch.zeros(3, H, W), gt, "cpu")
    o.canvas[0].copy_(torch.from_numpy(prev))
    o.clicks = clicks
    return o


def test_box_slot_in_the_padded_layout_maps_back_to_the_sequential_slot(host_transforms):
    """Objects with different click counts in one batch.  fn: the object's last positive row, the same row in both
    layouts.  fp: the object's first free negative row n_obj + j (default 2 n_obj - 1) is row n_batch + j of the batch."""
    H, W = 40, 48
    gt = np.zeros((H, W), np.int32)
    gt[10:30, 12:36] = 1
    miss = np.zeros((H, W), np.float32)                          # nothing predicted: false negatives only
    over = np.zeros((H, W), np.float32)
    over[5:35, 6:44] = 0.9                                        # predicted far too large: false positives win
    P, N = (lambda r, c, i: Click(True, (r, c), i)), (lambda r, c, i: Click(False, (r, c), i))
    cases = [                                                     # (prev, clicks, own slot expected)
        (miss, [P(20, 20, 0)], 0),                                                   # fn, n_obj 1: slot n_obj - 1 = 0
        (miss, [P(20, 20, 0), N(3, 3, 1), P(15, 15, 2)], 1),                         # fn, n_obj 2: the last positive row, a real click
        (over, [P(20, 20, 0), N(3, 3, 1)], 1),                                       # fp, no free negative: default 2 n_obj - 1
        (over, [P(20, 20, 0), P(15, 15, 1)], 2),                                     # fp, n_obj 2: first free negative n_obj + 0
        (over, [P(20, 20, 0), N(3, 3, 1), P(15, 15, 2), P(25, 30, 3)], 4),           # fp, n_obj 3: n_obj + 1
        (over, [P(20, 20, 0), N(3, 3, 1), P(15, 15, 2), P(25, 30, 3), P(12, 14, 4), N(38, 2, 5)], 6),   # n_obj 4 = n_batch
    ]
    pred = _predictor()
    ev = batched.BatchedEvaluator(pred, 8, 0.8, as_prompt_type=1)
    objs = [_object(H, W, gt, prev, clicks) for prev, clicks, _ in cases]
    points_nd = pred.get_points_nd([o.clicks for o in objs]).float()
    n_batch = points_nd.shape[1] // 2
    assert n_batch == 4
    rows = [(o, None, False, ev._own_rows(o.clicks)) for o in objs]
    got = batched._host_boxes(rows, points_nd, n_batch, (H, W), None)
    for j, (o, (prev, clicks, own_slot)) in enumerate(zip(objs, cases)):
        own = pred.get_points_nd([clicks]).float()
        n_obj = own.shape[1] // 2
        assert n_obj == rows[j][3]
        want = get_next_promts(torch.from_numpy(prev)[None, None], torch.from_numpy(gt.astype(np.float32))[None, None], own,
                               None, as_allmask=False, jitter_box=False)[1][0].numpy()
        assert want[4] == own_slot and want[:4].all(), (j, want)
        assert np.array_equal(got[j, :4], want[:4]), (j, got[j], want)
        padded = int(got[j, 4])
        back = padded if padded < n_batch else n_obj + (padded - n_batch)
        assert back == own_slot, (j, padded, own_slot)
        assert (padded < n_batch) == (own_slot < n_obj)          # the polarity both consumers read off the slot
        assert padded == batched._padded_slot(own_slot, n_obj, n_batch)
    assert [int(s) for s in got[:, 4]] == [0, 1, 4, 4, 5, 6]


def test_dispatch_box_prompts_batched_and_scribbles_sequential(host_transforms, monkeypatch):
    ds = Dataset(sizes=((40, 56),), per_image=(2,))
    used = []
    orig = batched.BatchedEvaluator.__init__

    def spy(self, predictor, K, *a, **k):
        used.append((K, k.get("as_prompt_type")))
        orig(self, predictor, K, *a, **k)
    monkeypatch.setattr(batched.BatchedEvaluator, "__init__", spy)
    series, _ = evaluate_dataset(ds, _predictor(), batch_objects=4, max_iou_thr=0.8, max_clicks=3, as_prompt_type=1,
                                 batch_box_prompts=True)
    assert used == [(4, 1)] and len(series) == 2
    monkeypatch.setenv("VPU_EVAL_BATCH_BOX", "1")           # the same switch for an unchanged evaluation script
    monkeypatch.setenv("VPU_EVAL_BATCH", "3")
    again, _ = evaluate_dataset(ds, _predictor(), max_iou_thr=0.8, max_clicks=3, as_prompt_type=1)
    assert used == [(4, 1), (3, 1)] and [s.tolist() for s in again] == [s.tolist() for s in series]
    monkeypatch.delenv("VPU_EVAL_BATCH_BOX")
    monkeypatch.delenv("VPU_EVAL_BATCH")
    # not asked for: box prompts stay on the sequential loop, with the same series
    default, _ = evaluate_dataset(ds, _predictor(), batch_objects=4, max_iou_thr=0.8, max_clicks=3, as_prompt_type=1)
    assert len(used) == 2 and [s.tolist() for s in default] == [s.tolist() for s in series]
    del used[1]
    assert batched.batchable(_predictor(), None, 1) and not batched.batchable(_predictor(), None, 2)
    calls = []
    monkeypatch.setattr(vpu_evaluation, "evaluate_sample",
                        lambda image, gt_mask, predictor, **kw: calls.append(kw) or ([], np.zeros(1, np.float32), None))
    evaluate_dataset(ds, _predictor(), batch_objects=4, max_iou_thr=0.8, as_prompt_type=2, batch_box_prompts=True)
    assert used == [(4, 1)] and len(calls) == 2 and all(kw["as_prompt_type"] == 2 for kw in calls)
    with pytest.raises(AssertionError):
        batched.BatchedEvaluator(_predictor(), 4, 0.8, as_prompt_type=2)


def test_component_table_overflow_repeats_the_click_with_host_boxes(host_transforms, monkeypatch):
    """A group whose flag comes back set has its forward discarded and repeats the click with boxes from the host code:
    the series stay those of the sequential run."""
    seq, _ = _seq_reference(-1)
    raised = []
    orig = batched._HostOps.boxes

    def overflowing(self, rows, first, points_nd, n_batch, size, target_size, flag):
        if len(raised) < 5 and len(raised) % 2 == 0:
            self.flags[flag] = 1
            raised.append(len(rows))
            return torch.full((len(rows), 5), 7, dtype=torch.int32)           # boxes of a truncated table: never used
        raised.append(0)
        return orig(self, rows, first, points_nd, n_batch, size, target_size, flag)
    monkeypatch.setattr(batched._HostOps, "boxes", overflowing)
    got = _batched(Dataset(), _predictor(-1), 3, **KW)
    assert sum(1 for r in raised if r) == 3
    for (cs, i_s), (cb, i_b) in zip(seq, got):
        assert cs == cb and np.array_equal(i_s, i_b)
