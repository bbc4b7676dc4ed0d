"""CPU: the batched NoBRS scheduler (isegm/inference/batched.py) against the sequential ``evaluate_dataset``, with a stub
network and the host stand-ins of the batched kernels.  Output order, early stop and refill, the ZoomIn recalculation,
``VPU_EVAL_BATCH`` and the silent fall-back to the sequential loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd.isegm.inference import batched, vpu_evaluation
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.vpu_evaluation import evaluate_dataset, evaluate_sample


class StubNet:
    """Logits from the image brightness, the previous mask and Gaussian bumps at the clicks.  Each sample is computed
    alone (same shapes whatever the batch), and not-a-point rows are skipped, so the output of one sample does not depend
    on the batch it is in nor on the click padding."""
    with_prev_mask = True

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        assert as_prompt_type == 0
        B, _, H, W = image.shape
        n = points.shape[1] // 2
        yy = torch.arange(H, dtype=torch.float32)[:, None]
        xx = torch.arange(W, dtype=torch.float32)[None, :]
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
    """Images of different sizes; objects are noisy bright ellipses / boxes, some with an ignore (-1) band."""

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
                masks.append(g)
            self.samples.append(Sample((np.clip(img, 0, 1) * 255).astype(np.uint8), masks))

    def __len__(self):
        return len(self.samples)

    def get_sample(self, i):
        return self.samples[i]


def _predictor(skip_clicks=-1, **kw):
    return get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True,
                         zoom_in_params=dict(skip_clicks=skip_clicks, target_size=(32, 32), min_crop_size=12), **kw)


def _sequential(ds, pred, **kw):
    out = []
    for i in range(len(ds)):
        s = ds.get_sample(i)
        for oid in s.objects_ids:
            clicks, ious, _ = evaluate_sample(s.image, s.gt_mask(oid), pred, **kw)
            out.append(([(c.is_positive, int(c.coords[0]), int(c.coords[1]), c.indx) for c in clicks], ious))
    return out


def _batched(ds, pred, K, **kw):
    runner = batched.BatchedEvaluator(pred, K, **kw)
    return [([(c.is_positive, int(c.coords[0]), int(c.coords[1]), c.indx) for c in clicks], ious)
            for clicks, ious in runner.run(vpu_evaluation.dataset_objects(ds))]


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("skip_clicks", [-1, 0, 1])
def test_batched_scheduler_equals_sequential(host_transforms, K, skip_clicks):
    ds = Dataset()
    kw = dict(max_iou_thr=0.8, pred_thr=0.49, min_clicks=1, max_clicks=6)
    seq = _sequential(ds, _predictor(skip_clicks), **kw)
    lens = [len(i) for _, i in seq]
    # early stop for some objects, the full budget for others: refill and tail shrink both happen
    assert min(lens) < 6 and max(lens) == 6, lens
    got = _batched(ds, _predictor(skip_clicks), K, **kw)
    assert len(got) == len(seq) == 8
    for (cs, i_s), (cb, i_b) in zip(seq, got):
        assert cs == cb
        assert i_s.dtype == i_b.dtype and np.array_equal(i_s, i_b)
    # through the public interface: the same series, in dataset order
    series, secs = evaluate_dataset(ds, _predictor(skip_clicks), batch_objects=K, **kw)
    assert [s.tolist() for s in series] == [i.tolist() for _, i in seq] and secs >= 0


def test_recalculation_fires_in_the_zero_skip_case(host_transforms, monkeypatch):
    """skip_clicks=0: the first click runs at full size and the ZoomIn re-runs it zoomed when the predicted box covers
    little of the image; the test above only means something for that case if it does happen."""
    fired = []
    orig = batched.BatchedEvaluator._wants_recalc

    def spy(self, o):
        r = orig(self, o)
        fired.append(r)
        return r
    monkeypatch.setattr(batched.BatchedEvaluator, "_wants_recalc", spy)
    _batched(Dataset(), _predictor(0), 3, max_iou_thr=0.8, max_clicks=3)
    assert any(fired)


def test_min_clicks_and_budget(host_transforms):
    ds = Dataset(sizes=((40, 56), (36, 36)), per_image=(2, 2), seed=3)
    kw = dict(max_iou_thr=0.0, pred_thr=0.49, min_clicks=3, max_clicks=5)
    seq = _sequential(ds, _predictor(), **kw)
    assert all(len(i) == 3 for _, i in seq)
    assert [c for c, _ in _batched(ds, _predictor(), 3, **kw)] == [c for c, _ in seq]


def test_env_knob_selects_the_batched_path(host_transforms, monkeypatch):
    ds = Dataset()
    used = []
    orig = batched.BatchedEvaluator.__init__

    def spy(self, predictor, K, *a, **k):
        used.append(K)
        orig(self, predictor, K, *a, **k)
    monkeypatch.setattr(batched.BatchedEvaluator, "__init__", spy)
    kw = dict(max_iou_thr=0.8, max_clicks=4)
    monkeypatch.setenv("VPU_EVAL_BATCH", "4")
    series, _ = evaluate_dataset(ds, _predictor(), **kw)
    assert used == [4]
    monkeypatch.delenv("VPU_EVAL_BATCH")
    ref, _ = evaluate_dataset(ds, _predictor(), **kw)
    assert used == [4]                              # default: sequential
    assert [s.tolist() for s in series] == [s.tolist() for s in ref]
    evaluate_dataset(ds, _predictor(), batch_objects=1, **kw)
    assert used == [4]


def test_silent_fallback_to_the_sequential_loop(host_transforms, monkeypatch):
    ds = Dataset(sizes=((40, 56),), per_image=(2,))
    calls = []

    def fake_sample(image, gt_mask, predictor, max_iou_thr, **kw):
        calls.append(kw)
        return [], np.zeros(1, np.float32), None
    monkeypatch.setattr(vpu_evaluation, "evaluate_sample", fake_sample)

    def refuse(*a, **k):
        raise AssertionError("the batched path must not run here")
    monkeypatch.setattr(batched.BatchedEvaluator, "run", refuse)
    cb = lambda *a: None
    evaluate_dataset(ds, _predictor(), batch_objects=4, max_iou_thr=0.8, callback=cb)
    evaluate_dataset(ds, _predictor(), batch_objects=4, max_iou_thr=0.8, as_prompt_type=1)
    evaluate_dataset(ds, _predictor(predictor_params=dict(max_size=40)), batch_objects=4, max_iou_thr=0.8)
    evaluate_dataset(ds, get_predictor(StubNet(), "NoBRS", "cpu", zoom_in_params=dict(target_size=32)), batch_objects=4,
                     max_iou_thr=0.8)                           # a scalar target_size
    assert len(calls) == 8
    assert not batched.batchable(_predictor(), callback=cb)
    assert not batched.batchable(_predictor(), as_prompt_type=2)
    assert not batched.batchable(_predictor(predictor_params=dict(max_size=40)))
    assert batched.batchable(_predictor()) and batched.batchable(get_predictor(StubNet(), "NoBRS", "cpu", zoom_in_params=None))
