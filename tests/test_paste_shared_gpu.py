"""GPU: ``vpu_roi_paste_batched`` at shapes below a block and with a tail (csrc/evalbatch.hip: its canvas, mask and statistics
come through the record reduction and the pixel function that the session and annotation kernels share), and
``vpu_session_paste_batched`` against it on the same inputs.  Shapes, rois and maps are those of test_sessions_gpu.py."""
import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference import batched
from pvpuformer_amd.isegm.inference.transforms import ZoomIn

from sessions_cases import PRED_THR
from test_sessions_gpu import BOX_THR, MAP, SIZES, _launch, _maps, _need_gpu, _roi

pytestmark = pytest.mark.gpu

KINDS = ("whole", "interior", "two corners", "one row", "copy")


def _objects():
    """One evaluation object per size: a ground truth with pixels on both sides of any mask (40 % set, at random) and a valid
    map with holes (15 % of the pixels at random and one whole row are ignored)."""
    g = torch.Generator().manual_seed(3)
    objs = []
    for j, (H, W) in enumerate(SIZES):
        gt = (torch.rand(H, W, generator=g) < 0.4).numpy().astype(np.int32)
        gt[torch.rand(H, W, generator=g).numpy() < 0.15] = -1
        gt[H // 2, :] = -1
        objs.append(batched._Object(j, torch.zeros(3, H, W, device="cuda"), gt, "cuda"))
    return objs


def _paste(objs, members, rois, probs):
    """One launch of vpu_roi_paste_batched over ``members`` (indices into SIZES) -> the int32 [8] statistics of each."""
    ops = batched._DeviceOps("cuda")
    ops.begin(len(members))
    ops.out.fill_(-1)                                       # (stale records)
    for k, (j, roi) in enumerate(zip(members, rois)):
        o = objs[j]
        o.canvas[1 - o.prev].fill_(7.0)                     # (stale canvas and mask everywhere)
        o.mask.fill_(9)
        ops.add(o, roi, j, k)
    ops.upload()
    ops.paste([objs[j] for j in members], 0, len(members), probs, PRED_THR, BOX_THR)
    out = ops.readback()
    return [out[k, 2:].view(np.int32) for k in range(len(members))]


def _launches(n):
    return [list(range(len(SIZES)))] if n == 4 else [[j] for j in range(len(SIZES))]


@pytest.mark.parametrize("n", [4, 1])
def test_roi_paste_kernel_small_shapes(n):
    _need_gpu()
    probs = _maps().cuda()
    objs = _objects()
    both_sides = False
    for kind in KINDS:
        for members in _launches(n):
            rois = [_roi(kind, *SIZES[j]) for j in members]
            for j, roi, stats in zip(members, rois, _paste(objs, members, rois, probs)):
                H, W = SIZES[j]
                o, tag = objs[j], (kind, n, (H, W))
                canvas = o.canvas[1 - o.prev]
                z = ZoomIn(target_size=(MAP, MAP))
                z._object_roi, z._probs = roi, torch.zeros(1, 1, H, W, device="cuda")
                assert torch.equal(canvas, z.inv_transform(probs[j:j + 1])[0, 0]), tag
                # mask and statistics: exactly those of the kernel's own canvas
                values = canvas.cpu().numpy()
                mask = values > np.float32(PRED_THR)
                assert np.array_equal(o.mask.cpu().numpy(), mask.astype(np.uint8)), tag
                gt, valid = o.gt.cpu().numpy() != 0, o.valid.cpu().numpy() != 0
                inter, uni = int((mask & gt & valid).sum()), int(((mask | gt) & valid).sum())
                both_sides |= 0 < inter < int((gt & valid).sum()) and bool((mask & ~gt & valid).any())
                on = np.argwhere(values > np.float32(BOX_THR))
                box = [len(on), on[:, 0].min(), on[:, 0].max(), on[:, 1].min(), on[:, 1].max()] if len(on) else [0, H, -1, W, -1]
                assert stats.tolist() == [inter, uni] + [int(v) for v in box] + [0], tag
                if (roi[1] - roi[0] + 1, roi[3] - roi[2] + 1) == (MAP, MAP):
                    # the planted threshold values lie inside the roi, outside mask and box
                    r0, c0 = roi[0], roi[2]
                    assert values[r0 + 2, c0 + 4] == np.float32(PRED_THR) and not mask[r0 + 2, c0 + 4], tag
                    if j != 2:
                        assert values[r0 + 1, c0 + 28] == np.float32(BOX_THR) and mask[r0 + 1, c0 + 28], tag
                        assert stats[2:7].tolist() == [12 * 13, r0 + 9, r0 + 20, c0 + 12, c0 + 24], tag
                    else:
                        assert stats[2:7].tolist() == [0, H, -1, W, -1], tag
    assert both_sides                                       # the ground truth does lie on both sides of a mask


@pytest.mark.parametrize("form", [0, 1])
def test_session_paste_equals_roi_paste(form):
    """The same maps and rois through both kernels: identical canvas bytes, the session's {count, box} is the paste's, and
    its area is the number of pixels in the paste's uint8 mask."""
    _need_gpu()
    probs = _maps().cuda()
    objs = _objects()
    members = list(range(len(SIZES)))
    for kind in KINDS:
        rois = [_roi(kind, *SIZES[j]) for j in members]
        stats = _paste(objs, members, rois, probs)
        for j, (canvas, rec, _) in zip(members, _launch(members, rois, probs, form)):
            o, tag = objs[j], (kind, form, SIZES[j])
            assert torch.equal(canvas.view(torch.int32), o.canvas[1 - o.prev].view(torch.int32)), tag
            assert rec[1:6].tolist() == stats[j][2:7].tolist(), tag
            assert int(rec[0]) == int(o.mask.sum()), tag
            assert rec[6:].tolist() == [0, 0], tag
