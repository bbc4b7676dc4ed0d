"""The device operations the predictor transforms are built on (module attributes, looked up at call time, so a CPU
test can substitute stand-ins): the ``align_corners=True`` bilinear resize, the bounding box of a thresholded
probability map joined with the positive clicks, and the tile gather / blend of ``Crops``.  All are HIP kernels
(``vpu_upsample_ac_fwd``, ``vpu_mask_bbox``, ``vpu_crops_gather``, ``vpu_crops_blend``); there is no CPU path in the product."""
import torch

from pvpuformer_amd import ops


def resize_align_corners(x, size):
    """``F.interpolate(x, size, mode='bilinear', align_corners=True)`` for a CUDA fp32 NCHW tensor."""
    if not x.is_cuda:
        raise RuntimeError("the predictor transforms run on the GPU only (no CPU resize path exists)")
    n, c, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    src = x.contiguous().float()
    if (h, w) == (H, W):
        return src.clone()
    dst = torch.empty(n, c, H, W, device=x.device, dtype=torch.float32)
    ops.upsample_ac_fwd(src, dst, n * c, h, w, H, W)
    return dst


def crops_gather(image_nd, y_off, x_off, crop_height, crop_width):
    """The tiles of a CUDA [1, C, H, W] tensor, [ny * nx, C, crop_height, crop_width] in (y outer, x inner) order, in one launch
    (``vpu_crops_gather``); ``y_off`` / ``x_off``: int32 offset arrays on the image's device."""
    if not image_nd.is_cuda:
        raise RuntimeError("the predictor transforms run on the GPU only (no CPU tiling path exists)")
    return ops.crops_gather(image_nd[0].contiguous().float(), y_off, x_off, int(crop_height), int(crop_width))


def crops_blend(prob_map, y_off, x_off, height, width):
    """[ny * nx, 1, ch, cw] tile probabilities -> [1, 1, height, width]: added in tile order, divided by the number of covering
    tiles (``vpu_crops_blend``)."""
    if not prob_map.is_cuda:
        raise RuntimeError("the predictor transforms run on the GPU only (no CPU tiling path exists)")
    probs = prob_map[:, 0].contiguous().float()
    return ops.crops_blend(probs, y_off, x_off, int(height), int(width))[None, None]


def mask_box(prob, thr, positive_clicks=()):
    """(count, rmin, rmax, cmin, cmax) of ``prob[0, 0] > thr`` joined with the integer (row, col) positive clicks: the map
    stays on the device, five integers come back (the one host synchronisation of a ZoomIn step)."""
    if not prob.is_cuda:
        raise RuntimeError("the predictor transforms run on the GPU only (no CPU path exists)")
    clicks = None
    if len(positive_clicks):
        clicks = torch.tensor([[int(r), int(c)] for r, c in positive_clicks], dtype=torch.int32).to(prob.device, non_blocking=True)
    p = prob[0, 0].contiguous().float().unsqueeze(0)
    return tuple(ops.mask_bbox(p, thr, clicks)[0].tolist())
