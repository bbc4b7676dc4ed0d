"""Shared by test_crops_cpu.py and test_crops_gpu.py: torch stand-ins of the two ``Crops`` device operations (the
reference's formulas restated: slice and cat; zeros, ``+=``, ``div``), a ``Crops`` that always uses them, the kernel cases
and a stub network that records its calls."""
import os
from unittest import mock

import numpy as np
import torch

from pvpuformer_amd.isegm.inference.transforms import Crops, _device

from sessions_cases import StubNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crops.npz")

# (H, W, crop_height, crop_width, min_overlap)
KERNEL_CASES = [
    (32, 32, 32, 32, 0.2),       # one tile
    (33, 36, 32, 32, 0.2),       # row offset 1, column offset 4
    (47, 70, 32, 32, 0.2),       # column offsets 19 and 38, W % 4 == 2
    (100, 37, 32, 32, 0.5),      # overlap three deep in rows, odd W
    (50, 90, 24, 40, 0.2),       # a crop that is not square
    (45, 61, 30, 30, 0.2),       # cw % 4 != 0
]
FIXTURE_CASES = ("a", "b")


def fixture():
    return np.load(GOLDEN)


def host_gather(image_nd, y_off, x_off, crop_height, crop_width):
    """[1, C, H, W] -> [ny * nx, C, ch, cw]: one slice per tile, y outer and x inner, concatenated."""
    return torch.cat([image_nd[:, :, dy:dy + crop_height, dx:dx + crop_width]
                      for dy in y_off.tolist() for dx in x_off.tolist()], dim=0)


def host_blend(prob_map, y_off, x_off, height, width):
    """[ny * nx, 1, ch, cw] -> [1, 1, H, W]: every tile added into zeros at its place in tile order, divided by the float32
    map of how many tiles cover each pixel (counted tile by tile in float64, as the reference does)."""
    ch, cw = prob_map.shape[2:]
    canvas = torch.zeros((1, 1, height, width), dtype=prob_map.dtype, device=prob_map.device)
    counts = np.zeros((height, width))
    t = 0
    for dy in y_off.tolist():
        for dx in x_off.tolist():
            canvas[0, 0, dy:dy + ch, dx:dx + cw] += prob_map[t, 0]
            counts[dy:dy + ch, dx:dx + cw] += 1
            t += 1
    return torch.div(canvas, torch.tensor(counts, device=prob_map.device, dtype=torch.float32))


class StandInCrops(Crops):
    """``Crops`` whose two device operations are the torch stand-ins, whatever ``_device`` holds."""

    def transform(self, image_nd, clicks_lists):
        with mock.patch.object(_device, "crops_gather", host_gather):
            return super().transform(image_nd, clicks_lists)

    def inv_transform(self, prob_map):
        with mock.patch.object(_device, "crops_blend", host_blend):
            return super().inv_transform(prob_map)


class RecordingNet(StubNet):
    """``StubNet`` (each row computed alone from its image and clicks) that keeps the shape of every call and its points."""

    def __init__(self, with_prev_mask=True):
        self.with_prev_mask = with_prev_mask
        self.calls = []

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        self.calls.append((tuple(image.shape), points.clone()))
        if not self.with_prev_mask:
            image = torch.cat([image, torch.zeros_like(image[:, :1])], dim=1)
        return super().__call__(image, points, prompts, as_prompt_type)
