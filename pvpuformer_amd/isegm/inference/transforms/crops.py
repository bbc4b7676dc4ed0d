"""Crops (isegm/inference/transforms/crops.py:11-97): a network input at least as large as ``crop_size`` is cut into a grid
of overlapping tiles of exactly that size, which run as one batch; on the way back the tiles' probabilities are averaged
where they overlap.  The network thus keeps seeing its trained resolution however large the image (or the ZoomIn target) is.

GPU-resident: all tiles are taken in one launch and blended in one launch (``_device.crops_gather`` / ``crops_blend``).  The
offsets depend on the input size alone, so their device copies and the coverage map ``_counts`` are built once per
(height, width), not per click; the tiles form a grid, so ``_counts`` is the outer product of two 1-D coverage counts."""
import math

import numpy as np
import torch

from . import _device
from .base import BaseTransform


def get_offsets(length, crop_size, min_overlap_ratio=0.2):
    """Start positions of the fewest tiles of ``crop_size`` that cover ``length`` with at least ``min_overlap_ratio`` of a
    tile shared by neighbours, in the reference's float arithmetic (crops.py:79-97): equal steps of ``crop_size`` minus the
    truncated overlap, the tail clamped so that the last tile ends at ``length``."""
    if length == crop_size:
        return [0]
    ratio = length / crop_size
    count = math.ceil((ratio - min_overlap_ratio) / (1 - min_overlap_ratio))
    overlap_width = int(crop_size * ((count - ratio) / (count - 1)))
    step, last = crop_size - overlap_width, length - crop_size
    return [min(i * step, last) for i in range(count)]


def _coverage(offsets, crop_size, length):
    """How many tiles cover each of ``length`` positions (int64 [length])."""
    edges = np.zeros(length + 1, np.int64)
    for o in offsets:
        edges[o] += 1
        edges[o + crop_size] -= 1
    return np.cumsum(edges[:-1])


class Crops(BaseTransform):
    def __init__(self, crop_size=(320, 480), min_overlap=0.2):
        super().__init__()
        self.crop_height, self.crop_width = crop_size
        self.min_overlap = min_overlap
        self._grid = None               # what depends on (height, width, device) only: see _grid_for
        self.reset()

    def _grid_for(self, height, width, device):
        """(x_offsets, y_offsets, their int32 device copies, _counts) of a height x width input, kept while the size stays."""
        key = (int(height), int(width), torch.device(device))
        if self._grid is None or self._grid[0] != key:
            xs = get_offsets(width, self.crop_width, self.min_overlap)
            ys = get_offsets(height, self.crop_height, self.min_overlap)
            cover = [torch.from_numpy(_coverage(o, c, n).astype(np.float32)).to(device)
                     for o, c, n in ((ys, self.crop_height, height), (xs, self.crop_width, width))]
            self._grid = (key, xs, ys, self._upload(xs, device), self._upload(ys, device), torch.outer(cover[0], cover[1]))
        return self._grid[1:]

    @staticmethod
    def _upload(offsets, device):
        return torch.tensor(list(offsets), dtype=torch.int32).to(device)

    def _device_offsets(self, device):
        """The device copies of the offsets in force (the cached ones unless a restored state names others)."""
        g = self._grid
        if g is not None and g[0][2] == torch.device(device) and list(g[1]) == list(self.x_offsets) and list(g[2]) == list(self.y_offsets):
            return g[3], g[4]
        return self._upload(self.x_offsets, device), self._upload(self.y_offsets, device)

    @property
    def num_tiles(self):
        """Tiles of the last ``transform`` call (1 when the input passed through)."""
        return 1 if self._counts is None else len(self.x_offsets) * len(self.y_offsets)

    def transform(self, image_nd, clicks_lists):
        assert image_nd.shape[0] == 1 and len(clicks_lists) == 1
        height, width = image_nd.shape[2:4]
        self._counts = None
        if height < self.crop_height or width < self.crop_width:
            return image_nd, clicks_lists
        self.x_offsets, self.y_offsets, x_dev, y_dev, self._counts = self._grid_for(height, width, image_nd.device)
        tiles = _device.crops_gather(image_nd, y_dev, x_dev, self.crop_height, self.crop_width)
        clicks = clicks_lists[0]
        shifted = [[c.copy(coords=(c.coords[0] - dy, c.coords[1] - dx)) for c in clicks]
                   for dy in self.y_offsets for dx in self.x_offsets]
        return tiles, shifted

    def inv_transform(self, prob_map):
        if self._counts is None:
            return prob_map
        x_dev, y_dev = self._device_offsets(prob_map.device)
        height, width = self._counts.shape
        return _device.crops_blend(prob_map, y_dev, x_dev, height, width)

    def get_state(self):
        return self.x_offsets, self.y_offsets, self._counts

    def set_state(self, state):
        self.x_offsets, self.y_offsets, self._counts = state

    def reset(self):
        self.x_offsets = None
        self.y_offsets = None
        self._counts = None
