"""Region clean-up on the device: small islands dropped, small holes filled.

``tidy(M, seeds, min_area, max_hole, keep)`` on a binary map ``M`` [H, W]; ``seeds`` is a list of (row, col, positive), a seed
outside the image is ignored:

  T1  foreground components are the 8-connected components of ``M``.
  T2  a component is protected when it holds a positive seed.
  T3  kept are the protected components plus, by ``keep``: "all" every component of area >= ``min_area``; "seeded" nothing
      more (without a positive seed on the foreground the result is empty: there is no fallback); "largest" the one of
      greatest area, ties going to the smallest linear index of its first pixel in raster order (``min_area`` is not read).
  T4  M1 = the union of the kept components.
  T5  holes are the 4-connected components of ``~M1`` that hold no pixel of the first or last row or column; a hole is
      filled when its area is <= ``max_hole`` and it holds no negative seed (``max_hole`` 0: none, None: every hole).
  T6  M2 = M1 | filled.
  T7  every fp32 map of the call is copied to its output with 0.0 where M & ~M2 and 1.0 where M2 & ~M; every other pixel
      keeps its bits (an island removed inside a hole that is then filled stays as it was).
  T8  the record is int32 [8] = {|M2|, |M & ~M2|, |M2 & ~M|, rmin, rmax, cmin, cmax, kept components}, the box (H, -1, W, -1)
      of an empty M2; the packed mask of M2 has ``pack_mask``'s bit order.  The kept components are counted as they stand
      in the result: the last entry is the number of 8-connected components of M2.

Islands first, holes from the result: a speck inside a pinhole goes with the pinhole.  The rule is idempotent.  Filling adds
no component and splits none; it joins two only where a kept island lies inside a hole that is filled (the hole is the
4-connected background between the ring and the island), and the record then counts them as the one component they have
become, so a second ``tidy`` of the result returns the same record.

``vpu_regions_tidy_batched`` (csrc/evalbatch.hip, section 9) does this for n maps of different sizes without a component
table and without a host round trip (``DeviceRegionOps``); ``host_regions_tidy`` is the numpy + scipy stand-in
(``HostRegionOps``), which a CPU pool runs on and which a pool's ``ops_regions`` may be replaced by."""
import ctypes

import numpy as np
import torch
from scipy import ndimage

from ._batchcore import PackedLayout, host_count_box, pack_mask, unpack_mask

KEEP_MODES = {"all": 0, "seeded": 1, "largest": 2}      # VPU_TIDY_ALL / SEEDED / LARGEST
INT32_MAX = 2 ** 31 - 1
_EIGHT = np.ones((3, 3), dtype=np.int32)
_FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.int32)


def check_tidy_args(who, min_area, max_hole, keep):
    """The checked (min_area, max_hole) of a ``tidy`` call, ``max_hole`` None -> INT32_MAX; ValueError for an unknown ``keep`` or
    a negative area."""
    if keep not in KEEP_MODES:
        raise ValueError(f"{who}: keep must be one of {sorted(KEEP_MODES)}, not {keep!r}")
    max_hole = INT32_MAX if max_hole is None else max_hole
    for name, v in (("min_area", min_area), ("max_hole", max_hole)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v <= INT32_MAX:
            raise ValueError(f"{who}: {name} must be an integer in 0 .. {INT32_MAX}, not {v!r}")
    return int(min_area), int(max_hole)


def click_seeds(clicks):
    """[(row, col, positive)] of a list of ``Click`` or of (is_positive, (row, col))."""
    out = []
    for c in clicks:
        positive, (row, col) = (c.is_positive, c.coords) if hasattr(c, "is_positive") else (c[0], c[1])
        out.append((int(row), int(col), bool(positive)))
    return out


# ------------------------------------------------------------------------------------------------------ the host stand-in
def host_regions_tidy(add, total, H, W, seeds, min_area, max_hole, keep, thr):
    """Stand-in of vpu_regions_tidy_batched for one map.  ``add`` / ``total``: fp32 [H, W] or None (zeros); neither is
    written -> (add_out or None, total_out or None, packed mask uint64, record int32 [8])."""
    min_area, max_hole = check_tidy_args("host_regions_tidy", min_area, max_hole, keep)
    zeros = np.zeros((H, W), dtype=np.float32)
    M = np.maximum(zeros if total is None else total, zeros if add is None else add) > np.float32(thr)
    seeds = [(r, c, bool(p)) for r, c, p in seeds if 0 <= r < H and 0 <= c < W]
    # T1-T4
    lab, k = ndimage.label(M, structure=_EIGHT)
    areas = np.bincount(lab.reshape(-1), minlength=k + 1)
    kept = np.zeros(k + 1, dtype=bool)
    for r, c, positive in seeds:
        if positive and lab[r, c]:
            kept[lab[r, c]] = True
    if keep == "all":
        kept[1:] |= areas[1:] >= min_area
    elif keep == "largest" and k:
        first = np.full(k + 1, H * W, dtype=np.int64)
        np.minimum.at(first, lab.reshape(-1), np.arange(H * W))
        best = max(range(1, k + 1), key=lambda j: (areas[j], -first[j]))
        kept[best] = True
    M1 = kept[lab]
    # T5-T6
    back, kb = ndimage.label(~M1, structure=_FOUR)
    sizes = np.bincount(back.reshape(-1), minlength=kb + 1)
    blocked = np.zeros(kb + 1, dtype=bool)
    blocked[0] = True
    blocked[np.concatenate((back[0], back[-1], back[:, 0], back[:, -1]))] = True
    for r, c, positive in seeds:
        if not positive:
            blocked[back[r, c]] = True
    blocked[0] = True
    M2 = M1 | (~blocked & (sizes <= max_hole))[back]
    # T7-T8
    outs = []
    for src in (add, total):
        out = None if src is None else np.array(src, dtype=np.float32, copy=True).reshape(H, W)
        if out is not None:
            out[M & ~M2] = 0.0
            out[M2 & ~M] = 1.0
        outs.append(out)
    area, *box = host_count_box(M2, H, W)
    components = ndimage.label(M2, structure=_EIGHT)[1]
    rec = np.array([area, int((M & ~M2).sum()), int((M2 & ~M).sum())] + box + [components], dtype=np.int32)
    return outs[0], outs[1], pack_mask(M2), rec


# ------------------------------------------------------------------------------------------------------ the two routes
class TidyItem:
    """One map of a ``tidy`` call.  ``add`` / ``total``: fp32 [H, W] tensors or None (zeros); ``add_out`` / ``total_out``: the
    tensors the edited maps are written to (only for a map that is given), or None; an output may be its own input.
    ``seeds``: [(row, col, positive)]."""

    def __init__(self, H, W, add=None, total=None, add_out=None, total_out=None, seeds=(), min_area=0, max_hole=0, keep="all"):
        self.H, self.W, self.add, self.total, self.add_out, self.total_out = int(H), int(W), add, total, add_out, total_out
        self.seeds = [(int(r), int(c), bool(p)) for r, c, p in seeds]
        self.min_area, self.max_hole = check_tidy_args("tidy", min_area, max_hole, keep)
        self.keep = keep
        if (add is None and add_out is not None) or (total is None and total_out is not None):
            raise ValueError("tidy: an output map without its input map")


class DeviceRegionOps:
    """The HIP kernels: descriptors and seeds go up in one copy, records and packed masks come back in one."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self._ops, self.device = _lib, ops, torch.device(device)

    def tidy(self, items, thr, read):
        """``read``: "masks" -> [(record, mask bool [H, W])], "records" -> [(record, None)] (one read-back each), None ->
        nothing is read back and nothing waited for."""
        n, layout = len(items), PackedLayout([(it.H, it.W) for it in items])
        out = torch.empty(layout.size, device=self.device, dtype=torch.int64)
        size = ctypes.sizeof(self._lib.TidyObj)
        seeds_at, total = [], n * size
        for it in items:
            seeds_at.append(total)
            total += 12 * len(it.seeds)
        scratch_at, ints = [], 0
        for it in items:
            assert it.H >= 1 and it.W >= 1 and it.H * it.W < 2 ** 31
            scratch_at.append(ints)
            ints += (self._ops.tidy_scratch_ints(it.H * it.W) + 3) // 4 * 4         # every slice 16-byte aligned
        scratch = torch.empty(ints, device=self.device, dtype=torch.int32)
        dev = torch.empty(total, device=self.device, dtype=torch.uint8)
        assert out.data_ptr() % 8 == 0 and scratch.data_ptr() % 16 == 0 and dev.data_ptr() % 8 == 0
        raw, rows = np.empty(total, dtype=np.uint8), []
        for i, it in enumerate(items):
            for t in (it.add, it.total, it.add_out, it.total_out):
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == it.H * it.W
                                     and t.device == out.device and t.data_ptr() % 16 == 0)
            d = self._lib.TidyObj()
            for name in ("add", "total", "add_out", "total_out"):
                t = getattr(it, name)
                setattr(d, name, t.data_ptr() if t is not None else None)
            d.bits = out.data_ptr() + 8 * layout.bits_at(i)
            d.rec = out.data_ptr() + 8 * layout.rec_at(i)
            d.seeds = dev.data_ptr() + seeds_at[i] if it.seeds else None
            d.scratch = scratch.data_ptr() + 4 * scratch_at[i]
            d.H, d.W, d.n_seeds, d.min_area, d.max_hole, d.keep = it.H, it.W, len(it.seeds), it.min_area, it.max_hole, KEEP_MODES[it.keep]
            rows.append(d)
            if it.seeds:
                # (a coordinate that does not fit an int32 is outside every image: -1 is ignored as it would be)
                s = np.array(it.seeds, dtype=np.int64).reshape(-1, 3)
                s[(np.abs(s) > INT32_MAX).any(1)] = (-1, -1, 0)
                raw[seeds_at[i]:seeds_at[i] + 12 * len(it.seeds)].view(np.int32)[...] = s.astype(np.int32).reshape(-1)
        raw[:n * size] = np.frombuffer(bytes((self._lib.TidyObj * n)(*rows)), dtype=np.uint8)
        host = torch.from_numpy(raw).pin_memory()                     # (alive until the launches are enqueued)
        dev.copy_(host, non_blocking=True)
        self._ops.regions_tidy_batched(dev, host, n, thr)
        if read is None:
            self._pending = host                                      # (the copy up may still be in flight)
            return None
        got = (out if read == "masks" else out[:layout.rec_at(n)]).cpu().numpy()        # the call's one synchronisation
        return [layout.decode(got, i, read == "masks") for i in range(n)]


class HostRegionOps:
    """The numpy + scipy stand-in behind the same call; maps on a device are copied to the host and the edited ones back."""

    def __init__(self, device=None):
        self.device = device

    @staticmethod
    def _host(t):
        return None if t is None else t.detach().cpu().numpy()

    def tidy(self, items, thr, read):
        got = []
        for it in items:
            add, total, words, rec = host_regions_tidy(self._host(it.add), self._host(it.total), it.H, it.W, it.seeds, it.min_area,
                                                       it.max_hole, it.keep, thr)
            for dst, src in ((it.add_out, add), (it.total_out, total)):
                if dst is not None:
                    dst.copy_(torch.from_numpy(src).reshape(dst.shape))
            got.append((rec, unpack_mask(words, it.H, it.W) if read == "masks" else None))
        return None if read is None else got
