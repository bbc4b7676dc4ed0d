"""Run-length maps: a session's mask or an annotation's label map as the runs of COCO's column-major stream.

For an ``H x W`` map of integer values ``v(r, c)`` the stream is ``i = c * H + r``; a run starts at ``i`` when ``i == 0`` or
``v_i != v_{i-1}``.  The predecessor relation crosses column boundaries -- that of ``(0, c)`` is ``(H - 1, c - 1)`` -- so a
value that continues from the bottom of one column into the top of the next starts no run.  A ``RunMap`` is the list of
``(start, value)`` in increasing ``start``; it has at least one entry.  ``counts(label)`` is COCO's uncompressed ``counts``
of the binary mask ``v == label`` (the compressed string form is not produced here).

``vpu_runs_count_batched`` / ``vpu_runs_write_batched`` (csrc/evalbatch.hip, section 8) encode n maps of different sizes
on the device; what crosses to the host is ``4 (n + 1)`` bytes of offsets and 8 bytes per run, in two read-backs with the
exact allocation between them.  ``host_runs_encode`` is the numpy stand-in (``HostRunOps``), which runs
on a CPU pool and may replace ``ops_runs`` of a device pool.

The way back: ``RunMap.from_coco`` reads COCO's uncompressed form, ``stack_objects`` merges a list of
binary maps into one label ``RunMap`` on the host without a raster, and ``vpu_runs_decode_batched`` (section 9 of the same
file) decodes n streams into n maps on the device; what crosses to the device is 40 bytes per map and 8 bytes per run, in
one copy, and nothing comes back.  ``host_runs_decode`` is its stand-in."""
import ctypes

import numpy as np
import torch

from ._batchcore import upload_structs

KIND_PROB, KIND_LABELS = 0, 1     # vpu_runs_obj.kind: fp32 map > thr (values 0 / 1), 16-bit label map
#                                 # vpu_unrun_obj.kind: fp32 map of value == label, 16-bit label map


class RunMap:
    """``size = (H, W)``; ``starts`` / ``values``: int32 [n], the stream index at which each run starts and its value."""

    def __init__(self, size, starts, values):
        self.size = (int(size[0]), int(size[1]))
        self.starts = np.ascontiguousarray(starts, dtype=np.int32)
        self.values = np.ascontiguousarray(values, dtype=np.int32)
        assert self.starts.ndim == 1 and self.starts.shape == self.values.shape and len(self.starts) >= 1 and self.starts[0] == 0

    def __len__(self):
        return len(self.starts)

    def lengths(self):
        return np.diff(self.starts, append=np.int32(self.size[0] * self.size[1]))

    def decode(self):
        """uint16 [H, W]: the map of values."""
        H, W = self.size
        return np.ascontiguousarray(np.repeat(self.values.astype(np.uint16), self.lengths()).reshape(W, H).T)

    def counts(self, label=1):
        """COCO's uncompressed counts of ``v == label``: a list of ints that alternates clear / set, starts with the clear
        count (0 when the first stream pixel is set) and sums to H * W; neighbouring runs that are alike are merged."""
        on = self.values == np.int32(label)
        first = np.flatnonzero(np.concatenate(([True], on[1:] != on[:-1])))
        counts = np.add.reduceat(self.lengths().astype(np.int64), first).tolist()
        return [0] + counts if on[0] else counts

    def to_coco(self, label=1):
        return dict(size=[self.size[0], self.size[1]], counts=self.counts(label))

    def area(self, label=1):
        return int(self.lengths()[self.values == np.int32(label)].sum())

    @classmethod
    def from_coco(cls, seg, label=1):
        """The map with values 0 / ``label`` of ``seg = dict(size=[H, W], counts=[...])``, COCO's uncompressed form: counts
        alternate clear / set and start with the clear count.  Zero counts are dropped and the neighbours merged, so starts
        increase strictly and neighbouring values differ.  ValueError for counts that are negative, not integers or do not
        sum to H * W; TypeError for the compressed string form, which is not read here (there is nothing to check a
        restatement of that coder against)."""
        counts = seg["counts"]
        if isinstance(counts, (str, bytes, bytearray)):
            raise TypeError("RunMap.from_coco: compressed (string) counts are not read; pass the uncompressed list")
        H, W = (int(v) for v in seg["size"])
        if not (isinstance(label, (int, np.integer)) and 1 <= label <= 65535):
            raise ValueError(f"RunMap.from_coco: label {label!r} is not an integer in 1 .. 65535")
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"RunMap.from_coco: size {H} x {W} (H, W >= 1, H * W < 2^31)")
        c = np.asarray(counts)
        if c.ndim != 1 or (len(c) and c.dtype.kind not in "iu"):
            raise ValueError("RunMap.from_coco: counts must be a flat list of integers")
        c = c.astype(np.int64)
        if (c < 0).any() or int(c.sum()) != H * W:
            raise ValueError(f"RunMap.from_coco: counts are negative or do not sum to H * W = {H * W}")
        starts = np.cumsum(c) - c
        values = np.where(np.arange(len(c)) % 2 == 1, np.int32(label), np.int32(0))
        starts, values = starts[c > 0], values[c > 0]
        first = np.concatenate(([True], values[1:] != values[:-1]))
        return cls((H, W), starts[first], values[first])

    def check(self):
        """ValueError unless the stream is one the decoder may be given: starts[0] == 0, starts increase strictly, the last
        start is below H * W, values lie in 0 .. 65535."""
        H, W = self.size
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"RunMap: size {H} x {W} (H, W >= 1, H * W < 2^31)")
        if self.starts.ndim != 1 or self.starts.shape != self.values.shape or len(self.starts) < 1:
            raise ValueError("RunMap: starts and values must be two flat arrays of one length, at least 1")
        if self.starts[0] != 0 or (np.diff(self.starts.astype(np.int64)) <= 0).any() or self.starts[-1] >= H * W:
            raise ValueError("RunMap: starts must begin at 0, increase strictly and stay below H * W")
        if (self.values < 0).any() or (self.values > 65535).any():
            raise ValueError("RunMap: values must lie in 0 .. 65535")
        return self

    def box(self, label=1):
        """Inclusive ``(rmin, rmax, cmin, cmax)`` of ``v == label`` from the runs, without a raster; ``(H, -1, W, -1)`` when no
        pixel holds ``label``.  A run that crosses a column boundary spans the rows 0 .. H - 1."""
        return _box(self.size, self.starts, self.lengths(), self.values == np.int32(label))


def _box(size, starts, lengths, on):
    H, W = size
    if not on.any():
        return (H, -1, W, -1)
    first = starts[on].astype(np.int64)
    last = first + lengths[on].astype(np.int64) - 1
    c0, c1 = first // H, last // H
    rmin = np.where(c1 > c0, 0, first % H).min()          # a run that reaches the next column holds the bottom row of this
    rmax = np.where(c1 > c0, H - 1, last % H).max()       # one and the top row of that one
    return (int(rmin), int(rmax), int(c0.min()), int(c1.max()))


# ------------------------------------------------------------------------------------------------------ host stand-in
def _values(array, kind, thr):
    array = np.asarray(array)
    assert array.ndim == 2 and kind in (KIND_PROB, KIND_LABELS)
    if kind == KIND_PROB:
        assert array.dtype == np.float32
        return (array > np.float32(thr)).astype(np.uint16)
    assert array.dtype in (np.uint16, np.int16)
    return array.view(np.uint16)


def host_runs_encode(array, kind, thr=0.0):
    """Stand-in of the two kernels for one map: ``array`` fp32 [H, W] (kind 0: v = array > thr, strict, in fp32) or 16-bit
    [H, W] (kind 1: v = the value as uint16) -> RunMap."""
    v = _values(array, kind, thr)
    flat = v.flatten(order="F")
    starts = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1))
    return RunMap(v.shape, starts, flat[starts])


def host_runs_decode(rm, kind, label=1):
    """Stand-in of vpu_runs_decode_batched for one map: kind 1 -> uint16 [H, W] of the values, kind 0 -> fp32 [H, W] of
    ``value == label``."""
    assert kind in (KIND_PROB, KIND_LABELS)
    v = rm.decode()
    return v if kind == KIND_LABELS else (v.astype(np.int32) == int(label)).astype(np.float32)


def as_run_map(value, label=1):
    """``value``: a RunMap (as it is) or a COCO ``dict(size, counts)`` (``from_coco(value, label)``), checked."""
    rm = value if isinstance(value, RunMap) else RunMap.from_coco(value, label)
    return rm.check()


def stack_objects(size, maps, labels=None):
    """Binary maps painted into ONE label map in list order, later ones over earlier ones, as ``AnnotationPool.finish`` does.
    ``maps``: RunMaps or COCO dicts of ``size``, a pixel set where ``v != 0``; ``labels``: one per map, integers in
    1 .. 65535, default 1 .. K -> ``(RunMap, records)``, ``records[k] = dict(label, area, box, overwritten)`` with ``finish``'s
    definitions: area and box of the map as given, ``overwritten`` = those of its pixels that held another, earlier label when
    it was painted.  Works on the union of the break points; no raster is built.  K == 0 gives the single run (0, 0)."""
    H, W = int(size[0]), int(size[1])
    maps = [as_run_map(m) for m in maps]
    K = len(maps)
    labels = list(range(1, K + 1)) if labels is None else list(labels)
    if len(labels) != K:
        raise ValueError(f"stack_objects: {len(labels)} labels for {K} maps")
    for label in labels:
        if not (isinstance(label, (int, np.integer)) and 1 <= label <= 65535):
            raise ValueError(f"stack_objects: label {label!r} is not an integer in 1 .. 65535")
    for m in maps:
        if m.size != (H, W):
            raise ValueError(f"stack_objects: a map of {m.size} among maps of {(H, W)}")
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"stack_objects: size {H} x {W} (H, W >= 1, H * W < 2^31)")
    breaks = np.unique(np.concatenate([np.zeros(1, dtype=np.int32)] + [m.starts for m in maps]))
    lengths = np.diff(breaks.astype(np.int64), append=np.int64(H * W))
    current = np.zeros(len(breaks), dtype=np.int32)
    records = []
    for m, label in zip(maps, labels):
        on = m.values[np.searchsorted(m.starts, breaks, side="right") - 1] != 0
        over = on & (current != 0) & (current != np.int32(label))
        records.append(dict(label=int(label), area=int(lengths[on].sum()), box=_box((H, W), m.starts, m.lengths(), m.values != 0),
                            overwritten=int(lengths[over].sum())))
        current[on] = label
    first = np.concatenate(([True], current[1:] != current[:-1]))
    return RunMap((H, W), breaks[first], current[first]), records


# ------------------------------------------------------------------------------------------------------ the op classes
def _check_decode_item(rm, dst, kind, label):
    rm.check()
    _check_item(dst, kind)
    assert tuple(dst.shape) == rm.size and (kind == KIND_LABELS or 0 <= int(label) <= 65535)


def _check_item(tensor, kind):
    assert kind in (KIND_PROB, KIND_LABELS) and tensor.dim() == 2 and tensor.is_contiguous()
    assert tensor.dtype == (torch.float32 if kind == KIND_PROB else torch.int16)
    assert tensor.shape[0] >= 1 and tensor.shape[1] >= 1 and tensor.numel() < 2 ** 31


class DeviceRunOps:
    """The HIP kernels.  ``encode(items)``, items [(tensor [H, W], kind, thr)], fp32 for kind 0, int16 storage of uint16
    labels for kind 1 -> [RunMap].  The descriptors go up in one pinned copy; the header comes back (synchronisation 1,
    ``4 (n + 1)`` bytes), exactly ``header[n]`` entries are allocated and written, and they come back (synchronisation 2,
    8 bytes per run)."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self._ops, self.device = _lib, ops, torch.device(device)

    def encode(self, items):
        n = len(items)
        if n == 0:
            return []
        rows = []
        for tensor, kind, thr in items:
            _check_item(tensor, kind)
            assert tensor.device == self.device or (tensor.is_cuda and self.device.index is None)
            assert tensor.data_ptr() % (16 if kind == KIND_PROB else 8) == 0
            d = self._lib.RunsObj()
            d.src, d.H, d.W, d.kind, d.thr = tensor.data_ptr(), tensor.shape[0], tensor.shape[1], kind, float(thr)
            rows.append(d)
        host, desc, _ = upload_structs(self.device, (self._lib.RunsObj * n)(*rows))    # (host: alive until the last read-back)
        sizes = [tuple(t.shape) for t, _, _ in items]
        scratch = torch.empty(self._ops.runs_scratch_len(sizes), device=self.device, dtype=torch.int32)
        header = torch.empty(n + 1, device=self.device, dtype=torch.int32)
        self._ops.runs_count_batched(desc, host, n, scratch, header)
        at = header.cpu().numpy()                                                      # synchronisation 1
        entries = torch.empty(int(at[n]), 2, device=self.device, dtype=torch.int32)
        self._ops.runs_write_batched(desc, host, n, scratch, entries)
        got = entries.cpu().numpy()                                                    # synchronisation 2
        return [RunMap(sizes[k], got[at[k]:at[k + 1], 0], got[at[k]:at[k + 1], 1]) for k in range(n)]

    def decode(self, items):
        """``items``: [(RunMap, dst [H, W], kind, label)]; ``dst`` is written in place: fp32 1 / 0 of ``value == label`` (kind 0,
        16-byte aligned) or the values in int16 storage (kind 1, 8-byte aligned).  The descriptors and, behind them, all
        entries go up in ONE pinned copy, each descriptor pointing into that buffer; one launch, nothing comes back."""
        n = len(items)
        if n == 0:
            return
        size = ctypes.sizeof(self._lib.UnrunObj)
        assert (n * size) % 8 == 0
        at, total = [], n * size
        for rm, dst, kind, label in items:
            _check_decode_item(rm, dst, kind, label)
            assert dst.device == self.device or (dst.is_cuda and self.device.index is None)
            assert dst.data_ptr() % (16 if kind == KIND_PROB else 8) == 0
            at.append(total)
            total += 8 * len(rm)
        dev = torch.empty(total, device=self.device, dtype=torch.uint8)
        assert dev.data_ptr() % 8 == 0
        raw = np.empty(total, dtype=np.uint8)
        rows = []
        for (rm, dst, kind, label), off in zip(items, at):
            d = self._lib.UnrunObj()
            d.dst, d.entries, d.H, d.W = dst.data_ptr(), dev.data_ptr() + off, rm.size[0], rm.size[1]
            d.n_runs, d.kind, d.label, d.pad = len(rm), kind, int(label) if kind == KIND_PROB else 0, 0
            rows.append(d)
            raw[off:off + 8 * len(rm)].view(np.int32).reshape(-1, 2)[...] = np.stack((rm.starts, rm.values), axis=1)
        raw[:n * size] = np.frombuffer(bytes((self._lib.UnrunObj * n)(*rows)), dtype=np.uint8)
        host = torch.from_numpy(raw).pin_memory()                     # (alive until the launch is enqueued)
        dev.copy_(host, non_blocking=True)
        self._ops.runs_decode_batched(dev, host, n)


class HostRunOps:
    """The numpy stand-in behind the same call; maps on a device are copied to the host."""

    def __init__(self, device=None):
        self.device = device

    def encode(self, items):
        out = []
        for tensor, kind, thr in items:
            _check_item(tensor, kind)
            out.append(host_runs_encode(tensor.detach().cpu().numpy(), kind, thr))
        return out

    def decode(self, items):
        for rm, dst, kind, label in items:
            _check_decode_item(rm, dst, kind, label)
            got = host_runs_decode(rm, kind, label)
            dst.copy_(torch.from_numpy(got.view(np.int16) if kind == KIND_LABELS else got))
