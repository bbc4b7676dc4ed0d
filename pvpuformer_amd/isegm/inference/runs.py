"""Run-length maps: a session's mask or an annotation's label map as the runs of COCO's column-major stream.

For an ``H x W`` map of integer values ``v(r, c)`` the stream is ``i = c * H + r``; a run starts at ``i`` when ``i == 0`` or
``v_i != v_{i-1}``.  The predecessor relation crosses column boundaries -- that of ``(0, c)`` is ``(H - 1, c - 1)`` -- so a
value that continues from the bottom of one column into the top of the next starts no run.  A ``RunMap`` is the list of
``(start, value)`` in increasing ``start``; it has at least one entry.  ``counts(label)`` is COCO's uncompressed ``counts``
of the binary mask ``v == label`` (the compressed string form is not produced here).

``vpu_runs_count_batched`` / ``vpu_runs_write_batched`` (csrc/evalbatch.hip, section 8) encode n maps of different sizes
on the device; what crosses to the host is ``4 (n + 1)`` bytes of offsets and 8 bytes per run, in two read-backs with the
exact allocation between them.  ``host_runs_encode`` is the numpy stand-in (``HostRunOps``), which runs
on a CPU pool and may replace ``ops_runs`` of a device pool."""
import numpy as np
import torch

KIND_PROB, KIND_LABELS = 0, 1     # vpu_runs_obj.kind: fp32 map > thr (values 0 / 1), 16-bit label map


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


# ------------------------------------------------------------------------------------------------------ the op classes
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
        raw = bytes((self._lib.RunsObj * n)(*rows))
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()       # (alive until the last read-back)
        desc = host.to(self.device, non_blocking=True)
        sizes = [tuple(t.shape) for t, _, _ in items]
        scratch = torch.empty(self._ops.runs_scratch_len(sizes), device=self.device, dtype=torch.int32)
        header = torch.empty(n + 1, device=self.device, dtype=torch.int32)
        self._ops.runs_count_batched(desc, host, n, scratch, header)
        at = header.cpu().numpy()                                                      # synchronisation 1
        entries = torch.empty(int(at[n]), 2, device=self.device, dtype=torch.int32)
        self._ops.runs_write_batched(desc, host, n, scratch, entries)
        got = entries.cpu().numpy()                                                    # synchronisation 2
        return [RunMap(sizes[k], got[at[k]:at[k + 1], 0], got[at[k]:at[k + 1], 1]) for k in range(n)]


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
