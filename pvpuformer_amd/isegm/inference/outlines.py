"""Outlines: a binary map as closed polygon loops on the pixel lattice, exact and canonical.

O1  Pixel ``(r, c)`` is the unit square ``[c, c + 1] x [r, r + 1]`` in ``(x, y)``, y down; outside the image all is clear.
O2  A boundary edge is a unit edge between a set pixel and a clear one, oriented with the set pixel on its right: the top
    edge of a set pixel runs East, its right edge South, its bottom edge West, its left edge North.
O3  The successor of an edge turns left when the pixel ahead on the left is set, else goes straight when the pixel ahead on
    the right is set, else turns right.  At a saddle it always turns left: foreground is 8-connected, holes are 4-connected
    (as in ``tidy``), and the edges fall into closed loops.
O4  A loop is its corners in the order of travel, from its corner of smallest ``(y, x)``; loops are ordered by that corner.
O5  Outer loops have a positive signed area and first step East, hole loops a negative one and first step South; the areas
    sum to the number of set pixels.
O6  The way back: ``+1`` per North step and ``-1`` per South step at column ``x``, summed along each row, is the map.

``vpu_outline_count_batched`` / ``vpu_outline_trace_batched`` (csrc/outline.hip) trace n maps of different sizes on the device;
what crosses to the host is ``4 (n + 1)`` bytes of offsets, then 8 bytes per corner and about one word per loop, in two
read-backs with the exact allocation between them.  ``host_outline`` is the numpy stand-in (``HostOutlineOps``), which runs on
a CPU pool and may replace ``ops_outlines`` of a device pool.

With a ``tolerance`` (pixels) both op classes return ``Polygons`` (polygons.py): the same loops simplified by
Douglas-Peucker on the device, after which only the kept corners cross to the host, in three read-backs."""
import numpy as np
import torch

from ._batchcore import upload_structs
from .polygons import Polygons, check_request, empty_polygons, host_simplify
from .runs import KIND_LABELS, KIND_PROB

EAST, SOUTH, WEST, NORTH = 0, 1, 2, 3


class Outline:
    """``size = (H, W)``; ``points``: int32 [V, 2], the corners ``(x, y)`` of all loops, loop after loop in the order of
    travel; ``offsets``: int32 [L + 1], loop ``l`` is ``points[offsets[l]:offsets[l + 1]]``."""

    def __init__(self, size, points, offsets):
        self.size = (int(size[0]), int(size[1]))
        self.points = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        assert self.offsets.ndim == 1 and len(self.offsets) >= 1

    def __len__(self):
        return len(self.offsets) - 1

    def loops(self):
        """The loops, each int32 [n, 2] of ``(x, y)``."""
        return [self.points[a:b] for a, b in zip(self.offsets[:-1], self.offsets[1:])]

    def _next(self):
        """The index of every corner's successor in its loop."""
        nxt = np.arange(1, len(self.points) + 1)
        nxt[self.offsets[1:] - 1] = self.offsets[:-1]
        return nxt

    def areas(self):
        """int64 [L]: the signed area of every loop, ``1/2 sum(x_i y_{i+1} - x_{i+1} y_i)``: positive for outer loops."""
        if len(self) == 0:
            return np.zeros(0, dtype=np.int64)
        p = self.points.astype(np.int64)
        q = p[self._next()]
        return np.add.reduceat(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1], self.offsets[:-1].astype(np.int64)) // 2

    def holes(self):
        """bool [L]: which loops bound a hole."""
        return self.areas() < 0

    def area(self):
        """The number of set pixels."""
        return int(self.areas().sum())

    def box(self):
        """Inclusive ``(rmin, rmax, cmin, cmax)`` of the set pixels; ``(H, -1, W, -1)`` for an outline without loops."""
        if len(self.points) == 0:
            return (self.size[0], -1, self.size[1], -1)
        x, y = self.points[:, 0], self.points[:, 1]
        return (int(y.min()), int(y.max()) - 1, int(x.min()), int(x.max()) - 1)

    def decode(self):
        """bool [H, W]: the map (O6)."""
        H, W = self.size
        acc = np.zeros((H + 1, W + 1), dtype=np.int32)
        if len(self.points):
            p, q = self.points, self.points[self._next()]
            up = (p[:, 0] == q[:, 0]) & (q[:, 1] < p[:, 1])           # a North step covers the rows q.y .. p.y - 1 with +1
            down = (p[:, 0] == q[:, 0]) & (q[:, 1] > p[:, 1])         # a South step the rows p.y .. q.y - 1 with -1
            np.add.at(acc, (q[up, 1], p[up, 0]), 1)
            np.add.at(acc, (p[up, 1], p[up, 0]), -1)
            np.add.at(acc, (p[down, 1], p[down, 0]), -1)
            np.add.at(acc, (q[down, 1], p[down, 0]), 1)
        return np.cumsum(np.cumsum(acc, axis=0), axis=1)[:H, :W] == 1

    def to_coco(self, holes=False):
        """COCO's polygon form: a list of flat ``[x0, y0, x1, y1, ...]`` float lists, the outer loops only unless ``holes``."""
        keep = np.ones(len(self), dtype=bool) if holes else ~self.holes()
        return [loop.reshape(-1).astype(np.float64).tolist() for loop, k in zip(self.loops(), keep) if k]

    def simplify(self, tolerance):
        """Polygons (polygons.py): the loops simplified within ``tolerance`` pixels, rules S1-S6."""
        return host_simplify(self, tolerance)

    def check(self):
        """ValueError unless this is what a trace can return: offsets from 0 to V increasing by at least 4, lattice points,
        steps that alternate between horizontal and vertical, every loop starting at its corner of smallest (y, x), visited
        once, with its first step East (outer) or South (hole), and the starts strictly ascending in (y, x)."""
        H, W = self.size
        pts, off = self.points.astype(np.int64), self.offsets.astype(np.int64)
        if H < 1 or W < 1:
            raise ValueError(f"Outline: size {H} x {W} (H, W >= 1)")
        if off[0] != 0 or off[-1] != len(pts) or (np.diff(off) < 4).any() or (np.diff(off) % 2).any():
            raise ValueError("Outline: offsets must run from 0 to the number of points in even steps of at least 4")
        if len(pts) == 0:
            return self
        if (pts < 0).any() or (pts[:, 0] > W).any() or (pts[:, 1] > H).any():
            raise ValueError("Outline: a point outside the lattice 0 .. W x 0 .. H")
        step = pts[self._next()] - pts
        flat = step[:, 1] == 0
        if ((step[:, 0] == 0) == flat).any() or (flat == flat[self._next()]).any():
            raise ValueError("Outline: steps must be horizontal or vertical, not null, and alternate")
        key = pts[:, 1] * (W + 1) + pts[:, 0]
        starts = key[off[:-1]]
        if (np.minimum.reduceat(key, off[:-1]) != starts).any() or (np.add.reduceat((key == np.repeat(starts, np.diff(off))), off[:-1]) != 1).any():
            raise ValueError("Outline: a loop must start at its corner of smallest (y, x) and visit it once")
        if (np.diff(starts) <= 0).any():
            raise ValueError("Outline: the loops' starts must ascend strictly in (y, x)")
        first, areas = step[off[:-1]], self.areas()
        east, south = (first[:, 0] > 0) & (first[:, 1] == 0), (first[:, 0] == 0) & (first[:, 1] > 0)
        if (areas == 0).any() or (east != (areas > 0)).any() or (south != (areas < 0)).any():
            raise ValueError("Outline: an outer loop (positive area) steps East first, a hole (negative area) South")
        return self


def empty_outline(size):
    return Outline(size, np.zeros((0, 2), dtype=np.int32), np.zeros(1, dtype=np.int32))


# ------------------------------------------------------------------------------------------------------ host stand-in
# The 2 x 2 neighbourhood of a lattice vertex, NW = 1, NE = 2, SW = 4, SE = 8: its number of corners, and the leave direction of
# the one that comes first in row-major order (the second corner of a saddle leaves the opposite way).
_CORNERS = np.zeros(16, dtype=np.int64)
_CORNERS[[1, 2, 4, 8, 7, 11, 13, 14]] = 1
_CORNERS[[6, 9]] = 2
_LEAVES = np.zeros(16, dtype=np.int64)
_LEAVES[[1, 2, 4, 8, 7, 11, 13, 14, 9, 6]] = [WEST, NORTH, SOUTH, EAST, SOUTH, WEST, EAST, NORTH, WEST, NORTH]


def _binary(array, kind, thr, label):
    array = np.asarray(array)
    assert array.ndim == 2 and kind in (KIND_PROB, KIND_LABELS)
    if kind == KIND_PROB:
        assert array.dtype == np.float32
        return array > np.float32(thr)
    assert array.dtype in (np.uint16, np.int16) and 0 <= int(label) <= 65535
    return array.view(np.uint16) == np.uint16(label)


def host_outline(mask):
    """Stand-in of the kernels for one binary map, bool [H, W] -> Outline, without walking: every corner gets its rank R in
    row-major order (at a saddle the corner whose horizontal edge lies to the West first) and its rank C in column-major
    order (the corner whose vertical edge lies to the North first); its successor is R + 1 / R - 1 when it leaves East /
    West and the corner of column rank C + 1 / C - 1 when it leaves South / North.  Pointer doubling over the successors
    gives every corner its loop's leader (the smallest R on it) and its distance to it, hence its place."""
    m = np.asarray(mask)
    assert m.ndim == 2 and m.dtype == bool and m.shape[0] >= 1 and m.shape[1] >= 1
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), dtype=np.int64)
    p[1:-1, 1:-1] = m
    cfg = p[:-1, :-1] | (p[:-1, 1:] << 1) | (p[1:, :-1] << 2) | (p[1:, 1:] << 3)          # [H + 1, W + 1], per lattice vertex
    ys, xs = np.nonzero(_CORNERS[cfg])                                                     # row-major
    reps = _CORNERS[cfg[ys, xs]]
    y, x, c = np.repeat(ys, reps), np.repeat(xs, reps), np.repeat(cfg[ys, xs], reps)
    V = len(y)
    if V == 0:
        return empty_outline((H, W))
    R = np.arange(V)
    second = np.concatenate(([False], (y[1:] == y[:-1]) & (x[1:] == x[:-1]))).astype(np.int64)
    leave = _LEAVES[c] ^ (2 * second)
    in_column = np.where(c == 9, 1 - second, np.where(c == 6, second, 0))
    by_column = np.lexsort((in_column, y, x))                                              # by_column[C] = R
    C = np.empty(V, dtype=np.int64)
    C[by_column] = R
    vertical = by_column[np.clip(C + np.where(leave == SOUTH, 1, -1), 0, V - 1)]
    succ = np.where(leave == EAST, R + 1, np.where(leave == WEST, R - 1, vertical))
    nxt, lead, dist, step = succ, R, np.zeros(V, dtype=np.int64), 1
    while step < V:
        other = lead[nxt]
        take = other < lead
        dist = np.where(take, step + dist[nxt], dist)
        lead = np.where(take, other, lead)
        nxt, step = nxt[nxt], 2 * step
    leader = lead == R
    length = np.where(leader, dist[succ] + 1, 0)
    begin = np.cumsum(length) - length
    place = begin[lead] + np.where(dist == 0, 0, length[lead] - dist)
    points = np.empty((V, 2), dtype=np.int32)
    points[place] = np.stack((x, y), axis=1)
    return Outline((H, W), points, np.concatenate((begin[leader], [V])))


# ------------------------------------------------------------------------------------------------------ the op classes
def _check_item(tensor, kind, thr, label):
    assert kind in (KIND_PROB, KIND_LABELS) and tensor.dim() == 2 and tensor.is_contiguous()
    assert tensor.dtype == (torch.float32 if kind == KIND_PROB else torch.int16)
    assert tensor.shape[0] >= 1 and tensor.shape[1] >= 1
    assert 0.0 <= float(thr) < 1.0 if kind == KIND_PROB else 0 <= int(label) <= 65535


class DeviceOutlineOps:
    """The HIP kernels.  ``trace(items)``, items [(tensor [H, W], kind, thr, label)]: fp32 and ``M = tensor > thr`` for kind
    0, int16 storage of uint16 labels and ``M = tensor == label`` for kind 1 -> [Outline].  The descriptors go up in one pinned
    copy; the header comes back (synchronisation 1, ``4 (n + 1)`` bytes); exactly the needed entries are allocated; points,
    offsets and loop counts come back in one copy (synchronisation 2).

    ``trace(items, tolerance)`` -> [Polygons]: the traced points stay on the device, ``vpu_outline_simplify_batched`` runs on
    them, the items' loop counts, first surviving loops, first kept points and the totals come back (synchronisation 2,
    ``12 (n + 1) + 16`` bytes), then exactly ``8 V' + 4 (L' + 1) + L'`` bytes: kept points, offsets, hole flags (3)."""

    def __init__(self, device):
        from pvpuformer_amd import _lib, ops
        self._lib, self._ops, self.device = _lib, ops, torch.device(device)

    def trace(self, items, tolerance=None):
        n = len(items)
        t = None if tolerance is None else check_request(tolerance, [tuple(item[0].shape) for item in items])
        if n == 0:
            return []
        rows = []
        for tensor, kind, thr, label in items:
            _check_item(tensor, kind, thr, label)
            assert tensor.device == self.device or (tensor.is_cuda and self.device.index is None)
            assert tensor.data_ptr() % (16 if kind == KIND_PROB else 8) == 0
            d = self._lib.OutlineObj()
            d.src, d.H, d.W, d.kind, d.thr, d.label, d.pad = tensor.data_ptr(), tensor.shape[0], tensor.shape[1], kind, float(thr), int(label), 0
            rows.append(d)
        host, desc, _ = upload_structs(self.device, (self._lib.OutlineObj * n)(*rows))   # (host: alive until the last read-back)
        sizes = [tuple(t.shape) for t, _, _, _ in items]
        scratch = torch.empty(self._ops.outline_scratch_len(sizes), device=self.device, dtype=torch.int32)
        header = torch.empty(n + 1, device=self.device, dtype=torch.int32)
        self._ops.outline_count_batched(desc, host, n, scratch, header)
        head = header.cpu()                                                              # synchronisation 1
        at = head.numpy()
        V = int(at[n])
        if V == 0:
            return [empty_outline(size) if t is None else empty_polygons(size, t) for size in sizes]
        if t is not None:
            return self._simplified(n, sizes, desc, host, scratch, header, head, t)
        most = V // 4 + 1                                      # a loop has four corners or more: offsets [L + 1] fits
        work = torch.empty(self._ops.outline_work_len(V), device=self.device, dtype=torch.int32)
        out = torch.empty(2 * V + most + n + 1, device=self.device, dtype=torch.int32)
        points, offsets, item_loops = out[:2 * V].view(V, 2), out[2 * V:2 * V + most], out[2 * V + most:]
        self._ops.outline_trace_batched(desc, host, n, scratch, header, head, work, points, offsets, item_loops)
        got = out.cpu().numpy()                                                          # synchronisation 2
        points, offsets, first = got[:2 * V].reshape(V, 2), got[2 * V:2 * V + most], got[2 * V + most:]
        return [Outline(sizes[k], points[at[k]:at[k + 1]], offsets[first[k]:first[k + 1] + 1] - at[k]) for k in range(n)]


    def _simplified(self, n, sizes, desc, host, scratch, header, head, t):
        ops, at = self._ops, head.numpy()
        V = int(at[n])
        loop_max = V // 4                                      # a loop has four corners or more
        work = torch.empty(ops.outline_work_len(V), device=self.device, dtype=torch.int32)
        exact = torch.empty(2 * V + loop_max + 1, device=self.device, dtype=torch.int32)
        points, offsets = exact[:2 * V].view(V, 2), exact[2 * V:]
        meta = torch.empty(3 * (n + 1) + 4, device=self.device, dtype=torch.int32)
        item_loops, firsts = meta[:n + 1], meta[n + 1:]
        ops.outline_trace_batched(desc, host, n, scratch, header, head, work, points, offsets, item_loops)
        work = torch.empty(ops.outline_simplify_work_len(V, loop_max), device=self.device, dtype=torch.int32)
        out = torch.empty(2 * V + loop_max + 2, device=self.device, dtype=torch.int32)       # (an even count: offsets 8-byte aligned)
        out_points, out_offsets = out[:2 * V].view(V, 2), out[2 * V:2 * V + loop_max + 1]
        out_hole = torch.empty(loop_max + 1, device=self.device, dtype=torch.uint8)
        ops.outline_simplify_batched(points, offsets, item_loops, n, V, loop_max, t, work, out_points, out_offsets, out_hole, firsts)
        got = meta.cpu().numpy()                                                          # synchronisation 2
        loops, first, start, (kept, alive, _, _) = got[:n + 1], got[n + 1:2 * n + 2], got[2 * n + 2:3 * n + 3], got[3 * n + 3:]
        kept, alive = int(kept), int(alive)
        packed = torch.cat((out[:2 * kept].view(torch.uint8), out_offsets[:alive + 1].view(torch.uint8), out_hole[:alive]))
        raw = packed.cpu().numpy()                                                        # synchronisation 3: 8 V' + 4 (L' + 1) + L' bytes
        assert raw.nbytes == 8 * kept + 4 * (alive + 1) + alive
        pts = raw[:8 * kept].view(np.int32).reshape(kept, 2)
        off = raw[8 * kept:8 * kept + 4 * (alive + 1)].view(np.int32)
        hole = raw[8 * kept + 4 * (alive + 1):].astype(bool)
        return [Polygons(sizes[k], pts[start[k]:start[k + 1]], off[first[k]:first[k + 1] + 1] - start[k], hole[first[k]:first[k + 1]],
                         t / 4.0, (at[k + 1] - at[k], loops[k + 1] - loops[k]), (loops[k + 1] - loops[k]) - (first[k + 1] - first[k]))
                for k in range(n)]


class HostOutlineOps:
    """The numpy stand-in behind the same call; maps on a device are copied to the host."""

    def __init__(self, device=None):
        self.device = device

    def trace(self, items, tolerance=None):
        if tolerance is not None:
            check_request(tolerance, [tuple(item[0].shape) for item in items])
        out = []
        for tensor, kind, thr, label in items:
            _check_item(tensor, kind, thr, label)
            outline = host_outline(_binary(tensor.detach().cpu().numpy(), kind, thr, label))
            out.append(outline if tolerance is None else host_simplify(outline, tolerance))
        return out
