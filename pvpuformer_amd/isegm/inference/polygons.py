"""Polygons: the loops of an ``Outline`` simplified within a pixel tolerance by Douglas-Peucker, exact in integers (DESIGN
section 19).  The input is one closed loop of an ``Outline``: positions ``0 .. n - 1``, position ``n`` the same as position 0.

S1  ``tolerance`` is in pixels, ``0 <= tolerance <= 1024``, quantised to quarter pixels: ``t = round(4 * tolerance)``.  ``H`` and
    ``W`` are at most 8191 when a tolerance is given.  All arithmetic is exact in int64: coordinate differences are below 2^13,
    cross products and squared lengths below 2^27, every product compared below 2^58.
S2  The distance of ``P`` to the chain end points ``A``, ``B`` is the distance to the segment, the rational ``num / den``.
    ``A == B``: ``num = |P - A|^2``, ``den = 1``.  Otherwise ``den = |B - A|^2``, ``dot = (P - A).(B - A)``, and
    ``dot <= 0``: ``num = |P - A|^2 den``; ``dot >= den``: ``num = |P - B|^2 den``; else ``num = cross(B - A, P - A)^2``.
S3  Position 0 (O4's start) is kept, and so is the position of largest ``|P_k - P_0|^2``, the smallest ``k`` on ties.
S4  For two consecutive kept positions ``i < j`` with a position between them take the ``k`` of largest ``num`` (``den`` is
    shared), the smallest ``k`` on ties, and keep it if and only if ``16 num > t^2 den``; repeat until no chain splits.  The
    kept set does not depend on the order in which chains are visited: recursion and rounds agree exactly.
S5  The kept vertices stay in loop order and still begin at O4's start.  A loop left with fewer than three vertices or with
    zero signed area is dropped and counted.  A loop's ``hole`` flag is the sign of the EXACT loop (O5).
S6  Every vertex of the exact loop lies within ``t / 4`` of the simplified segment that spans its position.  The result may
    intersect itself, as with every Douglas-Peucker; that is not repaired.

S3 is S4 on the chain ``(0, n)`` (``A == B == P_0``) with ``t = 0``, which is how the rounds below and the kernel start.
``vpu_outline_simplify_batched`` (csrc/outline.hip) runs on the points the trace left on the device: the exact points never
cross to the host.  ``host_simplify`` is the numpy stand-in, written in rounds as the kernel is."""
import math

import numpy as np

TOLERANCE_MAX = 1024        # S1, pixels
SIDE_MAX = 8191             # S1: H and W when a tolerance is given


def quantise(tolerance):
    """S1: ``t = round(4 * tolerance)``, quarter pixels (Python's ``round``: an exact half goes to the even t); ValueError for a
    tolerance that is negative, NaN or above 1024."""
    try:
        tol = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError(f"tolerance {tolerance!r} is not a number")
    if math.isnan(tol) or tol < 0.0 or tol > TOLERANCE_MAX:
        raise ValueError(f"tolerance {tolerance!r} (0 <= tolerance <= {TOLERANCE_MAX})")
    return int(round(4.0 * tol))


def check_request(tolerance, sizes):
    """The refusals of a simplified trace, before anything is launched -> t."""
    t = quantise(tolerance)
    for H, W in sizes:
        if H > SIDE_MAX or W > SIDE_MAX:
            raise ValueError(f"a map of {H} x {W}: sides are at most {SIDE_MAX} when a tolerance is given")
    return t


class Polygons:
    """``size = (H, W)``; ``points``: int32 [V', 2], the kept corners ``(x, y)`` of the surviving loops, loop after loop in the
    order of travel; ``offsets``: int32 [L' + 1]; ``hole``: bool [L'], from the exact loops' signs; ``tolerance``: the quantised
    tolerance ``t / 4`` in pixels; ``source = (V, L)``: the exact outline's counts; ``dropped``: the loops that collapsed."""

    def __init__(self, size, points, offsets, hole, tolerance, source, dropped):
        self.size = (int(size[0]), int(size[1]))
        self.points = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.hole = np.ascontiguousarray(hole, dtype=bool)
        self.tolerance = float(tolerance)
        self.source = (int(source[0]), int(source[1]))
        self.dropped = int(dropped)
        assert self.offsets.ndim == 1 and len(self.offsets) >= 1 and self.hole.ndim == 1

    def __len__(self):
        return len(self.offsets) - 1

    def loops(self):
        """The loops, each int32 [n, 2] of ``(x, y)``."""
        return [self.points[a:b] for a, b in zip(self.offsets[:-1], self.offsets[1:])]

    def _next(self):
        nxt = np.arange(1, len(self.points) + 1)
        nxt[self.offsets[1:] - 1] = self.offsets[:-1]
        return nxt

    def areas(self):
        """float64 [L']: the signed area of every simplified loop, ``1/2 sum(x_i y_{i+1} - x_{i+1} y_i)``, exact (a multiple of
        one half below 2^27).  Its sign may differ from ``hole`` once a loop intersects itself (S6)."""
        if len(self) == 0:
            return np.zeros(0, dtype=np.float64)
        p = self.points.astype(np.int64)
        q = p[self._next()]
        return np.add.reduceat(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1], self.offsets[:-1].astype(np.int64)) / 2.0

    def holes(self):
        """bool [L']: which loops bound a hole (S5: the exact loop's sign)."""
        return self.hole.copy()

    def to_coco(self, holes=False):
        """COCO's polygon form: a list of flat ``[x0, y0, x1, y1, ...]`` float lists, the outer loops only unless ``holes``."""
        keep = np.ones(len(self), dtype=bool) if holes else ~self.hole
        return [loop.reshape(-1).astype(np.float64).tolist() for loop, k in zip(self.loops(), keep) if k]

    def check(self):
        """ValueError unless this is what a simplified trace can return: offsets from 0 to V' increasing by at least 3, one hole
        flag per loop, lattice points, every loop starting at its smallest (y, x), and the starts ascending."""
        H, W = self.size
        pts, off = self.points.astype(np.int64), self.offsets.astype(np.int64)
        if H < 1 or W < 1:
            raise ValueError(f"Polygons: size {H} x {W} (H, W >= 1)")
        if off[0] != 0 or off[-1] != len(pts) or (np.diff(off) < 3).any():
            raise ValueError("Polygons: offsets must run from 0 to the number of points in steps of at least 3")
        if len(self.hole) != len(off) - 1:
            raise ValueError("Polygons: one hole flag per loop")
        if not (0.0 <= self.tolerance <= TOLERANCE_MAX) or self.tolerance * 4 != int(self.tolerance * 4) or self.dropped < 0:
            raise ValueError("Polygons: the tolerance is a number of quarter pixels in 0 .. 1024, dropped is not negative")
        if len(pts) == 0:
            return self
        if (pts < 0).any() or (pts[:, 0] > W).any() or (pts[:, 1] > H).any():
            raise ValueError("Polygons: a point outside the lattice 0 .. W x 0 .. H")
        key = pts[:, 1] * (W + 1) + pts[:, 0]
        starts = key[off[:-1]]
        if (np.minimum.reduceat(key, off[:-1]) != starts).any():
            raise ValueError("Polygons: a loop must start at its vertex of smallest (y, x)")
        if (np.diff(starts) < 0).any():
            raise ValueError("Polygons: the loops' starts must ascend in (y, x)")
        return self


def empty_polygons(size, t, source=(0, 0), dropped=0):
    return Polygons(size, np.zeros((0, 2), dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=bool), t / 4.0, source, dropped)


def simplify_loops(points, offsets, t):
    """Rules S2-S5 over the closed loops ``points[offsets[l]:offsets[l + 1]]`` (int [V, 2], int [L + 1]) at ``t`` quarter pixels,
    all loops together and in rounds as the kernel works -> (kept bool [V] with the dropped loops' vertices cleared, alive bool
    [L], hole bool [L], the number of rounds that split a chain)."""
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    V, L = len(pts), len(off) - 1
    assert off[0] == 0 and off[-1] == V and (np.diff(off) >= 1).all() and 0 <= int(t) <= 4 * TOLERANCE_MAX
    if V == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool), 0
    assert pts.min() >= 0 and pts.max() <= SIDE_MAX
    n = np.diff(off)
    # extended positions: loop l owns e = off[l] + l .. off[l + 1] + l, the last one the closing copy of its position 0
    E = V + L
    first = off[:-1] + np.arange(L)
    last = off[1:] + np.arange(L)
    src = np.arange(E) - np.repeat(np.arange(L), n + 1)           # the point behind every extended position
    src[last] = off[:-1]
    x, y = pts[src, 0], pts[src, 1]
    idx = np.arange(E)
    kept = np.zeros(E, dtype=bool)
    kept[first] = kept[last] = True
    live = ~kept                                                   # positions whose chain may still split
    tt, rounds = 0, 0                                              # S3 = S4 with t = 0 on the chain (0, n)
    while live.any():
        left = np.maximum.accumulate(np.where(kept, idx, -1))
        right = np.minimum.accumulate(np.where(kept, idx, E)[::-1])[::-1]
        p = idx[live]                                              # ascending: the positions of one chain are consecutive
        i, j = left[p], right[p]
        ax, ay, bx, by = x[i], y[i], x[j], y[j]
        ux, uy, vx, vy = bx - ax, by - ay, x[p] - ax, y[p] - ay
        den = ux * ux + uy * uy
        dot = vx * ux + vy * uy
        cross = ux * vy - uy * vx
        da = vx * vx + vy * vy
        db = (x[p] - bx) ** 2 + (y[p] - by) ** 2
        num = np.where(dot <= 0, da * den, np.where(dot >= den, db * den, cross * cross))
        same = den == 0
        num = np.where(same, da, num)
        den = np.where(same, 1, den)
        begin = np.flatnonzero(np.concatenate(([True], i[1:] != i[:-1])))
        chain = np.cumsum(np.concatenate(([True], i[1:] != i[:-1]))) - 1
        best = np.maximum.reduceat(num, begin)
        k = np.minimum.reduceat(np.where(num == best[chain], p, E), begin)
        split = 16 * best > tt * den[begin]
        kept[k[split]] = True
        live[p[~split[chain]]] = False                             # a chain that does not split never will
        live[k[split]] = False
        rounds += int(split.any())
        tt = int(t) * int(t)
    real = np.ones(E, dtype=bool)
    real[last] = False
    kept = kept[real]
    nxt = np.arange(1, V + 1)
    nxt[off[1:] - 1] = off[:-1]
    exact = np.add.reduceat(pts[:, 0] * pts[nxt, 1] - pts[nxt, 0] * pts[:, 1], off[:-1])
    count = np.add.reduceat(kept.astype(np.int64), off[:-1])
    kp = np.flatnonzero(kept)
    q = pts[kp]
    koff = np.concatenate(([0], np.cumsum(count)))
    knext = np.arange(1, len(kp) + 1)
    knext[koff[1:] - 1] = koff[:-1]                                # (every loop keeps its position 0)
    area = np.add.reduceat(q[:, 0] * q[knext, 1] - q[knext, 0] * q[:, 1], koff[:-1])
    alive = (count >= 3) & (area != 0)
    kept &= np.repeat(alive, n)
    return kept, alive, exact < 0, rounds


def host_simplify(outline, tolerance):
    """The numpy stand-in of ``vpu_outline_simplify_batched`` for one ``Outline`` -> Polygons."""
    t = check_request(tolerance, [outline.size])
    V, L = len(outline.points), len(outline)
    if V == 0:
        return empty_polygons(outline.size, t)
    kept, alive, hole, _ = simplify_loops(outline.points, outline.offsets, t)
    count = np.add.reduceat(kept.astype(np.int64), outline.offsets[:-1].astype(np.int64))[alive]
    return Polygons(outline.size, outline.points[kept], np.concatenate(([0], np.cumsum(count))), hole[alive], t / 4.0, (V, L),
                    L - int(alive.sum()))


def same_polygons(a, b):
    return (a.size == b.size and a.points.shape == b.points.shape and np.array_equal(a.points, b.points)
            and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.hole, b.hole) and a.tolerance == b.tolerance
            and a.source == b.source and a.dropped == b.dropped)
