"""Shared by test_simplify_cpu.py and test_simplify_gpu.py: (a) every shape and pattern of outline_cases.py traced with the
stand-in, (b) synthetic loops fed straight to the simplifier, the tolerances, and the sequential reference of each, computed
once."""
import numpy as np

from pvpuformer_amd import ops
from pvpuformer_amd.isegm.inference.outlines import Outline, host_outline

from outline_cases import PATTERNS, SHAPES, pattern
from simplify_ref import distance_ref, quantise_ref, simplify_ref

TOLERANCES = [0, 0.25, 0.5, 1, 1.5, 3, 1024]
T = ops.SIMPLIFY_THREADS
LENGTHS = [4, 5, 63, 64, 65, T - 1, T, T + 1, 4 * T + 1]
SYNTHETIC = ["square", "revisit", "pinned", "zigzag", "threshold", "comb", "sliver"]
SIDE = 8191                                     # S1's largest side
TEETH = 64


def _canonical(points):
    """The loop rotated to start at its first vertex of smallest (y, x), as O4 has it."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    assert p.min() >= 0 and p.max() <= SIDE
    key = p[:, 1] * (SIDE + 1) + p[:, 0]
    return np.roll(p, -int(np.argmin(key)), axis=0).astype(np.int32)


def _legs(corners, n):
    """A closed loop of n vertices: the corners, and the other n - len(corners) vertices dealt round robin to the legs between
    them, spread evenly along a leg and pushed 0, 1 or 2 lattice steps off it in turn: a staircase along every leg."""
    c = len(corners)
    if n <= c:
        return corners[:n]
    extra = [(n - c) // c + (1 if leg < (n - c) % c else 0) for leg in range(c)]
    out = []
    for leg in range(c):
        (ax, ay), (bx, by) = corners[leg], corners[(leg + 1) % c]
        out.append((ax, ay))
        m = extra[leg]
        for q in range(m):
            x, y = ax + (bx - ax) * (q + 1) // (m + 1), ay + (by - ay) * (q + 1) // (m + 1)
            push = q % 3
            if ax == bx:
                x += push if x == 0 else -push
            else:
                y += push if y < SIDE // 2 else -push
            out.append((min(max(x, 0), SIDE), min(max(y, 0), SIDE)))
    return out


def synthetic(name, n):
    """int32 [n, 2]: one closed loop of n >= 4 vertices inside 0 .. 8191."""
    if name == "square":                        # S1's bounds: differences of 8191 along the sides and the diagonal
        return _canonical(_legs([(0, 0), (SIDE, 0), (SIDE, SIDE), (0, SIDE), (0, 4096), (2048, 2048)], n))
    if name == "revisit":                       # out along a bent path and back over the same vertices: chains with A == B
        h = n // 2                              # region by region, zero area, dropped at every tolerance
        out = [(3 * q, (q * q) % 7 + 2 * q) for q in range(h + 1)]
        back = out[-2:0:-1] if n % 2 == 0 else out[-1:0:-1]
        return _canonical(out + back)
    if name == "pinned":                        # every vertex the same point: the chain (0, n) has A == B and never splits
        return _canonical([(17, 5)] * n)
    if name == "zigzag":                        # equal heights over a level chain: the best k is tied in every chain
        step = max(1, min(10, 8000 // n))
        out = [(step * q, 4 * (q % 2)) for q in range(n - 2)]
        return _canonical(out + [(step * (n - 3), 3000), (0, 3000)])
    if name == "threshold":                     # bumps of depth 1 and 3 under level and upright chains: 16 num == t^2 den at
        out = [(0, 0)]                          # tolerance 1 and 3 (not kept), and one of depth 2 and 4 each: a step beyond
        room = n - 4
        a = (room + 1) // 2
        for q in range(a):
            out.append((max(1, 3900 // (a + 1)) * (q + 1), 2 if (q == a // 2 and a > 1) else 1))
        out.append((4000, 0))
        for q in range(room - a):
            out.append((4000 - (4 if (q == 0 and room - a > 1) else 3), max(1, 1900 // (room - a + 1)) * (q + 1)))
        return _canonical(out + [(4000, 2000), (0, 2000)])
    if name == "comb":                          # teeth of falling height: every round keeps one tip or one valley, so the
        teeth = min(TEETH, (n - 2) // 2)        # rounds are no fewer than the teeth; the other vertices lie ON the top edge
        flat = n - 2 - 2 * teeth
        X = 20 * teeth + 20
        out = [(0, 0)] + [(X * (q + 1) // (flat + 1), 0) for q in range(flat)] + [(X, 0)]
        for q in range(teeth):
            out += [(X - 10 - 20 * q, 3000 - 10 * q), (X - 20 - 20 * q, 5)]
        return _canonical(out)
    if name == "sliver":                        # within a pixel of one segment: two vertices left at tolerance 1 and above,
        return _canonical([(0, 0)] + [(7 * q, q // 9 + q % 2) for q in range(1, n)])      # everything kept at tolerance 0
    raise KeyError(name)


def outline_case(name, shape):
    """The stand-in's Outline of a pattern of outline_cases.py, computed once."""
    key = ("outline", name, tuple(shape))
    if key not in _MEMO:
        _MEMO[key] = host_outline(pattern(name, *shape))
    return _MEMO[key]


def synthetic_case(name, n):
    """A synthetic loop as an Outline of one loop on the largest lattice (not a traceable one: ``check()`` is not for it)."""
    key = ("synthetic", name, n)
    if key not in _MEMO:
        _MEMO[key] = Outline((SIDE, SIDE), synthetic(name, n), [0, n])
    return _MEMO[key]


_MEMO = {}
OUTLINE_CASES = [("outline", name, shape) for shape in SHAPES for name in PATTERNS]
SYNTHETIC_CASES = [("synthetic", name, n) for name in SYNTHETIC for n in LENGTHS]
ALL_CASES = OUTLINE_CASES + SYNTHETIC_CASES


def source(case):
    return outline_case(*case[1:]) if case[0] == "outline" else synthetic_case(*case[1:])


def reference(case, tolerance):
    """simplify_ref of a case at a tolerance, computed once and shared: (points int32 [V', 2], offsets int32 [L' + 1], hole bool
    [L'], dropped, kept positions per exact loop)."""
    key = ("ref", case, tolerance)
    if key not in _MEMO:
        o = source(case)
        pts, off, hole, dropped, kept = simplify_ref(o.points.tolist(), o.offsets.tolist(), quantise_ref(tolerance))
        _MEMO[key] = (np.array(pts, dtype=np.int32).reshape(-1, 2), np.array(off, dtype=np.int32), np.array(hole, dtype=bool),
                      dropped, kept)
    return _MEMO[key]


def case_id(case):
    return f"{case[1]}-{case[2][0]}x{case[2][1]}" if case[0] == "outline" else f"{case[1]}-{case[2]}"


def assert_s6(o, kept_of, t, where):
    """S6 in exact integers: every vertex of a surviving exact loop within t / 4 of the simplified segment over its position."""
    for (a, b), kept in zip(zip(o.offsets[:-1], o.offsets[1:]), kept_of):
        if kept is None:
            continue
        loop = [(int(x), int(y)) for x, y in o.points[a:b]]
        n = len(loop)
        ends = kept + [n]
        assert kept[0] == 0, where
        for i, j in zip(ends[:-1], ends[1:]):
            for p in range(i, j + 1):
                num, den = distance_ref(loop[p % n], loop[i], loop[j % n])
                assert 16 * num <= t * t * den, (where, i, j, p)
