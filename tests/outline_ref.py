"""The reference of the outline tests: a sequential tracer that follows the unit boundary edges of a binary map one at a time
by rules O2 and O3, in plain Python.  It shares nothing with ``host_outline``, which never walks: no corner
ranks, no successor tables, no pointer doubling."""
import numpy as np

# a direction is its index here: East, South, West, North as (dx, dy), y down
STEPS = [(1, 0), (0, 1), (-1, 0), (0, -1)]


def _sides(x, y, d):
    """The pixels (row, col) on the right and on the left of the unit edge that leaves the vertex (x, y) in direction d."""
    if d == 0:
        return (y, x), (y - 1, x)
    if d == 1:
        return (y, x - 1), (y, x)
    if d == 2:
        return (y - 1, x - 1), (y, x - 1)
    return (y - 1, x), (y - 1, x - 1)


def outline_ref(mask):
    """bool [H, W] -> (points int32 [V, 2] of (x, y), offsets int32 [L + 1]): the loops of O4, each from its corner of smallest
    (y, x), ordered by that corner."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape

    def on(pixel):
        r, c = pixel
        return 0 <= r < H and 0 <= c < W and bool(m[r, c])

    def is_edge(x, y, d):
        right, left = _sides(x, y, d)
        return on(right) and not on(left)

    seen, loops = set(), []
    for y in range(H + 1):
        for x in range(W + 1):
            for d in range(4):
                if (x, y, d) in seen or not is_edge(x, y, d):
                    continue
                edges, at = [], (x, y, d)
                while at not in seen:
                    seen.add(at)
                    edges.append(at)
                    ex, ey, ed = at
                    nx, ny = ex + STEPS[ed][0], ey + STEPS[ed][1]
                    right, left = _sides(nx, ny, ed)                   # the pixels ahead
                    if on(left):
                        nd = (ed + 3) % 4                              # O3: turn left
                    elif on(right):
                        nd = ed                                        # straight on
                    else:
                        nd = (ed + 1) % 4                              # turn right
                    at = (nx, ny, nd)
                    assert is_edge(*at)
                assert at == edges[0]                                  # closed
                corners = [(ex, ey) for k, (ex, ey, ed) in enumerate(edges) if ed != edges[k - 1][2]]
                keys = [(cy, cx) for cx, cy in corners]
                first = keys.index(min(keys))
                assert keys.count(min(keys)) == 1                      # O4: the start is visited once
                loops.append(corners[first:] + corners[:first])
    loops.sort(key=lambda loop: (loop[0][1], loop[0][0]))
    starts = [loop[0] for loop in loops]
    assert len(set(starts)) == len(starts)                             # O4: no two loops start at one vertex
    points = np.array([p for loop in loops for p in loop], dtype=np.int32).reshape(-1, 2)
    offsets = np.concatenate(([0], np.cumsum([len(loop) for loop in loops]))).astype(np.int32)
    return points, offsets
