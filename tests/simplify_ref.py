"""An independent sequential Douglas-Peucker over closed loops: an explicit stack, plain Python ints, rules S1-S5 of
pvpuformer_amd/isegm/inference/polygons.py written down literally.  Shares no code with ``host_simplify``."""


def quantise_ref(tolerance):
    """S1: t = round(4 * tolerance)."""
    return round(4 * tolerance)


def distance_ref(p, a, b):
    """S2 -> (num, den): the squared distance of P to the segment A B as the rational num / den."""
    px, py = p[0] - a[0], p[1] - a[1]
    if a == b:
        return px * px + py * py, 1
    bx, by = b[0] - a[0], b[1] - a[1]
    den = bx * bx + by * by
    dot = px * bx + py * by
    if dot <= 0:
        return (px * px + py * py) * den, den
    if dot >= den:
        qx, qy = p[0] - b[0], p[1] - b[1]
        return (qx * qx + qy * qy) * den, den
    cross = bx * py - by * px
    return cross * cross, den


def simplify_loop_ref(loop, t):
    """One closed loop [(x, y)] of n vertices at t quarter pixels -> the sorted kept positions (S3, S4)."""
    n = len(loop)
    pos = [(int(x), int(y)) for x, y in loop]
    pos.append(pos[0])                                  # position n is position 0
    far, best = 0, 0
    for k in range(n):                                  # S3: the largest |P_k - P_0|^2, the smallest k on ties
        d = (pos[k][0] - pos[0][0]) ** 2 + (pos[k][1] - pos[0][1]) ** 2
        if d > best:
            far, best = k, d
    kept = {0, far}
    stack = [(0, far), (far, n)] if far > 0 else [(0, n)]
    while stack:                                        # S4
        i, j = stack.pop()
        if j - i < 2:
            continue
        k_best, num_best, den = -1, -1, 1
        for k in range(i + 1, j):
            num, den = distance_ref(pos[k], pos[i], pos[j])
            if num > num_best:                          # strictly: the smallest k wins ties
                k_best, num_best = k, num
        if 16 * num_best > t * t * den:
            kept.add(k_best)
            stack.append((i, k_best))
            stack.append((k_best, j))
    return sorted(kept)


def area2_ref(vertices):
    """Twice the signed area of a closed loop."""
    total = 0
    for i in range(len(vertices)):
        x0, y0 = vertices[i]
        x1, y1 = vertices[(i + 1) % len(vertices)]
        total += int(x0) * int(y1) - int(x1) * int(y0)
    return total


def simplify_ref(points, offsets, t):
    """All loops (S5) -> (points [[x, y]], offsets, hole flags, dropped, the kept positions of every exact loop or None for a
    dropped one)."""
    out_points, out_offsets, hole, dropped, kept_of = [], [0], [], 0, []
    for a, b in zip(offsets[:-1], offsets[1:]):
        loop = [(int(x), int(y)) for x, y in points[a:b]]
        kept = simplify_loop_ref(loop, t)
        simple = [loop[k] for k in kept]
        if len(simple) < 3 or area2_ref(simple) == 0:
            dropped += 1
            kept_of.append(None)
            continue
        kept_of.append(kept)
        out_points.extend([x, y] for x, y in simple)
        out_offsets.append(len(out_points))
        hole.append(area2_ref(loop) < 0)
    return out_points, out_offsets, hole, dropped, kept_of
