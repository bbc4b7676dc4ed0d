"""Shared by test_runs_cpu.py and test_runs_gpu.py: the shapes and patterns of the run-length tests, the stream rule per pixel
in plain Python, and the script that drives the pools' three run-length calls after every step."""
import numpy as np

from pvpuformer_amd import ops

B, C = ops.RUNS_BAND_ROWS, ops.RUNS_COLS
THR = 0.5
LABELS = np.array([0, 1, 2, 65535], dtype=np.uint16)

# one pixel; every predecessor in the previous column; one column; several quads and bands; the band and column-group edges
SHAPES = [(1, 1), (1, 70), (70, 1), (47, 70), (33, 130), (127, 129),
          (B - 1, 5), (B, 5), (B + 1, 5), (2 * B + 1, 3),
          (3, C - 1), (3, C), (3, C + 1), (3, 2 * C + 1)]
PATTERNS = ["zero", "set", "checkerboard", "columns", "boundary", "rows", "ellipse", "random"]


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def pattern(name, H, W, seed=0):
    """bool / small-integer [H, W] array ``p`` with values in 0 .. 3: the index into ``LABELS`` (kind 1), set where p != 0
    (kind 0)."""
    rs = np.random.RandomState(1000 * H + W + seed)
    rr, cc = np.mgrid[0:H, 0:W]
    if name == "zero":
        p = np.zeros((H, W), dtype=np.int64)
    elif name == "set":
        p = np.ones((H, W), dtype=np.int64)
    elif name == "checkerboard":
        # i = c * H + r alternates along the stream, across the column boundary too: H * W runs
        p = (cc * H + rr) % 2
    elif name == "columns":
        p = cc % 2
    elif name == "boundary":
        # random inside; even boundaries c -> c + 1 continue (bottom of c == top of c + 1), odd ones differ in both kinds
        p = rs.randint(0, 4, size=(H, W))
        for c in range(W - 1):
            last = p[H - 1, c]
            p[0, c + 1] = last if c % 2 == 0 else (0 if last != 0 else 1 + c % 3)
    elif name == "rows":
        p = rr % 2
    elif name == "ellipse":
        p = (((rr - 0.5 * (H - 1)) / (0.35 * H + 0.5)) ** 2 + ((cc - 0.5 * (W - 1)) / (0.35 * W + 0.5)) ** 2 <= 1.0).astype(np.int64)
    elif name == "random":
        p = rs.randint(0, 4, size=(H, W))
    else:
        raise KeyError(name)
    return p


def case(kind, name, H, W, seed=0):
    """The source array of a case: kind 1 -> uint16 labels from {0, 1, 2, 65535}; kind 0 -> fp32 around THR: the clear pixels
    hold THR itself (the comparison is strict) or a value below, the set ones the next float above THR or a value above."""
    p = pattern(name, H, W, seed)
    if kind == 1:
        return LABELS[p]
    rs = np.random.RandomState(7 + H * W + seed)
    edge = rs.rand(H, W) < 0.5
    low = np.where(edge, np.float32(THR), (rs.rand(H, W) * THR).astype(np.float32))
    high = np.where(edge, np.nextafter(np.float32(THR), np.float32(1)), (THR + 0.01 + rs.rand(H, W) * 0.4).astype(np.float32))
    return np.where(p != 0, high, low).astype(np.float32)


def values_of(array, kind, thr=THR):
    """uint16 [H, W]: the integer values the runs are of."""
    if kind == 0:
        return (array > np.float32(thr)).astype(np.uint16)
    return array.view(np.uint16)


def stream_runs(v):
    """(starts, values) by the rule, one pixel at a time along i = c * H + r."""
    H, W = v.shape
    starts, values, prev = [], [], None
    for i in range(H * W):
        x = int(v[i % H, i // H])
        if i == 0 or x != prev:
            starts.append(i)
            values.append(x)
        prev = x
    return starts, values


def stream_counts(v, label):
    """COCO's uncompressed counts of v == label, one pixel at a time."""
    H, W = v.shape
    counts, state, n = [], False, 0
    for i in range(H * W):
        on = int(v[i % H, i // H]) == label
        if on != state:
            counts.append(n)
            state, n = on, 0
        n += 1
    counts.append(n)
    return counts


def decode_counts(seg):
    """bool [H, W] of a ``dict(size, counts)``, one pixel at a time."""
    H, W = seg["size"]
    out, i, on = np.zeros((H, W), dtype=bool), 0, False
    for n in seg["counts"]:
        for _ in range(n):
            out[i % H, i // H] = on
            i += 1
        on = not on
    assert i == H * W
    return out


def same_runs(a, b):
    return (a.size == b.size and a.starts.dtype == b.starts.dtype == np.int32 and a.values.dtype == b.values.dtype == np.int32
            and np.array_equal(a.starts, b.starts) and np.array_equal(a.values, b.values))


def run_pool_script(ann, images, check):
    """A short script on every image of ``images`` [(image, (row, col))] at once: clicks, a partial finish, a finish, an
    overlapping second object, an undo, a reopen.  ``check(where, aids, masks)`` runs after every step; ``masks`` are the masks
    the step returned ({aid: bool [H, W]}) or None."""
    aids = [ann.open(image) for image, _ in images]
    centre = {aid: c for aid, (_, c) in zip(aids, images)}
    shape = {aid: image.shape[:2] for aid, (image, _) in zip(aids, images)}

    def click(where, positive, dr, dc):
        at = {aid: (positive, (int(np.clip(centre[aid][0] + dr, 0, shape[aid][0] - 1)),
                               int(np.clip(centre[aid][1] + dc, 0, shape[aid][1] - 1)))) for aid in aids}
        check(where, aids, ann.click(at))

    check("open", aids, None)
    click("click 1", True, 0, 0)
    click("click 2", True, 4, -5)
    for aid in aids:
        ann.partially_finish(aid)
    check("partial finish", aids, None)
    click("click 3", True, -6, 7)
    for aid in aids:
        assert ann.finish(aid) is not None
    check("finish 1", aids, None)
    click("second object, over the first", True, 3, 2)
    click("second object, click 2", False, 0, 12)
    for aid in aids:
        ann.undo(aid)
    check("undo", aids, None)
    for aid in aids:
        assert ann.finish(aid) is not None
    check("finish 2", aids, None)
    for aid in aids:
        try:
            ann.reopen(aid, 1)
        except KeyError:                    # object 2 covers all of object 1
            ann.reopen(aid, 2)
    check("reopen", aids, None)
    click("click on the reopened object", True, 8, -7)
    for aid in aids:
        assert ann.finish(aid) is not None
    check("finish 3", aids, None)
    return aids
