"""Shared by test_outlines_cpu.py and test_outlines_gpu.py: the shapes and patterns of the outline tests, the two source kinds,
and the script that drives the pools' outline calls after every step."""
import numpy as np

from pvpuformer_amd import ops

from outline_ref import outline_ref

B, C = ops.OUTLINE_BAND_ROWS, ops.OUTLINE_COLS
THR = 0.5
LABELS = np.array([0, 1, 2, 65535], dtype=np.uint16)

# the lattice is (H + 1) x (W + 1): widths C - 1, C, C + 1 put its last column on both sides of a wave edge, heights B - 1, B,
# B + 1 its last row on both sides of a band edge; 2 C + 1 and 2 B + 1 make a third wave and a third band of one vertex
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (47, 70), (33, 130), (127, 129),
          (3, C - 1), (3, C), (3, C + 1), (3, 2 * C + 1),
          (B - 1, 5), (B, 5), (B + 1, 5), (2 * B + 1, 5)]
PATTERNS = ["zero", "set", "corners", "checkerboard0", "checkerboard1", "diagonal", "antidiagonal", "two_diagonal", "diamond",
            "rings", "corner_ring", "comb", "spiral", "random10", "random30", "random50", "random80", "absent"]


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def pattern(name, H, W, seed=0):
    """bool [H, W]."""
    rs = np.random.RandomState(1000 * H + W + seed)
    rr, cc = np.mgrid[0:H, 0:W]
    if name in ("zero", "absent"):
        return np.zeros((H, W), dtype=bool)
    if name == "set":
        return np.ones((H, W), dtype=bool)
    if name == "corners":                       # one pixel in each image corner
        return ((rr == 0) | (rr == H - 1)) & ((cc == 0) | (cc == W - 1))
    if name.startswith("checkerboard"):         # every inner vertex a saddle
        return (rr + cc) % 2 == int(name[-1])
    if name == "diagonal":                      # a staircase: one loop that touches itself at every saddle
        return rr == cc
    if name == "antidiagonal":
        return rr == W - 1 - cc
    if name == "two_diagonal":                  # two pixels that touch at a corner: one loop of 8 corners
        p = np.zeros((H, W), dtype=bool)
        p[0, 0] = True
        p[min(1, H - 1), min(1, W - 1)] = True
        return p
    if name == "diamond":                       # 6 x 6 tiles: the pixels at city-block distance 1 from (1, 1) or, in every other
        k = cc // 6 % 2                         # tile column, 2 from (2, 2).  Closed by corner contact alone; the hole starts at a
        return np.abs(rr % 6 - 1 - k) + np.abs(cc % 6 - 1 - k) == 1 + k      # saddle that the outer loop passes as well
    if name == "rings":                         # nested: outer loop, hole, outer loop, ...
        return np.minimum(np.minimum(rr, H - 1 - rr), np.minimum(cc, W - 1 - cc)) % 2 == 0
    if name == "corner_ring":                   # four bars that touch only at their corners, tiled: .##. / #..# / #..# / .##.
        r, c = rr % 5, cc % 5
        return (((r == 0) | (r == 3)) & ((c == 1) | (c == 2))) | (((c == 0) | (c == 3)) & ((r == 1) | (r == 2)))
    if name == "comb":
        return (rr == 0) | (cc % 2 == 0)
    if name == "spiral":                        # the rings, each cut below its top-left corner and bridged to the next one
        p = pattern("rings", H, W)
        for d in range(0, min(H, W) // 2 - 1, 2):
            p[d + 1, d] = False
            p[d + 2, d + 1] = True
        return p
    if name.startswith("random"):
        return rs.rand(H, W) < int(name[6:]) / 100.0
    raise KeyError(name)


_CASES = {}


def case(kind, name, shape):
    """(source array, thr, label, the binary map M, the reference (points, offsets)) of a case, computed once.
    kind 0 -> fp32 around THR: the clear pixels hold THR itself (the comparison is strict) or a value below, the set ones the
    next float above THR or a value above.  kind 1 -> uint16 labels from {0, 1, 2, 65535}: the traced label rotates over the
    four with the pattern, the clear pixels hold the other three; "absent" is a map of the other three alone."""
    key = (kind, name, tuple(shape))
    if key in _CASES:
        return _CASES[key]
    H, W = shape
    m = pattern(name, H, W)
    rs = np.random.RandomState(7 + H * W + PATTERNS.index(name))
    if kind == 1:
        label = int(LABELS[PATTERNS.index(name) % 4])
        others = LABELS[LABELS != label]
        src = np.where(m, np.uint16(label), others[rs.randint(0, 3, size=(H, W))]).astype(np.uint16)
        assert np.array_equal(src == label, m)
    else:
        label = 0
        edge = rs.rand(H, W) < 0.5
        low = np.where(edge, np.float32(THR), (rs.rand(H, W) * THR).astype(np.float32))
        high = np.where(edge, np.nextafter(np.float32(THR), np.float32(1)), (THR + 0.01 + rs.rand(H, W) * 0.4).astype(np.float32))
        src = np.where(m, high, low).astype(np.float32)
        assert np.array_equal(src > np.float32(THR), m)
    ref_key = ("ref", name, tuple(shape))
    if ref_key not in _CASES:
        _CASES[ref_key] = outline_ref(m)
    _CASES[key] = (src, THR, label, m, _CASES[ref_key])
    return _CASES[key]


def same_outline(a, b):
    return (a.size == b.size and a.points.dtype == b.points.dtype == np.int32 and a.offsets.dtype == b.offsets.dtype == np.int32
            and a.points.shape == b.points.shape and np.array_equal(a.points, b.points) and np.array_equal(a.offsets, b.offsets))


def run_pool_script(ann, images, check):
    """The script of the run-length tests with a clean-up step, on every image of ``images`` [(image, (row, col))] at once:
    clicks, a partial finish, a finish, an overlapping second object, an undo, a reopen, a tidy.  ``check(where, aids, masks)``
    runs after every step; ``masks`` are the masks the step returned ({aid: bool [H, W]}) or None."""
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
    check("tidy", aids, ann.tidy(aids, min_area=6, max_hole=None))
    for aid in aids:
        assert ann.finish(aid) is not None
    check("finish 3", aids, None)
    return aids
