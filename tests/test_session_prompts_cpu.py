"""CPU: drawn boxes and strokes in ``SessionPool.predict`` (isegm/inference/sessions.py) with the host stand-ins and a stub
network that records the ``prompts`` it was given: the coordinate map, the box row and its slot, the per-session generator,
the recalculation round, the errors, and the two per-row exports in the built library."""
import ctypes
import random

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.engine.prompt_sim import cal_box
from pvpuformer_amd.isegm.inference import sessions
from pvpuformer_amd.isegm.inference.batched import _padded_slot
from pvpuformer_amd.isegm.inference.clicker import Click
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool
from pvpuformer_amd.isegm.inference.transforms import Roi

from sessions_cases import StubNet, blob_image

IMG = 32          # the stub's "constructor image size": the length of a stroke profile


class RecordingNet(StubNet):
    """StubNet's logits from image and clicks; every call's (points, prompts, as_prompt_type) is kept."""
    image_size = (IMG, IMG)

    def __init__(self):
        self.calls = []

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        self.calls.append((points.clone(), prompts, as_prompt_type))
        return StubNet.__call__(self, image, points)


def _pool(net, skip_clicks=-1, zoom=True, flip=True, **kw):
    zp = dict(skip_clicks=skip_clicks, target_size=(IMG, IMG), min_crop_size=12) if zoom else None
    return SessionPool(get_predictor(net, "NoBRS", "cpu", with_flip=flip, zoom_in_params=zp), **kw)


def _np(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


def _want_xy(points, roi, size, mirror):
    """The map restated with ``Roi.to_crop`` in Python floats, ``int()`` and the click lists' mirror."""
    out = []
    for r, c in points:
        y, x = Roi(*roi).to_crop((r, c), size)
        x, y = int(x), int(y)
        out.append((size[1] - 1 - x if mirror else x, y))
    return np.array(out, dtype=np.int64)


def _want_box(xy, slot):
    x0, x1, y0, y1 = xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()
    return [int(0.5 * (x0 + x1)), int(0.5 * (y0 + y1)), int(x1 - x0), int(y1 - y0), slot]


def test_forward_types_and_the_no_box_row():
    """All clicks: the plain call.  Clicks and a box: type 1 with (0, 0, 0, 0, -1) for the others.  A stroke: type 3."""
    net = RecordingNet()
    pool = _pool(net, zoom=False, max_sessions=3)
    sids = [pool.open(blob_image(40, 48, seed=j)[0], seed=j) for j in range(3)]
    clicks = {sid: [Click(True, (20, 24), 0)] for sid in sids}
    pool.predict(clicks)
    assert net.calls[-1][1] is None and net.calls[-1][2] == 0
    pool.predict(clicks, boxes={sids[1]: (5, 6, 30, 40)})
    points, prompts, ptype = net.calls[-1]
    assert ptype == 1 and len(prompts) == 3 and prompts[2] is None and torch.equal(prompts[0], points)
    boxes = _np(prompts[1])
    assert boxes.dtype == np.int32 and boxes.shape == (6, 5)
    assert boxes[[0, 2, 3, 5]].tolist() == [[0, 0, 0, 0, -1]] * 4
    assert boxes[1].tolist() == [23, 17, 34, 25, 0] and boxes[4].tolist() == [int(0.5 * (41 + 7)), 17, 34, 25, 0]
    stroke = [(10, 8), (12, 20), (25, 30)]
    pool.predict(clicks, boxes={sids[1]: (5, 6, 30, 40)}, strokes={sids[2]: stroke})
    points, prompts, ptype = net.calls[-1]
    assert ptype == 3 and len(prompts) == 4 and pool.forwards == 3
    _, boxes, (curve, counts, profiles), kinds = prompts
    assert _np(kinds).tolist() == [0, 1, 2, 0, 1, 2] and _np(kinds).dtype == np.int32
    assert _np(boxes)[:, 4].tolist() == [-1, 0, -1, -1, 0, -1]
    assert _np(counts).tolist() == [0, 0, 3, 0, 0, 3] and tuple(curve.shape) == (6, 3, 2) and tuple(profiles.shape) == (6, 2 * IMG)
    assert _np(curve)[2].tolist() == [[8, 10], [20, 12], [30, 25]]                  # (x, y), as they are: not resampled
    assert _np(curve)[5].tolist() == [[39, 10], [27, 12], [17, 25]]
    assert _np(profiles).dtype == np.float64 and _np(profiles)[2].any() and not _np(profiles)[[0, 1, 3, 4]].any()
    # the drawn prompt held for that call only
    pool.predict(clicks)
    assert net.calls[-1][2] == 0


def test_coordinate_map_under_a_held_roi_and_on_the_flip_row():
    net = RecordingNet()
    pool = _pool(net, max_sessions=1)
    image, centre = blob_image(60, 80, seed=0)
    sid = pool.open(image)
    clicks = [Click(True, centre, 0)]
    pool.predict({sid: clicks})
    clicks.append(Click(False, (centre[0] + 4, centre[1] - 6), 1))
    corners = (centre[0] - 7, centre[1] + 9, centre[0] + 6, centre[1] - 11)
    pool.predict({sid: clicks}, boxes={sid: corners})
    roi = pool.get_states(sid)["roi"]
    assert roi is not None and tuple(roi) != (0, 59, 0, 79)              # a real crop, resized to (32, 32)
    boxes = _np(net.calls[-1][1][1])
    pts = [corners[:2], corners[2:]]
    for row, mirror in ((0, False), (1, True)):
        assert boxes[row].tolist() == _want_box(_want_xy(pts, roi, (IMG, IMG), mirror), 0), (row, boxes[row])
    assert boxes[0, 0] + boxes[1, 0] in (IMG - 1, IMG - 2)               # mirrored centres (the halves truncate)
    # the function itself: truncation toward zero on both sides of the roi, and the mirror of the truncated column
    xy = sessions.map_drawn([(0, 0), (59, 79), (10.5, 20.25)], (10, 49, 20, 69), (32, 32), False)
    assert xy.tolist() == [[int(32 * -20 / 50), int(32 * -10 / 40)], [int(32 * 59 / 50), int(32 * 49 / 40)],
                           [int(32 * 0.25 / 50), int(32 * 0.5 / 40)]]
    xm = sessions.map_drawn([(0, 0), (59, 79), (10.5, 20.25)], (10, 49, 20, 69), (32, 32), True)
    assert np.array_equal(xm[:, 0], 31 - xy[:, 0]) and np.array_equal(xm[:, 1], xy[:, 1])
    # the whole image, unscaled: the identity on pixels
    pix = [(0, 0), (59, 79), (17, 33)]
    assert sessions.map_drawn(pix, (0, 59, 0, 79), (60, 80), False).tolist() == [[c, r] for r, c in pix]


def test_corner_order_is_normalised():
    net = RecordingNet()
    pool = _pool(net, zoom=False, max_sessions=1)
    sid = pool.open(blob_image(40, 48, seed=1)[0])
    rows = []
    for box in ((5, 6, 30, 41), (30, 41, 5, 6), (5, 41, 30, 6), (30, 6, 5, 41)):
        pool.predict({sid: [Click(True, (20, 20), 0)]}, boxes={sid: box})
        rows.append(_np(net.calls[-1][1][1]).tolist())
    assert rows[0][0] == [23, 17, 35, 25, 0] and all(r == rows[0] for r in rows[1:])


@pytest.mark.parametrize("script", ["", "+", "++-", "+---", "--"])
def test_slot_and_row_against_cal_box(script):
    """``cal_box(as_allmask=False, jitter_box=False)`` on the session's own point layout with the box as the missing
    region, its slot moved into the forward's padded layout; a neighbour with four positive clicks makes the padding."""
    H, W = 40, 48
    net = RecordingNet()
    pool = _pool(net, zoom=False, flip=False, max_sessions=2)
    a, b = (pool.open(blob_image(H, W, seed=j)[0]) for j in range(2))
    mine = [Click(ch == "+", (3 + 2 * k, 5 + 3 * k), k) for k, ch in enumerate(script)]
    other = [Click(True, (4 + k, 9 + k), k) for k in range(4)]
    box = (8, 30, 21, 11)                                       # (r0, c0, r1, c1), corners in "any order"
    pool.predict({a: mine, b: other}, boxes={a: box})
    points, prompts, ptype = net.calls[-1]
    assert ptype == 1 and points.shape[1] // 2 == 4
    region = np.zeros((1, H, W), bool)
    region[0, 8:22, 11:31] = True
    own = pool.pred.get_points_nd([mine]).float().numpy()
    n_own = own.shape[1] // 2
    want = cal_box(region, region, np.zeros_like(region), own, as_allmask=False, jitter_box=False)[0]
    assert int(want[4]) == n_own - 1 == sessions.own_slot(n_own)
    want[4] = _padded_slot(int(want[4]), n_own, 4)
    got = _np(prompts[1])
    assert got[0].tolist() == want.tolist() and got[1].tolist() == [0, 0, 0, 0, -1]
    if not script:        # a box-only call: the points are all padding, the box takes row 0
        assert (points[0] == -1).all() and got[0, 4] == 0
    # cal_box's degenerate row (a centre or an extent below 1): the all-zero row
    assert sessions.box_row(np.array([[0, 5], [1, 9]]), 3) == (0, 0, 0, 0, 0)
    assert sessions.box_row(np.array([[7, 5], [7, 9]]), 3) == (0, 0, 0, 0, 0)


def _stroke(H, W, seed, P=40):
    rs = np.random.RandomState(seed)
    rows = np.clip(np.cumsum(rs.randint(-2, 4, P)) + H // 4, 0, H - 1)
    cols = np.clip(np.cumsum(rs.randint(-2, 5, P)) + W // 5, 0, W - 1)
    return np.stack([rows, cols], 1)


def _profiles_of(net, row):
    return _np(net.calls[-1][1][2][2])[row].copy()


def test_a_sessions_profiles_do_not_depend_on_who_shares_its_forward():
    """Each session draws from its own generator, for its row and then for its flip row; the global ``random`` is not
    touched."""
    H, W = 40, 48
    images = [blob_image(H, W, seed=j)[0] for j in range(2)]
    strokes = [_stroke(H, W, 3), _stroke(H, W, 4)]
    click = [Click(True, (20, 24), 0)]
    random.seed(99)
    before = random.getstate()
    shared_net = RecordingNet()
    shared = _pool(shared_net, max_sessions=2)
    sids = [shared.open(im, seed=11 + j) for j, im in enumerate(images)]
    shared.predict({sid: click for sid in sids}, strokes=dict(zip(sids, strokes)))
    assert shared.forwards == 1 and shared_net.calls[-1][2] == 3
    for j in range(2):
        net = RecordingNet()
        alone = _pool(net, max_sessions=1)
        sid = alone.open(images[j], seed=11 + j)
        alone.predict({sid: click}, strokes={sid: strokes[j]})
        for m in range(2):
            assert np.array_equal(_profiles_of(shared_net, 2 * m + j), _profiles_of(net, m)), (j, m)
        # the draws, in order: the row, then the flip row
        rng = random.Random(11 + j)
        for m in range(2):
            xy = sessions.map_drawn(strokes[j], (0, H - 1, 0, W - 1), (IMG, IMG), bool(m))
            curve, prof = sessions.stroke_row(xy, IMG, rng)
            assert np.array_equal(prof, _profiles_of(net, m)) and prof.any()
            assert np.array_equal(curve, _np(net.calls[-1][1][2][0])[m])
    assert random.getstate() == before


def test_generator_round_trips_through_get_states_and_set_states():
    H, W = 40, 48
    net = RecordingNet()
    pool = _pool(net, max_sessions=1)
    sid = pool.open(blob_image(H, W, seed=2)[0], seed=5)
    click, stroke = [Click(True, (20, 24), 0)], _stroke(H, W, 8)
    saved = pool.get_states(sid)
    assert "rng" in saved
    pool.predict({sid: click}, strokes={sid: stroke})
    first = [_profiles_of(net, m) for m in range(2)]
    pool.predict({sid: click}, strokes={sid: stroke})
    again = [_profiles_of(net, m) for m in range(2)]
    assert not all(np.array_equal(a, b) for a, b in zip(first, again))        # the generator went on
    pool.set_states(sid, saved)
    pool.predict({sid: click}, strokes={sid: stroke})
    assert all(np.array_equal(a, _profiles_of(net, m)) for m, a in enumerate(first))


def test_recalculation_round_maps_the_same_drawn_prompt_under_the_new_crop():
    """skip_clicks=0 and a small blob: round 1 runs on the whole image, the recalculation fires, round 2 runs zoomed with the
    box re-mapped and the stroke profiles drawn anew from the generator where round 1 left it."""
    H, W = 60, 80
    net = RecordingNet()
    pool = _pool(net, skip_clicks=0, max_sessions=2)
    images = [blob_image(H, W, seed=j, radius=0.15) for j in range(2)]
    a, b = (pool.open(im, seed=21 + j) for j, (im, _) in enumerate(images))
    centre = images[0][1]
    clicks = {a: [Click(True, centre, 0)], b: [Click(True, images[1][1], 0)]}
    corners = (centre[0] - 8, centre[1] - 9, centre[0] + 7, centre[1] + 10)
    stroke = np.stack([np.arange(20, 40), np.arange(30, 50)], 1)
    pool.predict(clicks, boxes={a: corners}, strokes={b: stroke})
    assert (pool.readbacks, pool.forwards) == (2, 2) and [c[2] for c in net.calls] == [3, 3]
    rois = [pool.get_states(sid)["roi"] for sid in (a, b)]
    assert all(r is not None for r in rois)
    rng = random.Random(22)
    pts = [corners[:2], corners[2:]]
    for call, size, roi_a, roi_b in ((net.calls[0], (H, W), (0, H - 1, 0, W - 1), (0, H - 1, 0, W - 1)),
                                     (net.calls[1], (IMG, IMG), rois[0], rois[1])):
        _, boxes, (curve, counts, profiles), kinds = call[1]
        assert _np(kinds).tolist() == [1, 2, 1, 2]
        for m in range(2):
            assert _np(boxes)[2 * m].tolist() == _want_box(_want_xy(pts, roi_a, size, bool(m)), 0)
            want_curve, want_prof = sessions.stroke_row(sessions.map_drawn(stroke, roi_b, size, bool(m)), IMG, rng)
            assert np.array_equal(_np(curve)[2 * m + 1], want_curve) and np.array_equal(_np(profiles)[2 * m + 1], want_prof)
    assert not np.array_equal(_np(net.calls[0][1][1]), _np(net.calls[1][1][1]))


def test_errors():
    net = RecordingNet()
    pool = _pool(net, max_sessions=2, max_stroke_points=16)
    a, b = (pool.open(blob_image(40, 48, seed=j)[0]) for j in range(2))
    click = [Click(True, (20, 24), 0)]
    line = [(5, 5), (9, 12)]
    bad = [dict(boxes={b: (1, 2, 3, 4)}),                              # not in clicks
           dict(strokes={b: line}),
           dict(boxes={a: (1, 2, 3, 4)}, strokes={a: line}),           # both
           dict(boxes={a: (1, 2, 40, 4)}), dict(boxes={a: (1, 2, 3, 48)}), dict(boxes={a: (-1, 2, 3, 4)}),
           dict(boxes={a: (1, 2, 3)}),
           dict(strokes={a: [(5, 5), (9, 48)]}), dict(strokes={a: [(5, 5), (-0.5, 3)]}),
           dict(strokes={a: [(5, 5)]}), dict(strokes={a: [(k, k) for k in range(17)]})]
    for kw in bad:
        with pytest.raises(ValueError):
            pool.predict({a: click}, **kw)
    with pytest.raises(ValueError):                                     # a stroke needs a click; a box does not
        pool.predict({a: []}, strokes={a: line})
    assert not net.calls
    pool.predict({a: []}, boxes={a: (39, 47, 0, 0)})                    # the image's own corners are inside
    assert net.calls[-1][2] == 1 and pool.forwards == 1
    pool.predict({a: click}, strokes={a: [(k, k) for k in range(16)]})
    assert net.calls[-1][2] == 3
    nosize = SessionPool(get_predictor(StubNet(), "NoBRS", "cpu", zoom_in_params=None))
    sid = nosize.open(blob_image(40, 48, seed=0)[0])
    with pytest.raises(ValueError):
        nosize.predict({sid: click}, strokes={sid: line})


def test_the_per_row_exports_are_in_the_built_library():
    import __graft_entry__ as ge
    ge.build()
    from pvpuformer_amd import _lib, ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vpu_pue_encode_rows", "vpu_draw_prompt_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(ops.pue_encode_rows) and callable(ops.draw_prompt_rows)
