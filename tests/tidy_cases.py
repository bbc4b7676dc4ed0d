"""Shared by test_tidy_cpu.py and test_tidy_gpu.py: the shapes, patterns, seeds and parameters of the region clean-up
(DESIGN section 17), the twins that restate ``SessionPool.tidy`` / ``AnnotationPool.tidy`` over private predictors and numpy
arrays with the per-pixel rules of tidy_ref.py, and the scripts both files drive."""
import itertools

import numpy as np
import torch

from pvpuformer_amd.isegm.inference.clicker import Click

from annotation_cases import TwinAnnotation, TwinPool, assert_same, rect_mask
from tidy_ref import tidy_ref

THR = 0.5
# the last two cross the 256-pixel turn of a wave, the 64-lane word and the H * W % 4 tail
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 5), (17, 13), (47, 70), (33, 130), (64, 64), (65, 257), (127, 129)]
DIAMOND = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=bool)


def shape_id(s):
    return f"{s[0]}x{s[1]}"


# ------------------------------------------------------------------------------------------------------------- patterns
def _spiral(H, W):
    """A one-pixel path that winds inwards from (0, 0) with one clear pixel between its turns: the longest union chain."""
    M = np.zeros((H, W), dtype=bool)
    r = c = 0
    dr, dc = 0, 1
    M[0, 0] = True

    def inside(y, x):
        return 0 <= y < H and 0 <= x < W

    while True:
        for _ in range(2):
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if inside(nr, nc) and not M[nr, nc] and not (inside(ar, ac) and M[ar, ac]):
                r, c = nr, nc
                M[r, c] = True
                break
            dr, dc = dc, -dr
        else:
            return M


def patterns(H, W, seed):
    """[(name, M bool [H, W], a pixel inside a hole of M or None)]; a pattern that needs more room than H x W is left out."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = [("clear", np.zeros((H, W), dtype=bool), None), ("set", np.ones((H, W), dtype=bool), None)]
    if H >= 3 and W >= 3:
        M = np.zeros((H, W), dtype=bool)
        M[H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] = DIAMOND
        out.append(("diamond", M, (H // 2, W // 2)))
    out.append(("checkerboard", (yy + xx) % 2 == 0, (1, 2) if H >= 3 and W >= 4 else None))
    depth = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    out.append(("nested rings", depth % 2 == 1, (2, 2) if H >= 7 and W >= 7 else None))
    out.append(("spiral", _spiral(H, W), None))
    M = np.zeros((H, W), dtype=bool)
    M[:, ::2] = True
    M[H - 1, :] = True
    out.append(("comb", M, None))
    R = min(H, W) // 2 - 1
    if R >= 1:
        out.append(("diagonal outline", np.abs(yy - H // 2) + np.abs(xx - W // 2) == R, (H // 2, W // 2)))
    if H >= 5 and W >= 5:
        for side, (rows, cols) in (("top", (slice(0, H // 2 + 1), W // 2)), ("bottom", (slice(H // 2, H), W // 2)),
                                   ("left", (H // 2, slice(0, W // 2 + 1))), ("right", (H // 2, slice(W // 2, W)))):
            M = np.ones((H, W), dtype=bool)
            M[rows, cols] = False           # a cavity in the centre that reaches one border through a one-pixel channel
            M[1, 1] = False                 # and a true hole beside it
            out.append((f"channel {side}", M, (1, 1)))
    for density in (0.3, 0.5, 0.6, 0.8):
        out.append((f"random {density}", rs.rand(H, W) < density, None))
    out.append(("at thr", rs.rand(H, W) < 0.5, None))
    return out


def maps_of(M, rs, at_thr=False):
    """(add, total) fp32 [H, W] with max(total, add) > THR exactly on ``M``; with ``at_thr`` every clear pixel has the value THR
    itself in one of the maps (the compare is strict)."""
    H, W = M.shape
    add, total = (rs.rand(H, W) * THR).astype(np.float32), (rs.rand(H, W) * THR).astype(np.float32)
    high = (THR + 0.01 + 0.49 * rs.rand(H, W)).astype(np.float32)
    first = rs.rand(H, W) < 0.5
    add[M & first] = high[M & first]
    total[M & ~first] = high[M & ~first]
    both = M & (rs.rand(H, W) < 0.2)
    add[both], total[both] = high[both], high[both][::-1]
    if at_thr:
        add[~M & first] = np.float32(THR)
        total[~M & ~first] = np.float32(THR)
    assert np.array_equal(np.maximum(add, total) > np.float32(THR), M)
    return add, total


def seeds_of(variant, M, hole, rs):
    """The seed lists of the issue: none, on the foreground, on the background, inside a hole, on the border, duplicated,
    outside the image."""
    H, W = M.shape
    fg, bg = np.argwhere(M), np.argwhere(~M)
    pick = lambda at: tuple(int(v) for v in at[rs.randint(len(at))])
    if variant == 0:
        return []
    if variant == 1:
        return [(*pick(fg), True) for _ in range(2)] if len(fg) else []
    if variant == 2:
        return [(*pick(bg), False), (*pick(bg), True)] if len(bg) else []
    if variant == 3:
        at = hole if hole is not None else (pick(bg) if len(bg) else (0, 0))
        return [(*at, False)]
    if variant == 4:
        return [(0, 0, True), (H - 1, W - 1, False), (0, W - 1, True), (H - 1, 0, False)]
    if variant == 5:
        at = pick(fg) if len(fg) else (0, 0)
        return [(*at, True), (*at, True), (*at, False), (*at, True)]
    return [(-1, 0, True), (H, 0, True), (0, W, False), (0, -1, False), (2 ** 31 - 1, 0, True), (H // 2, W // 2, True)]


N_SEED_VARIANTS = 7
PARAMS = list(itertools.product((0, 1, 2, 5, "above"), (0, 1, 4, None), ("all", "seeded", "largest")))


def cases(shape):
    """[dict(name, H, W, add, total, seeds, min_area, max_hole, keep)] of one shape: every pattern, with seed variants and
    parameter triples taken in rotation so that the shapes together see every value of each."""
    H, W = shape
    per_pattern = 6 if H * W <= 4096 else 2
    out, q = [], H * 31 + W
    for name, M, hole in patterns(H, W, seed=H * 1000 + W):
        for j in range(per_pattern):
            rs = np.random.RandomState(q)
            add, total = maps_of(M, rs, at_thr=name == "at thr")
            min_area, max_hole, keep = PARAMS[(q * 7) % len(PARAMS)]
            out.append(dict(name=f"{name} #{j}", H=H, W=W, add=add, total=total, seeds=seeds_of(q % N_SEED_VARIANTS, M, hole, rs),
                            min_area=H * W + 1 if min_area == "above" else min_area, max_hole=max_hole, keep=keep))
            q += 1
    return out


def call_args(case, add=True, total=True):
    """The positional arguments of tidy_ref / host_regions_tidy for ``case``, without one of the maps on demand."""
    return (case["add"] if add else None, case["total"] if total else None, case["H"], case["W"], case["seeds"], case["min_area"],
            case["max_hole"], case["keep"], THR)


def bits_equal(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- the twins
def _seeds(clicks):
    return [(int(c.coords[0]), int(c.coords[1]), bool(c.is_positive)) for c in clicks]


class TidyTwinAnnotation(TwinAnnotation):
    def tidy(self, min_area, max_hole, keep):                                   # R9
        if self.empty:
            return np.zeros((self.H, self.W), dtype=bool)
        self.snapshot()
        total = self.mask if self.mask is not None else (self.parts if self.has_parts else None)
        add = self.pred.prev_prediction[0, 0].cpu().numpy() if len(self.clicker) else None
        got = tidy_ref(add, total, self.H, self.W, _seeds(self.clicker.get_clicks()), min_area, max_hole, keep, self.thr)
        if add is not None:
            states = self.pred.get_states()
            states["prev_prediction"] = torch.from_numpy(got["add_out"])[None, None].to(self.pred.device)
            self.pred.set_states(states)
        if self.mask is not None:
            self.mask = got["total_out"]
        elif self.has_parts:
            self.parts = got["total_out"]
        return got["mask"]


class TidyTwinPool(TwinPool):
    def open(self, image):
        self.held.append(TidyTwinAnnotation(self.make, image, self.thr, self.max_undo))
        return len(self.held) - 1

    def tidy(self, aids, min_area=0, max_hole=0, keep="all"):
        return {aid: self.held[aid].tidy(min_area, max_hole, keep) for aid in aids}


def run_annotation_script(a, b, images, finite=False, on_tidy=None):
    """The issue's script on every image at once, pools ``a`` and ``b`` side by side (``b`` None: ``a`` alone), compared after
    every call.  ``on_tidy(where, aid, before, mask, kwargs)``: called for every mask ``a.tidy`` returns, with ``a``'s
    ``current_prob`` from before the call.  -> the log [(where, {aid: mask})]."""
    pools = [p for p in (a, b) if p is not None]
    aids = None
    for p in pools:
        got = [p.open(image) for image, _ in images]
        assert aids is None or got == aids
        aids = got
    shape = {aid: image.shape[:2] for aid, (image, _) in zip(aids, images)}
    centre = {aid: c for aid, (_, c) in zip(aids, images)}
    log = []

    def at(aid, dr, dc):
        H, W = shape[aid]
        return (int(np.clip(centre[aid][0] + dr, 0, H - 1)), int(np.clip(centre[aid][1] + dc, 0, W - 1)))

    def check(where, results=None):
        if results is not None:
            for aid in aids:
                assert results[0][aid].dtype == np.bool_ and results[0][aid].shape == tuple(shape[aid]), (where, aid)
                for other in results[1:]:
                    assert np.array_equal(results[0][aid], other[aid]), (where, aid, "returned mask")
            log.append((where, results[0]))
        if len(pools) == 2:
            assert_same(a, b, aids, where)
        if finite:
            for aid in aids:
                assert torch.isfinite(a.current_prob(aid)).all(), (where, aid)

    def click(where, positive, dr, dc):
        clicks = {aid: (positive, at(aid, dr, dc)) for aid in aids}
        check(where, [p.click(clicks) for p in pools])

    def tidy(where, **kw):
        before = {aid: a.current_prob(aid)[0, 0].cpu().numpy().copy() for aid in aids} if on_tidy else None
        results = [p.tidy(aids, **kw) for p in pools]
        check(where, results)
        for aid in aids if on_tidy else ():
            on_tidy(where, aid, before[aid], results[0][aid], kw)

    def each(where, name, *args):
        results = [{aid: getattr(p, name)(aid, *args) for aid in aids} for p in pools]
        for other in results[1:]:
            for aid in aids:
                ra, rb = results[0][aid], other[aid]
                assert np.array_equal(ra, rb) if isinstance(ra, np.ndarray) else ra == rb, (where, aid)
        check(where)
        return results[0]

    small = int(0.4 * min(s[0] for s in shape.values()))
    check("open")
    tidy("tidy of an empty object")
    click("click 1", True, 0, 0)
    click("click 2 (an island in the background)", True, -small, 3)
    click("click 3 (a hole in the object)", False, 2, -3)
    tidy("tidy with the clicks as seeds", min_area=10 ** 6, max_hole=None)      # island and hole are both protected by their clicks
    tidy("tidy, largest", keep="largest", max_hole=None)
    click("click 4 (on the edited map)", True, 4, 4)
    before = {aid: a.current_prob(aid).cpu().numpy().copy() for aid in aids}
    tidy("tidy, seeded", keep="seeded", max_hole=2)
    each("undo", "undo")
    for aid in aids:
        assert np.array_equal(a.current_prob(aid).cpu().numpy().view(np.uint32), before[aid].view(np.uint32)), ("undo", aid)
    each("partial finish", "partially_finish")
    tidy("tidy on the parts", min_area=40, max_hole=None)   # no clicks left: island and hole go
    click("click 5", True, 6, -5)
    tidy("tidy on parts and clicks", min_area=5, max_hole=4)
    each("finish 1", "finish")
    for p in pools:
        for aid in aids:
            m = rect_mask(*shape[aid])
            m[3, 2] = False                     # a pinhole
            m[shape[aid][0] - 2, shape[aid][1] - 3] = True      # and a speck
            p.set_mask(aid, m)
    check("set_mask")
    tidy("tidy on the initial mask", min_area=2, max_hole=1)
    each("finish 2", "finish")
    for aid in aids:                            # label 1; where nothing is left of it both pools refuse alike and label 2 is reopened
        outcome = []
        for p in pools:
            try:
                p.reopen(aid, 1)
                outcome.append(1)
            except KeyError:
                p.reopen(aid, 2)
                outcome.append(2)
        assert len(set(outcome)) == 1, (aid, outcome)
    check("reopen")
    tidy("tidy on the reopened object", keep="largest", max_hole=None)
    each("finish 3", "finish")
    return log


# ------------------------------------------------------------------------------------------------------------- sessions
class SessionTwin:
    """Session ``sid`` of ``pool`` beside a private predictor whose previous prediction takes tidy_ref's edits."""

    def __init__(self, pool, make_predictor, image):
        from pvpuformer_amd.isegm.inference.clicker import Clicker
        self.pool, self.sid = pool, pool.open(image)
        self.pred = make_predictor()
        self.pred.set_input_image(image)
        self.clicker = Clicker(device=None)
        self.H, self.W = image.shape[:2]

    def click(self, positive, coords):
        self.clicker.add_click(Click(bool(positive), (int(coords[0]), int(coords[1]))))

    def tidy(self, thr, seeds=None, **kw):
        prev = self.pred.prev_prediction[0, 0].cpu().numpy()
        seeds = _seeds(self.clicker.get_clicks()) if seeds is None else seeds
        got = tidy_ref(prev, None, self.H, self.W, seeds, kw.get("min_area", 0), kw.get("max_hole", 0), kw.get("keep", "all"), thr)
        self.pred.prev_prediction = torch.from_numpy(got["add_out"])[None, None].to(self.pred.device)
        return got["mask"]


def session_state(pool, sid):
    s = pool._session(sid)
    return s.roi, s.box, s.rng.getstate()


def run_session_script(pool, twins, exact=True):
    """Clicks, ``tidy`` and more clicks on all ``twins`` of ``pool``; with ``exact`` the pool's maps must be the private
    predictors' bit for bit after every call, so that a click after ``tidy`` has seen the edited map."""
    thr = pool.pred_thr

    def predict(where):
        got = pool.predict({t.sid: t.clicker for t in twins})
        for t in twins:
            if exact:
                t.pred.get_prediction(t.clicker)
                assert torch.equal(pool.probs(t.sid), t.pred.prev_prediction), (where, t.sid)
            assert np.array_equal(got[t.sid], pool.probs(t.sid)[0, 0].cpu().numpy() > np.float32(thr)), (where, t.sid)

    def tidy(where, seeds=None, **kw):
        states = {t.sid: session_state(pool, t.sid) for t in twins}
        reads = pool.readbacks
        named = None if seeds is None else {t.sid: [(p, (r, c)) for r, c, p in seeds(t)] for t in twins}
        got = pool.tidy([t.sid for t in twins], seeds=named, **kw)
        assert pool.readbacks == reads + 1 and sorted(got) == sorted(t.sid for t in twins), where
        for t in twins:
            assert session_state(pool, t.sid) == states[t.sid], (where, t.sid, "ZoomIn state or generator")
            assert got[t.sid].dtype == np.bool_ and got[t.sid].shape == (t.H, t.W), (where, t.sid)
            if exact:
                want = t.tidy(thr, seeds=None if seeds is None else seeds(t), **kw)
                assert np.array_equal(got[t.sid], want), (where, t.sid)
                assert torch.equal(pool.probs(t.sid), t.pred.prev_prediction), (where, t.sid)
            else:
                assert np.array_equal(got[t.sid], pool.probs(t.sid)[0, 0].cpu().numpy() > np.float32(thr)), (where, t.sid)
        return got

    for t in twins:
        t.click(True, (t.H // 2, t.W // 2))
    predict("click 1")
    for t in twins:
        t.click(True, (2, t.W - 3))             # an island
    predict("click 2")
    for t in twins:
        t.click(False, (t.H // 2 + 2, t.W // 2 - 3))    # a hole
    predict("click 3")
    kept = tidy("the clicks protect", min_area=10 ** 6, max_hole=None)
    first = lambda t: _seeds(t.clicker.get_clicks()[:1])
    cleaned = tidy("only the first click", seeds=first, min_area=10 ** 6, max_hole=None)
    for t in twins:
        t.click(True, (t.H // 2 - 3, t.W // 2 + 4))
    predict("click 4 (the network input is the edited map)")
    tidy("largest", keep="largest", max_hole=3)
    return kept, cleaned
