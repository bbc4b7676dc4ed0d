"""GPU: a prompt kind per row.  ``vpu_pue_encode_rows`` and ``vpu_draw_prompt_rows`` (csrc/prompt.hip) against the single-type
exports run on every sample alone, bit for bit; ``SessionPool.predict`` with drawn boxes and strokes against the model's
single-type forward, one session at a time (ViT-B, fp32 engine mode, bit for bit; bf16 reported)."""
import random

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool
from pvpuformer_amd.isegm.inference.transforms import Roi
from test_batched_eval_box_gpu import _need_gpu, _vitb             # (the cached ViT-B models)
from test_sessions_gpu import _synth_image

pytestmark = pytest.mark.gpu

PRED_THR = 0.49
NO_BOX = (0, 0, 0, 0, -1)


# ------------------------------------------------------------------------------------------------ 1. the two kernels
def test_pue_encode_rows_equals_the_single_type_launches_sample_by_sample():
    """img 64, n = 3 of num_max 24, one sample per case; every operand a sample's kind must not read holds live values (a
    real box on click and stroke rows, non-zero profiles on click and box rows)."""
    _need_gpu()
    from pvpuformer_amd import ops
    from pvpuformer_amd.engine import click_lut
    img, n, nmax, ld = 64, 3, 24, 136
    E = 2 * img + 3
    pad = (-1.0, -1.0, -1.0)
    cases = [  # (kind, positive rows, negative rows, box, profile)
        (0, [(20, 30, 0), (40.7, 12.2, 2), pad], [(50, 12, 1), pad, pad], (30, 28, 20, 16, 0), "live"),       # kind 0
        (1, [(20, 30, 0), (41, 13, 1), pad], [(50, 12, 2), pad, pad], (30, 28, 20, 16, 1), "live"),           # box, positive slot
        (1, [(22, 31, 0), pad, pad], [(50, 12, 1), pad, pad], (40, 24, 14, 18, n + 1), "live"),               # box, negative slot
        (1, [(23, 33, 0), pad, pad], [(9, 12, 1), pad, pad], NO_BOX, "live"),                                 # box row, slot -1
        (2, [(20, 30, 0), (44, 17, 1), pad], [(50, 12, 2), pad, pad], (30, 28, 20, 16, 0), "live"),           # stroke, two positives
        (2, [pad, pad, pad], [(50, 12, 0), (3, 60, 1), pad], (30, 28, 20, 16, 0), "live"),                    # stroke, no positive
        (2, [(25, 35, 0), pad, pad], [pad, pad, pad], (30, 28, 20, 16, 0), "zero"),                           # stroke, zero profile
    ]
    B = len(cases)
    points = torch.tensor([pos + neg for _, pos, neg, _, _ in cases], dtype=torch.float32).cuda()
    kinds = torch.tensor([c[0] for c in cases], dtype=torch.int32).cuda()
    boxes = torch.tensor([c[3] for c in cases], dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(5)
    prof = torch.rand(B, 2 * img, generator=g, dtype=torch.float64)
    for b, c in enumerate(cases):
        if c[4] == "zero":
            prof[b] = 0
    prof = prof.cuda()
    lut = torch.from_numpy(click_lut()).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        got = torch.full((B, 2 * nmax, ld), 7.0, device="cuda", dtype=dtype)
        got64 = torch.full((B, 2 * nmax, E), 7.0, device="cuda", dtype=torch.float64)
        ops.pue_encode_rows(points, kinds, boxes, prof, lut, got, got64, B, n, nmax, img, ld)
        for b, (kind, *_) in enumerate(cases):
            want = torch.full((1, 2 * nmax, ld), 7.0, device="cuda", dtype=dtype)
            want64 = torch.full((1, 2 * nmax, E), 7.0, device="cuda", dtype=torch.float64)
            pts = points[b:b + 1].contiguous()
            ops.pue_encode(pts, boxes[b:b + 1].contiguous() if kind == 1 else None, lut, want, want64, 1, n, nmax, img, ld)
            if kind == 2:
                ops.pue_scribble_rows(pts, prof[b:b + 1].contiguous(), want, want64, 1, n, nmax, img, ld)
            assert torch.equal(got[b].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (dtype, b)
            assert torch.equal(got64[b].view(torch.int64), want64[0].view(torch.int64)), (dtype, b)
        # the cases are what they say: the stroke row landed in the last valid positive row, or nowhere
        assert torch.equal(got64[4, 1, :2 * img], prof[4]) and got64[4, 1, 2 * img] == 1 and got64[4, 0, 2 * img] == 1
        assert not torch.equal(got64[4, 0, :2 * img], prof[4])
        assert got64[5, :n, E - 1].tolist() == [1.0] * n                              # not-a-point rows, untouched
        assert float(got64[6, 0, :2 * img].abs().max()) == 0.0 and got64[6, 0, 2 * img:].tolist() == [1.0, 0.0, 0.0]
        assert not torch.equal(got64[1], got64[0]) and float(got[..., E:].float().abs().max()) == 0.0


def test_draw_prompt_rows_equals_the_single_type_launches_row_by_row():
    """64 x 64 planes pre-filled with the disk maps of two clicks per row, Pmax = 9; the padding behind a row's count holds
    vertices that would show if they were drawn."""
    _need_gpu()
    from pvpuformer_amd import ops
    H = W = 64
    Pmax, n = 9, 2
    rs = np.random.RandomState(11)
    long_curve = np.stack([np.linspace(4, 58, 9), 30 + 20 * np.sin(np.linspace(0, 3, 9))], 1).astype(np.int32)
    outside = np.array([(-9, 20), (30, 30), (30, 30), (70, 75), (40, -6)], dtype=np.int32)    # off-canvas ends, a repeated point
    rows = [  # (kind, count, vertices, box)
        (2, 0, [], NO_BOX),
        (2, 1, [(20, 20)], NO_BOX),
        (2, 2, [(10, 50), (50, 44)], NO_BOX),
        (2, 9, long_curve, NO_BOX),
        (2, 5, outside, (30, 28, 20, 16, 0)),
        (1, 9, long_curve, (30, 28, 20, 16, 0)),           # a box row (its curve is not read)
        (1, 0, [], NO_BOX),                                # a no-box row
        (1, 0, [], (40, 24, 14, 18, n + 1)),               # (beyond the issue's list: a box in the negative channel)
        (0, 9, long_curve, (30, 28, 20, 16, 0)),           # (and a click row whose box and curve are not read)
    ]
    B = len(rows)
    curve = np.zeros((B, Pmax, 2), np.int32)
    curve[:] = (5, 60)
    curve[:, 1::2] = (60, 3)
    for b, (_, count, verts, _) in enumerate(rows):
        if count:
            curve[b, :count] = np.asarray(verts, np.int32)
    points = -np.ones((B, 2 * n, 3), np.float32)
    for b in range(B):
        points[b, 0] = (rs.randint(5, 59), rs.randint(5, 59), 0)
        points[b, n] = (rs.randint(5, 59), rs.randint(5, 59), 1)
    points = torch.from_numpy(points).cuda()
    kinds = torch.tensor([r[0] for r in rows], dtype=torch.int32).cuda()
    counts = torch.tensor([r[1] for r in rows], dtype=torch.int32).cuda()
    boxes = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
    curve = torch.from_numpy(curve).cuda()
    base = torch.full((B, 2, H, W), 7.0, device="cuda")
    ops.disk_maps(points, None, base, B, n, H, W, 5.0)
    got = base.clone()
    ops.draw_prompt_rows(kinds, boxes, curve, counts, got, B, Pmax, n, H, W)
    for b, (kind, count, _, _) in enumerate(rows):
        want = torch.full((1, 2, H, W), 7.0, device="cuda")
        pts = points[b:b + 1].contiguous()
        ops.disk_maps(pts, boxes[b:b + 1].contiguous() if kind == 1 else None, want, 1, n, H, W, 5.0)
        if kind == 2 and count >= 1:
            ops.draw_polyline(curve[b:b + 1, :count].contiguous(), want, 1, count, H, W)
        assert torch.equal(got[b], want[0]), b
        drawn = kind == 2 and count >= 2 or kind == 1 and int(boxes[b, 4]) >= 0
        assert torch.equal(got[b], base[b]) != drawn, b
        assert float(base[b].sum()) > 0 and set(got[b].unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(got[7, 0], base[7, 0]) and not torch.equal(got[7, 1], base[7, 1])       # the negative channel
    # Pmax = 1 and 2: the grid keeps its four segment blocks for the box rows
    for pm in (1, 2):
        small = base.clone()
        ops.draw_prompt_rows(kinds, boxes, curve[:, :pm].contiguous(), counts, small, B, pm, n, H, W)
        for b in (5, 6, 7, 8):
            assert torch.equal(small[b], got[b]), (pm, b)
        assert torch.equal(small[0], base[0]) and torch.equal(small[1], base[1])


def test_type_3_is_inference_only():
    _need_gpu()
    model = _vitb("f32")
    img = torch.zeros(1, 4, 448, 448, device="cuda")
    points = torch.tensor([[[100.0, 120.0, 0.0], [-1.0, -1.0, -1.0]]], device="cuda")
    prompts = (points, torch.tensor([NO_BOX], dtype=torch.int32),
               (torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                torch.zeros(1, 896, dtype=torch.float64)), torch.zeros(1, dtype=torch.int32))
    with torch.enable_grad(), pytest.raises(RuntimeError):
        model(img, points, prompts, 3)
    with torch.no_grad():           # kind 0 everywhere: the plain forward's numbers
        assert torch.equal(model(img, points, prompts, 3)["instances"], model(img, points)["instances"])


# ------------------------------------------------------------------------------------------------ 2. end to end
def _xy(points, roi, size, mirror):
    """Image (row, col) -> network (x, y): the session's click map (``Roi.to_crop``), truncated, mirrored for the flip row."""
    out = []
    for r, c in points:
        y, x = Roi(*roi).to_crop((float(r), float(c)), size)
        x, y = int(x), int(y)
        out.append((size[1] - 1 - x if mirror else x, y))
    return np.array(out, dtype=np.int64)


def _rect(xy):
    x0, x1, y0, y1 = xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()
    return [int(0.5 * (x0 + x1)), int(0.5 * (y0 + y1)), int(x1 - x0), int(y1 - y0)]


class _Private:
    """One session of the pool beside its private predictor."""

    def __init__(self, pool, make, image, seed):
        self.sid, self.pred, self.clicker, self.seed = pool.open(image, seed=seed), make(), Clicker(device=None), seed
        self.pred.set_input_image(image)
        self.H, self.W = image.shape[:2]
        self.rng_state = None

    def add(self, positive, coords):
        self.clicker.add_click(Click(bool(positive), (int(coords[0]), int(coords[1]))))

    def run(self, box=None, stroke=None):
        """The model's single-type forward on this session alone (two rows: the crop and its mirror image)."""
        pred = self.pred
        if box is None and stroke is None:
            return pred.get_prediction(self.clicker)
        with torch.no_grad():
            image_nd, lists, _ = pred._net_input(self.clicker, None)
            points = pred.get_points_nd(lists).float()
            roi, size = pred.zoom_in._object_roi, tuple(image_nd.shape[2:])
            n_own = points.shape[1] // 2
            if box is not None:
                rows = [_rect(_xy([box[:2], box[2:]], roi, size, m)) + [n_own - 1] for m in (False, True)]
                prompts, ptype = (points, torch.tensor(rows, dtype=torch.int32).cuda(), None), 1
            else:
                xy = [_xy(stroke, roi, size, m) for m in (False, True)]
                scr = np.stack(xy)[:, None].astype(np.float64)
                rects = np.array([[_rect(v)] for v in xy], dtype=np.int64)
                prompts, ptype = (points, None, (scr, rects)), 2
                keep = random.getstate()           # the model's profile walk draws from the global generator
                if self.rng_state is None:
                    random.seed(self.seed)
                else:
                    random.setstate(self.rng_state)
            logits = pred.net(image_nd, points, prompts, ptype)["instances"]
            if stroke is not None:
                self.rng_state = random.getstate()
                random.setstate(keep)
            out = pred._finish(logits, image_nd)
            assert not pred.zoom_in.check_possible_recalculation()
            pred.prev_prediction = out
            return out.cpu().numpy()[0, 0]


def _scenario(model, exact):
    """a clicks only, b a box (and no click), c a stroke, d a box on a session that holds a roi around an earlier prediction;
    then a second call with one more click each and nothing drawn.  -> [(where, name, pool map, private map, pool mask)]."""
    zoom = dict(skip_clicks=-1, target_size=(448, 448))
    make = lambda: get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom)
    pool = SessionPool(make(), max_sessions=4, pred_thr=PRED_THR)
    sizes = [(448, 448), (480, 640), (448, 448), (480, 640)]
    ss, centres = {}, {}
    for j, (name, (H, W)) in enumerate(zip("abcd", sizes)):
        image, centres[name] = _synth_image(H, W, seed=80 + j)
        ss[name] = _Private(pool, make, image, seed=40 + j)
    a, b, c, d = (ss[k] for k in "abcd")
    # d: an earlier prediction (a bright rectangle) and the roi ZoomIn holds around it
    canvas = torch.zeros(480, 640, device="cuda")
    canvas[150:331, 220:441] = 0.9
    held = Roi(150, 330, 220, 440).grown(1.4, 200).clipped(480, 640)
    assert tuple(held) not in ((0, 479, 0, 639),)
    pool.set_states(d.sid, {"roi": tuple(held), "box": (181 * 221, 150, 330, 220, 440), "prev_prediction": canvas})
    d.pred.prev_prediction = canvas[None, None].clone()
    z = d.pred.zoom_in
    z._object_roi, z._probs, z._input_image_shape = tuple(held), canvas[None, None].clone(), (1, 4, 480, 640)
    for k, off in enumerate(((0, 0), (-14, 9), (11, -12))):
        a.add(True, (min(max(centres["a"][0] + off[0], 0), 447), min(max(centres["a"][1] + off[1], 0), 447)))
    c.add(True, centres["c"])
    c.add(False, (6, 11))
    d.add(True, (200, 300))
    d.add(True, (300, 400))
    d.add(False, (160, 230))
    box_b = (400, 500, 120, 150)                               # corners in "any order"
    box_d = (170, 240, 320, 430)
    t = np.linspace(0.0, 1.0, 37)
    cr, cc = centres["c"]
    stroke = np.stack([np.clip(cr - 60 + 120 * t, 0, 447), np.clip(cc + 50 * np.sin(5 * t), 0, 447)], 1).astype(np.int64)
    log, seen, forward = [], [], model.forward

    def spy(image, points=None, prompts=None, as_prompt_type=0, *a, **k):      # (rows, prompt type) of every forward
        seen.append((image.shape[0], as_prompt_type))
        return forward(image, points, prompts, as_prompt_type, *a, **k)

    def compare(where, got, want):
        for name, s in ss.items():
            probs = pool.probs(s.sid)
            if exact:
                assert torch.equal(probs, s.pred.prev_prediction), (where, name)
                assert np.array_equal(got[s.sid], want[name] > PRED_THR), (where, name)
            log.append((where, name, probs[0, 0].cpu().numpy().copy(), want[name].copy(), got[s.sid]))

    model.forward = spy
    try:
        return _two_calls(pool, ss, centres, held, (box_b, box_d, stroke), compare, seen, log)
    finally:
        del model.forward


def _two_calls(pool, ss, centres, held, drawn, compare, seen, log):
    a, b, c, d = (ss[k] for k in "abcd")
    (box_b, box_d, stroke), (cr, cc) = drawn, centres["c"]
    got = pool.predict({a.sid: a.clicker, b.sid: [], c.sid: c.clicker, d.sid: d.clicker},
                       boxes={b.sid: box_b, d.sid: box_d}, strokes={c.sid: stroke})
    assert tuple(pool.get_states(d.sid)["roi"]) == tuple(held)            # d kept the roi it held
    want = {"a": a.run(), "b": b.run(box=box_b), "c": c.run(stroke=stroke), "d": d.run(box=box_d)}
    assert tuple(d.pred.zoom_in._object_roi) == tuple(held)
    compare("call 1", got, want)
    a.add(False, (5, 9))
    b.add(True, centres["b"])
    c.add(True, (min(cr + 25, 447), max(cc - 30, 0)))
    d.add(False, (310, 250))
    got = pool.predict({s.sid: s.clicker for s in ss.values()})
    compare("call 2", got, {name: s.run() for name, s in ss.items()})
    assert pool.forwards == 2 and pool.readbacks == 2          # every input is zoomed to 448 x 448: one forward per call
    # the pool's two forwards (eight rows): per-row kinds, then plain clicks; the private ones (two rows) single-type
    assert [t for rows, t in seen if rows == 8] == [3, 0]
    assert [t for rows, t in seen if rows == 2] == [0, 1, 2, 1, 0, 0, 0, 0]
    return log


def test_end_to_end_fp32_drawn_prompts_equal_the_single_type_forwards():
    _need_gpu()
    log = _scenario(_vitb("f32"), exact=True)
    assert len(log) == 8
    # the drawn prompts were read: the box session's first map is not its click-free, prompt-free one
    first = {name: got for where, name, got, _, _ in log if where == "call 1"}
    assert np.isfinite(first["b"]).all() and first["b"].max() > 0


def test_end_to_end_bf16_drawn_prompts_report():
    """bf16 is not compared bit for bit (the GEMM instantiation depends on the row count: eight rows in the pool's forward,
    two in a private one).  In the manner of test_end_to_end_bf16_box_prompts_report, whose network this is: that report
    asserts no bound on the map difference, so none is asserted here; the figure is printed per session and call (maximum
    map difference relative to the private map's maximum) beside the mask IoU.

    Observed on one MI355X (ViT-B, random weights, the four sessions above): see DESIGN.md section 12."""
    _need_gpu()
    log = _scenario(_vitb("bf16"), exact=False)
    worst = 0.0
    for where, name, got, want, mask in log:
        err = np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-12)
        ref = want > PRED_THR
        iou = (mask & ref).sum() / max((mask | ref).sum(), 1)
        worst = max(worst, err)
        print(f"[bf16-report] drawn prompts, session {name} {where}: pool map vs single-type forward {err:.4g}, mask IoU {iou:.4f}")
        assert np.isfinite(got).all() and np.isfinite(want).all()
    print(f"[bf16-report] drawn prompts, maximum over sessions and calls: {worst:.4g}")
