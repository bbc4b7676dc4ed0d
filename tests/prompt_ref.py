"""Inputs and references of tests/prompt_cases.py, sharing nothing with the kernels of csrc/prompt.hip: scipy.ndimage for the exact
distance transform and the components, oracle/vpu_oracle.py (the restatements the golden files pin against the reference model)
for the chamfer transform, the PuE rows, the disk maps and the rasteriser, numpy for the reductions.  Also the second, dumber
references the CPU test holds the first ones against (``dumb``) and the references with an error planted (``planted``) that the
table has to tell from the true ones.

``inputs(c)`` -> dict of numpy arrays, a pure function of the row; ``reference(c, inp)`` -> dict of what the launch must give."""
import zlib

import numpy as np
from scipy import ndimage

import vpu_oracle as vo
from prompt_cases import PUE_BOX_SIDES, case_id, pue_sweep

S8 = np.ones((3, 3), bool)
BBOX_THR = np.float32(0.49)


def _rng(c):
    key = c._replace(dtype="", opt={k: v for k, v in c.opt.items() if k != "out64"})       # one input set per pue geometry
    return np.random.RandomState(zlib.crc32(case_id(key).encode()) & 0x7FFFFFFF)


# ------------------------------------------------------------------------------------------------ masks
def _mask(regime, b, H, W, rs):
    m = np.ones((H, W), np.uint8)
    if regime == "corner":
        y, x = ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0))[b % 4]
        m[y, x] = 0
    elif regime == "corner0":
        m[0, 0] = 0
    elif regime == "sparse":
        m[rs.rand(H, W) < 0.05] = 0
        m[rs.randint(H), rs.randint(W)] = 0
    elif regime == "line2":
        if W >= H:
            m[:, W // 3: W // 3 + 2] = 0
        else:
            m[H // 3: H // 3 + 2, :] = 0
    elif regime == "zeros":
        m[:] = 0
    else:
        assert regime == "ones", regime
    return m


def mask_planes(c, rs):
    s = c.shape
    return np.stack([_mask(r, b, s["H"], s["W"], rs) for r in c.regime.split("+") for b in range(s["B"])])


# ------------------------------------------------------------------------------------------------ components
def _cc_mask(c, rs):
    B, H, W = c.shape["B"], c.shape["H"], c.shape["W"]
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((B, H, W), bool)
    r = c.regime
    if r in ("noise45", "noise60"):
        m = rs.rand(B, H, W) < (0.45 if r == "noise45" else 0.6)
    elif r == "checker":
        m[:] = (yy + xx) % 2 == 0
    elif r in ("diag_down", "diag_up"):
        for b in range(B):
            m[b] = ((xx - yy if r == "diag_down" else xx + yy) + b) % 3 == 0
    elif r == "comb":                                  # vertical runs joined by a spine on the last row
        m[:] = (xx % 2 == 0) | (yy == H - 1)
        m[1] = (xx % 3 == 0) | (yy == H - 1)
    elif r == "run256":                                # plane 0: a run starting at column 256; 1: one crossing it; 2: both kinds
        m[0, :, 256:] = True
        m[1, :, 250:min(W, 262)] = True
        m[2, 0::2, 256:] = True
        m[2, 1::2, 100:257] = True
        m[:, :, 0] |= (yy[:, 0] % 2 == 0)
    elif r == "plane_edge":                            # the last row of a plane and the first of the next: never joined
        m[:, H - 1, :] = True
        m[:, 0, :] = True
        if H > 2:
            m[:, 1, :] = False
    elif r == "col_edge":                              # the last column and the first: a row's end does not touch the next row
        m[:, :, W - 1] = True
        m[:, :, 0] = True
        if W > 2:
            m[:, :, 1] = False
            m[:, :, W - 2] = False
        if H > 1 and W > 2:
            m[:, 1::2, 0] = False
            m[:, 0::2, W - 1] = False
    elif r in ("k_exact", "k_plus1"):                  # kmax, kmax + 1 isolated pixels over both planes
        k = c.opt["kmax"] + (r == "k_plus1")
        for i in range(k):
            m[i % B, (i % 2) * 2, 3 + 14 * i] = True
    elif r == "two_in_wave":                           # two components inside the first 64 pixels of a row, a third in the next wave
        m[0, 0, 3:11] = True
        m[0, 0, 20:31] = True
        m[0, 2, 70:75] = True
        m[1, 1, 0:2] = True
        m[1, 1, 62:64] = True
    else:
        assert r == "cross_wave", r                    # one run over the wave boundary at column 64, one over 128
        m[0, 0, 50:81] = True
        m[1, 2, 120:130] = True
        m[1, 0, 5] = True
    return m.astype(np.uint8)


def cc_reference(mask, structure=S8):
    """roots int32 [B, H, W] (the smallest linear index of the pixel's component over the whole batch, -1 on background) and the
    table rows (root, count, ymin, ymax, xmin, xmax) in ascending root = scipy's label order, plane after plane"""
    B, H, W = mask.shape
    roots = np.full((B, H, W), -1, np.int32)
    table = []
    lin = np.arange(H * W).reshape(H, W)
    for b in range(B):
        lab, n = ndimage.label(mask[b], structure=structure)
        if n == 0:
            continue
        idx = np.arange(1, n + 1)
        mins = np.asarray(ndimage.minimum(lin, lab, idx)).astype(np.int64)
        assert np.all(np.diff(mins) > 0)                                   # labels ascend with the first pixel
        roots[b] = np.where(lab > 0, (mins + b * H * W)[np.maximum(lab, 1) - 1], -1)
        counts = np.asarray(ndimage.sum(np.ones_like(lab), lab, idx)).astype(np.int64)
        for k, sl in enumerate(ndimage.find_objects(lab)):
            table.append((mins[k] + b * H * W, counts[k], sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1))
    return roots, np.array(table, np.int64).reshape(-1, 6)


def cc_flood(mask, conn4=False, wrap=False):
    """flood fill on linear indices.  ``wrap``: the neighbours are taken on the flattened batch without looking at the row or
    plane a pixel is in (the planted error of a merge kernel without its x guards)"""
    B, H, W = mask.shape
    flat = mask.ravel() != 0
    N = flat.size
    roots = np.full(N, -1, np.int32)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([] if conn4 else [(-1, -1), (-1, 1), (1, -1), (1, 1)])
    for s in range(N):
        if not flat[s] or roots[s] >= 0:
            continue
        roots[s] = s
        stack = [s]
        while stack:
            i = stack.pop()
            b, rem = divmod(i, H * W)
            y, x = divmod(rem, W)
            for dy, dx in steps:
                if wrap:
                    j = i + dy * W + dx
                    ok = 0 <= j < N
                else:
                    ok = 0 <= y + dy < H and 0 <= x + dx < W
                    j = i + dy * W + dx
                if ok and flat[j] and roots[j] < 0:
                    roots[j] = s
                    stack.append(j)
    return roots.reshape(B, H, W)


# ------------------------------------------------------------------------------------------------ distance transforms
def edt_d2(mask, border):
    """exact integer squared distances [B, H, W] (int64; -1: no zero pixel to measure against) through scipy's float64"""
    out = np.empty(mask.shape, np.int64)
    for b, m in enumerate(mask):
        if border:
            d = ndimage.distance_transform_edt(np.pad(m, 1, "constant"))[1:-1, 1:-1]
        elif m.all():
            out[b] = -1
            continue
        else:
            d = ndimage.distance_transform_edt(m)
        out[b] = np.rint(d * d).astype(np.int64)
    return out


def edt_reference(mask, border):
    out = np.empty(mask.shape, np.float32)
    for b, m in enumerate(mask):
        if border:
            out[b] = ndimage.distance_transform_edt(np.pad(m, 1, "constant")).astype(np.float32)[1:-1, 1:-1]
        elif m.all():
            out[b] = np.inf
        else:
            out[b] = ndimage.distance_transform_edt(m).astype(np.float32)
    return out


def edt_brute(mask, border):
    """O(N^2): every pixel against every zero pixel (and the ring of the border), in integers"""
    B, H, W = mask.shape
    out = np.empty(mask.shape, np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for b, m in enumerate(mask):
        zy, zx = np.nonzero(m == 0)
        if border:
            ring = [(y, x) for y in (-1, H) for x in range(-1, W + 1)] + [(y, x) for x in (-1, W) for y in range(H)]
            zy = np.concatenate([zy, np.array([p[0] for p in ring])])
            zx = np.concatenate([zx, np.array([p[1] for p in ring])])
        if len(zy) == 0:
            out[b] = np.inf
            continue
        d2 = ((yy[..., None] - zy) ** 2 + (xx[..., None] - zx) ** 2).min(-1)
        out[b] = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return out


def chamfer_reference(mask, border):
    return np.stack([vo.chamfer_l2_5x5(np.pad(m, 1))[1:-1, 1:-1] if border else vo.chamfer_l2_5x5(m) for m in mask])


# ------------------------------------------------------------------------------------------------ disk maps
def _disk_inputs(c, rs):
    n, H, W = c.shape["n"], c.shape["H"], c.shape["W"]
    names = c.regime.split("+")
    P = -np.ones((len(names), 2 * n, 3), np.float32)

    def put(b, i, r, col):
        P[b, i] = (r, col, i)
    for b, name in enumerate(names):
        if name == "int_r2":              # integer clicks: the pixels at (3, 4), (4, 3), (5, 0), (0, 5) are at exactly r^2 = 25
            put(b, 0, min(H - 1, 6), min(W - 1, 7)); put(b, n - 1, H - 1, W - 1)
            put(b, n, 0, 0); put(b, 2 * n - 1, H // 2, W // 2)
        elif name == "half":
            put(b, 0, min(H - 1, 6) + 0.5, W // 2 + 0.5); put(b, n - 1, 0.5, 0.5)
            put(b, n, H - 0.5, W - 0.5); put(b, 2 * n - 1, H // 2 - 0.5, min(W - 1, 4) + 0.5)
        elif name == "frac":
            for i in list(rs.permutation(n)[:5]) + list(n + rs.permutation(n)[:3]):
                put(b, i, rs.rand() * (H - 1), rs.rand() * (W - 1))
        elif name == "neg_one":           # max(row, col) >= 0: a click, measured from outside the canvas
            put(b, 0, -2.0, min(3, W - 1)); put(b, n - 1, -0.5, -0.5)           # (both negative: no click)
            put(b, n, min(2, H - 1), -3.5); put(b, 2 * n - 1, -0.5, 0.0)
        elif name == "beyond":
            put(b, 0, H + 3, W - 1); put(b, n - 1, H - 0.5, W + 4.25)
            put(b, n, H + 5, W + 5); put(b, 2 * n - 1, -6.0, W + 2)
        elif name == "all":
            for i in range(2 * n):
                put(b, i, rs.rand() * (H - 1), rs.rand() * (W - 1))
        else:
            assert name == "none", name
    out = dict(points=P)
    if c.opt["box"]:
        bx = np.array([[W // 2, H // 2, W // 2, H // 2, 0], [0, 0, 0, 0, 0], [W // 2, H // 2, 2 * W + 10, 2 * H + 10, n],
                       [W // 2, H // 2, 7, 5, 2 * n - 1], [W - 1, H - 1, 9, 12, n - 1], [W // 2, H // 2, 6, 6, -1],
                       [W // 3, H // 3, 1, 1, 0]], np.int32)
        out["boxes"] = bx[:len(names)]
    return out


def disk_reference(inp, n, H, W, radius):
    d = vo.disk_maps(inp["points"], H, W, radius)
    if "boxes" in inp:
        for b, bx in enumerate(inp["boxes"]):
            if bx[4] >= 0:                # a negative slot: no box in this sample
                d[b] = vo.box_outline(d[b], bx, n)
    return d


def disk_integer(points, H, W, r2, strict=False):
    """exact integers, for samples whose valid clicks are all integers (others: None)"""
    pts = np.asarray(points)
    n = pts.shape[1] // 2
    rr, cc = np.mgrid[0:H, 0:W]
    out = []
    for b in range(pts.shape[0]):
        valid = ~(np.maximum(pts[b, :, 0], pts[b, :, 1]) < 0)
        if not np.all(pts[b, valid, :2] == np.rint(pts[b, valid, :2])):
            out.append(None)
            continue
        d = np.zeros((2, H, W), np.float32)
        for i in np.flatnonzero(valid):
            d2 = (rr - int(pts[b, i, 0])) ** 2 + (cc - int(pts[b, i, 1])) ** 2
            d[i // n] = np.maximum(d[i // n], (d2 < r2) if strict else (d2 <= r2))
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ PuE rows
def _pack_clicks(clicks, n):
    """(row, col, order) triples into the slots of as many samples as they need, 2n each"""
    B = (len(clicks) + 2 * n - 1) // (2 * n)
    P = -np.ones((B * 2 * n, 3), np.float32)
    P[:len(clicks)] = np.array(clicks, np.float32)
    return P.reshape(B, 2 * n, 3)


def _pue_inputs(c):
    n, img = c.shape["n"], c.shape["img"]
    mid = img // 2
    sweep = pue_sweep(img)
    if c.regime == "axes":
        clicks = [(v, mid, k) for k, v in enumerate(sweep)] + [(mid, v, 100 + k) for k, v in enumerate(sweep)]
        clicks += [(mid, mid, -1), (-1, -1, 7), (mid + 0.5, mid - 0.5, 8)]      # order -1 / coordinates -1 under a valid order
        return dict(points=_pack_clicks(clicks, n))
    if c.regime == "corners":
        return dict(points=_pack_clicks([(u, v, 3) for u in sweep for v in sweep], n))
    S = PUE_BOX_SIDES
    if c.regime == "boxes":
        bx = [(mid, mid, w, h) for w in S for h in S]
        for cc in (0, img - 1):
            bx += [b for s in S for b in ((cc, cc, s, s), (cc, cc, s, 60), (cc, cc, 60, s))]
        bx += [(0, img - 1, 60, 60), (img - 1, 0, 60, 60)]
    else:
        assert c.regime == "boxes_diag", c.regime
        bx = [(cc, cc, s, s) for cc in (0, mid, img - 1) for s in S]
    bx.append((0, 0, 0, 0))                                                     # the all-zero box: an empty row
    slots = [(0, n - 1, n, 2 * n - 1)[i % 4] for i in range(len(bx))]
    for slot in (-1, 2 * n, 2 * n + 5):                                         # no box / beyond the slots: the click rows alone
        bx.append((mid, mid, 60, 60))
        slots.append(slot)
    boxes = np.array([b + (s,) for b, s in zip(bx, slots)], np.int32)
    P = -np.ones((len(bx), 2 * n, 3), np.float32)
    P[:, 0] = (mid // 2, mid // 2 + 3.5, 0)                                     # a click the box may replace
    P[:, n] = (mid + 2, 1, 1)
    return dict(points=P, boxes=boxes)


def pue_reference(inp, n, num_max, img, click=None, box=None):
    """float64 [B, 2 num_max, 2 img + 3] and which rows are box rows.  A sample whose box names no slot (negative, or beyond the
    2n slots) is encoded as without a box.  ``click`` / ``box``: the functions to run (default: the oracle's)."""
    click = click or (lambda p: vo.pue_click(p, num_max, img))
    box = box or (lambda p, b: vo.pue_box(p, b, num_max, img))
    P = inp["points"]
    if "boxes" not in inp:
        return dict(rows=click(P), box_rows=np.zeros((P.shape[0], 2 * num_max), bool))
    bx = inp["boxes"]
    has = (bx[:, 4] >= 0) & (bx[:, 4] < 2 * n)
    rows = np.zeros((P.shape[0], 2 * num_max, 2 * img + 3), np.float64)
    rows[has] = box(P[has], bx[has])
    if (~has).any():
        rows[~has] = click(P[~has])
    box_rows = np.zeros((P.shape[0], 2 * num_max), bool)
    slot = bx[:, 4]
    padded = np.where(slot < n, slot, slot - n + num_max)                       # the row of slot i once each half is padded
    box_rows[np.flatnonzero(has), padded[has]] = True
    return dict(rows=rows, box_rows=box_rows)


def _box_vectors_round(cx, cy, w, h, img=448):
    """vo.box_vectors with sigma = round(radius / 3) where the reference divides with floor (the planted error)"""
    zx, zy = np.zeros(img, np.float64), np.zeros(img, np.float64)
    if cx + cy + w + h == 0:
        return zx, zy
    luts, rads = [], []
    for L in (w, h):
        k = L // 2 * 2 - 1
        r = (k - 1) // 2
        s = int(round(r / 3))
        if s == 0:
            return zx, zy
        t = np.arange(0, k, 1, np.float32)
        luts.append(np.exp(-((t - k // 2) ** 2) / (2 * s ** 2)))
        rads.append(r)
    return vo._gauss_pair(int(cx), int(cy), rads[0], rads[1], luts[0], luts[1], img)


class _patched:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __enter__(self):
        self.old = getattr(vo, self.name)
        setattr(vo, self.name, self.fn)

    def __exit__(self, *a):
        setattr(vo, self.name, self.old)


# ------------------------------------------------------------------------------------------------ rasteriser
def _line_inputs(c, rs):
    B, P, H, W = c.shape["B"], c.shape["P"], c.shape["H"], c.shape["W"]
    if c.opt["kind"] == "box":
        n = 24
        bx = [[W // 2, H // 2, W // 2, H // 2, 0], [0, 0, 0, 0, 0], [W // 2, H // 2, 2 * W + 10, 2 * H + 10, 1],
              [0, 0, W, H, n], [W - 1, H - 1, 5, 5, 2 * n - 1], [5000, -5000, 100, 100, 3], [W // 2, H // 2, 10000, 3, 4],
              [W // 2, H // 2, 2 * (W // 2), 2 * (H // 2), 5], [W // 2, H // 2, 1, 1, n + 1], [W // 2, H // 2, 30, 30, -1],
              [W // 2, H // 2, 2, 40, 6], [-5000, H // 2, 10020, 9, n + 2]]
        return dict(boxes=np.array(bx[:B], np.int32), n=n)
    cur = np.zeros((B, P, 2), np.int64)
    for b in range(B):
        if c.regime == "far":              # every other vertex far outside, +-5000
            inside = np.column_stack((rs.randint(0, W, P), rs.randint(0, H, P)))
            far = np.column_stack((rs.choice([-5000, 5000], P), rs.choice([-5000, 5000], P)))
            if b % 2:
                far[:, b // 2 % 2] = rs.randint(-50, 150, P)
            cur[b] = np.where((np.arange(P)[:, None] + b) % 2 == 0, inside, far)
        elif c.regime == "border":         # segments parallel to the border, on it and one pixel off it
            xs, ys = [-1, 0, 1, W - 2, W - 1, W], [-1, 0, 1, H - 2, H - 1, H]
            x, y = rs.choice(xs), rs.choice(ys)
            for k in range(P):
                if (k + b) % 2:
                    x = rs.choice(xs + [rs.randint(-3, W + 3)])
                else:
                    y = rs.choice(ys + [rs.randint(-3, H + 3)])
                cur[b, k] = (x, y)
        elif c.regime == "slope45":        # |dx| = |dy| and |dx| = |dy| +- 1: where x-major turns y-major
            p = np.array([W // 2, H // 2])
            for k in range(P):
                cur[b, k] = p
                d = rs.randint(1, 21)
                e = d + (-1, 0, 1)[(k + b) % 3]
                step = np.array([d, e] if (k + b) % 2 else [e, d]) * rs.choice([-1, 1], 2)
                p = p + step
                if not (-10 <= p[0] < W + 10 and -10 <= p[1] < H + 10):
                    p = p - 2 * step
        else:
            assert c.regime == "zero_len", c.regime
            cur[b] = np.cumsum(rs.randint(-4, 5, size=(P, 2)), 0) + np.array([W // 2, H // 2])
            cur[b, P // 2] = cur[b, P // 2 - 1]
    return dict(curve=cur.astype(np.int32))


def line_reference(c, inp):
    H, W = c.shape["H"], c.shape["W"]
    out = np.zeros((c.shape["B"], 2, H, W), np.float32)
    for b in range(c.shape["B"]):
        if c.opt["kind"] == "box":
            if inp["boxes"][b, 4] >= 0:
                out[b] = vo.box_outline(out[b], inp["boxes"][b], inp["n"])
        else:
            out[b] = vo.polyline_raster(out[b], inp["curve"][b])
    return out


# ------------------------------------------------------------------------------------------------ reductions
def _bbox_inputs(c, rs):
    B, H, W = c.shape["B"], c.shape["H"], c.shape["W"]
    thr = BBOX_THR
    lo, hi = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    clicks = None
    if c.regime == "thr":                  # one ulp below, equal, one ulp above
        prob = np.array([lo, thr, hi, 0, 1, thr, lo], np.float32)[rs.randint(0, 7, (B, H, W))]
    elif c.regime in ("empty", "empty_clicks"):
        prob = np.array([lo, thr, 0], np.float32)[rs.randint(0, 3, (B, H, W))]
        if c.regime == "empty_clicks":
            clicks = np.array([[H // 2, W // 3], [H - 1, W // 2]], np.int32)
    elif c.regime == "clicks_outside":
        prob = np.zeros((B, H, W), np.float32)
        prob[:, H // 3: H // 3 * 2 + 1, W // 3: W // 3 * 2 + 1] = hi
        clicks = np.array([[0, W - 1], [H - 1, 0], [H // 2, W // 2]], np.int32)
    else:
        assert c.regime == "corners", c.regime
        prob = np.full((B, H, W), thr, np.float32)
        for b in range(B):
            y, x = ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0))[b % 4]
            prob[b, y, x] = 1.0
    out = dict(prob=prob, thr=thr)
    if clicks is not None:
        out["clicks"] = clicks
    return out


def bbox_reference(inp, ge=False):
    prob, thr = inp["prob"], inp["thr"]
    B, H, W = prob.shape
    out = np.zeros((B, 5), np.int32)
    for b in range(B):
        m = prob[b] >= thr if ge else prob[b] > thr
        ys, xs = np.nonzero(m)
        cnt = len(ys)
        if "clicks" in inp:
            ys, xs = np.concatenate([ys, inp["clicks"][:, 0]]), np.concatenate([xs, inp["clicks"][:, 1]])
        out[b] = (cnt, ys.min(), ys.max(), xs.min(), xs.max()) if len(ys) else (0, H, -1, W, -1)
    return out


def _argmax_inputs(c, rs):
    P, H, W = c.shape["P"], c.shape["H"], c.shape["W"]
    HW = H * W
    dist = (rs.rand(P, HW) * 50).astype(np.float32)
    keep = (rs.rand(HW) < 0.9).astype(np.uint8)
    gap = dict(tie_wave=5, tie_waves=64, tie_blocks=256).get(c.regime)
    for p in range(P):
        i0 = (10 + 300 * p) % HW
        if gap is not None:                # the maximum twice: the first one in raster order wins
            i1 = min(i0 + gap, HW - 1)
            dist[p, [i0, i1]] = 99.0
            keep[[i0, i1]] = 1
        elif c.regime == "under_keep":     # the largest value sits under a clicked pixel
            dist[p, i0] = 1000.0
            keep[i0] = 0
        elif c.regime == "inf":
            i1, i2 = min(i0 + 700, HW - 1), min(i0 + 3, HW - 1)
            dist[p, [i0, i1]] = np.inf
            dist[p, i2] = np.inf
            keep[[i0, i1]] = 1
            if i2 not in (i0, i1):
                keep[i2] = 0
    if c.regime == "zero":
        dist[:] = 0
        keep[: HW // 2] = 1
    return dict(dist=dist.reshape(P, H, W), keep=keep.reshape(H, W))


def argmax_reference(inp, last=False):
    """the key csrc/prompt.hip documents: (float bits of the maximum) << 32 | (0xFFFFFFFF - first index in raster order)"""
    dist, keep = inp["dist"], inp["keep"]
    v = np.where(keep[None] != 0, dist, np.float32(0)).reshape(dist.shape[0], -1)
    if last:
        idx = v.shape[1] - 1 - np.argmax(v[:, ::-1], axis=1)
    else:
        idx = np.argmax(v, axis=1)
    bits = v[np.arange(len(idx)), idx].view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64))


def _errmask_inputs(c, rs):
    H, W = c.shape["H"], c.shape["W"]
    combo = (np.arange(H * W) + rs.randint(8)) % 8
    val = np.array([1, 255, 2], np.uint8)[np.arange(H * W) % 3]
    return {name: (((combo >> bit) & 1) * val).astype(np.uint8).reshape(H, W) for bit, name in enumerate(("pred", "gt", "valid"))}


def errmask_reference(inp):
    p, g, v = (inp[k] != 0 for k in ("pred", "gt", "valid"))
    return np.stack([g & ~p & v, ~g & p & v]).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the interface
def inputs(c):
    rs = _rng(c)
    if c.entry in ("edt", "chamfer5"):
        return dict(mask=mask_planes(c, rs))
    if c.entry in ("cc", "cc_table"):
        return dict(mask=_cc_mask(c, rs))
    if c.entry == "disk":
        return _disk_inputs(c, rs)
    if c.entry == "pue":
        return _pue_inputs(c)
    if c.entry == "line":
        return _line_inputs(c, rs)
    if c.entry == "bbox":
        return _bbox_inputs(c, rs)
    if c.entry == "argmax":
        return _argmax_inputs(c, rs)
    if c.entry == "errmask":
        return _errmask_inputs(c, rs)
    if c.entry == "refuse":
        return {}
    raise KeyError(f"no input generator for entry {c.entry!r}")


def reference(c, inp):
    s = c.shape
    if c.entry == "edt":
        return dict(dist=edt_reference(inp["mask"], c.opt["border"]))
    if c.entry == "chamfer5":
        return dict(dist=chamfer_reference(inp["mask"], c.opt["border"]))
    if c.entry in ("cc", "cc_table"):
        roots, table = cc_reference(inp["mask"])
        return dict(roots=roots, table=table)
    if c.entry == "disk":
        return dict(disks=disk_reference(inp, s["n"], s["H"], s["W"], c.opt["radius"]))
    if c.entry == "pue":
        return pue_reference(inp, s["n"], s["num_max"], s["img"])
    if c.entry == "line":
        return dict(disks=line_reference(c, inp))
    if c.entry == "bbox":
        return dict(box=bbox_reference(inp))
    if c.entry == "argmax":
        return dict(key=argmax_reference(inp))
    if c.entry == "errmask":
        return dict(masks=errmask_reference(inp))
    if c.entry == "refuse":
        return dict(refused=True)
    raise KeyError(f"no reference for entry {c.entry!r}")


DUMB_PIXELS = 7000         # the second references are quadratic or interpreted: rows up to this many pixels ...
CC_DUMB_PIXELS = 2400      # ... and the flood fill, pixel by pixel in Python, up to this many (3 planes of 2 x 257 are 1542)


def dumb(c, inp):
    """a second reference by other means, or None where the row is too large or the entry has none"""
    s = c.shape
    if c.entry == "edt" and inp["mask"].size <= 1600:
        return dict(dist=edt_brute(inp["mask"], c.opt["border"]))
    if c.entry in ("cc", "cc_table") and inp["mask"].size <= CC_DUMB_PIXELS:
        return dict(roots=cc_flood(inp["mask"]))
    if c.entry == "disk" and not c.opt["box"] and s["H"] * s["W"] <= DUMB_PIXELS:
        return dict(disks=disk_integer(inp["points"], s["H"], s["W"], c.opt["radius"] ** 2))
    return None


PLANTED = dict(edt=("isqrt", "sat28"), cc=("conn4", "wrap"), disk=("lt_r2",), argmax=("last_index",), bbox=("ge_thr",),
               pue=("floor", "corner_ge", "box_round"))


def planted(c, inp, kind):
    """the reference of the row with the error ``kind`` planted, in the layout of ``reference``; None: does not apply to the row"""
    s = c.shape
    if kind in ("isqrt", "sat28"):
        d2 = edt_d2(inp["mask"], c.opt["border"])
        ref = edt_reference(inp["mask"], c.opt["border"])
        if kind == "isqrt":                # (int)sqrt: the fraction dropped
            return dict(dist=np.where(d2 >= 0, np.floor(np.sqrt(np.maximum(d2, 0).astype(np.float64))), np.inf).astype(np.float32))
        return dict(dist=np.where(d2 >= 1 << 28, np.float32(np.inf), ref))
    if kind in ("conn4", "wrap"):
        if inp["mask"].size > CC_DUMB_PIXELS:
            return None
        return dict(roots=cc_flood(inp["mask"], conn4=kind == "conn4", wrap=kind == "wrap"))
    if kind == "lt_r2":
        if c.opt["box"] or s["H"] * s["W"] > DUMB_PIXELS:
            return None
        return dict(disks=disk_integer(inp["points"], s["H"], s["W"], c.opt["radius"] ** 2, strict=True))
    if kind == "last_index":
        return dict(key=argmax_reference(inp, last=True))
    if kind == "ge_thr":
        return dict(box=bbox_reference(inp, ge=True))
    if kind == "floor":                    # floor where astype(int32) truncates toward zero
        q = dict(inp, points=inp["points"].copy())
        q["points"][..., :2] = np.floor(q["points"][..., :2])
        return pue_reference(q, s["n"], s["num_max"], s["img"])
    if kind == "corner_ge":                # the corner test with an exclusive upper bound
        with _patched("_in_img", lambda x, y, w, h: not (x < 0 or x >= w or y < 0 or y >= h)):
            return pue_reference(inp, s["n"], s["num_max"], s["img"])
    if kind == "box_round":
        if "boxes" not in inp:
            return None
        with _patched("box_vectors", _box_vectors_round):
            return pue_reference(inp, s["n"], s["num_max"], s["img"])
    raise KeyError(kind)


_CACHE = {}


def case_data(c):
    """(inputs, reference) of a row, computed once for the rows that share them (the dtype / out64 forms of a PuE geometry) and
    kept for the last few rows only; neither may be written to"""
    key = case_id(c._replace(dtype="", opt={k: v for k, v in c.opt.items() if k != "out64"}))
    if key not in _CACHE:
        while len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE)))
        inp = inputs(c)
        _CACHE[key] = (inp, reference(c, inp))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the recorded reference
GOLDEN_FILE = "prompt_edges.npz"


def golden_key(c):
    """rows whose expected output the reference model itself recorded (tests/golden/prompt_edges.npz, written by
    oracle/make_golden.py::prompt_edge_fixtures): the PuE rows at its image size, the disk maps without a box at its radius"""
    s = c.shape
    if c.entry == "pue" and s["img"] == 448:
        return f"pue_n{s['n']}_{c.regime}"
    if c.entry == "disk" and not c.opt["box"] and c.opt["radius"] == 5:
        return f"disk_n{s['n']}_{s['H']}x{s['W']}"
    return None
