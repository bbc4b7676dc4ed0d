"""The launches tests/test_tail_f64.py makes on the tail of the training step, one row each (entry, dtype, shape, options, input
regime), and the launchers' arithmetic restated from csrc/loss.hip and csrc/optim.hip.  tests/test_tail_cases_cpu.py checks that
the table reaches every branch and edge of that arithmetic and sweeps the invariants the kernels rely on without checking them;
tests/tail_ref.py draws the inputs of a row and computes its float64 reference.

Entries: "p2cl_up" (vpu_p2cl_up_fwd_bwd), "p2cl_up_items" (the same, more items than workgroups, under reserved CUs), "p2cl"
(vpu_p2cl_fwd_bwd), "nfl_dice" (vpu_nfl_dice_fwd_bwd), "finalize" (vpu_loss_finalize), "adam" (vpu_adam_step), "adam_groups"
(vpu_adam_step_groups), "adam_hyper" (vpu_adam_step_hyper), "dropout" (vpu_dropout_mask), "refuse" (arguments a launcher turns
down before any launch).  Regimes: see tail_ref.inputs."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "entry dtype shape opt regime")

P2_BAND_MAX, P2_SPAN, P2_W_MAX = 8, 5, 512
P2_LDS_LIMIT = 160 * 1024 - 6144
NFL_NBLK = 32


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def p2cl_band(w):
    """p2cl_band(): anchor rows per item, so that (band + 1) * w threads fit one workgroup (VPU_P2CL_BAND unset)"""
    return min(P2_BAND_MAX, 1024 // max(w, 1) - 1)


def anchors(n, N):
    """ac_i0 of every full-resolution index, in fp32 as the kernel computes it: min(int(fl(fl((n-1)/(N-1)) * Y)), n - 1)"""
    s = np.float32(n - 1) / np.float32(N - 1) if N > 1 else np.float32(0)
    t = s * np.arange(N, dtype=np.float32)
    assert t.dtype == np.float32
    return np.minimum(t.astype(np.int64), n - 1), s


def first_rows(n, N):
    """tYall as p2cl_up_kernel builds it (entry 1 + y for y = -1 .. n + 1): the walk starts at int(fl(1 / s) * y) - 1 and goes
    up, so it finds the first index anchored at or below y only if that start does not lie beyond it.  Returns (the kernel's
    table, the true table, the anchors)."""
    a, s = anchors(n, N)
    fh = np.float32(1) / s if s > 0 else np.float32(0)
    ar = np.arange(-1, n + 2)
    true = np.searchsorted(a, ar, side="left")
    est = np.clip((fh * ar.astype(np.float32)).astype(np.int64) - 1, 0, N)
    return np.where(ar > 0, np.maximum(est, true), 0), true, a


def block_rows(t, h, band):
    """pixel rows of every (band, halo) item: the first row anchored at max(r0 - 1, 0) .. the last row anchored at r1 - 1"""
    r0 = np.arange(0, h, band)
    r1 = np.minimum(r0 + band, h)
    return t[1 + r1] - t[1 + np.maximum(r0 - 1, 0)]


def max_rows_of(band, h, H):
    return ((band + 1) * (H - 1)) // (h - 1) + 2


def p2cl_up_plan(h, w, H, W, S=2):
    """vpu_p2cl_up_fwd_bwd: which check refuses, or the launch it makes"""
    band = p2cl_band(w)
    if (S % 2 or band < 1 or h < 2 or h > P2_W_MAX or w < 2 or W % 4 or H - 1 >= P2_SPAN * (h - 1)
            or W - 1 >= P2_SPAN * (w - 1)):
        return dict(admitted=False, refusal="args", band=band)
    assert H >= 1 and W >= 4, "the table stays away from empty maps"
    nband = (h + band - 1) // band
    max_rows = max_rows_of(band, h, H)
    shmem = ((2 * band + 2) * w + (band + 2 + max_rows) * W) * 4
    if shmem > P2_LDS_LIMIT or (band + 1) * (W // 4) > 1024:
        return dict(admitted=False, refusal="lds" if shmem > P2_LDS_LIMIT else "block", band=band, shmem=shmem)
    nthr = ((band + 1) * max(W // 4, w) + 63) // 64 * 64
    ty, ty_true, ay = first_rows(h, H)
    tx, tx_true, ax = first_rows(w, W)
    return dict(admitted=True, refusal=None, band=band, nband=nband, last_band_rows=h - (nband - 1) * band, max_rows=max_rows,
                shmem=shmem, nthr=nthr, launch_threads=min(nthr, 1024), rounded_up=nthr != (band + 1) * max(W // 4, w),
                nrp=min(nthr, 1024) // W, wide_quads=W // 4 > w, all_edge=h <= 2 and w <= 2,
                ratio_one=H == h and W == w, down=(H < h, W < w),
                tables_exact=bool((ty == ty_true).all() and (tx == tx_true).all()),
                monotone=bool((np.diff(ay) >= 0).all() and (np.diff(ax) >= 0).all()),
                max_cell_rows=int(np.diff(ty[1:h + 2]).max()), max_cell_cols=int(np.diff(tx[1:w + 2]).max()),
                max_block_rows=int(block_rows(ty, h, band).max()))


def nfl_plan(HW):
    """nfl_dice_sums_kernel / nfl_dice_grad_kernel: 32 chunk blocks per sample over HW / 4 quads, 256 threads each"""
    n4 = HW // 4
    per = (n4 + NFL_NBLK - 1) // NFL_NBLK
    live = (n4 + per - 1) // per
    return dict(admitted=HW % 4 == 0, n4=n4, per=per, empty=NFL_NBLK - live, last_partial=n4 % per != 0, trips=(per + 255) // 256)


def nfl_final_blocks(B):
    return (B + 63) // 64


def finalize_plan(B, npart):
    """loss_finalize_kernel: one workgroup of 256 threads strides over B samples and npart partials"""
    return dict(admitted=B >= 1 and npart >= 1, trips_out=(B + 255) // 256, trips_part=(npart + 255) // 256,
                idle_threads=max(256 - max(B, npart), 0), idle_out=max(256 - B, 0), idle_part=max(256 - npart, 0))


def adam_plan(n, seg_end=()):
    """adam_kernel: a thread per 4-element group; the last group is partial when n % 4; the segment of a group is found by its
    first element in a binary search over seg_end"""
    n4 = (n + 3) // 4
    ends = [e - 4 for e in seg_end if e >= 4 and e % 4 == 0 and e - 4 < n]
    depth, k = 0, len(seg_end)
    while k > 1:
        k, depth = (k + 1) // 2, depth + 1
    return dict(admitted=n > 0, n4=n4, tail=n % 4, blocks=(n4 + 255) // 256, groups_at_segment_end=ends, depth=depth,
                nseg=len(seg_end))


# ------------------------------------------------------------------------------------------------ the table
P2_SHAPES = [(2, 2, 2, 4), (512, 2, 512, 4), (9, 3, 9, 4), (17, 5, 17, 8), (16, 128, 16, 128), (9, 8, 5, 4), (10, 342, 12, 344),
             (10, 341, 12, 344), (2, 512, 4, 1028), (7, 300, 14, 1200), (9, 113, 33, 452), (12, 12, 52, 52), (6, 7, 25, 28),
             # one shape per band value the shapes above leave out (w 256 -> 3, 204 -> 4, 170 -> 5, 146 -> 6; 128 is 7); the first has
             # nrp == 1: 1024 threads, W 516
             (5, 256, 7, 516), (6, 204, 11, 208), (7, 170, 9, 172), (8, 146, 17, 148)]
P2_REGIMES = ("binary", "soft_ignore", "saturated")
P2CL_HW = (4, 4092, 4096, 4100)
NFL_HW = (4, 124, 128, 132, 4 * 32 * 256, 4 * 32 * 256 + 4)
NFL_B = (1, 65)
NFL_REGIMES = ("mixed", "one_ignored", "all0", "all1", "pm20")
FINALIZE = ((1, 1), (12, 255), (257, 256), (300, 8064))
ADAM_N = (1, 3, 4, 5, 8, 1023, 1024, 1027)
ADAM_STEPS = (1, 2, 3, 1000)
ADAM_REGIMES = ("unit", "tiny", "zero", "small_p")
DROPOUT_N = (1, 255, 256, 257, 3072)


def seg_layout(name):
    """(n, seg_end): tensors start on 8-element boundaries, the padding behind a tensor belongs to it (optim.py), the buffer ends
    with the last tensor's last element.  Returns also the tensors' own sizes."""
    sizes = dict(two8=[8, 8], three=[5, 8, 14], thousand=[(7 * i) % 19 + 1 if i % 5 else 8 for i in range(1000)])[name]
    starts, o = [], 0
    for s in sizes:
        starts.append(o)
        o += (s + 7) // 8 * 8
    n = starts[-1] + sizes[-1]
    seg_end = starts[1:] + [n]
    return n, seg_end, sizes, starts


def _adam_rows():
    out, k = [], 0

    def opt(k, **kw):
        o = dict(step=ADAM_STEPS[(k + k // 4) % 4], gs=(1.0, 0.5)[(k // 2 + k // 8) % 2], shadow=k % 3 != 0,
                 wd=(0.0, 0.02)[(k // 3) % 2], decoupled=(k // 5) % 2 == 1, layout=None)
        o.update(kw)
        return o
    for n in ADAM_N:
        for r in ADAM_REGIMES:
            out.append(Case("adam", "f32", dict(n=n), opt(k, decoupled=False), r))
            out.append(Case("adam_hyper", "f32", dict(n=n), opt(k + 1, layout="none"), r))
            out.append(Case("adam_groups", "f32", dict(n=n), opt(k + 2, layout="one"), r))
            k += 1
    for lay in ("two8", "three", "thousand"):
        n = seg_layout(lay)[0]
        for r in ADAM_REGIMES:
            for dec in (False, True):
                for wd in (0.0, 0.02):
                    out.append(Case("adam_groups", "f32", dict(n=n), opt(k, layout=lay, decoupled=dec, wd=wd), r))
                    out.append(Case("adam_hyper", "f32", dict(n=n), opt(k + 1, layout=lay, decoupled=dec, wd=wd), r))
                    k += 1
    return out


def _refusals():
    up = lambda h, w, H, W, S=2: dict(h=h, w=w, H=H, W=W, S=S)
    out = [Case("refuse", "f32", up(12, 12, 48, 48, S=3), dict(fn="p2cl_up"), "S odd"),
           Case("refuse", "f32", up(12, 12, 48, 50), dict(fn="p2cl_up"), "W % 4"),
           Case("refuse", "f32", up(1, 12, 1, 48), dict(fn="p2cl_up"), "h 1"),
           Case("refuse", "f32", up(513, 12, 513, 48), dict(fn="p2cl_up"), "h 513"),
           Case("refuse", "f32", up(12, 1, 48, 4), dict(fn="p2cl_up"), "w 1"),
           Case("refuse", "f32", up(2, 513, 4, 516), dict(fn="p2cl_up"), "w 513"),
           Case("refuse", "f32", up(12, 12, 56, 52), dict(fn="p2cl_up"), "ratio 5 in H"),
           Case("refuse", "f32", up(12, 12, 52, 56), dict(fn="p2cl_up"), "ratio 5 in W"),
           Case("refuse", "f32", up(9, 113, 33, 456), dict(fn="p2cl_up"), "block"),
           Case("refuse", "f32", dict(H=3, W=5, S=2), dict(fn="p2cl"), "HW % 4"),
           Case("refuse", "f32", dict(H=2, W=4, S=3), dict(fn="p2cl"), "S odd"),
           Case("refuse", "f32", dict(HW=6), dict(fn="nfl_dice"), "HW % 4")]
    for bad in ("B 0", "npart 0", "out null", "part null", "res null"):
        out.append(Case("refuse", "f32", {}, dict(fn="finalize"), bad))
    for fn, bads in (("adam", ("n 0", "step 0")), ("adam_groups", ("n 0", "step 0", "nseg 0", "seg_end null", "seg_lr null",
                                                                   "seg_wd null")),
                     ("adam_hyper", ("n 0", "hyper null", "seg_end null", "seg_scale null", "seg_wd null"))):
        out += [Case("refuse", "f32", {}, dict(fn=fn), bad) for bad in bads]
    return out


def _build():
    out = []
    for (h, w, H, W) in P2_SHAPES:
        for r in P2_REGIMES:
            for slots in (False, True):
                out.append(Case("p2cl_up", "f32", dict(B=2, S=4, h=h, w=w, H=H, W=W), dict(slots=slots), r))
    out.append(Case("p2cl_up_items", "f32", dict(B=8, S=24, h=17, w=5, H=17, W=8), dict(slots="consecutive"), "soft_ignore"))
    for HW in P2CL_HW:
        for r in P2_REGIMES:
            out.append(Case("p2cl", "f32", dict(B=2, S=4, HW=HW), dict(slots=True), r))
    for HW in NFL_HW:
        for B in NFL_B:
            for r in NFL_REGIMES:
                out.append(Case("nfl_dice", "f32", dict(B=B, HW=HW), {}, r))
    out += [Case("finalize", "f32", dict(B=B, npart=npart), {}, "decades") for B, npart in FINALIZE]
    out += _adam_rows()
    for n in DROPOUT_N:
        for keep in (1.0, 0.9):
            out.append(Case("dropout", "f32", dict(n=n), dict(keep=keep), "three_calls"))
    return out + _refusals()


CASES = _build()
ENTRIES = ("p2cl_up", "p2cl_up_items", "p2cl", "nfl_dice", "finalize", "adam", "adam_groups", "adam_hyper", "dropout", "refuse")


def rows(entry):
    return [c for c in CASES if c.entry == entry]


def case_id(c):
    kv = lambda d: "_".join(f"{k}{v}" for k, v in d.items())
    return "-".join(s for s in (c.entry, kv(c.shape), kv(c.opt), c.regime.replace(" ", "_")) if s)
