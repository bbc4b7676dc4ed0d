"""The launches tests/test_spatial_f64.py makes, one row each (entry point, dtype, shape, options, input regime), and the
launchers' arithmetic restated from csrc/spatial.hip (product library: every vpu_lab_getenv knob -- VPU_BILINEAR_SPLIT_R,
VPU_CONVSEG_NBLK -- reads as unset).  tests/test_spatial_cases_cpu.py checks that the table reaches every branch and edge of
that arithmetic.

Entries: "bil_fwd" (vpu_bilinear_cl_fwd), "bil_bwd" (vpu_bilinear_cl_bwd), "upsum" (vpu_upsum_relu), "ac" (vpu_upsample_ac_fwd,
then _bwd), "cs_fwd" (vpu_convseg_fwd), "cs_bwd" (vpu_convseg_bwd), "hgf" (vpu_head_grad_fused), "winperm" (vpu_window_permute,
both directions and the round trip), "ps2" (vpu_pixel_shuffle2, both directions), "s2d" (vpu_space_to_depth2_crop, both
directions), "unsh" (vpu_pixel_unshuffle2_sums), "im2col" (vpu_patch_im2col / _prenorm / _floor).
Regimes: see spatial_ref.inputs."""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "entry dtype shape opt regime")

DTYPES = ("bf16", "f32")
VEC_C = (64, 128, 256, 512)
f32 = np.float32


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def bilinear_bwd_plan(B, h, w, H, W, C):
    """which form vpu_bilinear_cl_bwd takes: "int4" (sliced int4<8>, C == 256), "int" (int<2|4|8>), "generic" """
    R = H // h if (H % h == 0 and W % w == 0 and H // h == W // w) else 0
    if R == 8 and C == 256:                       # VPU_BILINEAR_SPLIT_R unset: the sliced form from ratio 8 only
        npix = B * h * w
        nblk = (npix + 1) // 2
        return dict(form="int4", R=R, nblk=nblk, grid=8 * ((nblk + 7) // 8), half_live=npix % 2 == 1)
    if R in (2, 4, 8):
        return dict(form="int", R=R)
    return dict(form="generic", R=R)


def upsum_plan(H, W, maps):
    """quad: upsum_relu2_kernel (2 x 2 output pixels per lane); else one pixel per lane"""
    quad = len(maps) > 0 and H % 2 == 0 and W % 2 == 0
    for h, w in maps:
        quad = quad and H % h == 0 and W % w == 0 and H // h >= 2 and W // w >= 2
    return dict(quad=quad)


def convseg_fwd_plan(rows, C, aligned=True):
    if not (C in VEC_C and aligned):
        return dict(vec=False, grid=(rows + 3) // 4)
    ppw = 64 // (C // 8)
    trips = (rows + ppw - 1) // ppw
    return dict(vec=True, ppw=ppw, trips=trips, grid=min(max(trips // 4, 1), 4096), capped=trips // 4 > 4096)


def convseg_bwd_nblk(rows):
    return min(max(rows // 64, 1), 512)          # VPU_CONVSEG_NBLK unset: the cap is 512


def convseg_bwd_plan(rows, C, dtype, aligned=True):
    """vpu_convseg_bwd (and vpu_head_grad_fused, which only has the vec form): nblk workgroups of `per` rows each"""
    if C > 512:
        return dict(error=True)
    nblk = convseg_bwd_nblk(rows)
    per = (rows + nblk - 1) // nblk
    return dict(error=False, vec=dtype == "bf16" and C in VEC_C and aligned, nblk=nblk, per=per, capped=rows // 64 > 512,
                empty_tail=sum(1 for b in range(nblk) if b * per >= rows))


def head_grad_fused_plan(rows, C, dtype, aligned=True):
    if dtype != "bf16" or C not in VEC_C or not aligned or rows < 1:
        return dict(error=True)
    return convseg_bwd_plan(rows, C, dtype)


def _ac_idx(d, scale, n):
    """src_index_ac in fp32 (-ffp-contract=off): taps i0, i1 and the weight of i1"""
    s = f32(scale * f32(d))
    i0 = min(int(s), n - 1)
    return i0, i0 + (1 if i0 < n - 1 else 0), f32(s - f32(i0))


def ac_bwd_window(n_in, n_out, parent=False):
    """upsample_ac_bwd_kernel's candidate window [lo, hi] of output indices per input index along one axis, in the kernel's fp32
    arithmetic.  ``parent``: the arithmetic before the n_in == 1 fix (the window collapsed to [0, 1])."""
    sc = f32(f32(n_in - 1) / f32(n_out - 1)) if n_out > 1 else f32(0)
    fc = f32(f32(1) / sc) if sc > 0 else f32(0)
    out = []
    for i in range(n_in):
        lo = int(math.floor(f32(fc * f32(i - 1)))) - 1
        hi = int(math.ceil(f32(fc * f32(i + 1)))) + 1
        if n_in == 1 and not parent:
            lo, hi = 0, n_out - 1
        out.append((max(lo, 0), min(hi, n_out - 1)))
    return out


def ac_contributors(n_in, n_out):
    """per input index the output indices whose fp32 taps land on it with a non-zero weight"""
    sc = f32(f32(n_in - 1) / f32(n_out - 1)) if n_out > 1 else f32(0)
    hit = [[] for _ in range(n_in)]
    for d in range(n_out):
        i0, i1, l = _ac_idx(d, sc, n_in)
        wts = {}
        wts[i0] = wts.get(i0, 0.0) + float(f32(1) - l)
        wts[i1] = wts.get(i1, 0.0) + float(l)
        for i, v in wts.items():
            if v != 0.0:
                hit[i].append(d)
    return hit


def ac_bwd_plan(h, w, H, W, parent=False):
    wy, wx = ac_bwd_window(h, H, parent), ac_bwd_window(w, W, parent)
    fast = [hi - lo < 16 for lo, hi in wx]        # per thread: the 16-slot column-weight form
    return dict(wy=wy, wx=wx, fast_all=all(fast), fast_any=any(fast))


def patch_im2col_plan(H, W, P, floor=False):
    K3 = 3 * P * P
    K3P = (K3 + 7) // 8 * 8
    return dict(vec=P % 8 == 0 and (not floor or W % 4 == 0), K3=K3, K3P=K3P, pad=K3P - K3, gh=H // P, gw=W // P,
                cropped=H % P != 0 or W % P != 0)


def pixel_unshuffle2_nblk(C):
    chunks = C // 8
    return 0 if chunks < 1 or chunks > 1024 else (1024 // chunks) * chunks


def grid_trips(total, cap=16384):
    """grid-stride trips of the 256-thread, 16384-block-capped layout kernels over ``total`` 8-element chunks"""
    grid = min(max((total + 255) // 256, 1), cap)
    return (total + grid * 256 - 1) // (grid * 256)


# ------------------------------------------------------------------------------------------------ the table
def _k(entry, dtype, regime="ord", opt=None, **shape):
    return Case(entry, dtype, dict(shape), dict(opt or {}), regime)


BIL_FWD_SHAPES = (((3, 5), (6, 10)), ((5, 7), (12, 9)), ((12, 9), (5, 7)), ((4, 6), (4, 6)), ((1, 1), (4, 6)), ((4, 6), (1, 1)),
                  ((1, 5), (8, 10)))


def _bil(entry, dt, lo, hi, C, B, regime="ord", **opt):
    return _k(entry, dt, regime, opt, B=B, h=lo[0], w=lo[1], H=hi[0], W=hi[1], C=C)


def _bil_cases():
    out = []
    for dt in DTYPES:
        for i, (lo, hi) in enumerate(BIL_FWD_SHAPES):
            out.append(_bil("bil_fwd", dt, lo, hi, (8, 24)[i % 2], 1 + i % 3))
        out.append(_bil("bil_fwd", dt, (5, 7), (12, 9), 24, 2, ld_in=40, ld_out=48, off=8))
        # backward: int<R>
        for R in (2, 4, 8):
            out.append(_bil("bil_bwd", dt, (3, 5), (3 * R, 5 * R), 24, 1 + R % 3))
        out.append(_bil("bil_bwd", dt, (1, 5), (2, 10), 8, 2))
        out.append(_bil("bil_bwd", dt, (5, 1), (10, 2), 8, 3))
        out.append(_bil("bil_bwd", dt, (3, 5), (12, 20), 24, 2, ld_in=40, ld_out=48, off=8))
        # sliced int4<8> at C == 256, and its neighbours in C
        out.append(_bil("bil_bwd", dt, (3, 3), (24, 24), 256, 1))           # 9 pixels: the last block is half live (square: 3 x 3)
        out.append(_bil("bil_bwd", dt, (2, 3), (16, 24), 256, 2))
        out.append(_bil("bil_bwd", dt, (1, 1), (8, 8), 256, 1))
        out.append(_bil("bil_bwd", dt, (2, 3), (16, 24), 256, 1, ld_in=272, ld_out=264, off=8))
        out.append(_bil("bil_bwd", dt, (2, 3), (16, 24), 248, 1))
        out.append(_bil("bil_bwd", dt, (2, 3), (16, 24), 264, 1))
        # generic
        out.append(_bil("bil_bwd", dt, (2, 3), (32, 48), 8, 1))             # ratio 16
        out.append(_bil("bil_bwd", dt, (3, 5), (6, 20), 8, 2))              # H / h = 2, W / w = 4
        for i, (lo, hi) in enumerate(BIL_FWD_SHAPES[1:]):
            out.append(_bil("bil_bwd", dt, lo, hi, (8, 24)[i % 2], 1 + i % 3))
        out.append(_bil("bil_bwd", dt, (5, 7), (12, 9), 24, 2, ld_in=48, ld_out=40, off=8))
    for R in (2, 4, 8):                                                     # exact: integers, fp32, power-of-two ratios
        out.append(_bil("bil_fwd", "f32", (3, 5), (3 * R, 5 * R), 8, 2, "int"))
        out.append(_bil("bil_bwd", "f32", (3, 5), (3 * R, 5 * R), 24, 2, "int"))
    out.append(_bil("bil_bwd", "f32", (3, 3), (24, 24), 256, 1, "int"))
    out.append(_bil("bil_bwd", "f32", (2, 3), (16, 24), 256, 2, "int"))
    return out


def _upsum_cases():
    out = []
    rows = [  # (H, W), maps, n is len(maps)
        ((9, 10), ((3, 5),)),                         # odd H: one pixel per lane
        ((6, 10), ((6, 10),)),                        # ratio 1
        ((12, 10), ((5, 7),)),                        # non-integer
        ((12, 20), ((6, 10), (5, 7))),                # one integer and one non-integer map
        ((6, 10), ()),                                # n = 0: relu alone
        ((6, 10), ((3, 5),)),                         # 2 x 2 form: ratio 2
        ((6, 12), ((2, 4),)),                         # 3
        ((12, 24), ((2, 4),)),                        # 6
        ((12, 20), ((3, 5),)),                        # 4
        ((16, 24), ((2, 3),)),                        # 8
        ((6, 20), ((3, 5),)),                         # per axis (2, 4)
        ((16, 24), ((8, 12), (4, 6), (2, 3))),        # n = 3: ratios 2, 4, 8
        ((16, 24), ((8, 12), (4, 6))),                # n = 2
        ((4, 6), ((1, 1),)),                          # a 1 x 1 low map
    ]
    for dt in DTYPES:
        for i, ((H, W), maps) in enumerate(rows):
            out.append(_k("upsum", dt, "ord", dict(maps=maps), B=1 + i % 3, H=H, W=W, C=(8, 40)[i % 2]))
        for (H, W), maps in (rows[0], rows[4], rows[11]):
            out.append(_k("upsum", dt, "relu", dict(maps=maps), B=2, H=H, W=W, C=8))
    for (H, W), maps in (rows[5], rows[8], rows[9], rows[11]):
        out.append(_k("upsum", "f32", "int", dict(maps=maps), B=2, H=H, W=W, C=8))
    return out


AC_SHAPES = (((5, 7), (17, 25)), ((3, 4), (17, 25)), ((7, 5), (23, 18)), ((23, 18), (7, 5)), ((6, 9), (6, 9)), ((4, 6), (1, 1)),
             ((4, 6), (1, 9)), ((2, 2), (9, 9)), ((1, 1), (9, 7)), ((1, 5), (9, 10)), ((5, 1), (10, 9)))


def _ac_cases():
    out = []
    for i, (lo, hi) in enumerate(AC_SHAPES):
        for planes in ((1, 3) if i < 3 else ((1, 3)[i % 2],)):
            out.append(_k("ac", "f32", planes=planes, h=lo[0], w=lo[1], H=hi[0], W=hi[1]))
    out.append(_k("ac", "f32", "int", planes=3, h=5, w=3, H=9, W=9))        # steps 1/2 and 1/4: exact coordinates
    return out


def _head_cases():
    out = []
    for dt in DTYPES:
        # ---- convseg_fwd
        for C in VEC_C + (8, 40, 72, 520):
            ppw = 64 // (C // 8) if C in VEC_C else 4
            for j, rows in enumerate(sorted({1, max(ppw - 1, 1), 85})):
                HW = (1, 5, 17 if rows == 85 else rows)[(j + C // 8) % 3]          # 1, 5, rows / B
                out.append(_k("cs_fwd", dt, "mask0" if (j + C // 64) % 2 else "ord", dict(mask=(j + C // 64) % 2), rows=rows, HW=HW, C=C))
        out.append(_k("cs_fwd", dt, "mask0", dict(mask=1), rows=16400, HW=4100, C=512))            # grid capped at 4096
        out.append(_k("cs_fwd", dt, "mask0", dict(mask=1, shift_x=16), rows=85, HW=17, C=256))
        out.append(_k("cs_fwd", dt, "mask0", dict(mask=1, shift_w=16), rows=85, HW=17, C=256))
        out.append(_k("cs_fwd", dt, "mask0", dict(mask=1, shift_mask=16), rows=85, HW=17, C=256))
        out.append(_k("cs_fwd", dt, "relu", dict(mask=0), rows=85, HW=5, C=128))
        # ---- convseg_bwd
        for i, C in enumerate(VEC_C + (8, 40, 72)):
            for j, rows in enumerate((1, 63, 129)):
                accum = (i + j) % 4
                HW = (1, 5, 43)[(i + j) % 3]
                m = (i + j) % 2
                out.append(_k("cs_bwd", dt, ("mask0" if m else "relu"), dict(mask=m, accum=accum), rows=rows, HW=HW, C=C))
        for accum in (0, 1, 2, 3):
            out.append(_k("cs_bwd", dt, "relu", dict(mask=1, accum=accum), rows=129, HW=50, C=256))
        out.append(_k("cs_bwd", dt, "mask0", dict(mask=1, accum=3), rows=12863, HW=50, C=64))      # 200 workgroups, the last two empty
        out.append(_k("cs_bwd", dt, "mask0", dict(mask=1, accum=1), rows=32837, HW=50, C=64))      # capped at 512 workgroups
        out.append(_k("cs_bwd", dt, "relu", dict(mask=1, accum=3, shift_dx=8), rows=129, HW=5, C=256))
        out.append(_k("cs_bwd", dt, "ord", dict(mask=0, accum=0, raises=1), rows=63, HW=5, C=520))
    # ---- head_grad_fused (bf16 only)
    for i, C in enumerate(VEC_C):
        for j, rows in enumerate((1, 63, 129)):
            m = (i + j) % 2
            out.append(_k("hgf", "bf16", ("mask0" if m else "relu"), dict(mask=m), rows=rows, HW=(1, 5, 50)[(i + j) % 3], C=C))
        out.append(_k("hgf", "bf16", "relu", dict(mask=1), rows=129, HW=(50, 5, 1, 50)[i], C=C))
    out.append(_k("hgf", "bf16", "mask0", dict(mask=1), rows=12863, HW=50, C=64))
    out.append(_k("hgf", "bf16", "mask0", dict(mask=1), rows=32837, HW=50, C=64))
    out.append(_k("hgf", "f32", "ord", dict(mask=0, raises=1), rows=63, HW=5, C=64))
    out.append(_k("hgf", "bf16", "ord", dict(mask=0, raises=1), rows=63, HW=5, C=72))
    out.append(_k("hgf", "bf16", "ord", dict(mask=0, raises=1, shift_dx=8), rows=63, HW=5, C=64))
    return out


def _layout_cases():
    out = []
    for dt in DTYPES:
        for i, (g, wg) in enumerate(((4, 2), (6, 3), (5, 5), (4, 1))):
            for C in (8, 72):
                out.append(_k("winperm", dt, B=1 + (i + C // 72) % 3, g=g, wg=wg, C=C))
        for C in (8, 40):
            for bias in (0, 1):
                out.append(_k("ps2", dt, opt=dict(bias=bias), B=2 + bias, h=3, w=5, C=C))
        for g in (2, 3, 4, 5, 7):
            for C in (8, 24):
                out.append(_k("s2d", dt, B=1 + g % 3, g=g, C=C))
        for C in (8, 64, 200, 2048):
            out.append(_k("unsh", dt, B=2, h=3, w=5, C=C))
            out.append(_k("unsh", dt, B=1, h=1, w=1, C=C))
        out.append(_k("unsh", dt, "int", B=3, h=3, w=5, C=200))
        out.append(_k("unsh", dt, opt=dict(raises=1), B=1, h=1, w=1, C=2056))
        for P in (16, 8, 14):
            for prenorm in (0, 1):
                out.append(_k("im2col", dt, opt=dict(prenorm=prenorm, floor=0, wg=2), B=2, H=4 * P, W=6 * P, P=P))
        for W in (53, 52):
            for prenorm in (0, 1):
                out.append(_k("im2col", dt, opt=dict(prenorm=prenorm, floor=1, wg=2), B=2, H=37, W=W, P=8))
    # past the 16384-block grid cap: a second grid-stride trip (33.6 M elements; bit-exact, no float64)
    out.append(_k("winperm", "bf16", B=1, g=64, wg=8, C=8200))
    return out


CASES = _bil_cases() + _upsum_cases() + _ac_cases() + _head_cases() + _layout_cases()


def elements(c):
    s = c.shape
    e = c.entry
    if e in ("bil_fwd", "bil_bwd"):
        return s["B"] * s["H"] * s["W"] * s["C"]
    if e == "upsum":
        return s["B"] * s["H"] * s["W"] * s["C"]
    if e == "ac":
        return s["planes"] * max(s["H"] * s["W"], s["h"] * s["w"])
    if e in ("cs_fwd", "cs_bwd", "hgf"):
        return s["rows"] * s["C"]
    if e == "winperm":
        return s["B"] * s["g"] * s["g"] * s["C"]
    if e in ("ps2", "unsh"):
        return s["B"] * 4 * s["h"] * s["w"] * s["C"]
    if e == "s2d":
        return s["B"] * s["g"] * s["g"] * s["C"]
    if e == "im2col":
        p = patch_im2col_plan(s["H"], s["W"], s["P"])
        return s["B"] * p["gh"] * p["gw"] * 2 * p["K3P"]
    raise ValueError(e)


CPU_ELEMS = 1 << 24          # rows with more elements run on the CPU at C = 8


def cpu_case(c):
    """the row the CPU checks run: itself, or (too large for the CPU) the same launch at C = 8"""
    if elements(c) <= CPU_ELEMS:
        return c
    assert c.entry == "winperm", c
    return Case(c.entry, c.dtype, dict(c.shape, C=8), c.opt, c.regime)
