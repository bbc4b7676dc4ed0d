"""The launches tests/test_prompt_exact.py makes, one row each (entry, dtype, shape, options, input regime), and the launchers'
arithmetic restated from csrc/prompt.hip.  tests/test_prompt_cases_cpu.py checks that the table reaches every branch and edge of
that arithmetic; tests/prompt_ref.py draws the inputs of a row and computes what the launch has to give, bit for bit.

Entries: "edt" (vpu_edt), "chamfer5" (vpu_chamfer5), "cc" (vpu_cc_roots, then vpu_cc_table with room for every component),
"cc_table" (the same with kmax = 8), "disk" (vpu_disk_maps, with or without the box outline on top), "pue" (vpu_pue_encode),
"line" (vpu_draw_polyline; opt kind = "box": the outline alone through vpu_disk_maps), "bbox" (vpu_mask_bbox), "argmax"
(vpu_masked_argmax), "errmask" (vpu_error_masks), "refuse" (arguments a launcher turns down before any launch).
Regimes: see prompt_ref.inputs.  A regime "a+b+c" of the mask entries puts the planes of a, b and c into one launch."""
from collections import namedtuple

Case = namedtuple("Case", "entry dtype shape opt regime")

INT_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def disk_plan(n):
    """disk_maps_kernel: the valid clicks of a polarity are ballot-compacted by the first wave when all 2n slots fit its 64
    lanes; beyond that every slot is copied and walked.  LDS: [2n][2] floats and the two counts."""
    assert 1 <= n <= 1024
    compact = 2 * n <= 64
    return dict(form="compact" if compact else "fallback", lds=2 * n * 2 * 4 + 2 * 4, live_lanes=2 * n if compact else 0,
                top_lane=compact and 2 * n == 64, copy_trips=0 if compact else (2 * n + 255) // 256)


def disk_grid(H, W):
    return dict(blocks=(H * W + 255) // 256, part_block=H * W % 256 != 0, under_one_block=H * W < 256)


CH_A, CH_B, CH_C, CH_INF = 65536, 91750, 143976, 0x3FFFFFFF


def chamfer_plan(W, border, H=1):
    """chamfer5_kernel: one workgroup per mask, a thread per padded column, a wave scan and a scan over <= 16 wave totals"""
    pad = 1 if border else 0
    Wp = W + 2 * pad
    threads = (Wp + 63) // 64 * 64
    return dict(Wp=Wp, Hp=H + 2 * pad, admitted=W >= 1 and 1 <= H <= 16000 and Wp <= 1024, threads=threads, waves=threads // 64,
                lds=3 * (Wp + 4) * 4, idle_lanes=threads - Wp, taps2_in_guard=Wp < 3, taps2_reach_guard_everywhere=Wp < 5,
                # an all-ones mask without border: row i of the forward pass is CH_INF + (i + 1) a, and the taps add <= c
                walk_max=None if border else CH_INF + H * CH_A + CH_C)


EDT_LEGACY_SENTINEL = 1 << 28          # the row pass up to this table: d^2 >= 2^28 came out +inf
EDT_SENTINEL = 0xF0000000              # unsigned now


def edt_plan(H, W, border):
    """vpu_edt: a thread per column walks H rows twice; a block per row searches W candidates out of W squares in LDS.
    d2_bound: the largest squared distance a mask of this shape can hold (the far corner of a single zero; with the border the
    middle of the shorter side)."""
    admitted = 1 <= H <= 32767 and 1 <= W <= 8192
    d2_bound = min((H + 1) // 2, (W + 1) // 2) ** 2 if border else (H - 1) ** 2 + (W - 1) ** 2
    return dict(admitted=admitted, lds=4 * W, col_blocks=(W + 255) // 256, row_trips=(W + 255) // 256, d2_bound=d2_bound,
                d2_max_representable=EDT_SENTINEL - 1, sum_max=EDT_SENTINEL + (W - 1) ** 2,
                beyond_legacy=d2_bound >= EDT_LEGACY_SENTINEL)


def reduce_plan(H, W):
    """mask_bbox_kernel / masked_argmax_kernel: a block per 2048 pixels, at most 128; pixel i goes to block (i / 256) % blocks"""
    nb = (H * W + 2047) // 2048
    blocks = min(nb, 128)
    return dict(nb=nb, blocks=blocks, capped=nb > 128, trips=(H * W + blocks * 256 - 1) // (blocks * 256),
                idle_threads=max(blocks * 256 - H * W, 0), last_trip_partial=H * W % (blocks * 256) != 0)


def cc_plan(W):
    """cc_init_kernel: a block per row walks 256-column chunks and carries the run start; cc_merge_kernel: a thread per pixel"""
    chunks = (W + 255) // 256
    return dict(chunks=chunks, last_partial=W % 256 != 0, carry=chunks > 1, merge_blocks=chunks)


def pue_plan(n, num_max, img, ld):
    E = 2 * img + 3
    return dict(admitted=n <= num_max and ld >= E, E=E, rows=2 * num_max, nap_rows=2 * (num_max - n), pad_cols=ld - E,
                trips=(ld + 255) // 256, last_trip_partial=ld % 256 != 0)


# ------------------------------------------------------------------------------------------------ the table
def _k(entry, dtype, regime, opt=None, **shape):
    return Case(entry, dtype, dict(shape), dict(opt or {}), regime)


MASK_REGIMES = ("corner", "sparse", "line2", "ones", "zeros")


def holds(regime, H, W):
    """the masks a shape can hold: a corner zero needs a second pixel, the others a little room"""
    need = dict(corner=2, sparse=4, line2=3, ones=1, zeros=1, corner0=2)[regime]
    return H * W >= need


EDT_SMALL = ((1, 1, 1), (1, 1, 257), (1, 257, 1), (2, 3, 255), (2, 3, 256), (2, 3, 257), (1, 2, 8192))
EDT_TALL = ((1, 16383, 1), (1, 16384, 1), (1, 16385, 1), (1, 20000, 3), (1, 32767, 1))


def _edt_cases():
    out = []
    for B, H, W in EDT_SMALL:
        for border in (True, False):
            for regime in MASK_REGIMES:
                if holds(regime, H, W):
                    out.append(_k("edt", "u8", regime, dict(border=border), B=B, H=H, W=W))
    for B, H, W in EDT_TALL:                     # a single zero at (0, 0): the last row is H - 1 away
        out.append(_k("edt", "u8", "corner0", dict(border=False), B=B, H=H, W=W))
    out.append(_k("edt", "u8", "corner0", dict(border=True), B=1, H=20000, W=3))         # the border wins
    return out


CHAMFER_WP = (1, 2, 3, 5, 63, 64, 65, 129, 1023, 1024)
CHAMFER_H = (1, 2, 3, 7)


def _chamfer_cases():
    out = []
    for Wp in CHAMFER_WP:
        for border in (False, True):
            W = Wp - (2 if border else 0)
            if W < 1:
                continue
            for H in CHAMFER_H:
                regime = "+".join(r for r in MASK_REGIMES if holds(r, H, W))
                out.append(_k("chamfer5", "u8", regime, dict(border=border), B=1, H=H, W=W))
    out.append(_k("chamfer5", "u8", "ones+corner0", dict(border=False), B=1, H=16000, W=1))
    out.append(_k("chamfer5", "u8", "ones+corner0", dict(border=True), B=1, H=16000, W=1))
    return out


CC_W = (1, 2, 255, 256, 257, 513)
CC_H = (1, 2, 9)
CC_REGIMES = ("noise45", "noise60", "checker", "diag_down", "diag_up", "comb", "run256", "plane_edge", "col_edge")
CC_KMAX_ALL = 1 << 14                  # room for every component of a "cc" row
CC_KMAX = 8


def _cc_cases():
    out = []
    for W in CC_W:
        for H in CC_H:
            for regime in CC_REGIMES:
                if regime == "run256" and W <= 256:
                    continue
                out.append(_k("cc", "u8", regime, dict(kmax=CC_KMAX_ALL), B=3, H=H, W=W))
    for regime in ("k_exact", "k_plus1", "two_in_wave", "cross_wave"):
        out.append(_k("cc_table", "u8", regime, dict(kmax=CC_KMAX), B=2, H=3, W=130))
    return out


DISK_N = (1, 3, 24, 32, 33, 40)
DISK_HW = ((1, 1), (5, 1), (1, 300), (16, 16), (17, 255), (97, 131))
DISK_SAMPLES = ("int_r2", "half", "frac", "neg_one", "beyond", "none", "all")      # one sample of the batch each


def _disk_cases():
    out = []
    for n in DISK_N:
        for H, W in DISK_HW:
            for radius, box in ((5, False), (5, True), (3, False)):
                out.append(_k("disk", "f32", "+".join(DISK_SAMPLES), dict(radius=radius, box=box), B=len(DISK_SAMPLES), n=n, H=H, W=W))
    return out


PUE_SHAPES = ((24, 24, 448, 904), (3, 24, 448, 899), (1, 24, 448, 904), (5, 8, 32, 67), (5, 8, 32, 72))
PUE_CROSSED = ((24, 24, 448, 904), (5, 8, 32, 67))        # the rows that also take the corner and the box crossings


def pue_sweep(img):
    return (-11, -10, -9, -1.5, -0.5, 0, 0.99, 8, 9, 10, img - 11, img - 10, img - 9, img - 1, img - 0.01, img, img + 8, img + 9,
            img + 10)


PUE_BOX_SIDES = tuple(range(10)) + (10, 60)


def _pue_cases():
    out = []
    for shape in PUE_SHAPES:
        n, num_max, img, ld = shape
        regimes = ("axes", "corners", "boxes") if shape in PUE_CROSSED else ("axes", "boxes_diag")
        for regime in regimes:
            for dt in ("f32", "bf16"):
                for out64 in (True, False):
                    out.append(_k("pue", dt, regime, dict(out64=out64), n=n, num_max=num_max, img=img, ld=ld))
    return out


LINE_HW = ((97, 131), (1, 1), (1, 40), (40, 1))
LINE_P = (2, 3, 64)
LINE_REGIMES = ("far", "border", "slope45", "zero_len")


def _line_cases():
    out = []
    for H, W in LINE_HW:
        for P in LINE_P:
            for regime in LINE_REGIMES:
                out.append(_k("line", "f32", regime, dict(kind="polyline"), B=6, P=P, H=H, W=W))
        out.append(_k("line", "f32", "boxes", dict(kind="box"), B=12, P=4, H=H, W=W))
    return out


PLANES = ((1, 1), (3, 700), (45, 45), (32, 64), (513, 512))
BBOX_REGIMES = ("thr", "empty", "empty_clicks", "clicks_outside", "corners")
ARGMAX_REGIMES = ("noise", "tie_wave", "tie_waves", "tie_blocks", "under_keep", "zero", "inf")


def _reduce_cases():
    out = []
    for H, W in PLANES:
        for B in (1, 2, 64):
            for regime in BBOX_REGIMES:
                if B == 64 and H * W > 4096 and regime not in ("thr", "corners"):     # 64 planes of 513 x 512: 67 MB, twice
                    continue
                out.append(_k("bbox", "f32", regime, B=B, H=H, W=W))
        for P in (1, 5):
            for regime in ARGMAX_REGIMES:
                out.append(_k("argmax", "f32", regime, P=P, H=H, W=W))
        out.append(_k("errmask", "u8", "table", H=H, W=W))
    return out


def _refusals():
    return [_k("refuse", "u8", "edt", B=1, H=1, W=8193), _k("refuse", "u8", "edt", B=1, H=32768, W=1),
            _k("refuse", "u8", "chamfer5", dict(border=False), B=1, H=1, W=1025),
            _k("refuse", "u8", "chamfer5", dict(border=True), B=1, H=1, W=1023),
            _k("refuse", "u8", "chamfer5", dict(border=False), B=1, H=16001, W=1),
            _k("refuse", "f32", "bbox", B=65, H=2, W=2), _k("refuse", "f32", "disk", B=1, n=1025, H=2, W=2),
            _k("refuse", "f32", "pue", B=1, n=9, num_max=8, img=32, ld=67),
            _k("refuse", "f32", "pue", B=1, n=5, num_max=8, img=32, ld=66)]


CASES = (_edt_cases() + _chamfer_cases() + _cc_cases() + _disk_cases() + _pue_cases() + _line_cases() + _reduce_cases()
         + _refusals())
ENTRIES = ("edt", "chamfer5", "cc", "cc_table", "disk", "pue", "line", "bbox", "argmax", "errmask", "refuse")


def rows(entry):
    return [c for c in CASES if c.entry == entry]


def case_id(c):
    s = "-".join(f"{k}{v}" for k, v in c.shape.items())
    o = "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.opt.items())
    return "_".join(x for x in (c.dtype, s, o, c.regime.replace("+", ".")) if x)
