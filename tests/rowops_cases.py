"""The launches tests/test_rowops_f64.py makes, one row each (entry point, dtype, shape, options, input regime), and the
launchers' arithmetic restated from csrc/rowops.hip and csrc/spatial.hip (product library: every vpu_lab_getenv knob reads as
unset).  tests/test_rowops_cases_cpu.py checks that the table reaches every branch and edge of that arithmetic.

Entries: "ln" (vpu_layernorm_fwd[_pe], then vpu_layernorm_bwd[2] on its mean / rstd), "l2" (vpu_l2norm_fwd, then _bwd on its y /
inv), "colsum", "colsum_f32", "gn" (vpu_groupnorm_fwd, then _bwd), "psgn" (vpu_pixel_shuffle2_gn_stats, then
vpu_groupnorm_apply), "gate" (vpu_gate_stats + _apply + _bwd, or fused: vpu_gate_fwd_n + vpu_gate_bwd_n), "act" (vpu_act_bwd).
Regimes: see rowops_ref.inputs."""
from collections import namedtuple

Case = namedtuple("Case", "entry dtype shape opt regime")

DTYPES = ("bf16", "f32")


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def ln_fwd_plan(rows, C):
    """vpu_layernorm_fwd_pe: at most 2048 workgroups of 4 waves, one row per wave and trip"""
    NCH = 1 if C <= 512 else 2 if C <= 1024 else 4
    nb = (rows + 3) // 4
    trips = (nb + 2047) // 2048
    grid = (nb + trips - 1) // trips
    waves = grid * 4
    return dict(NCH=NCH, nb=nb, trips=trips, grid=grid, waves=waves,
                last_trip_partial=trips >= 2 and 0 < rows - (trips - 1) * waves < waves,
                live_lanes_last_chunk=((C - 1) % 512) // 8 + 1)


def ln_bwd_plan(rows, C, dtype, dy2):
    """vpu_layernorm_bwd2: nblk workgroups of NW waves, RW rows per wave and trip, PF: the next trip is prefetched"""
    nblk = min(max(rows // 16, 1), 512)
    NW = 8 if C > 1024 else 4
    RW = 2 if (C <= 1024 and dtype == "bf16" and not dy2) else 1
    half = nblk * NW
    stride = half * RW
    return dict(nblk=nblk, NW=NW, RW=RW, PF=C <= 1024, half=half, stride=stride, trips=(rows + stride - 1) // stride,
                second_row_missing=RW == 2 and rows % stride != 0)      # some wave's last trip has its first row only


def l2_plan(rows, C, aligned=True):
    vec = C in (64, 128, 256, 512) and aligned
    if not vec:
        return dict(vec=False, grid=(rows + 3) // 4)
    rpw = 64 // (C // 8)
    trips = (rows * (C // 8) + 63) // 64
    grid = min(max(trips // 4, 1), 8192)
    return dict(vec=True, rpw=rpw, trips=trips, grid=grid, capped=trips // 4 > 8192, part_wave=rows % rpw != 0,
                second_pass=rows > grid * 4 * rpw)


def colsum_plan(rows, C):
    if rows <= 64:
        return dict(small=True, grid=(C // 8 + 255) // 256)
    CL = 4 if C <= 128 else 8 if C <= 256 else 16
    return dict(small=False, CL=CL, slab=(rows + 63) // 64, col_blocks=(C + 8 * CL - 1) // (8 * CL), part_block=C % (8 * CL) != 0)


def colsum_f32_plan(rows, C):
    """8 row groups; a group takes two rows per trip (r, r + 8) while r + 8 < rows, then at most a single one"""
    pairs, singles = 0, 0
    for grp in range(8):
        r = grp
        while r + 8 < rows:
            pairs, r = pairs + 1, r + 16
        singles += r < rows
    return dict(blocks=(C + 31) // 32, part_block=C % 32 != 0, pairs=pairs, singles=singles)


def gn_plan(HW, C):
    """GnMap: 64 chunks of pixels per sample; a thread owns nrep channel chunks of one pixel slot"""
    nrep = (C // 8 + 255) // 256
    tpp = C // 8 // nrep
    slots = max(256 // tpp, 1)
    return dict(nrep=nrep, tpp=tpp, slots=slots, chunk=(HW + 63) // 64, idle_threads=256 - slots * tpp)


def gate_plan(N, C):
    return dict(slice=(N + 63) // 64, nchk=(C + 511) // 512)


# ------------------------------------------------------------------------------------------------ the table
def _k(entry, dtype, regime="ord", opt=None, **shape):
    return Case(entry, dtype, dict(shape), dict(opt or {}), regime)


LN_WIDTHS = (8, 256, 512, 520, 768, 1024, 1032, 1280, 2048)
LN_NARROW = (8, 520, 1032)            # the narrowest width of each NCH class: the multi-trip rows


def _ln_cases():
    out = []
    for dt in DTYPES:
        for C in LN_WIDTHS:                                                    # one trip; bf16 backward: second row missing
            out.append(_k("ln", dt, rows=40, C=C, opt=dict(dres=True)))
        for C in LN_NARROW:
            out.append(_k("ln", dt, rows=1, C=C, opt=dict(dres=True)))
            out.append(_k("ln", dt, rows=15, C=C))                             # no residual gradient
            out.append(_k("ln", dt, rows=8197, C=C, opt=dict(dres=True)))      # two trips, the second for 4097 of 4100 waves; nblk = 512
            out.append(_k("ln", dt, rows=16389, C=C))                          # three trips
        for pe_rows in (1, 7, 40, 64):                                         # 1, not dividing rows, rows, more than rows
            out.append(_k("ln", dt, rows=40, C=256, opt=dict(dres=True, dy2=True, pe_rows=pe_rows)))
        out.append(_k("ln", dt, rows=333, C=768, opt=dict(dy2=True, pe_rows=37)))
        out.append(_k("ln", dt, rows=40, C=1280, opt=dict(dres=True, dy2=True, pe_rows=7)))
        out.append(_k("ln", dt, rows=8197, C=8, opt=dict(dres=True, dy2=True, pe_rows=196)))
        for C in (8, 520, 1024, 2048):
            for regime in ("offset", "const", "zero", "wz"):
                out.append(_k("ln", dt, regime, rows=40, C=C, opt=dict(dres=True)))
    return out


def _l2_cases():
    out = []
    for dt in DTYPES:
        for C in (64, 128, 256, 512):
            out.append(_k("l2", dt, rows=1, C=C))
            out.append(_k("l2", dt, rows=85, C=C))            # rows % rpw != 0 (rpw = 8, 4, 2); a second pass for some waves
        for C in (8, 40, 520):
            out.append(_k("l2", dt, rows=77, C=C))
        out.append(_k("l2", dt, rows=77, C=256, opt=dict(shift_bytes=16)))      # misaligned: the scalar form
        for regime in ("offset", "zero"):
            out.append(_k("l2", dt, regime, rows=77, C=128))
    out.append(_k("l2", "bf16", rows=32773, C=512))                             # one row past the 8192-block cap: 16.8M elements
    return out


def _colsum_cases():
    out = []
    for dt in DTYPES:
        for C in (8, 128, 136, 256, 264, 520):
            for rows, beta in ((1, 0.0), (64, 1.0), (65, 0.5), (1000, 1.0)):
                out.append(_k("colsum", dt, rows=rows, C=C, opt=dict(beta=beta, ld=C + 8 if rows != 64 else C)))
        for rows in (65, 1000):
            out.append(_k("colsum", dt, "int", rows=rows, C=264, opt=dict(beta=1.0, ld=272)))
    for rows in (1, 8, 9, 16, 17, 25):
        out.append(_k("colsum_f32", "f32", rows=rows, C=40 if rows % 2 else 1000, opt=dict(beta=0.5 if rows == 9 else float(rows % 2))))
    out.append(_k("colsum_f32", "f32", "int", rows=25, C=72, opt=dict(beta=1.0)))
    return out


def _gn_cases():
    out = []
    pairs = ((8, 196), (8, 1), (192, 196), (192, 65), (192, 63), (2048, 64), (2064, 63), (2560, 65), (4096, 1), (4096, 64))
    for dt in DTYPES:
        for C, HW in pairs:
            for gelu in (0, 1):
                out.append(_k("gn", dt, B=2, HW=HW, C=C, opt=dict(gelu=gelu)))
        for regime in ("offset", "const", "zero", "wz", "tails"):
            out.append(_k("gn", dt, regime, B=3, HW=65, C=192, opt=dict(gelu=1)))
        out.append(_k("gn", dt, "tails", B=2, HW=63, C=2064, opt=dict(gelu=1)))
        for bias in (0, 1):
            out.append(_k("psgn", dt, B=3, h=9, w=11, HW=396, C=48, opt=dict(gelu=1, bias=bias)))
            out.append(_k("psgn", dt, B=2, h=3, w=5, HW=60, C=2064, opt=dict(gelu=0, bias=bias)))
    return out


def _gate_cases():
    out = []
    shapes = ((1, 1, 8), (7, 63, 520), (48, 65, 1280), (48, 196, 2048), (7, 196, 8), (1, 65, 2048))      # (nq, N, C)
    for dt in DTYPES:
        for i, (nq, N, C) in enumerate(shapes):
            B = 3 if C in (8, 520) else 2                     # B C not a multiple of 256 where C allows it
            out.append(_k("gate", dt, B=B, nq=nq, N=N, C=C, opt=dict(n=1, fused=0, accum=i % 2)))
            for n in (1, 2, 3):
                if n == 3 or i % 3 == n:
                    out.append(_k("gate", dt, B=B, nq=nq, N=N, C=C, opt=dict(n=n, fused=1, accum=(i + n) % 2)))
        for fused, n in ((0, 1), (1, 3)):
            out.append(_k("gate", dt, "ties", B=3, nq=7, N=63, C=520, opt=dict(n=n, fused=fused, accum=1)))
            out.append(_k("gate", dt, "ties", B=3, nq=48, N=65, C=8, opt=dict(n=n, fused=fused, accum=0)))
    return out


def _act_cases():
    out = []
    for dt in DTYPES:
        for kind in (0, 1):
            out.append(_k("act", dt, rows=37, cols=72, opt=dict(kind=kind, ld=(88, 80, 96))))
            out.append(_k("act", dt, rows=1, cols=8, opt=dict(kind=kind, ld=(8, 8, 8))))
            out.append(_k("act", dt, rows=300, cols=1024, opt=dict(kind=kind, ld=(1024, 1032, 1024))))
        out.append(_k("act", dt, "tails", rows=37, cols=72, opt=dict(kind=1, ld=(88, 80, 96))))
    return out


CASES = _ln_cases() + _l2_cases() + _colsum_cases() + _gn_cases() + _gate_cases() + _act_cases()


def elements(c):
    s = c.shape
    if c.entry in ("ln", "l2", "colsum", "colsum_f32"):
        return s["rows"] * s["C"]
    if c.entry == "act":
        return s["rows"] * s["cols"]
    if c.entry in ("gn", "psgn"):
        return s["B"] * s["HW"] * s["C"]
    return s["B"] * s["N"] * s["C"] * c.opt["n"]


CPU_ELEMS = 1 << 22          # rows with more elements run on the CPU at the same C with 40 rows


def cpu_case(c):
    """the row the CPU checks run: itself, or (too large for the CPU) the same launch at the same C with 40 rows"""
    if elements(c) <= CPU_ELEMS:
        return c
    assert c.entry in ("ln", "l2"), c
    return Case(c.entry, c.dtype, dict(c.shape, rows=40), c.opt, c.regime)
