"""CPU checks of the resize / head / layout test table (tests/spatial_cases.py) and of its bounds (tests/spatial_ref.py):
1. the table reaches every branch and edge of the launchers' arithmetic, and the restated upsample_ac_bwd window covers every
   contributing output row and column at every table shape (it does not under the arithmetic before the h == 1 / w == 1 fix);
2. the bounds accept an honest implementation -- the same operation in fp32 on the CPU (F.interpolate and autograd for the resizes,
   the formula in fp32 for the head kernels, index permutations for the layouts), rounded once to the row's dtype -- at the
   committed constants;
3. the bounds reject wrong float64 answers: each perturbed reference fails on at least one row of its kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

import spatial_ref as sr
from spatial_cases import (AC_SHAPES, BIL_FWD_SHAPES, CASES, DTYPES, VEC_C, ac_bwd_plan, ac_bwd_window, ac_contributors,
                           bilinear_bwd_plan, convseg_bwd_nblk, convseg_bwd_plan, convseg_fwd_plan, cpu_case, elements, grid_trips,
                           head_grad_fused_plan, patch_im2col_plan, pixel_unshuffle2_nblk, upsum_plan)


def _of(entry, **kw):
    return [c for c in CASES if c.entry == entry and all(c.shape.get(k, c.opt.get(k)) == v for k, v in kw.items())]


def _lohi(c):
    s = c.shape
    return ((s["h"], s["w"]), (s["H"], s["W"]))


# ------------------------------------------------------------------------------------------------ 1. coverage
def test_constants():
    assert set(sr.COEF) == {"rfwd", "rbwd", "head", "lsum"}
    for fam, v in sr.COEF.items():
        assert 0 < v <= sr.COEF_MAX and math.log2(v) == int(math.log2(v)), (fam, v)
    assert len({sr.case_id(c) for c in CASES}) == len(CASES)
    assert {c.shape["B"] for c in CASES if "B" in c.shape} >= {1, 2, 3}


def test_table_bilinear():
    for dt in DTYPES:
        fw = [c for c in _of("bil_fwd") if c.dtype == dt and c.regime == "ord"]
        assert {_lohi(c) for c in fw} == set(BIL_FWD_SHAPES)
        assert {c.shape["C"] for c in fw} == {8, 24}
        assert any(c.opt.get("ld_in", 0) > c.shape["C"] and c.opt.get("ld_out", 0) > c.shape["C"] and c.opt.get("off") for c in fw)
        assert all(c.shape["h"] != c.shape["w"] or c.shape["h"] == 1 for c in fw) and all(c.shape["H"] != c.shape["W"] or c.shape["H"] == 1 for c in fw)
        bw = [c for c in _of("bil_bwd") if c.dtype == dt]
        plan = lambda c: bilinear_bwd_plan(*(c.shape[k] for k in ("B", "h", "w", "H", "W", "C")))
        ints = [c for c in bw if plan(c)["form"] == "int"]
        assert {plan(c)["R"] for c in ints if _lohi(c)[0] == (3, 5) and c.shape["C"] == 24} == {2, 4, 8}
        assert any(c.shape["h"] == 1 and plan(c)["R"] == 2 for c in ints) and any(c.shape["w"] == 1 and plan(c)["R"] == 2 for c in ints)
        assert {c.shape["C"] for c in ints if plan(c)["R"] == 8} >= {248, 264}
        sl = [c for c in bw if plan(c)["form"] == "int4"]
        assert all(c.shape["C"] == 256 and plan(c)["R"] == 8 for c in sl)
        assert {(c.shape["h"], c.shape["w"], c.shape["B"]) for c in sl} >= {(3, 3, 1), (2, 3, 2), (1, 1, 1)}
        assert any(plan(c)["half_live"] for c in sl) and any(not plan(c)["half_live"] for c in sl)
        assert all(plan(c)["grid"] % 8 == 0 and plan(c)["grid"] >= plan(c)["nblk"] for c in sl)
        gen = [c for c in bw if plan(c)["form"] == "generic"]
        assert any(plan(c)["R"] == 16 for c in gen)
        assert any(c.shape["H"] // c.shape["h"] == 2 and c.shape["W"] // c.shape["w"] == 4 and plan(c)["R"] == 0 for c in gen)
        assert {_lohi(c) for c in gen} >= set(BIL_FWD_SHAPES[1:])
        for form in ("int", "int4", "generic"):
            assert any(c.opt.get("ld_in", 0) > c.shape["C"] and c.opt.get("off") for c in bw if plan(c)["form"] == form), form
    # R == 4 at C == 256 stays with int<4> (the sliced int4<4> form is laboratory-only)
    assert bilinear_bwd_plan(1, 2, 3, 8, 12, 256)["form"] == "int"
    ex = [c for c in CASES if c.entry in ("bil_fwd", "bil_bwd") and c.regime == "int"]
    assert all(c.dtype == "f32" for c in ex)
    for e in ("bil_fwd", "bil_bwd"):
        assert {c.shape["H"] // c.shape["h"] for c in ex if c.entry == e} == {2, 4, 8}
    assert any(bilinear_bwd_plan(*(c.shape[k] for k in ("B", "h", "w", "H", "W", "C")))["form"] == "int4" for c in ex)


def test_table_upsum():
    for dt in DTYPES:
        rows = [c for c in _of("upsum") if c.dtype == dt]
        assert {len(c.opt["maps"]) for c in rows} == {0, 1, 2, 3} and {c.shape["C"] for c in rows} == {8, 40}
        assert all(c.shape["H"] <= 24 and c.shape["W"] <= 24 for c in rows)
        q = lambda c: upsum_plan(c.shape["H"], c.shape["W"], c.opt["maps"])["quad"]
        one, two = [c for c in rows if not q(c)], [c for c in rows if q(c)]
        assert any(c.shape["H"] % 2 for c in one)
        assert any(c.opt["maps"] == ((c.shape["H"], c.shape["W"]),) for c in one)
        assert any(len(c.opt["maps"]) == 1 and c.shape["H"] % c.opt["maps"][0][0] for c in one)
        assert any(len(c.opt["maps"]) == 2 and c.shape["H"] % c.opt["maps"][0][0] == 0 and c.shape["H"] % c.opt["maps"][1][0] for c in one)
        assert any(not c.opt["maps"] for c in one)
        ratios = lambda c: {(c.shape["H"] // h, c.shape["W"] // w) for h, w in c.opt["maps"]}
        single = set().union(*[ratios(c) for c in two if len(c.opt["maps"]) == 1])
        assert single >= {(2, 2), (3, 3), (6, 6), (4, 4), (8, 8), (2, 4)}
        assert any(ratios(c) == {(2, 2), (4, 4), (8, 8)} for c in two)
        assert any(c.opt["maps"] == ((1, 1),) for c in two)
        assert {"ord", "relu"} <= {c.regime for c in rows}
    assert {c.dtype for c in _of("upsum") if c.regime == "int"} == {"f32"}


def test_table_upsample_ac_and_window():
    rows = _of("ac")
    assert {_lohi(c) for c in rows if c.regime == "ord"} == set(AC_SHAPES) and {c.shape["planes"] for c in rows} == {1, 3}
    assert any(c.regime == "int" and _lohi(c) == ((5, 3), (9, 9)) for c in rows)
    plans = {_lohi(c): ac_bwd_plan(c.shape["h"], c.shape["w"], c.shape["H"], c.shape["W"]) for c in rows}
    assert plans[((5, 7), (17, 25))]["fast_all"]
    slow = plans[((3, 4), (17, 25))]                       # interior columns: an 18-wide window, the slow path; border columns: fast
    assert [hi - lo < 16 for lo, hi in slow["wx"]] == [True, False, False, True]
    for need in (((1, 1), (9, 7)), ((1, 5), (9, 10)), ((5, 1), (10, 9)), ((4, 6), (1, 1)), ((4, 6), (1, 9)), ((2, 2), (9, 9))):
        assert need in plans

    def uncovered(parent):
        bad = []
        for (lo, hi) in plans:
            for n_in, n_out in ((lo[0], hi[0]), (lo[1], hi[1])):
                win, hit = ac_bwd_window(n_in, n_out, parent), ac_contributors(n_in, n_out)
                for i in range(n_in):
                    if hit[i] and (min(hit[i]) < win[i][0] or max(hit[i]) > win[i][1]):
                        bad.append((n_in, n_out, i))
        return bad

    assert uncovered(parent=False) == []
    # the arithmetic before the fix drops output rows / columns 2 .. n_out - 1 of a one-row / one-column input
    assert set(uncovered(parent=True)) == {(1, 9, 0), (1, 7, 0)}
    # h > 1 is untouched by the fix
    for n_in in range(2, 25):
        for n_out in range(1, 60):
            assert ac_bwd_window(n_in, n_out) == ac_bwd_window(n_in, n_out, parent=True)


def test_table_head():
    for dt in DTYPES:
        fw = [c for c in _of("cs_fwd") if c.dtype == dt]
        al = lambda c: not any(c.opt.get(k) for k in ("shift_x", "shift_w", "shift_mask"))
        plan = lambda c: convseg_fwd_plan(c.shape["rows"], c.shape["C"], al(c))
        assert {c.shape["C"] for c in fw if plan(c)["vec"]} == set(VEC_C)
        assert {c.shape["C"] for c in fw if not plan(c)["vec"] and al(c)} == {8, 40, 72, 520}
        for C in VEC_C:
            ppw = 64 // (C // 8)
            assert {c.shape["rows"] for c in fw if c.shape["C"] == C} >= {1, max(ppw - 1, 1), 85}
        cap = [c for c in fw if plan(c).get("capped")]
        assert len(cap) == 1 and cap[0].shape["rows"] == 16400 and cap[0].shape["C"] == 512 and plan(cap[0])["grid"] == 4096
        assert not convseg_fwd_plan(16387, 512)["capped"]
        assert {c.shape["HW"] for c in fw} >= {1, 5, 17} and {bool(c.opt["mask"]) for c in fw} == {False, True}
        for k in ("shift_x", "shift_w", "shift_mask"):
            mis = [c for c in fw if c.opt.get(k)]
            assert mis and all(c.opt[k] == 16 and c.shape["C"] in VEC_C and not plan(c)["vec"] for c in mis)
        bw = [c for c in _of("cs_bwd") if c.dtype == dt]
        bplan = lambda c: convseg_bwd_plan(c.shape["rows"], c.shape["C"], dt, not c.opt.get("shift_dx"))
        ok = [c for c in bw if not bplan(c)["error"]]
        assert [c.shape["C"] for c in bw if bplan(c)["error"]] == [520] and all(c.opt.get("raises") for c in bw if bplan(c)["error"])
        assert {c.shape["C"] for c in ok} == set(VEC_C) | {8, 40, 72}
        assert {c.shape["C"] for c in ok if bplan(c)["vec"]} == (set(VEC_C) if dt == "bf16" else set())
        assert {c.opt["accum"] for c in ok} == {0, 1, 2, 3} and {c.shape["rows"] for c in ok} == {1, 63, 129, 12863, 32837}
        assert {c.opt["accum"] for c in ok if c.shape["C"] == 256 and c.shape["rows"] == 129 and not c.opt.get("shift_dx")} == {0, 1, 2, 3}
        p = convseg_bwd_plan(129, 64, dt)
        assert p["nblk"] == 2 and p["per"] == 65 and p["empty_tail"] == 0
        p = convseg_bwd_plan(12863, 64, dt)
        assert p["nblk"] == 200 and p["per"] == 65 and p["empty_tail"] >= 1 and not p["capped"]
        p = convseg_bwd_plan(32837, 64, dt)
        assert p["nblk"] == 512 and p["capped"] and convseg_bwd_nblk(63) == 1
        mis = [c for c in ok if c.opt.get("shift_dx")]
        assert mis and all(c.opt["shift_dx"] == 8 and c.shape["C"] in VEC_C and not bplan(c)["vec"] for c in mis)
    hg = _of("hgf")
    ok = [c for c in hg if not c.opt.get("raises")]
    assert {c.dtype for c in ok} == {"bf16"} and {c.shape["C"] for c in ok} == set(VEC_C)
    assert {c.shape["rows"] for c in ok} == {1, 63, 129, 12863, 32837} and {c.shape["HW"] for c in ok} == {1, 5, 50}
    assert {bool(c.opt["mask"]) for c in ok} == {False, True} and {"relu", "mask0"} <= {c.regime for c in ok}
    assert all(not head_grad_fused_plan(c.shape["rows"], c.shape["C"], c.dtype)["error"] for c in ok)
    assert any(c.shape["rows"] % c.shape["HW"] and c.shape["HW"] < c.shape["rows"] for c in ok)      # images straddle workgroups
    bad = [c for c in hg if c.opt.get("raises")]
    assert sorted((c.dtype, c.shape["C"], c.opt.get("shift_dx", 0)) for c in bad) == [("bf16", 64, 8), ("bf16", 72, 0), ("f32", 64, 0)]
    assert all(head_grad_fused_plan(c.shape["rows"], c.shape["C"], c.dtype, not c.opt.get("shift_dx"))["error"] for c in bad)
    # the planted values of the `relu` and `mask0` regimes
    c = [c for c in ok if c.regime == "relu"][0]
    x = sr.inputs(c, "cpu")["x"].float().view(-1)
    assert bool((x == 0).any()) and bool((torch.signbit(x) & (x == 0)).any()) and bool(((x > 0) & (x < 1e-20)).any()) and bool(((x < 0) & (x > -1e-20)).any())
    m = sr._mask0(3, 64, "cpu")
    assert bool((m == 0).any(1).all()) and not torch.equal(m[0], m[1]) and not torch.equal(m[1], m[2])
    assert set(m.unique().tolist()) == {0.0, torch.tensor(1.0 / 0.9, dtype=torch.float32).item()}


def test_table_layout():
    for dt in DTYPES:
        wp = [c for c in _of("winperm") if c.dtype == dt and c.shape["C"] <= 72]
        assert {(c.shape["g"], c.shape["wg"]) for c in wp} == {(4, 2), (6, 3), (5, 5), (4, 1)} and {c.shape["C"] for c in wp} == {8, 72}
        ps = [c for c in _of("ps2") if c.dtype == dt]
        assert {(c.shape["h"], c.shape["w"]) for c in ps} == {(3, 5)} and {c.shape["C"] for c in ps} == {8, 40} and {c.opt["bias"] for c in ps} == {0, 1}
        sd = [c for c in _of("s2d") if c.dtype == dt]
        assert {c.shape["g"] for c in sd} == {2, 3, 4, 5, 7} and {c.shape["C"] for c in sd} == {8, 24}
        un = [c for c in _of("unsh") if c.dtype == dt]
        assert {c.shape["C"] for c in un if not c.opt.get("raises")} == {8, 64, 200, 2048}
        assert [c.shape["C"] for c in un if c.opt.get("raises")] == [2056] and pixel_unshuffle2_nblk(2056) > 0
        assert {(c.shape["h"], c.shape["w"]) for c in un} == {(3, 5), (1, 1)}
        assert [pixel_unshuffle2_nblk(C) for C in (8, 64, 200, 2048)] == [1024, 1024, 1000, 1024]
        assert any(c.shape["B"] * c.shape["h"] * c.shape["w"] * (c.shape["C"] // 8) < 256 for c in un)       # most threads idle
        im = [c for c in _of("im2col") if c.dtype == dt]
        plain = [c for c in im if not c.opt["floor"]]
        assert {c.shape["P"] for c in plain} == {16, 8, 14} and {c.opt["prenorm"] for c in plain} == {0, 1}
        for c in plain:
            p = patch_im2col_plan(c.shape["H"], c.shape["W"], c.shape["P"])
            assert (p["gh"], p["gw"]) == (4, 6) and c.opt["wg"] == 2 and not p["cropped"]
            assert p["vec"] == (c.shape["P"] != 14) and p["pad"] == (4 if c.shape["P"] == 14 else 0)
        fl_ = [c for c in im if c.opt["floor"]]
        assert {(c.shape["H"], c.shape["W"], c.opt["prenorm"]) for c in fl_} == {(37, 53, 0), (37, 53, 1), (37, 52, 0), (37, 52, 1)}
        for c in fl_:
            p = patch_im2col_plan(c.shape["H"], c.shape["W"], c.shape["P"], floor=True)
            assert p["cropped"] and p["vec"] == (c.shape["W"] == 52) and (p["gh"], p["gw"]) == (4, 6)
    big = [c for c in _of("winperm") if c.shape["C"] > 72]
    assert len(big) == 1 and big[0].dtype == "bf16" and 33 << 20 > elements(big[0]) > 32 << 20
    assert grid_trips(elements(big[0]) // 8) == 2 and all(grid_trips(elements(c) // 8) == 1 for c in CASES if c is not big[0] and c.entry != "ac")


# ------------------------------------------------------------------------------------------------ 2. an honest fp32 implementation
def _interp(x, size, align):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=align)


def _rows_mask(mask, rows, HW):
    return 1.0 if mask is None else mask[torch.arange(rows) // HW]


class Honest:
    def rejects(self, c, inp):
        s = c.shape
        if c.entry == "cs_bwd":
            assert convseg_bwd_plan(s["rows"], s["C"], c.dtype)["error"]
        elif c.entry == "hgf":
            assert head_grad_fused_plan(s["rows"], s["C"], c.dtype, not c.opt.get("shift_dx"))["error"]
        else:
            assert c.entry == "unsh" and s["C"] > 2048

    def bil_fwd(self, c, x):
        return _interp(x.float().permute(0, 3, 1, 2), (c.shape["H"], c.shape["W"]), False).permute(0, 2, 3, 1).contiguous().to(x.dtype)

    def bil_bwd(self, c, dout):
        B, H, W, C = dout.shape
        x = torch.zeros(B, C, c.shape["h"], c.shape["w"], requires_grad=True)
        _interp(x, (H, W), False).backward(dout.float().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous().to(dout.dtype)

    def upsum(self, c, io0, zs):
        t = io0.float()
        for z in zs:
            t = t + _interp(z.float().permute(0, 3, 1, 2), io0.shape[1:3], False).permute(0, 2, 3, 1)
        return torch.relu(t).to(io0.dtype)

    def ac_fwd(self, c, x):
        return _interp(x[None], (c.shape["H"], c.shape["W"]), True)[0]

    def ac_bwd(self, c, dout):
        x = torch.zeros(1, dout.shape[0], c.shape["h"], c.shape["w"], requires_grad=True)
        _interp(x, dout.shape[1:], True).backward(dout[None])
        return x.grad[0]

    def cs_fwd(self, c, x, w, bias, mask):
        return (x.float() * w * _rows_mask(mask, x.shape[0], c.shape["HW"])).sum(1) + bias

    def cs_bwd(self, c, dout, x, w, mask, dx0, accum):
        xf, d, m = x.float(), dout[:, None], _rows_mask(mask, x.shape[0], c.shape["HW"])
        t = d * w * m
        if accum & 1:
            t = t + dx0.float()
        if accum & 2:
            t = torch.where(xf > 0, t, torch.zeros_like(t))
        return dict(dx=t.to(x.dtype), dw=(d * xf * m).sum(0), db=dout.sum().reshape(1))

    def hgf(self, c, dfn, y, inv, dout, x, w, mask):
        xf, d, m, g, yf = x.float(), dout[:, None], _rows_mask(mask, x.shape[0], c.shape["HW"]), dfn.float(), y.float()
        t = inv[:, None] * (g - yf * (g * yf).sum(1, keepdim=True)) + d * w * m
        return dict(dx=torch.where(xf > 0, t, torch.zeros_like(t)).to(x.dtype), dw=(d * xf * m).sum(0), db=dout.sum().reshape(1))

    def winperm(self, c, x, to_raster):
        B, g, wg, C = c.shape["B"], c.shape["g"], c.shape["wg"], x.shape[-1]
        idx = torch.arange(g * g)
        ty, tx = idx // g, idx % g
        tw = ((ty // wg) * (g // wg) + tx // wg) * wg * wg + (ty % wg) * wg + tx % wg
        y = torch.empty_like(x)
        if to_raster:
            y[:, idx] = x[:, tw]
        else:
            y[:, tw] = x[:, idx]
        return y

    def ps2(self, c, t, bias, inverse):
        B, h, w, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        if inverse:
            return F.pixel_unshuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(B * h * w, 4 * C)
        y = F.pixel_shuffle(t.view(B, h, w, 4 * C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        return (y.float() + bias).to(t.dtype) if bias is not None else y.contiguous()

    def s2d(self, c, t, inverse):
        B, g, C = c.shape["B"], c.shape["g"], c.shape["C"]
        h = g // 2
        if not inverse:
            return F.pixel_unshuffle(t[:, :2 * h, :2 * h].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(B * h * h, 4 * C)
        out = torch.zeros(B, g, g, C, dtype=t.dtype)
        out[:, :2 * h, :2 * h] = F.pixel_shuffle(t.view(B, h, h, 4 * C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        return out

    def unsh(self, c, src):
        B, h, w, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        dst = F.pixel_unshuffle(src.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(B * h * w, 4 * C)
        return dst, src.float().view(-1, C).sum(0).double()

    def im2col(self, c, img4, disks):
        P, wg = c.shape["P"], c.opt["wg"]
        B, _, H, W = img4.shape
        gh, gw = H // P, W // P
        mean, std = torch.tensor(sr.IM_MEAN).view(1, 3, 1, 1), torch.tensor(sr.IM_STD).view(1, 3, 1, 1)
        rgb = img4[:, :3] if c.opt["prenorm"] else (img4[:, :3] - mean) / std
        full = torch.cat([rgb, img4[:, 3:], disks], 1)[:, :, :gh * P, :gw * P]
        u = F.unfold(full, P, stride=P).transpose(1, 2).reshape(B, gh * gw, 2, 3 * P * P)
        u = F.pad(u, (0, (-3 * P * P) % 8)).reshape(B, gh // wg, wg, gw // wg, wg, -1).permute(0, 1, 3, 2, 4, 5)
        return u.reshape(B * gh * gw, -1).to(sr.tdtype(c.dtype))


_SEEN = set()


def _cpu_rows():
    rows = []
    for c in CASES:
        cc = cpu_case(c)
        if sr.case_id(cc) not in _SEEN:
            _SEEN.add(sr.case_id(cc))
            rows.append(cc)
    return rows


@pytest.mark.parametrize("case", _cpu_rows(), ids=sr.case_id)
def test_bounds_accept_honest_fp32(case):
    torch.manual_seed(0)
    sr.verify(case, Honest(), "cpu")


# ------------------------------------------------------------------------------------------------ 3. wrong float64 answers
def _fails(fam, wrong, true):
    return sr.any_fails(fam, dict(o=wrong.ref), dict(o=true), sr.COEF[fam])


def _rejects(case, perturb):
    """does the bound of ``case`` reject the reference perturbed by ``perturb`` (None: the perturbation does not apply to it)"""
    dt, e, o, s = case.dtype, case.entry, case.opt, case.shape
    if o.get("raises") or elements(case) > 1 << 18:
        return None
    inp = sr.inputs(case, "cpu")
    if perturb in ("align-swapped", "half-pixel-off", "no-clamp", "swap-axes", "untransposed"):
        if e not in ("bil_fwd", "bil_bwd", "ac") or (perturb == "swap-axes" and (e == "ac" or s["h"] == s["w"] or s["H"] == s["W"])):
            return None
        align = e == "ac"
        x, dout = (inp["x"][..., None], inp["dout"][..., None]) if e == "ac" else (inp["x"], inp["dout"])
        if perturb == "untransposed":
            if e == "bil_fwd":
                return None
            return _fails("rbwd", sr.resize_bwd_ref(dt, dout, s["h"], s["w"], align, perturb), sr.resize_bwd_ref(dt, dout, s["h"], s["w"], align))
        if e == "bil_bwd":
            return _fails("rbwd", sr.resize_bwd_ref(dt, dout, s["h"], s["w"], align, perturb), sr.resize_bwd_ref(dt, dout, s["h"], s["w"], align))
        return _fails("rfwd", sr.resize_fwd_ref(dt, x, s["H"], s["W"], align, perturb), sr.resize_fwd_ref(dt, x, s["H"], s["W"], align))
    if e == "upsum" and perturb in ("no-relu", "drop-map"):
        if perturb == "drop-map" and not o["maps"]:
            return None
        return _fails("rfwd", sr.upsum_ref(dt, inp["io0"], inp["zs"], perturb), sr.upsum_ref(dt, inp["io0"], inp["zs"]))
    if e == "cs_fwd" and perturb in ("mask-row-0", "no-bias"):
        if perturb == "mask-row-0" and (inp["mask"] is None or s["rows"] <= s["HW"]):
            return None
        a = (inp["x"], inp["w"], inp["bias"], inp["mask"], s["HW"])
        return sr.any_fails("head", {k: v.ref for k, v in sr.convseg_fwd_ref(*a, perturb).items()}, sr.convseg_fwd_ref(*a), sr.COEF["head"])
    if e in ("cs_bwd", "hgf") and perturb in ("mask-row-0", "x>=0", "accum0-ignored", "no-inv", "sum-without-y"):
        if perturb == "mask-row-0" and (inp["mask"] is None or s["rows"] <= s["HW"]):
            return None
        if e == "cs_bwd":
            if perturb in ("no-inv", "sum-without-y") or (perturb == "x>=0" and not o["accum"] & 2) or (perturb == "accum0-ignored" and not o["accum"] & 1):
                return None
            a = (dt, inp["dout"], inp["x"], inp["w"], inp["mask"], inp["dx0"], o["accum"], s["HW"])
            wrong, true = sr.convseg_bwd_ref(*a, perturb), sr.convseg_bwd_ref(*a)
        else:
            if perturb == "accum0-ignored":
                return None
            a = (dt, inp["dfn"], inp["y"], inp["inv"], inp["dout"], inp["x"], inp["w"], inp["mask"], s["HW"])
            wrong, true = sr.head_grad_fused_ref(*a, perturb), sr.head_grad_fused_ref(*a)
        return sr.any_fails("head", {k: v.ref for k, v in wrong.items()}, true, sr.COEF["head"])
    if e == "ps2" and perturb in ("no-bias", "dj-di"):
        if perturb == "no-bias" and inp["bias"] is None:
            return None
        a = (dt, inp["src"], inp["bias"], s["B"], s["h"], s["w"], s["C"])
        return _fails("lsum", sr.ps2_fwd_ref(*a, perturb), sr.ps2_fwd_ref(*a))
    if e == "winperm" and perturb == "ty-tx-swapped":
        return not all(torch.equal(sr.winperm_ref(inp["x"], s["g"], s["wg"], d, perturb), sr.winperm_ref(inp["x"], s["g"], s["wg"], d)) for d in (False, True))
    if e == "s2d" and perturb == "border-unwritten":
        return not torch.equal(sr.s2d_inv_ref(inp["s"], s["B"], s["g"], s["C"], perturb), sr.s2d_inv_ref(inp["s"], s["B"], s["g"], s["C"]))
    if e == "im2col" and perturb == "wrong-channel" and not o["prenorm"]:
        a = (dt, inp["img4"], inp["disks"], s["P"], o["wg"], o["prenorm"])
        return _fails("lsum", sr.im2col_ref(*a, perturb), sr.im2col_ref(*a))
    return None


PERTURBATIONS = [("bil_fwd", "align-swapped"), ("ac", "align-swapped"), ("bil_fwd", "half-pixel-off"), ("bil_bwd", "half-pixel-off"),
                 ("bil_fwd", "no-clamp"), ("bil_bwd", "no-clamp"), ("bil_fwd", "swap-axes"), ("bil_bwd", "swap-axes"),
                 ("bil_bwd", "untransposed"), ("ac", "untransposed"), ("upsum", "no-relu"), ("upsum", "drop-map"),
                 ("cs_fwd", "mask-row-0"), ("cs_bwd", "mask-row-0"), ("hgf", "mask-row-0"), ("cs_bwd", "x>=0"), ("hgf", "x>=0"),
                 ("cs_bwd", "accum0-ignored"), ("hgf", "no-inv"), ("hgf", "sum-without-y"), ("cs_fwd", "no-bias"), ("ps2", "no-bias"),
                 ("ps2", "dj-di"), ("winperm", "ty-tx-swapped"), ("s2d", "border-unwritten"), ("im2col", "wrong-channel")]


@pytest.mark.parametrize("entry,perturb", PERTURBATIONS)
def test_bounds_reject_wrong_float64_answers(entry, perturb):
    """every applicable row is tried until one rejects; the rows that apply are counted so that none of this is vacuous"""
    applied = 0
    for c in CASES:
        if c.entry != entry:
            continue
        r = _rejects(cpu_case(c), perturb)
        if r is None:
            continue
        applied += 1
        if r:
            return
    raise AssertionError(f"{perturb}: accepted by all {applied} rows of {entry} it applies to")
