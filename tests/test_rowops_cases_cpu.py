"""CPU checks of the row-kernel test table (tests/rowops_cases.py) and of the bounds (tests/rowops_ref.py):
1. the table reaches every branch and edge of the launchers' arithmetic;
2. the bounds accept an honest implementation -- the same operation in fp32 on the CPU (torch's functional where there is one,
   else the formula in fp32), rounded once to the row's dtype -- at the committed constants;
3. the bounds reject wrong float64 answers: each perturbed reference fails on at least one row of its kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowops_ref as rr
from rowops_cases import (CASES, DTYPES, LN_WIDTHS, cpu_case, colsum_f32_plan, colsum_plan, elements, gate_plan, gn_plan,
                          l2_plan, ln_bwd_plan, ln_fwd_plan)


def _of(entry, **kw):
    return [c for c in CASES if c.entry == entry and all(c.shape.get(k, c.opt.get(k)) == v for k, v in kw.items())]


# ------------------------------------------------------------------------------------------------ 1. coverage
def test_constants():
    for fam, v in rr.COEF.items():
        assert 0 < v <= rr.COEF_MAX and math.log2(v) == int(math.log2(v)), (fam, v)


def test_table_layernorm():
    ln = _of("ln")
    for dt in DTYPES:
        rows = [c for c in ln if c.dtype == dt]
        assert {c.shape["C"] for c in rows} == set(LN_WIDTHS)
        for nch in (1, 2, 4):
            plans = [(c, ln_fwd_plan(c.shape["rows"], c.shape["C"])) for c in rows]
            mine = [(c, p) for c, p in plans if p["NCH"] == nch]
            assert any(p["trips"] == 1 and c.shape["rows"] > 1 for c, p in mine)
            assert any(p["trips"] >= 2 and p["last_trip_partial"] for c, p in mine)
            assert any(p["trips"] == 3 for c, p in mine)
            assert any(c.shape["rows"] == 1 for c, p in mine)
            multi = [c for c, p in mine if p["trips"] >= 2]
            assert {c.shape["C"] for c in multi} == {{1: 8, 2: 520, 4: 1032}[nch]}       # the narrowest width of the class
        assert {ln_fwd_plan(1, C)["live_lanes_last_chunk"] for C in (8, 520, 1032)} == {1}       # one live lane in the last chunk
        pe = [c for c in rows if c.opt.get("pe_rows")]
        assert any(c.opt["pe_rows"] == 1 for c in pe) and any(c.opt["pe_rows"] == c.shape["rows"] for c in pe)
        assert any(c.opt["pe_rows"] > c.shape["rows"] for c in pe)
        assert any(1 < c.opt["pe_rows"] < c.shape["rows"] and c.shape["rows"] % c.opt["pe_rows"] for c in pe)
        assert {ln_fwd_plan(c.shape["rows"], c.shape["C"])["NCH"] for c in pe} == {1, 2, 4}
        assert any(ln_fwd_plan(c.shape["rows"], c.shape["C"])["trips"] >= 2 for c in pe)
        # backward
        bp = [(c, ln_bwd_plan(c.shape["rows"], c.shape["C"], dt, c.opt.get("dy2"))) for c in rows]
        assert {1, 15, 40} <= {c.shape["rows"] for c in rows}
        for nw in (4, 8):
            assert any(p["nblk"] == 512 and p["NW"] == nw for c, p in bp)
            assert any(p["nblk"] == 1 and p["NW"] == nw for c, p in bp)
        assert any(c.opt.get("dres") for c in rows) and any(not c.opt.get("dres") for c in rows)
        assert any(c.opt.get("dy2") and c.opt.get("dres") for c in rows) and any(c.opt.get("dy2") and not c.opt.get("dres") for c in rows)
        assert {p["PF"] for c, p in bp} == {True, False}
        if dt == "bf16":
            assert {p["RW"] for c, p in bp} == {1, 2}
            assert any(p["second_row_missing"] and p["trips"] == 1 for c, p in bp)
            assert any(p["second_row_missing"] and p["trips"] >= 2 and p["nblk"] == 512 for c, p in bp)
        else:
            assert {p["RW"] for c, p in bp} == {1}
        assert {"ord", "offset", "const", "zero", "wz"} <= {c.regime for c in rows}
    assert max(elements(c) for c in CASES) * 8 < 256 << 20          # the largest float64 intermediate


def test_table_l2norm():
    l2 = _of("l2")
    for dt in DTYPES:
        rows = [c for c in l2 if c.dtype == dt]
        for C in (64, 128, 256, 512):
            plans = [l2_plan(c.shape["rows"], C) for c in rows if c.shape["C"] == C and not c.opt.get("shift_bytes")]
            assert all(p["vec"] for p in plans) and plans[0]["rpw"] == 512 // C
            assert any(p["part_wave"] for p in plans) or C == 512
            assert any(p["second_pass"] for p in plans)
            assert any(c.shape["rows"] == 1 for c in rows if c.shape["C"] == C)
        assert {c.shape["C"] for c in rows if not l2_plan(c.shape["rows"], c.shape["C"])["vec"]} == {8, 40, 520}
        mis = [c for c in rows if c.opt.get("shift_bytes")]
        assert mis and all(c.shape["C"] == 256 and c.opt["shift_bytes"] == 16 for c in mis)
        assert not l2_plan(77, 256, aligned=False)["vec"]
        assert {"offset", "zero"} <= {c.regime for c in rows}
    big = [c for c in l2 if l2_plan(c.shape["rows"], c.shape["C"]).get("capped")]
    assert len(big) == 1 and big[0].dtype == "bf16" and 16 << 20 <= elements(big[0]) < 18 << 20
    p = l2_plan(big[0].shape["rows"], big[0].shape["C"])
    assert p["grid"] == 8192 and p["second_pass"] and l2_plan(big[0].shape["rows"] - 5, big[0].shape["C"])["capped"] is False


def test_table_colsum():
    for dt in DTYPES:
        rows = [c for c in _of("colsum") if c.dtype == dt]
        assert {c.shape["rows"] for c in rows} == {1, 64, 65, 1000}
        assert {c.shape["C"] for c in rows} == {8, 128, 136, 256, 264, 520}
        assert colsum_plan(64, 256)["small"] and not colsum_plan(65, 256)["small"]
        for CL in (4, 8, 16):
            plans = [colsum_plan(c.shape["rows"], c.shape["C"]) for c in rows]
            mine = [p for p in plans if not p["small"] and p["CL"] == CL]
            assert any(p["part_block"] for p in mine) and any(p["slab"] == 2 for p in mine) and any(p["slab"] == 16 for p in mine)
        assert any(c.opt["ld"] > c.shape["C"] for c in rows) and any(c.opt["ld"] == c.shape["C"] for c in rows)
        assert {c.opt["beta"] for c in rows} == {0.0, 1.0, 0.5}
        assert any(c.regime == "int" for c in rows)
    f32 = _of("colsum_f32")
    assert {c.shape["rows"] for c in f32} == {1, 8, 9, 16, 17, 25}
    assert all(colsum_f32_plan(c.shape["rows"], c.shape["C"])["part_block"] for c in f32)
    assert [colsum_f32_plan(r, 40)["pairs"] for r in (1, 8, 9, 16, 17, 25)] == [0, 0, 1, 8, 8, 9]
    assert [colsum_f32_plan(r, 40)["singles"] for r in (1, 8, 9, 16, 17, 25)] == [1, 8, 7, 0, 1, 7]
    assert {c.opt["beta"] for c in f32} == {0.0, 1.0, 0.5}


def test_table_groupnorm():
    for dt in DTYPES:
        rows = [c for c in _of("gn") if c.dtype == dt]
        assert {c.shape["C"] for c in rows} == {8, 192, 2048, 2064, 2560, 4096}
        assert {c.shape["HW"] for c in rows} == {1, 63, 64, 65, 196}
        assert all(c.shape["HW"] <= 65 for c in rows if c.shape["C"] >= 2048)
        assert {c.opt["gelu"] for c in rows} == {0, 1}
        plans = {c.shape["C"]: gn_plan(c.shape["HW"], c.shape["C"]) for c in rows}
        assert plans[2048]["nrep"] == 1 and plans[2064]["nrep"] == 2 and plans[4096]["nrep"] == 2
        assert plans[2048]["idle_threads"] == 0 and plans[2064]["idle_threads"] == 127 and plans[2560]["idle_threads"] == 96
        assert plans[8]["slots"] == 256 and plans[4096]["slots"] == 1
        assert {gn_plan(c.shape["HW"], c.shape["C"])["chunk"] for c in rows} == {1, 2, 4}
        assert {"ord", "offset", "const", "zero", "wz", "tails"} <= {c.regime for c in rows}
        ps = [c for c in _of("psgn") if c.dtype == dt]
        assert {c.opt["bias"] for c in ps} == {0, 1} and all(c.shape["HW"] == 4 * c.shape["h"] * c.shape["w"] for c in ps)
        assert any(c.shape["h"] * c.shape["w"] < 64 for c in ps) and any(c.shape["h"] * c.shape["w"] > 64 for c in ps)


def test_table_gates():
    for dt in DTYPES:
        rows = [c for c in _of("gate") if c.dtype == dt]
        for fused in (0, 1):
            mine = [c for c in rows if c.opt["fused"] == fused]
            assert {c.shape["nq"] for c in mine} == {1, 7, 48}
            assert {c.shape["N"] for c in mine} == {1, 63, 65, 196}
            assert {c.shape["C"] for c in mine} == {8, 520, 1280, 2048}
            assert any(c.shape["B"] * c.shape["C"] % 256 for c in mine)
            assert {c.opt["accum"] for c in mine} == {0, 1}
            assert any(c.regime == "ties" for c in mine)
            assert {gate_plan(c.shape["N"], c.shape["C"])["slice"] for c in mine} == {1, 2, 4}
        assert {c.opt["n"] for c in rows if c.opt["fused"]} == {1, 2, 3}
        assert {gate_plan(c.shape["N"], c.shape["C"])["nchk"] for c in rows if c.opt["fused"]} == {1, 2, 3, 4}
    # the planted maxima of the `ties` regime: twice in one 8-element chunk, in two lanes, in every column
    c = [c for c in _of("gate") if c.regime == "ties" and c.shape["C"] == 520][0]
    K = rr.inputs(c, "cpu")["Ks"][0].double()
    tied = (K == K.amax(2, keepdim=True))
    cols = [tied[0, r].nonzero().flatten().tolist() for r in range(4)]
    assert len(cols[0]) == 2 and cols[0][0] // 8 == cols[0][1] // 8
    assert len(cols[1]) == 3 and len({v // 8 for v in cols[1]}) == 3 and len({(v // 8) % 64 for v in cols[1]}) == 2    # two chunks of one lane too
    assert len(cols[2]) == 520 and len(cols[3]) == 1
    Q = rr.inputs(c, "cpu")["Qs"][0].double()
    tq = (Q == Q.amax(1, keepdim=True)).sum(1)[0]
    assert tq[0] == 2 and tq[1] == c.shape["nq"] and tq[2] == 1


def test_table_act_bwd():
    for dt in DTYPES:
        rows = [c for c in _of("act") if c.dtype == dt]
        assert {c.opt["kind"] for c in rows} == {0, 1}
        for kind in (0, 1):
            assert any(all(ld != c.shape["cols"] for ld in c.opt["ld"]) for c in rows if c.opt["kind"] == kind)
        assert any(c.regime == "tails" for c in rows)


# ------------------------------------------------------------------------------------------------ 2. an honest fp32 implementation
class Honest:
    def ln_fwd(self, c, x, w, b, eps, pe):
        xf = x.float()
        y = F.layer_norm(xf, (xf.shape[1],), w, b, eps).to(x.dtype)
        out = dict(y=y, mean=xf.mean(1), rstd=(xf.var(1, unbiased=False) + eps).rsqrt())
        if pe is not None:
            out["y2"] = (y.float() + pe.float()[torch.arange(xf.shape[0]) % pe.shape[0]]).to(x.dtype)
        return out

    def ln_bwd(self, c, dy, dy2, x, w, mean, rstd, dres):
        xf, wf = x.float().requires_grad_(True), w.clone().requires_grad_(True)
        bf = torch.zeros_like(w).requires_grad_(True)
        d = dy.float() + (dy2.float() if dy2 is not None else 0.0)
        F.layer_norm(xf, (xf.shape[1],), wf, bf, rr.LN_EPS).backward(d)
        dx = xf.grad + (dres.float() if dres is not None else 0.0)
        return dict(dx=dx.to(x.dtype), dw=wf.grad, db=bf.grad)

    def l2_fwd(self, c, x):
        xf = x.float()
        inv = 1.0 / xf.norm(dim=1).clamp_min(1e-12)
        return dict(y=(xf * inv[:, None]).to(x.dtype), inv=inv)

    def l2_bwd(self, c, dy, y, inv):
        d, yf = dy.float(), y.float()
        return dict(dx=(inv[:, None] * (d - yf * (d * yf).sum(1, keepdim=True))).to(dy.dtype))

    def colsum(self, c, x, out0, beta):
        return dict(out=(beta * out0 if beta != 0.0 else 0.0) + x.float().sum(0))

    def _gn(self, xf, w, b, eps, gelu):
        t = F.group_norm(xf.transpose(1, 2), 1, w, b, eps).transpose(1, 2)
        return F.gelu(t) if gelu else t

    def gn_fwd(self, c, x, w, b, eps, gelu):
        xf = x.float()
        return dict(y=self._gn(xf, w, b, eps, gelu).to(x.dtype), mean=xf.mean((1, 2)),
                    rstd=(xf.var((1, 2), unbiased=False) + eps).rsqrt())

    def gn_bwd(self, c, dy, x, w, b, mean, rstd, gelu):
        xf, wf, bf = x.float().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        self._gn(xf, wf, bf, rr.GN_EPS, gelu).backward(dy.float())
        return dict(dx=xf.grad.to(x.dtype), dw=wf.grad, db=bf.grad)

    def psgn(self, c, src, bias, w, b, eps, gelu):
        B, h, wd, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        y1 = src.float().view(B, h, wd, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 4 * h * wd, C)
        y1 = (y1 + (bias if bias is not None else 0.0)).to(src.dtype)
        return dict(y1=y1, **self.gn_fwd(c, y1, w, b, eps, gelu))

    def gate_fwd(self, c, Qs, Ks, x):
        cg = torch.stack([torch.sigmoid(Q.float().amax(1)) for Q in Qs])
        sg = torch.stack([torch.sigmoid(K.float().amax(2)) for K in Ks])
        argq = torch.stack([rr.lowest_argmax(Q.float(), 1) for Q in Qs]).int()
        argc = torch.stack([rr.lowest_argmax(K.float(), 2) for K in Ks]).int()
        outs = [(x.float() * (1.0 + cg[i][:, None, :] + sg[i][:, :, None])).to(x.dtype) for i in range(len(Qs))]
        return dict(cg=cg, sg=sg, argq=argq, argc=argc, outs=outs)

    def gate_bwd(self, c, douts, x, cg, argq, sg, argc, dx0, accum, dQ0s, dK0s):
        xf = x.float()
        dx = dx0.float().clone() if accum else torch.zeros_like(xf)
        out = {}
        for i, dout in enumerate(douts):
            d = dout.float()
            dx = dx + d * (1.0 + cg[i][:, None, :] + sg[i][:, :, None])
            T = d * xf
            dK, dQ = dK0s[i].float().clone(), dQ0s[i].float().clone()
            dK.scatter_add_(2, argc[i].long()[:, :, None], (T.sum(2) * sg[i] * (1 - sg[i]))[:, :, None])
            dQ.scatter_add_(1, argq[i].long()[:, None, :], (T.sum(1) * cg[i] * (1 - cg[i]))[:, None, :])
            out[f"dK{i}"], out[f"dQ{i}"] = dK.to(x.dtype), dQ.to(x.dtype)
        out["dx"] = dx.to(x.dtype)
        return out

    def act_bwd(self, c, dy, aux, kind):
        d, a = dy.float(), aux.float()
        if kind == 0:
            return dict(dz=(d * (a > 0)).to(dy.dtype))
        dg = 0.5 * (1.0 + torch.erf(a * math.sqrt(0.5))) + a * torch.exp(-0.5 * a * a) * (1.0 / math.sqrt(2.0 * math.pi))
        return dict(dz=(d * dg).to(dy.dtype))


_SEEN = set()


def _cpu_rows():
    rows = []
    for c in CASES:
        cc = cpu_case(c)
        if rr.case_id(cc) not in _SEEN:
            _SEEN.add(rr.case_id(cc))
            rows.append(cc)
    return rows


@pytest.mark.parametrize("case", _cpu_rows(), ids=rr.case_id)
def test_bounds_accept_honest_fp32(case):
    torch.manual_seed(0)
    rr.verify(case, Honest(), "cpu")


# ------------------------------------------------------------------------------------------------ 3. wrong float64 answers
def _refs(o):
    return {k: v.ref for k, v in o.items()}


def _rejects(case, perturb):
    """does the bound of ``case`` reject the reference perturbed by ``perturb`` (None: the perturbation does not apply to it)"""
    dt, e, o = case.dtype, case.entry, case.opt
    if elements(case) > 1 << 18:
        return None
    inp = rr.inputs(case, "cpu")
    if e == "ln":
        if perturb in ("cols-8", "var/(C-1)", "noeps", "pe+1", "y2-unrounded"):
            if (perturb == "cols-8" and case.shape["C"] == 8) or (perturb == "noeps" and case.regime != "const"):
                return None
            if perturb in ("pe+1", "y2-unrounded") and (inp["pe"] is None or (perturb == "y2-unrounded" and dt != "bf16")):
                return None
            a = (dt, inp["x"], inp["w"], inp["b"], rr.LN_EPS, inp["pe"])
            return rr.any_fails("ln", _refs(rr.ln_fwd_ref(*a, perturb=perturb)), rr.ln_fwd_ref(*a))
        if perturb in ("dw-last-row", "no-xhat-term", "dres-twice"):
            if perturb == "dres-twice" and inp["dres"] is None:
                return None
            a = (dt, inp["dy"], inp["dy2"], inp["x"], inp["w"], inp["dres"], rr.LN_EPS)
            return rr.any_fails("ln", _refs(rr.ln_bwd_ref(*a, perturb=perturb)), rr.ln_bwd_ref(*a))
    if e == "l2" and perturb == "inv-neighbour" and case.shape["rows"] > 1:
        fw = rr.l2_fwd_ref(dt, inp["x"])
        y, inv = rr.fl(fw["y"].ref, dt), fw["inv"].ref.float()
        return rr.any_fails("l2", _refs(rr.l2_bwd_ref(dt, inp["dy"], y, inv, perturb)), rr.l2_bwd_ref(dt, inp["dy"], y, inv))
    if e == "gn":
        a = (inp["x"], inp["w"], inp["b"], rr.GN_EPS, o["gelu"])
        if perturb == "HW-1" and case.shape["HW"] > 1:
            return rr.any_fails("gn", _refs(rr.gn_fwd_ref(dt, *a, perturb=perturb)), rr.gn_fwd_ref(dt, *a))
        if perturb == "tanh-gelu" and dt == "f32" and o["gelu"]:
            fw = rr.any_fails("gn", _refs(rr.gn_fwd_ref(dt, *a, perturb=perturb)), rr.gn_fwd_ref(dt, *a))
            bw = rr.any_fails("gn", _refs(rr.gn_bwd_ref(dt, inp["dy"], *a, perturb=perturb)), rr.gn_bwd_ref(dt, inp["dy"], *a))
            return fw and bw
        if perturb == "no-xhat-term":
            return rr.any_fails("gn", _refs(rr.gn_bwd_ref(dt, inp["dy"], *a, perturb=perturb)), rr.gn_bwd_ref(dt, inp["dy"], *a))
    if e == "act" and perturb == "tanh-gelu" and dt == "f32" and o["kind"] == 1:
        return rr.any_fails("act", _refs(rr.act_bwd_ref(dt, inp["dy"], inp["aux"], 1, perturb)), rr.act_bwd_ref(dt, inp["dy"], inp["aux"], 1))
    if e == "gate" and perturb in ("argmax-last", "no-sg"):
        st = [rr.gate_stats_ref(Q, K) for Q, K in zip(inp["Qs"], inp["Ks"])]
        cg, sg = torch.stack([s[0]["cg"].ref.float() for s in st]), torch.stack([s[0]["sg"].ref.float() for s in st])
        if perturb == "no-sg":
            return rr.any_fails("gate", _refs(rr.gate_apply_ref(dt, inp["x"], cg[0], sg[0], perturb)), rr.gate_apply_ref(dt, inp["x"], cg[0], sg[0]))
        if case.regime != "ties":
            return None
        bad = [rr.gate_stats_ref(Q, K, perturb) for Q, K in zip(inp["Qs"], inp["Ks"])]
        b = lambda stats: (torch.stack([s[1] for s in stats]), torch.stack([s[2] for s in stats]))
        (aq, ac), (aqb, acb) = b(st), b(bad)
        rest = (inp["dx0"], o["accum"], inp["dQ0s"], inp["dK0s"])
        true, _ = rr.gate_bwd_ref(dt, inp["douts"], inp["x"], cg, aq, sg, ac, *rest)
        wrong, _ = rr.gate_bwd_ref(dt, inp["douts"], inp["x"], cg, aqb, sg, acb, *rest)
        return rr.any_fails("gate", _refs(wrong), true)
    if e in ("colsum", "colsum_f32") and perturb == "last-row":
        return rr.any_fails("colsum", _refs(rr.colsum_ref(inp["x"], inp["out0"], o["beta"], perturb)), rr.colsum_ref(inp["x"], inp["out0"], o["beta"]))
    return None


PERTURBATIONS = [("ln", "cols-8"), ("ln", "var/(C-1)"), ("ln", "noeps"), ("ln", "pe+1"), ("ln", "y2-unrounded"), ("ln", "dw-last-row"),
                 ("ln", "no-xhat-term"), ("ln", "dres-twice"), ("l2", "inv-neighbour"), ("gn", "HW-1"), ("gn", "tanh-gelu"),
                 ("gn", "no-xhat-term"), ("act", "tanh-gelu"), ("gate", "argmax-last"), ("gate", "no-sg"), ("colsum", "last-row"),
                 ("colsum_f32", "last-row")]


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
