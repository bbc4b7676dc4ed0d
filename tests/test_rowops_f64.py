"""The row and normalisation kernels against float64, per element, at the launchers' edges: LayerNorm (forward, PE form, backward
with one or two output gradients), L2 normalise, the column sums, GroupNorm(1, C) +- GELU (and vpu_groupnorm_apply on the
statistics of vpu_pixel_shuffle2_gn_stats), the DMA gates (single and the fused n-gate launches) and vpu_act_bwd.

The module walks tests/rowops_cases.py (tests/test_rowops_cases_cpu.py checks that the table reaches every launcher branch).  Per
row: inputs drawn on the GPU from a seeded generator, the launch through pvpuformer_amd.ops, the float64 reference on the GPU and
the bounds of tests/rowops_ref.py (|got - ref| <= REL |ref| + atol + c A; the module docstring there lists A per output).  Exact,
bit for bit: integer-valued column sums, the gates' arg-max indices (lowest index among equal maxima), the entries of dQ / dK away
from the arg-max, y = b on constant rows of the fp32 LayerNorm, relu backward.

Memory: every operand is a slice of a larger buffer with guard rows before and after (and gap columns where the entry point takes a
leading dimension), filled with a finite sentinel pattern that must come out bit-identical -- for inputs the whole buffer; outputs
are pre-filled with NaN, and none may survive.

c per kernel family (rowops_ref.COEF) is the next power of two at or above 4 x the worst value this module measured on one MI355X;
the module prints the worst value per (kernel, output) when it ends.  Measured worst c, and the constant it gives:
  LayerNorm   forward y 2.5e-7 (PE form; 2.3e-7 plain), y2 6.0e-8, mean 1.8e-7, rstd 7.4e-8;
              backward dx 1.5e-7, dw 1.4e-7, db 1.0e-7 (two gradients: 5.8e-8 / 3.6e-8 / 3.9e-8)            -> 2^-19 (1.9e-6)
  GroupNorm   forward y 1.5e-7, mean 4.9e-8, rstd 4.7e-8; apply on the fused statistics y 1.6e-7, rstd 5.2e-8;
              pixel_shuffle2_gn_stats map 6.0e-8; backward dx 1.5e-7, dw 1.1e-7, db 6.7e-8                   -> 2^-20 (9.5e-7)
  l2norm      y 1.8e-7, inv 1.5e-7, dx 1.1e-7                                                                -> 2^-20
  colsum      typed 1.7e-7, colsum_f32 1.2e-7                                                                -> 2^-20
  gates       cg 1.1e-7, sg 8.5e-8, out 1.4e-7, dx 1.8e-7, dQ 1.9e-7, dK 1.6e-7 (single and fused alike)     -> 2^-20
  act_bwd     gelu 1.7e-7, relu 0                                                                            -> 2^-20
Every value is a few fp32 roundings (2^-24 = 6.0e-8) of the result; none comes near the 2^-17 an fp32 path may not exceed."""
import pytest
import torch

import rowops_ref as rr
from rowops_cases import CASES, ln_bwd_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if rr.STATS:
        print("\n" + rr.summary())


class Kernels:
    """the kernels behind the interface rowops_ref.verify walks; every operand lives in a rowops_ref.Guarded buffer"""

    device = "cuda"

    def __init__(self, ops, tag):
        self.ops, self.tag, self.bufs = ops, tag, []

    def _in(self, t, name, ld=None, shift=0):
        t2 = t.reshape(-1, t.shape[-1])
        g = rr.Guarded(t2.shape[0], t2.shape[1], t.dtype, self.device, ld=ld, shift=shift, data=t2, name=name)
        self.bufs.append(g)
        return g.t

    def _out(self, rows, cols, dtype, name, ld=None, shift=0, init=None):
        g = rr.Guarded(rows, cols, dtype, self.device, ld=ld, shift=shift, name=name)
        if init is not None:                      # read-modify-write operand: starts from `init`, must end without a NaN
            g.t.copy_(init.reshape(rows, cols))
        self.bufs.append(g)
        return g.t

    def _done(self):
        if self.device == "cuda":
            torch.cuda.synchronize()
        for g in self.bufs:
            g.check(self.tag)
        self.bufs = []

    # ---- LayerNorm
    def ln_fwd(self, c, x, w, b, eps, pe):
        rows, C = x.shape
        X, W, Bv = self._in(x, "x"), self._in(w, "w"), self._in(b, "b")
        Y = self._out(rows, C, x.dtype, "y")
        M, R = self._out(1, rows, torch.float32, "mean"), self._out(1, rows, torch.float32, "rstd")
        out = dict(y=Y, mean=M[0], rstd=R[0])
        if pe is None:
            self.ops.layernorm_fwd(X, W, Bv, Y, M, R, rows, C, eps)
        else:
            P = self._in(pe, "pe")
            out["y2"] = self._out(rows, C, x.dtype, "y2")
            self.ops.layernorm_fwd_pe(X, W, Bv, Y, M, R, rows, C, eps, P, pe.shape[0], out["y2"])
        self._done()
        return out

    def ln_bwd(self, c, dy, dy2, x, w, mean, rstd, dres):
        rows, C = x.shape
        nblk = self.ops.layernorm_bwd_nblk(rows)
        assert nblk == ln_bwd_plan(rows, C, c.dtype, dy2 is not None)["nblk"]
        D, X, W = self._in(dy, "dy"), self._in(x, "x"), self._in(w, "w")
        M, R = self._in(mean, "mean"), self._in(rstd, "rstd")
        D2 = self._in(dy2, "dy2") if dy2 is not None else None
        Rs = self._in(dres, "dres") if dres is not None else None
        dx = self._out(rows, C, x.dtype, "dx")
        part = self._out(nblk * 2, C, torch.float32, "part")
        self.ops.layernorm_bwd(D, X, W, M, R, Rs, dx, part, rows, C, dy2=D2)
        self._done()
        p = part.view(nblk, 2, C).double().sum(0)
        return dict(dx=dx, dw=p[0], db=p[1])

    # ---- L2 normalise
    def l2_fwd(self, c, x):
        rows, C = x.shape
        sh = c.opt.get("shift_bytes", 0) // x.element_size()
        X = self._in(x, "x", shift=sh)
        Y, I = self._out(rows, C, x.dtype, "y", shift=sh), self._out(1, rows, torch.float32, "inv")
        self.ops.l2norm_fwd(X, Y, I, rows, C)
        self._done()
        return dict(y=Y, inv=I[0])

    def l2_bwd(self, c, dy, y, inv):
        rows, C = y.shape
        sh = c.opt.get("shift_bytes", 0) // y.element_size()
        D, Y, I = self._in(dy, "dy", shift=sh), self._in(y, "y", shift=sh), self._in(inv, "inv")
        dx = self._out(rows, C, y.dtype, "dx", shift=sh)
        self.ops.l2norm_bwd(D, Y, I, dx, rows, C)
        self._done()
        return dict(dx=dx)

    # ---- column sums
    def colsum(self, c, x, out0, beta):
        rows, C = x.shape
        out = self._out(1, C, torch.float32, "out", init=out0 if beta != 0.0 else None)
        if c.entry == "colsum_f32":
            self.ops.colsum_f32(self._in(x, "in"), out, rows, C, beta)
        else:
            X = self._in(x, "in", ld=c.opt["ld"])
            part = self._out(64, C, torch.float32, "part") if rows > 64 else None
            self.ops.colsum(X, c.opt["ld"], out, part, rows, C, beta)
        self._done()
        return dict(out=out[0])

    # ---- GroupNorm(1, C)
    def gn_fwd(self, c, x, w, b, eps, gelu):
        B, HW, C = x.shape
        nch = self.ops.groupnorm_nchunk()
        X, W, Bv = self._in(x, "x"), self._in(w, "w"), self._in(b, "b")
        Y = self._out(B * HW, C, x.dtype, "y")
        M, R = self._out(1, B, torch.float32, "mean"), self._out(1, B, torch.float32, "rstd")
        st = self._out(B * nch, 2, torch.float64, "stats")
        self.ops.groupnorm_fwd(X, W, Bv, Y, M, R, st, B, HW, C, eps, gelu)
        self._done()
        return dict(y=Y.view(B, HW, C), mean=M[0], rstd=R[0])

    def gn_bwd(self, c, dy, x, w, b, mean, rstd, gelu):
        B, HW, C = x.shape
        nch = self.ops.groupnorm_nchunk()
        D, X, W, Bv = self._in(dy, "dy"), self._in(x, "x"), self._in(w, "w"), self._in(b, "b")
        M, R = self._in(mean, "mean"), self._in(rstd, "rstd")
        dx = self._out(B * HW, C, x.dtype, "dx")
        part = self._out(B * nch * 2, C, torch.float32, "part")
        st = self._out(B * nch, 2, torch.float64, "stats")
        self.ops.groupnorm_bwd(D, X, W, Bv, M, R, dx, part, st, B, HW, C, gelu)
        self._done()
        p = part.view(B * nch, 2, C).double().sum(0)
        return dict(dx=dx.view(B, HW, C), dw=p[0], db=p[1])

    def psgn(self, c, src, bias, w, b, eps, gelu):
        B, h, wd, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        HW = 4 * h * wd
        nch = self.ops.groupnorm_nchunk()
        S = self._in(src, "src")
        Bi = self._in(bias, "bias") if bias is not None else None
        y1 = self._out(B * HW, C, src.dtype, "y1")
        st = self._out(B * nch, 2, torch.float64, "stats")
        self.ops.pixel_shuffle2_gn_stats(S, y1, Bi, st, B, h, wd, C)
        self._done()
        Y1, St, W, Bv = self._in(y1, "y1"), self._in(st, "stats"), self._in(w, "w"), self._in(b, "b")
        Y = self._out(B * HW, C, src.dtype, "y")
        M, R = self._out(1, B, torch.float32, "mean"), self._out(1, B, torch.float32, "rstd")
        self.ops.groupnorm_apply(Y1, W, Bv, Y, M, R, St, B, HW, C, eps, gelu)
        self._done()
        return dict(y1=y1.view(B, HW, C), y=Y.view(B, HW, C), mean=M[0], rstd=R[0])

    # ---- gates
    def gate_fwd(self, c, Qs, Ks, x):
        n, (B, N, C), nq = len(Qs), x.shape, Qs[0].shape[1]
        Qg, Kg = [self._in(t, "Q") for t in Qs], [self._in(t, "K") for t in Ks]
        X = self._in(x, "x")
        cg, sg = self._out(n * B, C, torch.float32, "cg"), self._out(n * B, N, torch.float32, "sg")
        aq, ac = self._out(n * B, C, torch.int32, "argq"), self._out(n * B, N, torch.int32, "argc")
        outs = [self._out(B * N, C, x.dtype, "out") for _ in range(n)]
        if c.opt["fused"]:
            self.ops.gate_fwd_n(Qg, Kg, X, outs, cg, aq, sg, ac, B, nq, N, C)
        else:
            assert n == 1
            self.ops.gate_stats(Qg[0], Kg[0], cg, aq, sg, ac, B, nq, N, C)
            self.ops.gate_apply(X, cg, sg, outs[0], B, N, C)
        self._done()
        return dict(cg=cg.view(n, B, C), sg=sg.view(n, B, N), argq=aq.view(n, B, C), argc=ac.view(n, B, N),
                    outs=[o.view(B, N, C) for o in outs])

    def gate_bwd(self, c, douts, x, cg, argq, sg, argc, dx0, accum, dQ0s, dK0s):
        n, (B, N, C), nq = len(douts), x.shape, dQ0s[0].shape[1]
        Dg = [self._in(t, "dout") for t in douts]
        X, G, S = self._in(x, "x"), self._in(cg, "cg"), self._in(sg, "sg")
        AQ, AC = self._in(argq, "argq"), self._in(argc, "argc")
        dx = self._out(B * N, C, x.dtype, "dx", init=dx0 if accum else None)
        dQ = [self._out(B * nq, C, x.dtype, "dQ", init=t) for t in dQ0s]
        dK = [self._out(B * N, C, x.dtype, "dK", init=t) for t in dK0s]
        part = self._out(n * B * 64, C, torch.float32, "part")
        if c.opt["fused"]:
            self.ops.gate_bwd_n(Dg, X, G, AQ, S, AC, dx, accum, dQ, dK, part, B, nq, N, C)
        else:
            self.ops.gate_bwd(Dg[0], X, G, AQ, S, AC, dx, accum, dQ[0], dK[0], part, B, nq, N, C)
        self._done()
        out = dict(dx=dx.view(B, N, C))
        for i in range(n):
            out[f"dQ{i}"], out[f"dK{i}"] = dQ[i].view(B, nq, C), dK[i].view(B, N, C)
        return out

    # ---- act_bwd
    def act_bwd(self, c, dy, aux, kind):
        rows, cols = dy.shape
        l0, l1, l2 = c.opt["ld"]
        D, Av = self._in(dy, "dy", ld=l0), self._in(aux, "aux", ld=l1)
        dz = self._out(rows, cols, dy.dtype, "dz", ld=l2)
        self.ops.act_bwd(D, l0, Av, l1, dz, l2, rows, cols, kind, self.ops.code_of(dy))
        self._done()
        return dict(dz=dz)


@pytest.mark.parametrize("case", CASES, ids=rr.case_id)
def test_row(ops, case):
    rr.verify(case, Kernels(ops, rr.case_id(case)), Kernels.device)
