"""Every GEMM family and epilogue of vpu_gemm / vpu_gemm_grouped against float64, per element, at the edges of the dispatch: the
fp32 kernel, the 128 x 128 bf16 kernel (run-time and compile-time epilogues), K3S, split-K (the three reduce forms and the
in-launch combine, the weight-gradient form with column sums), the skinny kernels, K2 (256 x 128 and 256 x 256 tiles, heights 5 to
8), K5, and the grouped forms (skinny, K2 compile-time and run-time, K4P with classic and distributed column sums, general).

The module walks tests/gemm_cases.py (tests/test_gemm_cases_cpu.py checks that the table reaches every product instantiation).
Per row: inputs drawn on the GPU from a seeded generator; every operand, inputs included, in a rowops_ref.Guarded buffer (guard
rows before and after, gap columns up to the leading dimension; sentinels must come back bit-identical, outputs are pre-filled
with NaN and none may survive -- C, preact, colsum and the slab of distributed column sums all count as outputs); the launch through
pvpuformer_amd.ops; vpu_gemm_last_kernel() equal to the restated dispatch at this device's CU count, and of the family the row was
written for; the float64 reference on the GPU and the bounds of tests/gemm_ref.py.  Exact, bit for bit: the `sign` rows, and the
outputs of one descriptor under splitk_inlaunch 0 and 1.

c per family (gemm_ref.COEF) is the next power of two at or above 4 x the worst value this module measured on one MI355X; the
module prints the worst value per (kernel, output) when it ends.  Measured worst c, and the constant it gives:
  fp32 kernel            C 1.88e-6 (K = 1000, all-positive operands: one fp32 sum of 1000 terms; 4 x = 7.52e-6), preact 2.33e-7
                                                                                                                      -> 2^-17 (7.63e-6)
  128 x 128 kernel       C 1.34e-6 (K = 4096 un-split into an fp32 C, all-positive operands; 4 x = 5.36e-6), colsum 4.55e-8; its
                         bf16 outputs 0 to 1e-8 (the rounding of the result covers them)                              -> 2^-17
  split-K                C 3.31e-7 (ten slices of 448 and 16 of 256 into an fp32 C; the reduce forms and the in-launch combine
                         alike), colsum 4.59e-8                                                                       -> 2^-19 (1.91e-6)
  skinny                 C 6.28e-8, preact 3.87e-10                                                                   -> 2^-21 (4.77e-7)
  K3S                    C 1.39e-9, preact 0 (bf16 outputs only)                                                      -> 2^-27 (7.45e-9)
  K2                     C 2.60e-8, preact 6.19e-9                                                                    -> 2^-23 (1.19e-7)
  K5                     C 2.63e-8, preact 1.44e-8                                                                    -> 2^-23
  grouped                skinny grouped C 3.63e-7 (fp32 C, K = 4096), general C 1.54e-7, colsum 1.53e-8, K2 grouped C 2.45e-8,
                         preact 2.90e-9, its compile-time form C 1.43e-8                                              -> 2^-19
  K4P                    C 1.69e-6 (K = 4096, all-positive operands, one tile walks the whole K; 4 x = 6.76e-6), colsum 1.64e-8
                                                                                                                      -> 2^-17
The three families at 2^-17 are the ones whose table holds an fp32 output over an un-split K >= 1000 of all-positive operands:
sequential fp32 accumulation needs about 1e-6 Amp there (gemm_ref's docstring), so 4 x the measurement lands on the ceiling and not
above it.  A bf16 output needs almost none of c: REL |ref| covers the one rounding of the result.

Rows splitk-inlaunch-key2 and splitk-inlaunch-key2-colsum pin a dispatch rule: a split-K problem with transA = 1 / transB = 0 has no
slab form, so under splitk_inlaunch it runs the run-time kernel AND the reduce launch (vpu_gemm used to skip the reduce there, and C
was never written)."""
import pytest
import torch

import gemm_cases as gc
import gemm_ref as gr
from gemm_cases import CASES, BIAS, PREACT, RESID, SAVE_DGELU, AUXF

pytestmark = pytest.mark.gpu

RESTORE = dict(k2=-1, k3=-1, k5=-1, k5_grid=0, k5_split=-1, skinny=-1, skinny_group=-1, splitk_inlaunch=-1)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def workspace(ops):
    return torch.zeros(gc.WS_BYTES // 4, device="cuda", dtype=torch.float32)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if gr.STATS:
        print("\n" + gr.gemm_summary())


class Launcher:
    """one vpu_gemm / vpu_gemm_grouped call with every operand in a sentinel buffer"""

    def __init__(self, ops, workspace, tag):
        self.ops, self.ws, self.tag, self.bufs = ops, workspace, tag, []

    def _in(self, t, name, ld=None):
        g = gr.Guarded(t.shape[0], t.shape[1], t.dtype, "cuda", ld=ld, data=t, name=name)
        self.bufs.append(g)
        return g.t

    def _out(self, rows, cols, dtype, name, ld=None, shift=0, init=None):
        g = gr.Guarded(rows, cols, dtype, "cuda", ld=ld, shift=shift, name=name)
        if init is not None:
            g.t.copy_(init.reshape(rows, cols))
        self.bufs.append(g)
        return g.t

    def problem(self, p, t):
        """-> (args, kwargs) of ops.gemm and the output views"""
        M, N, K, Z, f = p["M"], p["N"], p["K"], p["batch"], p["flags"]
        td, od = gr.tdt(p["dtype"]), gr.out_dtype(p)
        A = t["A"].transpose(1, 2).reshape(Z * K, M) if p["tA"] else t["A"].reshape(Z * M, K)
        B = t["B"].reshape(Z * K, N) if p["tB"] else t["B"].transpose(1, 2).reshape(Z * N, K)
        Ad, Bd = self._in(A.contiguous(), "A", p["lda"]), self._in(B.contiguous(), "B", p["ldb"])
        Cd = self._out(Z * M, N, od, "C", p["ldc"], p["shift_c"], t.get("C0"))
        outs = dict(C=Cd)
        kw = dict(transA=p["tA"], transB=p["tB"], flags=f, alpha=p["alpha"], post_mul=p["post_mul"], post_add=p["post_add"],
                  batch=Z, inner=p["inner"], sA=p["sA"], sB=p["sB"], sC=p["sC"], sR=p["sR"], resid_period=p["period"],
                  workspace=self.ws if p["ws"] else None)
        if f & BIAS:
            kw["bias"] = self._in(t["bias"][None], "bias", gc.up(N, 8))
        if f & RESID:
            r = t["resid"]
            kw["resid"], kw["ldr"] = self._in(r.reshape(-1, N), "resid", p["ldr"]), p["ldr"]
        if f & AUXF:
            kw["aux"], kw["ldaux"] = self._in(t["aux"].reshape(Z * M, N), "aux", p["ldaux"]), p["ldaux"]
        if f & (PREACT | SAVE_DGELU):
            outs["preact"] = kw["preact"] = self._out(Z * M, N, td, "preact", p["ldc"])
        if p["colsum"]:
            if p["cs_tn"] > 1:
                rows = gr.dcs_rows(p)
                first = rows[0][0] * p["cs_tn"] + rows[0][1]
                assert [z * p["cs_tn"] + gt for z, gt, _, _ in rows] == list(range(first, first + len(rows)))
                slab = self._out(len(rows), M, torch.float32, "colsum slab", gc.up(M, 8))
                outs["colsum"] = slab
                kw.update(colsum=(slab, -first * gc.up(M, 8)), cs_tn=p["cs_tn"], cs_t0=p["cs_t0"], cs_ld=gc.up(M, 8))
            else:
                cs = self._out(1, Z * M, torch.float32, "colsum", gc.up(Z * M, 8), init=t["colsum0"])
                outs["colsum"] = cs
                kw["colsum"] = cs
        code = 0 if p["dtype"] == "bf16" else 1
        return ((Ad, Bd, Cd, M, N, K, p["lda"], p["ldb"], p["ldc"], code), kw), outs

    def run(self, case, pts):
        calls = [self.problem(p, t) for p, t in pts]
        if case.entry == "gemm":
            (args, kw), _ = calls[0]
            self.ops.gemm(*args, **kw)
        else:
            self.ops.gemm_grouped([c[0] for c in calls])
        torch.cuda.synchronize()
        for g in self.bufs:
            g.check(self.tag)
        self.bufs = []
        res = []
        for (p, t), (_, outs) in zip(pts, calls):
            Z, M, N = p["batch"], p["M"], p["N"]
            d = dict(C=outs["C"].reshape(Z, M, N))
            if "preact" in outs:
                d["preact"] = outs["preact"].reshape(Z, M, N)
            if "colsum" in outs:
                d["colsum"] = outs["colsum"].clone() if p["cs_tn"] > 1 else outs["colsum"].reshape(-1).clone()
            res.append(d)
        return res


def _set(ops, opts):
    for k, v in opts.items():
        ops.gemm_set_option(k, v)


@pytest.mark.parametrize("case", [c for c in CASES if c.gpu], ids=lambda c: c.name)
def test_gemm_f64(ops, workspace, case):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    pl = gc.plan(case, ncu)
    assert not pl.err and pl.family == case.family, \
        f"{case.name}: written for the {case.family} family, but at {ncu} CUs the dispatch plans {pl.kernel or pl.err} ({pl.family})"
    seen = {}

    def run(c, pts):
        res = Launcher(ops, workspace, c.name).run(c, pts)
        seen["kernel"] = ops.gemm_last_kernel()
        return res

    ops.gemm_set_option("reserve_cus", 0)
    try:
        _set(ops, case.opts)
        gots = gr.verify(case, pl, run, "cuda")
        assert seen["kernel"] == pl.kernel, f"{case.name}: launched {seen['kernel']}, the restated dispatch says {pl.kernel}"
        if pl.inlaunch:                    # the header promises the bits of the separate reduce launch
            ops.gemm_set_option("splitk_inlaunch", 0)
            again = run(case, gr.inputs(case, "cuda"))
            assert not gc.plan(case._replace(opts=dict(case.opts, splitk_inlaunch=0)), ncu).inlaunch
            for a, b in zip(gots, again):
                for name in a:
                    assert torch.equal(gr._bits(a[name]), gr._bits(b[name])), f"{case.name} {name}: splitk_inlaunch 0 and 1 differ"
    finally:
        _set(ops, {k: RESTORE[k] for k in case.opts})
        ops.gemm_set_option("splitk_inlaunch", -1)
