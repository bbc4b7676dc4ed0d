"""The resize, head and layout kernels of csrc/spatial.hip against float64, per element, at the launchers' edges: bilinear_cl_fwd
/ _bwd (generic, int<2|4|8>, sliced int4<8>), upsum_relu (one pixel and 2 x 2 per lane), upsample_ac_fwd / _bwd, convseg_fwd /
_bwd, head_grad_fused, window_permute, pixel_shuffle2, space_to_depth2_crop, pixel_unshuffle2_sums and patch_im2col[_prenorm|_floor].

The module walks tests/spatial_cases.py (tests/test_spatial_cases_cpu.py checks that the table reaches every launcher branch).  Per
row: inputs drawn on the GPU from a seeded generator, the launch through pvpuformer_amd.ops, the float64 reference on the GPU and the
bounds of tests/spatial_ref.py (|got - ref| <= REL |ref| + c A; the module docstring there derives A per output).  Exact, bit for
bit: the layouts, the integer-valued resizes at ratios 2 / 4 / 8 (forward, backward, sliced form, upsum_relu, align-corners at
steps 1/2 and 1/4), pixel_shuffle2's fp32 bias add, the zeros behind a closed ReLU gate, integer column sums.

Memory: every operand is a slice of a larger buffer (rowops_ref.Guarded) with guard rows before and after, gap columns where the
entry point takes a leading dimension (with an element offset: the channel-slice use), optionally shifted to break the alignment a
vector form needs; guards and gaps hold a finite sentinel and must come out bit-identical -- for inputs the whole buffer.  Outputs,
`part` / `part_b` included, are pre-filled with NaN and none may survive.  Launches the launcher must reject leave every buffer
untouched.

c per family (spatial_ref.COEF) is the next power of two at or above 4 x the worst value this module measured on one MI355X; the
module prints the worst value per (kernel, output) when it ends.  Measured worst c, and the constant it gives:
  resize forward   bilinear_cl_fwd 2.6e-8, upsum_relu 2.7e-8 (one pixel per lane) / 5.1e-8 (2 x 2), upsample_ac_fwd 2.4e-8  -> 2^-22 (2.4e-7)
  resize backward  bilinear_cl_bwd generic 2.9e-8, int<R> 2.7e-8, sliced int4<8> 1.5e-8; upsample_ac_bwd 1.6e-8               -> 2^-23 (1.2e-7)
  head             convseg_fwd 7.7e-8; convseg_bwd dx 1.5e-7, dw 1.0e-7, db 2.2e-8; head_grad_fused dx 6.3e-9 (bf16: REL carries
                   it), dw 8.9e-8, db 1.4e-8                                                                                    -> 2^-20 (9.5e-7)
  layout sums      pixel_unshuffle2_sums 9.6e-8, patch_im2col 8.4e-8 / _floor 8.5e-8 (prenorm: 0), pixel_shuffle2 0            -> 2^-21 (4.8e-7)
Every value is one or two fp32 roundings (2^-24 = 6.0e-8) of the result; none comes near the 2^-17 an fp32 path may not exceed.

Accepted gaps: a second grid-stride trip of the 16384-block-capped kernels other than window_permute (>= 33 M elements per case);
the `small == false` index path of upsample_ac_bwd (>= 2^31 cells); the laboratory-only int4<4> form of bilinear_cl_bwd.  A null or
misaligned pointer is passed only where the launcher itself rejects it, never to a kernel."""
import pytest
import torch

import rowops_ref as rr
import spatial_ref as sr
from spatial_cases import CASES, convseg_bwd_nblk, pixel_unshuffle2_nblk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    saved = dict(rr.STATS)                       # (the table of the row-kernel module, when both run in one process)
    rr.STATS.clear()
    yield
    if rr.STATS:
        print("\n" + sr.summary())
    for k, v in saved.items():
        rr.STATS[k] = max(rr.STATS.get(k, 0.0), v)


class Kernels:
    """the kernels behind the interface spatial_ref.verify walks; every operand lives in a rowops_ref.Guarded buffer"""

    device = "cuda"

    def __init__(self, ops, tag):
        self.ops, self.tag, self.bufs = ops, tag, []

    def _in(self, t, name, ld=None, shift=0):
        if t is None:
            return None
        t2 = t.reshape(-1, t.shape[-1])
        g = sr.Guarded(t2.shape[0], t2.shape[1], t.dtype, self.device, ld=ld, shift=shift, data=t2, name=name)
        self.bufs.append(g)
        return g.t

    def _out(self, rows, cols, dtype, name, ld=None, shift=0, init=None):
        g = sr.Guarded(rows, cols, dtype, self.device, ld=ld, shift=shift, name=name)
        if init is not None:                      # read-modify-write operand: starts from `init`, must end without a NaN
            g.t.copy_(init.reshape(rows, cols))
        self.bufs.append(g)
        return g.t

    def _done(self):
        torch.cuda.synchronize()
        for g in self.bufs:
            g.check(self.tag)
        self.bufs = []

    def _untouched(self):
        torch.cuda.synchronize()
        for g in self.bufs:
            assert bool((rr._bits(g.buf) == g.before).all()), f"{self.tag}: a rejected launch changed {g.name}"
        self.bufs = []

    # ---- resize
    def bil_fwd(self, c, x):
        B, h, w, H, W, C = (c.shape[k] for k in ("B", "h", "w", "H", "W", "C"))
        li, lo, off = c.opt.get("ld_in", C), c.opt.get("ld_out", C), c.opt.get("off", 0)
        X, Y = self._in(x, "in", ld=li, shift=off), self._out(B * H * W, C, x.dtype, "out", ld=lo, shift=off)
        self.ops.bilinear_cl_fwd(X, li, Y, lo, B, h, w, H, W, C, self.ops.code_of(x))
        self._done()
        return Y.reshape(B, H, W, C)

    def bil_bwd(self, c, dout):
        B, h, w, H, W, C = (c.shape[k] for k in ("B", "h", "w", "H", "W", "C"))
        li, lo, off = c.opt.get("ld_in", C), c.opt.get("ld_out", C), c.opt.get("off", 0)
        D, X = self._in(dout, "dout", ld=lo, shift=off), self._out(B * h * w, C, dout.dtype, "din", ld=li, shift=off)
        self.ops.bilinear_cl_bwd(D, lo, X, li, B, h, w, H, W, C, self.ops.code_of(dout))
        self._done()
        return X.reshape(B, h, w, C)

    def upsum(self, c, io0, zs):
        B, H, W, C = io0.shape
        io = self._out(B * H * W, C, io0.dtype, "io", init=io0)
        maps = [(self._in(z, f"z{i}"), z.shape[1], z.shape[2]) for i, z in enumerate(zs)]
        self.ops.upsum_relu(io, maps, B, H, W, C, self.ops.code_of(io0))
        self._done()
        return io.reshape(B, H, W, C)

    def ac_fwd(self, c, x):
        P, h, w, H, W = (c.shape[k] for k in ("planes", "h", "w", "H", "W"))
        X, Y = self._in(x, "in"), self._out(P * H, W, torch.float32, "out")
        self.ops.upsample_ac_fwd(X, Y, P, h, w, H, W)
        self._done()
        return Y.reshape(P, H, W)

    def ac_bwd(self, c, dout):
        P, h, w, H, W = (c.shape[k] for k in ("planes", "h", "w", "H", "W"))
        D, X = self._in(dout, "dout"), self._out(P * h, w, torch.float32, "din")
        self.ops.upsample_ac_bwd(D, X, P, h, w, H, W)
        self._done()
        return X.reshape(P, h, w)

    # ---- head
    def cs_fwd(self, c, x, w, bias, mask):
        rows, C = x.shape
        sh = lambda k, t: c.opt.get(k, 0) // t.element_size()
        X, Wv, Bv = self._in(x, "x", shift=sh("shift_x", x)), self._in(w, "w", shift=sh("shift_w", w)), self._in(bias, "bias")
        M = self._in(mask, "mask", shift=sh("shift_mask", w))
        out = self._out(1, rows, torch.float32, "out")
        self.ops.convseg_fwd(X, Wv, Bv, M, out, rows, c.shape["HW"], C)
        self._done()
        return out[0]

    def _head_operands(self, c, dout, x, w, mask, dx0=None):
        rows, C = x.shape
        nblk = self.ops.convseg_bwd_nblk(rows)
        assert nblk == convseg_bwd_nblk(rows)
        D, X, Wv, M = self._in(dout, "dout"), self._in(x, "x"), self._in(w, "w"), self._in(mask, "mask")
        dx = self._out(rows, C, x.dtype, "dx", shift=c.opt.get("shift_dx", 0) // x.element_size(), init=dx0)
        part, part_b = self._out(nblk, C, torch.float32, "part"), self._out(1, nblk, torch.float32, "part_b")
        return D, X, Wv, M, dx, part, part_b

    @staticmethod
    def _sums(part, part_b, rows):
        """dw / db from the partial rows, summed in float64; a workgroup whose row range is empty must have written zeros"""
        nblk = part.shape[0]
        per = (rows + nblk - 1) // nblk
        empty = torch.arange(nblk, device=part.device) * per >= rows
        assert bool((part[empty] == 0).all()) and bool((part_b[0][empty] == 0).all()), "an empty workgroup's partial row is not 0"
        return part.double().sum(0), part_b.double().sum().reshape(1)

    def cs_bwd(self, c, dout, x, w, mask, dx0, accum):
        rows, C = x.shape
        D, X, Wv, M, dx, part, part_b = self._head_operands(c, dout, x, w, mask, dx0 if accum & 1 else None)
        self.ops.convseg_bwd(D, X, Wv, M, dx, accum, part, part_b, rows, c.shape["HW"], C)
        self._done()
        dw, db = self._sums(part, part_b, rows)
        return dict(dx=dx, dw=dw, db=db)

    def hgf(self, c, dfn, y, inv, dout, x, w, mask):
        rows, C = x.shape
        G, Y, I = self._in(dfn, "dfn"), self._in(y, "y"), self._in(inv, "inv")
        D, X, Wv, M, dx, part, part_b = self._head_operands(c, dout, x, w, mask)
        self.ops.head_grad_fused(G, Y, I, D, X, Wv, M, dx, part, part_b, rows, c.shape["HW"], C)
        self._done()
        dw, db = self._sums(part, part_b, rows)
        return dict(dx=dx, dw=dw, db=db)

    def rejects(self, c, inp):
        """a launch the launcher must refuse: the argument error, and no buffer touched"""
        from pvpuformer_amd._lib import VpuError
        s = c.shape
        if c.entry == "unsh":
            B, h, w, C = (s[k] for k in ("B", "h", "w", "C"))
            S, dst = self._in(inp["src"], "src"), self._out(B * h * w, 4 * C, inp["src"].dtype, "dst")
            part = self._out(pixel_unshuffle2_nblk(C), C, torch.float32, "part")
            with pytest.raises(VpuError, match="pixel_unshuffle2_sums"):
                self._unsh_call(S, dst, part, B, h, w, C)
        elif c.entry == "cs_bwd":
            D, X, Wv, M, dx, part, part_b = self._head_operands(c, inp["dout"], inp["x"], inp["w"], inp["mask"])
            with pytest.raises(VpuError, match="convseg_bwd"):
                self.ops.convseg_bwd(D, X, Wv, M, dx, c.opt["accum"], part, part_b, s["rows"], s["HW"], s["C"])
        else:
            G, Y, I = self._in(inp["dfn"], "dfn"), self._in(inp["y"], "y"), self._in(inp["inv"], "inv")
            D, X, Wv, M, dx, part, part_b = self._head_operands(c, inp["dout"], inp["x"], inp["w"], inp["mask"])
            with pytest.raises(VpuError, match="head_grad_fused"):
                self.ops.head_grad_fused(G, Y, I, D, X, Wv, M, dx, part, part_b, s["rows"], s["HW"], s["C"])
        self._untouched()

    # ---- layout
    def winperm(self, c, x, to_raster):
        B, T, C = x.shape
        X, Y = self._in(x, "x"), self._out(B * T, C, x.dtype, "y")
        self.ops.window_permute(X, Y, B, c.shape["g"], c.shape["wg"], C, to_raster)
        self._done()
        return Y.reshape(B, T, C)

    def ps2(self, c, t, bias, inverse):
        B, h, w, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        S, Bv = self._in(t, "src"), self._in(bias, "bias")
        out = self._out(B * h * w, 4 * C, t.dtype, "dst") if inverse else self._out(B * 4 * h * w, C, t.dtype, "dst")
        self.ops.pixel_shuffle2(S, out, Bv, B, h, w, C, inverse=inverse)
        self._done()
        return out if inverse else out.reshape(B, 2 * h, 2 * w, C)

    def s2d(self, c, t, inverse):
        B, g, C = c.shape["B"], c.shape["g"], c.shape["C"]
        S = self._in(t, "src")
        out = self._out(B * g * g, C, t.dtype, "dst") if inverse else self._out(B * (g // 2) ** 2, 4 * C, t.dtype, "dst")
        self.ops.space_to_depth2_crop(S, out, B, g, C, inverse=inverse)
        self._done()
        return out.reshape(B, g, g, C) if inverse else out

    def _unsh_call(self, S, dst, part, B, h, w, C):
        # (ops.pixel_unshuffle2_sums allocates `part` itself; the same entry point with `part` in a guarded buffer)
        o = self.ops
        o._lib.call("vpu_pixel_unshuffle2_sums", o.ptr(S), o.ptr(dst), o.ptr(part), B, h, w, C, o.code_of(S), o._stream())

    def unsh(self, c, src):
        B, h, w, C = (c.shape[k] for k in ("B", "h", "w", "C"))
        nblk = self.ops._lib.load().vpu_pixel_unshuffle2_nblk(C)
        assert nblk == pixel_unshuffle2_nblk(C)
        S, dst = self._in(src, "src"), self._out(B * h * w, 4 * C, src.dtype, "dst")
        part = self._out(nblk, C, torch.float32, "part")
        self._unsh_call(S, dst, part, B, h, w, C)
        self._done()
        return dst, part.double().sum(0)

    def im2col(self, c, img4, disks):
        B, H, W, P = (c.shape[k] for k in ("B", "H", "W", "P"))
        K3P = (3 * P * P + 7) // 8 * 8
        I, Dk = self._in(img4, "img4"), self._in(disks, "disks")
        cols = self._out(B * (H // P) * (W // P), 2 * K3P, sr.tdtype(c.dtype), "cols")
        if c.opt["floor"]:
            self.ops.patch_im2col_floor(I, Dk, cols, B, H, W, P, c.opt["wg"], prenorm=bool(c.opt["prenorm"]))
        else:
            self.ops.patch_im2col(I, Dk, cols, B, H, W, P, c.opt["wg"], prenorm=bool(c.opt["prenorm"]))
        self._done()
        return cols


@pytest.mark.parametrize("case", CASES, ids=sr.case_id)
def test_spatial(ops, case):
    sr.verify(case, Kernels(ops, sr.case_id(case)), Kernels.device)
