"""Float64 references, per-element bounds, sentinel buffers and the case walker for the row and normalisation kernels
(csrc/rowops.hip: LayerNorm, L2 normalise, column sums, act_bwd; csrc/spatial.hip: GroupNorm(1, C) and the DMA gates).
Plain torch, importable without a GPU: tests/test_rowops_cases_cpu.py runs the same walker over an honest fp32 implementation
on the CPU, tests/test_rowops_f64.py over the kernels.

References.  One per operation, written out from the formula in float64 over exactly the values the kernel is given (bf16 or
fp32, upcast).  Where a kernel consumes something it produced itself -- the rounded y of the PE form of LayerNorm
(y2 = fl_T(y) + pe[row % pe_rows]), the rounded y and inv of the L2 backward, the gates' cg / sg in gate_apply and gate_bwd, the
rounded map of pixel_shuffle2_gn_stats -- the reference takes that produced value (``given``), so that a bf16 rounding boundary in
the producer is not charged to the consumer.  The backward references compute their own float64 statistics from x: the kernel is
handed the forward's fp32 mean / rstd, and the bound below carries the conditioning that costs.

Bounds.  Per element  |got - ref| <= REL |ref| + atol + c A  with REL = 2^-8 for a bf16 result and 0 for an fp32 one, A the sum
of the absolute contributions of that output (cancellation cannot hide an error) times the row's conditioning where one applies,
and c one constant per kernel family (COEF).  An element with A = 0 passes only when its error is exactly 0; no element is ever
left out of a check.

  LayerNorm, r = rstd, |mu|^ = mean |x|, kappa_row = max(1, max_c (|x| + |mu|^) r), g^ = |dy w| (dy: |dy| + |dy2|):
    y      (|x| + |mu|^) r |w| + |b|
    y2     |fl(y)| + |pe|
    dx     kappa_row r (g^ + mean g^ + |x^| mean(g^ |x^|)) + |dres|
    dw     sum_rows |dy| (|x| + |mu|^) r         db   sum_rows |dy|
    mean   mean |x|                              rstd kappa_row r
  (|mu|^ = mean |x|, not |mu|: the fp32 mean is off by 2^-24 of the sum of its absolute terms, whatever cancels in it -- a row of
  eight values whose mean happens to be 0.02 has |x| + |mu| r = 0.02 at a column near the mean, and torch's own fp32 LayerNorm
  then needs c = 1.3e-6 at that element.  kappa_row >= 1: on a row of zeros (|x| + |mu|^) r is 0, but rsqrt and the arithmetic
  after the statistics still round.)

  GroupNorm(1, C) takes the same forms with ONE difference: the kernels form the variance as E[x^2] - mu^2 from fp32 partial sums of
  8 (gn_stats_kernel) to 32 (pixel_shuffle2_gn_kernel) squares added up in float64, so the conditioning is
  kappa = max(1, E[x^2] / (var + eps)), not the two-pass one; it multiplies the y, rstd, dx and dw terms.
  With GELU (t = the affine output): y = t Phi(t), A = 1.13 A_t + |t| (1 + |erf|) / 2  (|GELU'| <= 1.13; 1 + erf cancels in the
  left tail), and the bf16 kernels' Abramowitz & Stegun 7.1.26 form adds atol = AS_ERR max(1, |t|) on Phi (AS_ERR = 1.5e-7), which the
  backward carries through dy GELU'(t) into dx / dw / db.  |GELU''| <= 0.8 turns the error of the recomputed t into one of GELU'.

  l2norm   y: |x| inv;  inv: inv;  dx: inv (|dy| + |y| sum |dy y|)
  colsum   |beta out0| + sum_rows |in|
  gates    cg / sg: s (1 + |m|) for s = sigmoid(m);  out: |x| (1 + cg + sg);  dx: |dx0| + sum_gates |dout| (1 + cg + sg);
           dK at the arg-max: |dK0| + s (1 - s) sum_c |dout x| (dQ alike over the rows); every other entry of dQ / dK has A = 0.
  act_bwd  |dy| ((1 + |erf|) / 2 + |a| phi(a));  relu is exact

_need / _within / _fails work as in tests/test_attention_f64.py: every check prints the smallest c that would have passed, and STATS
keeps the worst one per (kernel, output)."""
import math
import zlib
from collections import namedtuple

import torch

REL = 2.0 ** -8            # rounding of a bf16 result
AS_ERR = 1.5e-7            # Abramowitz & Stegun 7.1.26 on Phi, times max(1, |t|)
GUARD = 4                  # guard rows before and after every operand (even: the operand keeps its 32-byte alignment)
SENT16 = 0x4B5A            # bf16 1.43e7 -- the finite sentinel of tests/test_attention_f64.py
SENT32 = 0x4B5A4B5A        # fp32 1.43e7; the same bits as an int32
LN_EPS = 9.999999974752427e-07       # 1e-6f and 1e-5f: the values the kernels receive
GN_EPS = 9.999999747378752e-06
L2_FLOOR = 9.999999960041972e-13      # 1e-12f, the value the kernels clamp the norm with

# c per kernel family: the next power of two at or above 4 x the worst value measured on an MI355X (tests/test_rowops_f64.py
# lists the measurements); no constant above 2^-17 (two chained fp32 reductions of at most 32 + 6 terms each)
COEF = {"ln": 2.0 ** -19, "gn": 2.0 ** -20, "l2": 2.0 ** -20, "colsum": 2.0 ** -20, "gate": 2.0 ** -20, "act": 2.0 ** -20}
COEF_MAX = 2.0 ** -17

STATS = {}                 # (kernel, output) -> worst coefficient

Out = namedtuple("Out", "ref A rel atol")


def O(ref, A, rel=0.0, atol=0.0):
    return Out(ref, A, rel, atol)


def tdtype(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def rel_of(name):
    return REL if name == "bf16" else 0.0


def fl(t, name):
    """float64 -> the dtype's nearest value -> float64"""
    return t.to(tdtype(name)).double()


# ------------------------------------------------------------------------------------------------ bounds
def _need(got, ref, A, rel, atol=0.0):
    """smallest c with |got - ref| <= rel |ref| + atol + c A everywhere (inf where A == 0 and the error is not covered; NaN -> inf)"""
    err = (got.double() - ref).abs()
    over = (err - rel * ref.abs() - atol).clamp_min(0.0)
    inf = torch.full_like(over, math.inf)
    need = torch.where(A > 0, over / A.clamp_min(1e-300), torch.where(over > 0, inf, torch.zeros_like(over)))
    return torch.where(torch.isnan(err), inf, need)


def _within(tag, got, ref, A, coef, rel=0.0, key=None, atol=0.0):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    need = _need(got, ref, A.expand_as(ref) if A.shape != ref.shape else A, rel, atol)
    m = need.max().item() if need.numel() else 0.0
    print(f"[rowops f64] {tag}: {m:.2e} (bound {coef:.2e})")
    if key is not None:
        STATS[key] = max(STATS.get(key, 0.0), m)
    bad = ~(need <= coef)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} elements out of bound, first at {i}: got {got[i].item()!r}, "
                             f"ref {ref[i].item()!r}, A {A.expand_as(ref)[i].item()!r}")


def _fails(got, ref, A, coef, rel=0.0, atol=0.0):
    return bool((~(_need(got, ref, A.expand_as(ref), rel, atol) <= coef)).any())


def check(tag, family, kernel, got, outs, coef=None):
    coef = COEF[family] if coef is None else coef
    for name, o in outs.items():
        _within(f"{tag} {name}", got[name], o.ref, o.A, coef, o.rel, key=(kernel, name), atol=o.atol)


def any_fails(family, got, outs, coef=None):
    """does the bound reject ``got`` (name -> float64 tensor) on at least one output"""
    coef = COEF[family] if coef is None else coef
    return any(_fails(got[n], o.ref, o.A, coef, o.rel, o.atol) for n, o in outs.items() if n in got)


def summary():
    lines = ["[rowops f64] worst coefficient per kernel and output:"]
    for (k, o), v in sorted(STATS.items()):
        lines.append(f"  {k:28s} {o:6s} {v:.2e}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ sentinel buffers
def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


class Guarded:
    """An operand [rows, cols] with leading dimension ld >= cols as a slice of a larger buffer: GUARD rows before and after, gap
    columns cols..ld, optionally shifted by ``shift`` elements; guards and gaps hold the sentinel pattern and must come out
    bit-identical.  ``data``: an input (the whole buffer must come out unchanged); None: an output, pre-filled with NaN
    (integers: the sentinel itself, which no index or count equals)."""

    def __init__(self, rows, cols, dtype, device, ld=None, shift=0, data=None, name=""):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld, self.name, self.is_input = rows, cols, ld, name, data is not None
        n = (rows + 2 * GUARD) * ld + shift
        if dtype == torch.bfloat16:
            self.buf = torch.full((n,), SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)
        elif dtype == torch.float64:
            self.buf = torch.full((n,), SENT32 * (1 << 32) + SENT32, dtype=torch.int64, device=device).view(torch.float64)
        else:
            self.buf = torch.full((n,), SENT32, dtype=torch.int32, device=device).view(dtype)
        lo = GUARD * ld + shift
        self.t = self.buf[lo:lo + rows * ld].view(rows, ld)[:, :cols]
        if data is not None:
            self.t.copy_(data.reshape(rows, cols))
        elif dtype.is_floating_point:
            self.t.fill_(float("nan"))
        self.mask = torch.zeros(n, dtype=torch.bool, device=device)
        self.mask[lo:lo + rows * ld].view(rows, ld)[:, :cols] = True
        self.before = _bits(self.buf).clone()

    def check(self, tag):
        same = _bits(self.buf) == self.before
        if self.is_input:
            assert bool(same.all()), f"{tag}: input {self.name} changed"
            return
        bad = ~same & ~self.mask
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} cells outside output {self.name} changed, first at {int(bad.nonzero()[0])}"
        if self.t.dtype.is_floating_point:
            assert not bool(torch.isnan(self.t).any()), f"{tag}: output {self.name} keeps a NaN of its pre-fill (an element not written)"
        else:
            assert not bool((self.t == SENT32).any()), f"{tag}: output {self.name} keeps its pre-fill"


# ------------------------------------------------------------------------------------------------ float64 pieces
def Phi(t):
    return 0.5 * (1.0 + torch.erf(t * math.sqrt(0.5)))


def phi(t):
    return torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def A_Phi(t):
    return 0.5 * (1.0 + torch.erf(t * math.sqrt(0.5)).abs())


def gelu_tanh(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))


def dgelu_tanh(t):
    u = math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)
    th = torch.tanh(u)
    return 0.5 * (1.0 + th) + 0.5 * t * (1.0 - th * th) * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * t * t)


def lowest_argmax(V, dim, last=False):
    """index of the maximum along ``dim``; among equal maxima the lowest index (last=True: the highest -- the wrong rule)"""
    mx = V.amax(dim, keepdim=True)
    shape = [1] * V.dim()
    shape[dim] = V.shape[dim]
    idx = torch.arange(V.shape[dim], device=V.device).view(shape).expand_as(V)
    if last:
        return torch.where(V == mx, idx, torch.full_like(idx, -1)).amax(dim)
    return torch.where(V == mx, idx, torch.full_like(idx, V.shape[dim])).amin(dim)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_stats(X, eps, perturb=None):
    C = X.shape[1]
    Xs = X[:, :C - 8] if perturb == "cols-8" and C > 8 else X
    mu = Xs.mean(1, keepdim=True)
    var = ((Xs - mu) ** 2).mean(1, keepdim=True)
    if perturb == "var/(C-1)":
        var = var * C / (C - 1)
    r = (var + (0.0 if perturb == "noeps" else eps)).rsqrt()
    return mu, r


def ln_fwd_ref(dt, x, w, b, eps, pe=None, given_y=None, perturb=None):
    X, W, Bv = x.double(), w.double(), b.double()
    mu0, r0 = _ln_stats(X, eps)
    mu, r = _ln_stats(X, eps, perturb)
    spread = (X.abs() + X.abs().mean(1, keepdim=True)) * r0
    kappa = spread.amax(1, keepdim=True).clamp_min(1.0)
    y = (X - mu) * r * W + Bv
    outs = dict(y=O(y, spread * W.abs() + Bv.abs(), rel_of(dt)),
                mean=O(mu[:, 0], X.abs().mean(1)), rstd=O(r[:, 0], (kappa * r0)[:, 0]))
    if pe is not None:
        rows, pr = X.shape[0], pe.shape[0]
        ridx = torch.arange(rows, device=X.device)
        ridx = (ridx + 1) % pr if perturb == "pe+1" else ridx % pr
        P = pe.double()[ridx]
        ybase = y if perturb == "y2-unrounded" else (fl(y, dt) if given_y is None else given_y.double())
        outs["y2"] = O(ybase + P, ybase.abs() + P.abs(), rel_of(dt))
    return outs


def ln_bwd_ref(dt, dy, dy2, x, w, dres, eps, perturb=None):
    X, W = x.double(), w.double()
    mu, r = _ln_stats(X, eps)
    xh = (X - mu) * r
    spread = (X.abs() + X.abs().mean(1, keepdim=True)) * r
    kappa = spread.amax(1, keepdim=True).clamp_min(1.0)
    d = dy.double() + (dy2.double() if dy2 is not None else 0.0)
    dabs = dy.double().abs() + (dy2.double().abs() if dy2 is not None else 0.0)
    g = d * W
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = r * (g - m1 - (0.0 if perturb == "no-xhat-term" else xh * m2))
    R = dres.double() if dres is not None else torch.zeros_like(X)
    dx = dx + R * (2.0 if perturb == "dres-twice" else 1.0)
    dwt = d * xh
    dw = dwt[:-1].sum(0) if perturb == "dw-last-row" else dwt.sum(0)
    gh = dabs * W.abs()
    A_dx = kappa * r * (gh + gh.mean(1, keepdim=True) + xh.abs() * (gh * xh.abs()).mean(1, keepdim=True)) + R.abs()
    return dict(dx=O(dx, A_dx, rel_of(dt)), dw=O(dw, (dabs * spread).sum(0)), db=O(d.sum(0), dabs.sum(0)))


# ------------------------------------------------------------------------------------------------ GroupNorm(1, C)
def _gn_stats(X, eps, perturb=None):
    Xs = X[:, :X.shape[1] - 1] if perturb == "HW-1" and X.shape[1] > 1 else X
    mu = Xs.mean((1, 2), keepdim=True)
    var = ((Xs - mu) ** 2).mean((1, 2), keepdim=True)
    return mu, (var + eps).rsqrt(), var


def _gn_common(X, W, Bv, eps):
    mu, r, var = _gn_stats(X, eps)
    kappa = ((X * X).mean((1, 2), keepdim=True) / (var + eps)).clamp_min(1.0)
    spread = (X.abs() + X.abs().mean((1, 2), keepdim=True)) * r
    A_t = kappa * spread * W.abs() + Bv.abs()
    return mu, r, kappa, spread, A_t


def gn_fwd_ref(dt, x, w, b, eps, gelu, perturb=None):
    """x [B, HW, C]"""
    X, W, Bv = x.double(), w.double(), b.double()
    mu0, r0, kappa, spread, A_t = _gn_common(X, W, Bv, eps)
    mu, r, _ = _gn_stats(X, eps, perturb)
    t = (X - mu) * r * W + Bv
    if gelu:
        y = gelu_tanh(t) if perturb == "tanh-gelu" else t * Phi(t)
        A_y = 1.13 * A_t + t.abs() * A_Phi(t)
        atol = AS_ERR * t.abs().clamp_min(1.0) * t.abs() if dt == "bf16" else 0.0
    else:
        y, A_y, atol = t, A_t, 0.0
    return dict(y=O(y, A_y, rel_of(dt), atol), mean=O(mu[:, 0, 0], X.abs().mean((1, 2))),
                rstd=O(r[:, 0, 0], (kappa * r0)[:, 0, 0]))


def gn_bwd_ref(dt, dy, x, w, b, eps, gelu, perturb=None):
    X, W, Bv, D = x.double(), w.double(), b.double(), dy.double()
    mu, r, kappa, spread, A_t = _gn_common(X, W, Bv, eps)
    xh = (X - mu) * r
    t = xh * W + Bv
    if gelu:
        d = D * (dgelu_tanh(t) if perturb == "tanh-gelu" else Phi(t) + t * phi(t))
        dabs = D.abs() * (A_Phi(t) + t.abs() * phi(t) + 0.8 * A_t)
        e = D.abs() * (AS_ERR * t.abs().clamp_min(1.0)) if dt == "bf16" else torch.zeros_like(D)
    else:
        d, dabs, e = D, D.abs(), torch.zeros_like(D)
    g = d * W
    m = lambda v: v.mean((1, 2), keepdim=True)
    dx = r * (g - m(g) - (0.0 if perturb == "no-xhat-term" else xh * m(g * xh)))
    gh, eh = dabs * W.abs(), e * W.abs()
    A_dx = kappa * r * (gh + m(gh) + xh.abs() * m(gh * xh.abs()))
    a_dx = r * (eh + m(eh) + xh.abs() * m(eh * xh.abs()))
    return dict(dx=O(dx, A_dx, rel_of(dt), a_dx),
                dw=O((d * xh).sum((0, 1)), (kappa * dabs * spread).sum((0, 1)), 0.0, (e * xh.abs()).sum((0, 1))),
                db=O(d.sum((0, 1)), dabs.sum((0, 1)), 0.0, e.sum((0, 1))))


def pixel_shuffle2_ref(dt, src, bias, B, h, w, C):
    """src [B h w, 4 C] -> [B, 2h, 2w, C]: dst[b, 2y + dy, 2x + dx, c] = src[b, y, x, 4 c + 2 dy + dx] + bias[c]"""
    S = src.double().view(B, h, w, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * w, C)
    Bv = bias.double() if bias is not None else torch.zeros(C, dtype=torch.float64, device=src.device)
    return dict(y1=O((S + Bv).view(B, 4 * h * w, C), (S.abs() + Bv.abs()).view(B, 4 * h * w, C), rel_of(dt)))


# ------------------------------------------------------------------------------------------------ L2 normalise
def l2_fwd_ref(dt, x):
    X = x.double()
    n = (X * X).sum(1, keepdim=True).sqrt()
    inv = 1.0 / n.clamp_min(L2_FLOOR)
    return dict(y=O(X * inv, X.abs() * inv, rel_of(dt)), inv=O(inv[:, 0], inv[:, 0]))


def l2_bwd_ref(dt, dy, y, inv, perturb=None):
    """y, inv: the forward's own rounded outputs, as the kernel reads them"""
    D, Y, I = dy.double(), y.double(), inv.double()[:, None]
    Iu = torch.roll(I, 1, 0) if perturb == "inv-neighbour" else I
    s = (D * Y).sum(1, keepdim=True)
    return dict(dx=O(Iu * (D - Y * s), I * (D.abs() + Y.abs() * (D * Y).abs().sum(1, keepdim=True)), rel_of(dt)))


# ------------------------------------------------------------------------------------------------ column sums
def colsum_ref(x, out0, beta, perturb=None):
    X = x.double()
    Xs = X[:-1] if perturb == "last-row" else X
    base = beta * out0.double() if beta != 0.0 else torch.zeros_like(out0, dtype=torch.float64)
    return dict(out=O(base + Xs.sum(0), base.abs() + X.abs().sum(0)))


# ------------------------------------------------------------------------------------------------ gates
def gate_stats_ref(Q, K, perturb=None):
    """Q [B, nq, C], K [B, N, C] -> cg [B, C], argq [B, C], sg [B, N], argc [B, N]; lowest index wins among equal maxima"""
    Qd, Kd = Q.double(), K.double()
    last = perturb == "argmax-last"
    mq, mk = Qd.amax(1), Kd.amax(2)
    cg, sg = torch.sigmoid(mq), torch.sigmoid(mk)
    return dict(cg=O(cg, cg * (1 + mq.abs())), sg=O(sg, sg * (1 + mk.abs()))), lowest_argmax(Qd, 1, last), lowest_argmax(Kd, 2, last)


def gate_apply_ref(dt, x, cg, sg, perturb=None):
    X = x.double()
    f = 1.0 + cg.double()[:, None, :] + (0.0 if perturb == "no-sg" else sg.double()[:, :, None])
    fa = 1.0 + cg.double()[:, None, :] + sg.double()[:, :, None]
    return dict(out=O(X * f, X.abs() * fa, rel_of(dt)))


def gate_bwd_ref(dt, douts, x, cg, argq, sg, argc, dx0, accum, dQ0s, dK0s):
    """cg / argq [n, B, C], sg / argc [n, B, N] (given); douts / dQ0s / dK0s: lists of n.  Returns the bounds and, per gate,
    the masks of the entries of dQ / dK the gradient lands on (every other entry must keep its bits)."""
    X = x.double()
    n = len(douts)
    dx = dx0.double().clone() if accum else torch.zeros_like(X)
    A_dx = dx.abs()
    outs, masks = {}, {}
    for i in range(n):
        D = douts[i].double()
        g, s = cg[i].double(), sg[i].double()
        f = 1.0 + g[:, None, :] + s[:, :, None]
        dx = dx + D * f
        A_dx = A_dx + D.abs() * f
        T = D * X
        dsg, dcg = T.sum(2) * s * (1 - s), T.sum(1) * g * (1 - g)                    # [B, N], [B, C]
        a_sg, a_cg = T.abs().sum(2) * s * (1 - s), T.abs().sum(1) * g * (1 - g)
        dK, dQ = dK0s[i].double().clone(), dQ0s[i].double().clone()
        A_dK, A_dQ = torch.zeros_like(dK), torch.zeros_like(dQ)
        ic, iq = argc[i].long()[:, :, None], argq[i].long()[:, None, :]
        dK.scatter_add_(2, ic, dsg[:, :, None])
        A_dK.scatter_(2, ic, (dK0s[i].double().gather(2, ic).abs() + a_sg[:, :, None]))
        dQ.scatter_add_(1, iq, dcg[:, None, :])
        A_dQ.scatter_(1, iq, (dQ0s[i].double().gather(1, iq).abs() + a_cg[:, None, :]))
        outs[f"dK{i}"], outs[f"dQ{i}"] = O(dK, A_dK, rel_of(dt)), O(dQ, A_dQ, rel_of(dt))
        mk, mq = torch.zeros_like(dK, dtype=torch.bool), torch.zeros_like(dQ, dtype=torch.bool)
        mk.scatter_(2, ic, True)
        mq.scatter_(1, iq, True)
        masks[f"dK{i}"], masks[f"dQ{i}"] = mk, mq
    outs["dx"] = O(dx, A_dx, rel_of(dt))
    return outs, masks


# ------------------------------------------------------------------------------------------------ act_bwd
def act_bwd_ref(dt, dy, aux, kind, perturb=None):
    D, Av = dy.double(), aux.double()
    if kind == 0:
        return dict(dz=O(D * (Av > 0).double(), torch.zeros_like(D), 0.0))      # exact: A = 0
    dg = dgelu_tanh(Av) if perturb == "tanh-gelu" else Phi(Av) + Av * phi(Av)
    return dict(dz=O(D * dg, D.abs() * (A_Phi(Av) + Av.abs() * phi(Av)), rel_of(dt)))


# ------------------------------------------------------------------------------------------------ inputs
def _gen(case, device):
    seed = zlib.crc32(repr(case).encode()) & 0x7FFFFFFF
    return torch.Generator(device=device).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32)


def _rows_regime(g, regime, rows, C, scale=2.0, shift=0.3, sigma_off=0.1, mu_off=100.0):
    x = _randn(g, rows, C) * scale + shift
    if regime == "offset":
        x = mu_off + sigma_off * _randn(g, rows, C)
    elif regime == "const":      # rows of one value with few mantissa bits: the row sum is exact, the variance exactly 0
        v = ((torch.arange(rows, device=g.device) % 7).float() - 3.0) * 0.75
        x = v[:, None].expand(rows, C).clone()
    elif regime == "zero":
        x[::3] = 0.0
    return x


def _affine(g, regime, C):
    if regime == "wz":          # zeros and negative entries
        w = _randn(g, C)
        w[::5] = 0.0
        return w, _randn(g, C) * 0.2
    return 1 + _randn(g, C) * 0.2, _randn(g, C) * 0.2


def inputs(case, device):
    """the operands of a table row as a dict of tensors in the row's dtype (fp32 for weights), drawn on ``device``"""
    g = _gen(case, device)
    td = tdtype(case.dtype)
    s, o, e = case.shape, case.opt, case.entry
    if e == "ln":
        rows, C = s["rows"], s["C"]
        w, b = _affine(g, case.regime, C)
        d = dict(x=_rows_regime(g, case.regime, rows, C).to(td), w=w, b=b, dy=_randn(g, rows, C).to(td))
        d["dres"] = _randn(g, rows, C).to(td) if o.get("dres") else None
        d["dy2"] = _randn(g, rows, C).to(td) if o.get("dy2") else None
        d["pe"] = _randn(g, o["pe_rows"], C).to(td) if o.get("pe_rows") else None
        return d
    if e == "l2":
        rows, C = s["rows"], s["C"]
        x = _rows_regime(g, case.regime, rows, C, scale=1.0, shift=0.0)
        return dict(x=x.to(td), dy=_randn(g, rows, C).to(td))
    if e in ("colsum", "colsum_f32"):
        rows, C = s["rows"], s["C"]
        if case.regime == "int":
            x = torch.randint(-8, 9, (rows, C), generator=g, device=device).float()
            out0 = torch.randint(-8, 9, (C,), generator=g, device=device).float() * 2
        else:
            x, out0 = _randn(g, rows, C), _randn(g, C)
        return dict(x=x.to(td if e == "colsum" else torch.float32), out0=out0)
    if e in ("gn", "psgn"):
        B, HW, C = s["B"], s["HW"], s["C"]
        w, b = _affine(g, case.regime, C)
        x = _randn(g, B, HW, C) * 1.5 + 0.2
        if case.regime == "offset":                 # at most 4 sigma: the kernels' variance is one-pass
            x = _randn(g, B, HW, C) * 0.5 + 2.0
        elif case.regime == "const":
            x = ((torch.arange(B, device=device) % 5).float() - 1.0)[:, None, None].expand(B, HW, C).clone() * 0.75
        elif case.regime == "zero":
            x[0] = 0.0
        elif case.regime == "tails":                # GELU pre-activations over [-9, 9]: normalised values +-1.7, weights up to 5
            w = torch.linspace(-5.2, 5.2, C, device=device)
            b = torch.zeros(C, device=device)
        d = dict(x=x.to(td), w=w, b=b, dy=_randn(g, B, HW, C).to(td))
        if e == "psgn":
            d["src"] = (_randn(g, B * HW // 4, 4 * C) * 1.5 + 0.2).to(td)
            d["bias"] = _randn(g, C) if o.get("bias") else None
        return d
    if e == "gate":
        B, nq, N, C, n = s["B"], s["nq"], s["N"], s["C"], o["n"]
        Qs = [_randn(g, B, nq, C) for _ in range(n)]
        Ks = [_randn(g, B, N, C) for _ in range(n)]
        if case.regime == "ties":
            M = 6.0
            for K in Ks:                            # per row: twice in one 8-element chunk / in two lanes / in every column / none
                K.clamp_(max=5.0)
                K[:, 0::4, 2 % C] = M; K[:, 0::4, 5 % C] = M
                K[:, 1::4, 3 % C] = M; K[:, 1::4, (8 * 5 + 3) % C] = M; K[:, 1::4, C - 1] = M
                K[:, 2::4, :] = M
            for Q in Qs:                            # per channel: the maximum at two queries / at every query / once
                Q.clamp_(max=5.0)
                Q[:, 1 % nq, 0::3] = M; Q[:, nq - 1, 0::3] = M
                Q[:, :, 1::3] = M
        d = dict(Qs=[t.to(td) for t in Qs], Ks=[t.to(td) for t in Ks], x=_randn(g, B, N, C).to(td),
                 douts=[_randn(g, B, N, C).to(td) for _ in range(n)], dx0=_randn(g, B, N, C).to(td),
                 dQ0s=[_randn(g, B, nq, C).to(td) for _ in range(n)], dK0s=[_randn(g, B, N, C).to(td) for _ in range(n)])
        return d
    if e == "act":
        rows, cols = s["rows"], s["cols"]
        aux = _randn(g, rows, cols) * 1.5
        if case.regime == "tails":
            aux = (torch.rand(rows, cols, generator=g, device=device) * 18.0 - 9.0)
        aux[0, :8] = 0.0                             # relu at exactly 0 (and -0.0): no gradient
        aux[0, 1] = -0.0
        return dict(dy=_randn(g, rows, cols).to(td), aux=aux.to(td))
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------ the case walker
def _exact(tag, got, want):
    assert torch.equal(got, want), f"{tag}: not bit-identical ({int((got != want).sum())} elements differ)"


def verify(case, impl, device, tag=None):
    """Runs table row ``case`` through ``impl`` (the kernels, or an honest fp32 implementation) and applies every bound and
    exact check.  ``impl`` methods take and return plain tensors; the kernel implementation wraps them in sentinel buffers."""
    tag = tag or case_id(case)
    dt, s, o, e = case.dtype, case.shape, case.opt, case.entry
    inp = inputs(case, device)
    if e == "ln":
        fw = impl.ln_fwd(case, inp["x"], inp["w"], inp["b"], LN_EPS, inp["pe"])
        outs = ln_fwd_ref(dt, inp["x"], inp["w"], inp["b"], LN_EPS, inp["pe"], given_y=fw["y"])
        check(tag, "ln", "layernorm_fwd" + ("_pe" if inp["pe"] is not None else ""), fw, outs)
        if case.regime == "const" and dt == "f32":      # variance exactly 0, mean exactly the value: y = 0 * rstd * w + b
            _exact(f"{tag} y == b on constant rows", fw["y"], inp["b"].expand_as(fw["y"]).contiguous())
        bw = impl.ln_bwd(case, inp["dy"], inp["dy2"], inp["x"], inp["w"], fw["mean"], fw["rstd"], inp["dres"])
        check(tag, "ln", "layernorm_bwd" + ("2" if inp["dy2"] is not None else ""), bw,
              ln_bwd_ref(dt, inp["dy"], inp["dy2"], inp["x"], inp["w"], inp["dres"], LN_EPS))
    elif e == "l2":
        fw = impl.l2_fwd(case, inp["x"])
        check(tag, "l2", "l2norm_fwd", fw, l2_fwd_ref(dt, inp["x"]))
        bw = impl.l2_bwd(case, inp["dy"], fw["y"], fw["inv"])
        check(tag, "l2", "l2norm_bwd", bw, l2_bwd_ref(dt, inp["dy"], fw["y"], fw["inv"]))
    elif e in ("colsum", "colsum_f32"):
        got = impl.colsum(case, inp["x"], inp["out0"], o["beta"])
        outs = colsum_ref(inp["x"], inp["out0"], o["beta"])
        check(tag, "colsum", e, got, outs)
        if case.regime == "int":
            _exact(f"{tag} integer sums", got["out"], outs["out"].ref.float())
    elif e == "gn":
        fw = impl.gn_fwd(case, inp["x"], inp["w"], inp["b"], GN_EPS, o["gelu"])
        check(tag, "gn", "groupnorm_fwd", fw, gn_fwd_ref(dt, inp["x"], inp["w"], inp["b"], GN_EPS, o["gelu"]))
        bw = impl.gn_bwd(case, inp["dy"], inp["x"], inp["w"], inp["b"], fw["mean"], fw["rstd"], o["gelu"])
        check(tag, "gn", "groupnorm_bwd", bw, gn_bwd_ref(dt, inp["dy"], inp["x"], inp["w"], inp["b"], GN_EPS, o["gelu"]))
    elif e == "psgn":
        fw = impl.psgn(case, inp["src"], inp["bias"], inp["w"], inp["b"], GN_EPS, o["gelu"])
        check(tag, "gn", "pixel_shuffle2_gn_stats", fw, pixel_shuffle2_ref(dt, inp["src"], inp["bias"], s["B"], s["h"], s["w"], s["C"]))
        check(tag, "gn", "groupnorm_apply", fw, gn_fwd_ref(dt, fw["y1"], inp["w"], inp["b"], GN_EPS, o["gelu"]))
    elif e == "gate":
        n = o["n"]
        fw = impl.gate_fwd(case, inp["Qs"], inp["Ks"], inp["x"])
        kn = "gate_n" if o["fused"] else "gate"
        for i in range(n):
            st, aq, ac = gate_stats_ref(inp["Qs"][i], inp["Ks"][i])
            check(f"{tag} gate {i}", "gate", kn + "_stats", dict(cg=fw["cg"][i], sg=fw["sg"][i]), st)
            _exact(f"{tag} gate {i} argq (lowest index among equal maxima)", fw["argq"][i].long(), aq)
            _exact(f"{tag} gate {i} argc (lowest index among equal maxima)", fw["argc"][i].long(), ac)
            check(f"{tag} gate {i}", "gate", kn + "_apply", dict(out=fw["outs"][i]), gate_apply_ref(dt, inp["x"], fw["cg"][i], fw["sg"][i]))
        bw = impl.gate_bwd(case, inp["douts"], inp["x"], fw["cg"], fw["argq"], fw["sg"], fw["argc"], inp["dx0"], o["accum"],
                           inp["dQ0s"], inp["dK0s"])
        outs, masks = gate_bwd_ref(dt, inp["douts"], inp["x"], fw["cg"], fw["argq"], fw["sg"], fw["argc"], inp["dx0"], o["accum"],
                                   inp["dQ0s"], inp["dK0s"])
        check(tag, "gate", kn + "_bwd", bw, outs)
        for i in range(n):                               # away from the arg-max: the bits dQ / dK came in with
            for nm, t0 in ((f"dQ{i}", inp["dQ0s"][i]), (f"dK{i}", inp["dK0s"][i])):
                away = ~masks[nm]
                _exact(f"{tag} {nm} away from the arg-max", bw[nm][away], t0[away])
    elif e == "act":
        got = impl.act_bwd(case, inp["dy"], inp["aux"], o["kind"])
        outs = act_bwd_ref(dt, inp["dy"], inp["aux"], o["kind"])
        check(tag, "act", "act_bwd_" + ("gelu" if o["kind"] else "relu"), got, outs)
        if o["kind"] == 0:
            _exact(f"{tag} relu", got["dz"], (inp["dy"].float() * (inp["aux"].float() > 0)).to(inp["dy"].dtype))
    else:
        raise ValueError(e)


def case_id(c):
    kv = lambda d: ",".join(f"{k}={v}" for k, v in d.items())
    return f"{c.entry}-{c.dtype}-{kv(c.shape)}" + (f"-{kv(c.opt)}" if c.opt else "") + f"-{c.regime}"
