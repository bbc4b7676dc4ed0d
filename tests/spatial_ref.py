"""Float64 references, per-element bounds, inputs and the case walker for the resize, head and layout kernels of csrc/spatial.hip.
Plain torch, importable without a GPU: tests/test_spatial_cases_cpu.py runs the walker over an honest fp32 implementation on the
CPU, tests/test_spatial_f64.py over the kernels.  The bound machinery (Guarded, O, _need / _within / check / any_fails, fl, REL,
COEF_MAX, STATS / summary) is that of tests/rowops_ref.py, imported.

Bounds.  Per element |got - ref| <= REL |ref| + c A, REL = 2^-8 for a bf16 result and 0 for an fp32 one, c one constant per family
(COEF).  An element with A = 0 must match exactly; no element is left out.

Resize (bilinear_cl_fwd / _bwd, upsum_relu: half-pixel centres; upsample_ac_fwd / _bwd: align-corners).  The reference takes the
EXACT source coordinate s (half-pixel: max(0, (d + 1/2) h / H - 1/2); align-corners: d (h - 1) / (H - 1), 0 when H == 1), i0 =
min(floor(s), h - 1), i1 = min(i0 + 1, h - 1), weights (1 - l, l) with l = s - i0, as one [H, h] matrix per axis; the forward is
My x Mx^T, the backward the explicit transpose My^T dout Mx, all in float64.  A = sum_taps |w_t| |v_t| plus a coordinate term:
the kernel forms s in fp32 with at most three roundings (the scale h / H, the product, the subtraction), each at most half an ulp
of a value no larger than max(1, s), so |s_fp32 - s| <= delta = 3 2^-24 max(1, s).  A tap weight is l or 1 - l and moves by at most
delta; where the floor flips at an integer s the weight that changes hands is ~0 (the interpolant is continuous in s), so the
result moves by at most delta sum_taps |v_t| per axis.  In units of the 2^-24 that c counts in, that is
3 max(1, s_y, s_x) sum_taps |v_t|, added to A (for the gathers: summed over the contributing outputs).  Both axes together move a
product weight by at most twice that; every c is at least 2^-23 = 2 x 2^-24, which covers the factor.  For power-of-two ratios the
fp32 coordinates are exact and the term is slack; one formula serves all cases.
  upsum_relu: relu(io0 + sum_i resize(z_i)), A = |io0| + sum_i A_i.
  Exact: regime "int" (integers in [-64, 64]), fp32, ratios 2 / 4 / 8 (align-corners: steps 1/2 and 1/4) -- every weight is a
  multiple of 2^-8 or coarser, every product and partial sum is an integer multiple of 2^-8 below 2^15, exact in fp32: bit-equal.

Head (convseg_fwd / _bwd, head_grad_fused), from the comments in spatial.hip:
  out = sum_c x w mask[b] + bias                                  A = sum_c |x w mask| + |bias|
  dx  = [x > 0 if accum & 2] (dout w mask + (dx0 if accum & 1))   A = |dout w mask| + |dx0|, 0 where the gate closes
  fused dx = [x > 0] (inv (dfn - y sum dfn y) + dout w mask)      A = inv (|dfn| + |y| sum |dfn y|) + |dout w mask|, 0 where closed
  dw = sum_rows dout x mask, db = sum dout                        A = the sums of absolute terms
  The kernels' partial rows (part / part_b) are summed in float64 by the caller.  The gate is decided on the bits of x.

Layout (window_permute, pixel_shuffle2, space_to_depth2_crop, pixel_unshuffle2_sums, patch_im2col[_prenorm|_floor]): bit for bit
against an index permutation, except pixel_shuffle2's bias (fp32: exactly fl32(v + b); bf16: REL), the normalised rgb columns of
patch_im2col (A = (|v| + mean) / std) and pixel_unshuffle2_sums' part (A = sum |src|)."""
import torch

import rowops_ref as rr
from rowops_ref import COEF_MAX, REL, STATS, Guarded, O, _need, _within, any_fails, check, fl, rel_of, summary, tdtype  # noqa: F401
from spatial_cases import bilinear_bwd_plan, patch_im2col_plan, upsum_plan

# c per family: the next power of two at or above 4 x the worst value measured on an MI355X (tests/test_spatial_f64.py lists the
# measurements); none above rowops_ref.COEF_MAX = 2^-17
COEF = {"rfwd": 2.0 ** -22, "rbwd": 2.0 ** -23, "head": 2.0 ** -20, "lsum": 2.0 ** -21}

F64 = torch.float64
IM_MEAN = (0.485, 0.456, 0.406)
IM_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------ resize
def resize_matrix(n_in, n_out, align, device, perturb=None, scale=None):
    """weights M [n_out, n_in], tap indicator T (same shape), source coordinate s [n_out], float64.  ``scale``: the half-pixel
    step n_in / n_out (given only by the swapped-axes perturbation)."""
    d = torch.arange(n_out, dtype=F64, device=device)
    if perturb == "align-swapped":
        align = not align
    if align:
        s = d * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros_like(d)
    elif scale is None:
        s = ((2 * d + 1) * n_in / (2 * n_out) - 0.5).clamp_min(0.0)
    else:
        s = ((d + 0.5) * scale - 0.5).clamp_min(0.0)
    if perturb == "half-pixel-off":
        s = s + 0.5
    i0 = s.floor().clamp_max(n_in - 1).long()
    l = s - i0
    i1 = i0 + 1
    inside = i1 <= n_in - 1
    if perturb != "no-clamp":                       # the second tap is the first at the border
        i1 = torch.where(inside, i1, i0)
        inside = torch.ones_like(inside)
    M = torch.zeros(n_out, n_in, dtype=F64, device=device)
    M.scatter_add_(1, i0[:, None], (1.0 - l)[:, None])
    M.scatter_add_(1, i1.clamp_max(n_in - 1)[:, None], (l * inside)[:, None])     # (unclamped and outside: the weight is lost)
    T = torch.zeros_like(M)
    T.scatter_(1, i0[:, None], 1.0)
    T.scatter_(1, i1.clamp_max(n_in - 1)[:, None], 1.0)
    return M, T, s


def _axes(h, w, H, W, align, device, perturb):
    if perturb == "swap-axes":                      # the row weights from the column step and the other way round
        My, Ty, sy = resize_matrix(h, H, align, device, scale=w / W)
        Mx, Tx, sx = resize_matrix(w, W, align, device, scale=h / H)
    else:
        My, Ty, sy = resize_matrix(h, H, align, device, perturb)
        Mx, Tx, sx = resize_matrix(w, W, align, device, perturb)
    smax = torch.maximum(sy[:, None], sx[None, :]).clamp_min(1.0)          # [H, W]
    return My, Ty, Mx, Tx, smax


def resize_fwd_ref(dt, x, H, W, align, perturb=None):
    """x [B, h, w, C] -> [B, H, W, C]"""
    B, h, w, C = x.shape
    My, Ty, Mx, Tx, smax = _axes(h, w, H, W, align, x.device, perturb)
    X = x.double()
    ref = torch.einsum("Yy,byxc,Xx->bYXc", My, X, Mx)
    if perturb is not None:
        return O(ref, None, rel_of(dt))
    A = torch.einsum("Yy,byxc,Xx->bYXc", My.abs(), X.abs(), Mx.abs()) + 3.0 * smax[None, :, :, None] * torch.einsum(
        "Yy,byxc,Xx->bYXc", Ty, X.abs(), Tx)
    return O(ref, A, rel_of(dt))


def resize_bwd_ref(dt, dout, h, w, align, perturb=None):
    """dout [B, H, W, C] -> [B, h, w, C]: the transpose of the forward's matrix"""
    B, H, W, C = dout.shape
    if perturb == "untransposed":                   # the gradient resized down with the forward's rule instead of gathered
        return resize_fwd_ref(dt, dout, h, w, align, perturb="none")
    My, Ty, Mx, Tx, smax = _axes(h, w, H, W, align, dout.device, perturb)
    D = dout.double()
    ref = torch.einsum("Yy,bYXc,Xx->byxc", My, D, Mx)
    if perturb is not None:
        return O(ref, None, rel_of(dt))
    A = torch.einsum("Yy,bYXc,Xx->byxc", My.abs(), D.abs(), Mx.abs()) + 3.0 * torch.einsum(
        "Yy,bYXc,Xx->byxc", Ty, smax[None, :, :, None] * D.abs(), Tx)
    return O(ref, A, rel_of(dt))


def upsum_ref(dt, io0, zs, perturb=None):
    """io0 [B, H, W, C], zs: list of [B, h_i, w_i, C]"""
    B, H, W, C = io0.shape
    s, A = io0.double().clone(), io0.double().abs()
    for i, z in enumerate(zs):
        if perturb == "drop-map" and i == len(zs) - 1:
            continue
        o = resize_fwd_ref(dt, z, H, W, False)
        s, A = s + o.ref, A + o.A
    return O(s if perturb == "no-relu" else s.clamp_min(0.0), A, rel_of(dt))


# ------------------------------------------------------------------------------------------------ head
def _mask_rows(mask, rows, HW, C, device, perturb=None):
    if mask is None:
        return torch.ones(rows, C, dtype=F64, device=device)
    b = torch.arange(rows, device=device) // HW
    if perturb == "mask-row-0":
        b = torch.zeros_like(b)
    return mask.double()[b]


def convseg_fwd_ref(x, w, bias, mask, HW, perturb=None):
    rows, C = x.shape
    t = x.double() * w.double() * _mask_rows(mask, rows, HW, C, x.device, perturb)
    ta = x.double().abs() * w.double().abs() * _mask_rows(mask, rows, HW, C, x.device).abs()
    b = bias.double()[0]
    return dict(out=O(t.sum(1) + (0.0 if perturb == "no-bias" else b), ta.sum(1) + b.abs()))


def _gate(X, perturb):
    return (X >= 0) if perturb == "x>=0" else (X > 0)


def convseg_bwd_ref(dt, dout, x, w, mask, dx0, accum, HW, perturb=None):
    rows, C = x.shape
    X, D, Wv = x.double(), dout.double()[:, None], w.double()
    M, M0 = _mask_rows(mask, rows, HW, C, x.device, perturb), _mask_rows(mask, rows, HW, C, x.device)
    t, A = D * Wv * M, (D * Wv * M0).abs()
    if accum & 1:
        A = A + dx0.double().abs()
        if perturb != "accum0-ignored":
            t = t + dx0.double()
    if accum & 2:
        t, A = t * _gate(X, perturb), A * (X > 0)
    return dict(dx=O(t, A, rel_of(dt)), dw=O((D * X * M).sum(0), (D * X * M0).abs().sum(0)),
                db=O(D.sum().reshape(1), D.abs().sum().reshape(1)))


def head_grad_fused_ref(dt, dfn, y, inv, dout, x, w, mask, HW, perturb=None):
    rows, C = x.shape
    X, D, Wv, G, Y, I = x.double(), dout.double()[:, None], w.double(), dfn.double(), y.double(), inv.double()[:, None]
    M, M0 = _mask_rows(mask, rows, HW, C, x.device, perturb), _mask_rows(mask, rows, HW, C, x.device)
    s = G.sum(1, keepdim=True) if perturb == "sum-without-y" else (G * Y).sum(1, keepdim=True)
    n = (G - Y * s) * (1.0 if perturb == "no-inv" else I)
    t = (n + D * Wv * M) * _gate(X, perturb)
    A = (I * (G.abs() + Y.abs() * (G * Y).abs().sum(1, keepdim=True)) + (D * Wv * M0).abs()) * (X > 0)
    return dict(dx=O(t, A, rel_of(dt)), dw=O((D * X * M).sum(0), (D * X * M0).abs().sum(0)),
                db=O(D.sum().reshape(1), D.abs().sum().reshape(1)))


# ------------------------------------------------------------------------------------------------ layout
def winperm_ref(x, g, wg, to_raster, perturb=None):
    """x [B, g g, C]; raster -> window order, or back"""
    B, _, C = x.shape
    nw = g // wg
    if to_raster:
        y = x.view(B, nw, nw, wg, wg, C).permute(0, 1, 3, 2, 4, 5).reshape(B, g * g, C)
        return y.view(B, g, g, C).transpose(1, 2).reshape(B, g * g, C) if perturb == "ty-tx-swapped" else y
    if perturb == "ty-tx-swapped":
        x = x.view(B, g, g, C).transpose(1, 2).reshape(B, g * g, C)
    return x.view(B, nw, wg, nw, wg, C).permute(0, 1, 3, 2, 4, 5).reshape(B, g * g, C)


def ps2_fwd_perm(src, B, h, w, C, perturb=None):
    """src [B h w, 4 C] (column c 4 + di 2 + dj) -> [B, 2h, 2w, C]"""
    v = src.view(B, h, w, C, 2, 2)
    v = v.permute(0, 1, 5, 2, 4, 3) if perturb == "dj-di" else v.permute(0, 1, 4, 2, 5, 3)
    return v.reshape(B, 2 * h, 2 * w, C)


def ps2_inv_perm(x, B, h, w, C):
    """x [B, 2h, 2w, C] -> [B h w, 4 C]"""
    return x.view(B, h, 2, w, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B * h * w, 4 * C)


def ps2_fwd_ref(dt, src, bias, B, h, w, C, perturb=None):
    S = ps2_fwd_perm(src, B, h, w, C, perturb).double()
    if bias is None or perturb == "no-bias":
        return O(S, torch.zeros_like(S))
    v = S + bias.double()
    return O(fl(v, "f32") if dt == "f32" else v, torch.zeros_like(v), rel_of(dt))      # fp32: one correctly rounded add


def s2d_fwd_ref(x, B, g, C):
    h = g // 2
    return ps2_inv_perm(x.view(B, g, g, C)[:, :2 * h, :2 * h].contiguous(), B, h, h, C)


def s2d_inv_ref(s, B, g, C, perturb=None):
    h = g // 2
    out = torch.full((B, g, g, C), float("nan") if perturb == "border-unwritten" else 0.0, dtype=s.dtype, device=s.device)
    out[:, :2 * h, :2 * h] = ps2_fwd_perm(s, B, h, h, C)
    return out


def unsh_ref(src, B, h, w, C):
    S = src.double().view(-1, C)
    return ps2_inv_perm(src.view(B, 2 * h, 2 * w, C), B, h, w, C), O(S.sum(0), S.abs().sum(0))


def im2col_ref(dt, img4, disks, P, wg, prenorm, perturb=None):
    """img4 [B, 4, H, W], disks [B, 2, H, W] fp32 -> cols [B T, 2 K3P] in window token order; the bound as O with a per-element rel"""
    B, _, H, W = img4.shape
    p = patch_im2col_plan(H, W, P)
    gh, gw, K3, K3P = p["gh"], p["gw"], p["K3"], p["K3P"]
    dev = img4.device
    mean = torch.tensor(IM_MEAN, dtype=torch.float32, device=dev).double().view(1, 3, 1, 1)
    std = torch.tensor(IM_STD, dtype=torch.float32, device=dev).double().view(1, 3, 1, 1)
    if perturb == "wrong-channel":
        mean, std = mean.roll(1, 1), std.roll(1, 1)
    rgb = img4[:, :3].double()
    norm = not prenorm
    full = torch.cat([(rgb - mean) / std if norm else rgb, img4[:, 3:].double(), disks.double()], 1)
    Afull = torch.cat([(rgb.abs() + mean) / std if norm else torch.zeros_like(rgb), torch.zeros_like(img4[:, 3:].double()),
                       torch.zeros_like(disks.double())], 1)
    isn = torch.cat([torch.full_like(rgb, 1.0 if norm else 0.0), torch.zeros_like(img4[:, 3:].double()), torch.zeros_like(disks.double())], 1)

    def cols(t):
        t = t[:, :, :gh * P, :gw * P].reshape(B, 6, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B, gh, gw, 2, K3)
        t = torch.cat([t, torch.zeros(B, gh, gw, 2, K3P - K3, dtype=t.dtype, device=dev)], 4).reshape(B, gh, gw, 2 * K3P)
        return t.view(B, gh // wg, wg, gw // wg, wg, 2 * K3P).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, 2 * K3P)

    ref, A, n = cols(full), cols(Afull), cols(isn)
    ref = torch.where(n > 0, ref, fl(ref, dt))            # copies: the value rounded to the output type, exactly
    return O(ref, A, n * rel_of(dt))


# ------------------------------------------------------------------------------------------------ inputs
def _ints(g, *shape):
    return torch.randint(-64, 65, shape, generator=g, device=g.device).float()


def _relu_plant(x):
    """exact +0, -0 and +-tiny values among the ordinary ones (x: fp32, before the cast)"""
    f = x.view(-1)
    f[0::7] = 0.0
    f[1::7] = -0.0
    f[2::11] = 1e-30
    f[3::11] = -1e-30
    return x


def _mask0(B, C, device):
    """Dropout2d(0.1): whole channels at 0, the rest at 1 / 0.9 (fp32); a different set per image"""
    b, c = torch.arange(B, device=device)[:, None], torch.arange(C, device=device)[None, :]
    keep = ((c * 7 + b * 3) % 5 != 0).float()
    return keep * torch.tensor(1.0 / 0.9, dtype=torch.float32, device=device)


def inputs(case, device):
    g = rr._gen(case, device)
    td = tdtype(case.dtype)
    s, o, e = case.shape, case.opt, case.entry
    draw = _ints if case.regime == "int" else (lambda gg, *sh: rr._randn(gg, *sh))
    if e in ("bil_fwd", "bil_bwd"):
        B, h, w, H, W, C = (s[k] for k in ("B", "h", "w", "H", "W", "C"))
        return dict(x=draw(g, B, h, w, C).to(td), dout=draw(g, B, H, W, C).to(td))
    if e == "upsum":
        B, H, W, C = (s[k] for k in ("B", "H", "W", "C"))
        io0 = draw(g, B, H, W, C)
        if case.regime == "relu":
            io0 = _relu_plant(io0)
        return dict(io0=io0.to(td), zs=[draw(g, B, h, w, C).to(td) for h, w in o["maps"]])
    if e == "ac":
        return dict(x=draw(g, s["planes"], s["h"], s["w"]), dout=draw(g, s["planes"], s["H"], s["W"]))
    if e in ("cs_fwd", "cs_bwd", "hgf"):
        rows, HW, C = s["rows"], s["HW"], s["C"]
        B = -(-rows // HW)
        x = rr._randn(g, rows, C)
        if case.regime == "relu":
            x = _relu_plant(x)
        d = dict(x=x.to(td), w=rr._randn(g, C) * 0.2, bias=rr._randn(g, 1), dout=rr._randn(g, rows),
                 dx0=rr._randn(g, rows, C).to(td), mask=_mask0(B, C, device) if o.get("mask") else None)
        if e == "hgf":
            u = rr._randn(g, rows, C)
            nrm = u.double().norm(dim=1, keepdim=True)
            d["y"] = (u.double() / nrm).to(torch.bfloat16)
            d["inv"] = (1.0 / nrm[:, 0]).float()
            d["dfn"] = rr._randn(g, rows, C).to(td)
        return d
    if e == "winperm":
        if s["C"] > 4096:                                   # the large row: cheap distinct values, no normal draw of 33 M elements
            n = s["B"] * s["g"] * s["g"] * s["C"]
            return dict(x=(torch.arange(n, device=device, dtype=torch.int32) % 251 - 125).to(td).view(s["B"], s["g"] * s["g"], s["C"]))
        return dict(x=rr._randn(g, s["B"], s["g"] * s["g"], s["C"]).to(td))
    if e == "ps2":
        B, h, w, C = (s[k] for k in ("B", "h", "w", "C"))
        return dict(src=rr._randn(g, B * h * w, 4 * C).to(td), x=rr._randn(g, B, 2 * h, 2 * w, C).to(td),
                    bias=rr._randn(g, C) if o.get("bias") else None)
    if e == "s2d":
        B, gg, C = s["B"], s["g"], s["C"]
        return dict(x=rr._randn(g, B, gg, gg, C).to(td), s=rr._randn(g, B * (gg // 2) ** 2, 4 * C).to(td))
    if e == "unsh":
        B, h, w, C = (s[k] for k in ("B", "h", "w", "C"))
        return dict(src=draw(g, B, 2 * h, 2 * w, C).to(td))
    if e == "im2col":
        B, H, W = s["B"], s["H"], s["W"]
        return dict(img4=rr._randn(g, B, 4, H, W).abs(), disks=(rr._randn(g, B, 2, H, W) > 0.9).float())
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------ the case walker
_exact = rr._exact


def verify(case, impl, device, tag=None):
    """Runs table row ``case`` through ``impl`` (the kernels, or an honest fp32 implementation) and applies every bound and
    exact check.  ``impl`` methods take and return plain tensors; the kernel implementation wraps them in sentinel buffers."""
    tag = tag or case_id(case)
    dt, s, o, e = case.dtype, case.shape, case.opt, case.entry
    td = tdtype(dt)
    inp = inputs(case, device)
    exact = case.regime == "int" and dt == "f32"
    if o.get("raises"):
        impl.rejects(case, inp)
        return
    if e == "bil_fwd":
        got = impl.bil_fwd(case, inp["x"])
        ref = resize_fwd_ref(dt, inp["x"], s["H"], s["W"], False)
        check(tag, "rfwd", "bilinear_cl_fwd", dict(out=got), dict(out=ref), COEF["rfwd"])
        if exact:
            _exact(f"{tag} integer data", got, ref.ref.float())
    elif e == "bil_bwd":
        form = bilinear_bwd_plan(s["B"], s["h"], s["w"], s["H"], s["W"], s["C"])["form"]
        got = impl.bil_bwd(case, inp["dout"])
        ref = resize_bwd_ref(dt, inp["dout"], s["h"], s["w"], False)
        check(tag, "rbwd", "bilinear_cl_bwd_" + form, dict(din=got), dict(din=ref), COEF["rbwd"])
        if exact:
            _exact(f"{tag} integer data", got, ref.ref.float())
    elif e == "upsum":
        quad = upsum_plan(s["H"], s["W"], o["maps"])["quad"]
        got = impl.upsum(case, inp["io0"], inp["zs"])
        ref = upsum_ref(dt, inp["io0"], inp["zs"])
        check(tag, "rfwd", "upsum_relu" + ("2" if quad else ""), dict(io=got), dict(io=ref), COEF["rfwd"])
        if exact:
            _exact(f"{tag} integer data", got, ref.ref.float())
    elif e == "ac":
        got = impl.ac_fwd(case, inp["x"])
        ref = resize_fwd_ref(dt, inp["x"][..., None], s["H"], s["W"], True)
        check(tag, "rfwd", "upsample_ac_fwd", dict(out=got[..., None]), dict(out=ref), COEF["rfwd"])
        gb = impl.ac_bwd(case, inp["dout"])
        rb = resize_bwd_ref(dt, inp["dout"][..., None], s["h"], s["w"], True)
        check(tag, "rbwd", "upsample_ac_bwd", dict(din=gb[..., None]), dict(din=rb), COEF["rbwd"])
        if exact:
            _exact(f"{tag} integer data, forward", got, ref.ref.float()[..., 0])
            _exact(f"{tag} integer data, backward", gb, rb.ref.float()[..., 0])
    elif e == "cs_fwd":
        got = impl.cs_fwd(case, inp["x"], inp["w"], inp["bias"], inp["mask"])
        check(tag, "head", "convseg_fwd", dict(out=got), convseg_fwd_ref(inp["x"], inp["w"], inp["bias"], inp["mask"], s["HW"]), COEF["head"])
    elif e == "cs_bwd":
        got = impl.cs_bwd(case, inp["dout"], inp["x"], inp["w"], inp["mask"], inp["dx0"], o["accum"])
        ref = convseg_bwd_ref(dt, inp["dout"], inp["x"], inp["w"], inp["mask"], inp["dx0"], o["accum"], s["HW"])
        check(tag, "head", "convseg_bwd", got, ref, COEF["head"])
        if o["accum"] & 2:
            closed = ~(inp["x"].float() > 0)
            assert bool((got["dx"][closed] == 0).all()), f"{tag}: gradient where x <= 0"
    elif e == "hgf":
        got = impl.hgf(case, inp["dfn"], inp["y"], inp["inv"], inp["dout"], inp["x"], inp["w"], inp["mask"])
        ref = head_grad_fused_ref(dt, inp["dfn"], inp["y"], inp["inv"], inp["dout"], inp["x"], inp["w"], inp["mask"], s["HW"])
        check(tag, "head", "head_grad_fused", got, ref, COEF["head"])
        closed = ~(inp["x"].float() > 0)
        assert bool((got["dx"][closed] == 0).all()), f"{tag}: gradient where x <= 0"
    elif e == "winperm":
        g, wg = s["g"], s["wg"]
        yw = impl.winperm(case, inp["x"], False)
        _exact(f"{tag} to window order", yw, winperm_ref(inp["x"], g, wg, False))
        _exact(f"{tag} to raster order", impl.winperm(case, inp["x"], True), winperm_ref(inp["x"], g, wg, True))
        _exact(f"{tag} round trip", impl.winperm(case, yw, True), inp["x"])
    elif e == "ps2":
        B, h, w, C = (s[k] for k in ("B", "h", "w", "C"))
        got = impl.ps2(case, inp["src"], inp["bias"], False)
        ref = ps2_fwd_ref(dt, inp["src"], inp["bias"], B, h, w, C)
        check(tag, "lsum", "pixel_shuffle2", dict(out=got), dict(out=ref), COEF["lsum"])
        if inp["bias"] is None or dt == "f32":
            _exact(f"{tag} forward", got, ref.ref.to(td))
        _exact(f"{tag} inverse", impl.ps2(case, inp["x"], None, True), ps2_inv_perm(inp["x"], B, h, w, C))
    elif e == "s2d":
        B, g, C = s["B"], s["g"], s["C"]
        _exact(f"{tag} forward", impl.s2d(case, inp["x"], False), s2d_fwd_ref(inp["x"], B, g, C))
        _exact(f"{tag} inverse (zeros in the dropped row and column)", impl.s2d(case, inp["s"], True), s2d_inv_ref(inp["s"], B, g, C))
    elif e == "unsh":
        B, h, w, C = (s[k] for k in ("B", "h", "w", "C"))
        dst, sums = impl.unsh(case, inp["src"])
        rd, rs = unsh_ref(inp["src"], B, h, w, C)
        _exact(f"{tag} dst", dst, rd)
        check(tag, "lsum", "pixel_unshuffle2_sums", dict(sums=sums), dict(sums=rs), COEF["lsum"])
        if case.regime == "int":
            _exact(f"{tag} integer sums", sums, rs.ref)
    elif e == "im2col":
        got = impl.im2col(case, inp["img4"], inp["disks"])
        ref = im2col_ref(dt, inp["img4"], inp["disks"], s["P"], o["wg"], o["prenorm"])
        kn = "patch_im2col" + ("_floor" if o["floor"] else "") + ("_prenorm" if o["prenorm"] else "")
        check(tag, "lsum", kn, dict(cols=got), dict(cols=ref), COEF["lsum"])
        p = patch_im2col_plan(s["H"], s["W"], s["P"])
        if p["pad"]:
            pad = torch.cat([got[:, p["K3"]:p["K3P"]], got[:, p["K3P"] + p["K3"]:]], 1)
            assert bool((pad == 0).all()), f"{tag}: pad columns not 0"
    else:
        raise ValueError(e)


def case_id(c):
    kv = lambda d: ",".join(f"{k}={v}" for k, v in d.items())
    return f"{c.entry}-{c.dtype}-{kv(c.shape)}" + (f"-{kv(c.opt)}" if c.opt else "") + f"-{c.regime}"
