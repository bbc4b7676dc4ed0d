"""Inputs and float64 references for the rows of tests/tail_cases.py, on the CPU, sharing nothing with the kernels; every
reference takes ``plant``, the name of one error to plant (tests/test_tail_cases_cpu.py proves that the bounds tell each of them).

Bounds (tests/test_tail_f64.py asserts them, ``worst`` below measures them):
  loss sums                     |got - ref| <= 1e-5 |ref|                         (test_losses_gpu.py)
  loss gradients                |got - ref| <= 3e-5 A_i, A_i the float64 sum of the absolute contributions
  saturated planes, sums        + 2e-7 per pixel
  NFL / Dice gradient           + 1e-6 max A
  Adam                          see adam_bounds

Inputs that keep these bounds meaningful: low-resolution probabilities in [0.02, 0.98] except on saturated planes; NFL logits at
most 5 on the wrong side of a 0 / 1 label (pt = 1 - |t - p| holds 2^-24 absolute in fp32 whatever a kernel does: at 5, pt >= 6.7e-3
keeps 9e-6 relative, under the gradient bound; test_losses_gpu.py goes to 6 where the sums average); in the Adam rows the terms
of m' share the sign of g (p too where the decay is coupled), so that |upd_ref| carries the relative error of m' and no sum of
absolute terms is needed in the bound of p'."""
import zlib

import numpy as np
import torch

from tail_cases import NFL_NBLK, anchors, case_id, nfl_plan, p2cl_band, seg_layout

F64 = torch.float64
U = 2.0 ** -24
LOSS_COEF, GRAD_COEF, SAT_PIXEL, NFL_GRAD_ABS = 1e-5, 3e-5, 2e-7, 1e-6
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 5e-5


def rng(c):
    return np.random.RandomState(zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF)


def worst(got, ref, scale, atol=0.0):
    """the smallest coefficient c with |got - ref| <= c * scale + atol everywhere (inf where scale is 0 and they differ, or
    where got is not finite)"""
    got, ref, scale = (torch.as_tensor(t).to(F64) for t in (got, ref, scale))
    over = ((got - ref).abs() - atol).clamp_min(0.0)
    need = torch.where(scale > 0, over / scale.clamp_min(1e-300), torch.where(over > 0, float("inf"), 0.0))
    need = torch.where(torch.isfinite(got), need, torch.full_like(need, float("inf")))
    return float(need.max()) if need.numel() else 0.0


# ------------------------------------------------------------------------------------------------ P2CL
def interp_matrix(n, N, plant=None):
    """[N, n] float64 align_corners=True weights at the fp32 sampling positions (test_losses_gpu._interp_matrix), and the anchors"""
    i0n, s = anchors(n, N)
    t = torch.from_numpy((s * np.arange(N, dtype=np.float32)).astype(np.float64))
    i0 = torch.from_numpy(i0n)
    l1 = t - i0.to(F64)
    i1 = (i0 + 1).clamp_max(n - 2 if plant == "last_col_clamp" else n - 1)
    M = torch.zeros(N, n, dtype=F64)
    Y = torch.arange(N)
    M.index_put_((Y, i0), 1.0 - l1, accumulate=True)
    M.index_put_((Y, i1), l1, accumulate=True)
    return M, i0


def _labels(r, n, H, W, regime):
    lab = (r.rand(n, H, W) > 0.5).astype(np.float32)
    if regime == "soft_ignore":
        k = r.rand(n, H, W)
        lab[(lab == 0) & (k > 0.9)] = -0.0
        lab[k < 0.2] = 0.3
        lab[(k >= 0.2) & (k < 0.4)] = -1.0
    return lab


def p2_inputs(c):
    """low [B, S, h, w], gt [B, H, W], override [4, H, W] or None, slot index [B, S] int32 or None.  Regime "saturated": planes
    of exactly 0 or 1 against labels that match on the left half and oppose on the right."""
    s, r = c.shape, rng(c)
    B, S = s["B"], s["S"]
    if c.entry == "p2cl":
        h, w, H, W = 1, s["HW"], 1, s["HW"]
    else:
        h, w, H, W = s["h"], s["w"], s["H"], s["W"]
    low = (r.rand(B, S, h, w) * 0.96 + 0.02).astype(np.float32)
    gt = _labels(r, B, H, W, c.regime)
    if c.regime == "saturated":
        low[:] = 0.0
        low[:, 0::2] = 1.0
    ov = idx = None
    if c.opt["slots"]:
        ov = _labels(r, 4, H, W, c.regime)
        idx = -np.ones((B, S), np.int32)
        if c.opt["slots"] == "consecutive":          # planes 10, 11 (slot, then none at 12) and the last positive / first inverted
            idx[0, 10], idx[0, 11], idx[B - 1, S // 2 - 1], idx[B - 1, S // 2] = 0, 1, 2, 3
        else:
            idx[0, 0], idx[0, S - 1], idx[B - 1, S // 2 - 1], idx[B - 1, S // 2] = 0, 1, 2, 3
    return dict(low=low, gt=gt, ov=ov, idx=idx, gs=2.0 / (B * S * H * W))


def p2_labels(gt, idx, ov, S, plant=None):
    """[B, S, H, W] float64 labels and validity: the ground truth, logical_not of it in the second half of the slots (always
    valid: a -1 there is label 0), an override mask passed through where the slot index names one"""
    g = torch.from_numpy(gt).to(F64)
    pos = g[:, None].expand(-1, S // 2, -1, -1)
    inv = (g == 0).to(F64)[:, None].expand(-1, S // 2, -1, -1)
    lab = torch.cat([pos, inv], 1).clone()
    valid = torch.cat([pos != -1, torch.ones_like(inv, dtype=torch.bool) if plant != "ignore_inverted" else pos != -1], 1).clone()
    if idx is not None:
        for b, s in zip(*np.nonzero(idx >= 0)):
            o = torch.from_numpy(ov[idx[b, s]]).to(F64)
            lab[b, s], valid[b, s] = o, o != -1
    y = torch.where(valid, lab, torch.zeros_like(lab))
    if plant == "soft_as_one":
        y = (y != 0).to(F64)
    return y, valid


def p2_ref(inp, h, w, H, W, band=None, plant=None):
    """float64 P2CL of the upsampled planes: loss sums per (plane, band of ``band`` anchor rows; per plane if None), d loss / d low,
    A = the backward of the absolute contributions, npx = pixels per band.  h == H == 1 and w == W (the "p2cl" entry): the planes
    are the probabilities themselves, nothing is interpolated."""
    low = torch.from_numpy(inp["low"]).to(F64)
    B, S = low.shape[:2]
    gs = inp["gs"]
    e = 0.0 if plant == "no_eps" else 1e-12
    My, ay = interp_matrix(h, H)
    if h == H == 1 and w == W:
        back = lambda d: d
        up = low
    else:
        Mx, _ = interp_matrix(w, W, plant)
        back = lambda d: My.t() @ d @ Mx
        up = My @ low @ Mx.t()
    y, valid = p2_labels(inp["gt"], inp["idx"], inp["ov"], S, plant)
    v = valid.to(F64)
    loss = torch.where(valid, -(torch.log(up + e) * y + torch.log(1.0 - up + e) * (1.0 - y)), 0.0)
    dprob = gs * v * (-(y / (up + e)) + (1.0 - y) / (1.0 - up + e))
    absd = gs * v * (y.abs() / (up + e) + (1.0 - y).abs() / (1.0 - up + e))
    if plant in ("row5", "row6"):                      # the pixel rows of a cell beyond the first 4 / 5 are never walked
        first = torch.from_numpy(np.searchsorted(ay.numpy(), ay.numpy(), side="left"))
        dead = (torch.arange(H) - first) >= (4 if plant == "row5" else 5)
        loss, dprob = loss * ~dead[:, None], dprob * ~dead[:, None]
    nb = 1 if band is None else (h + band - 1) // band
    bidx = torch.zeros(H, dtype=torch.long) if band is None else ay // band
    bands = torch.zeros(B, S, nb, dtype=F64).index_add_(2, bidx, loss.sum(-1))
    dlow = back(dprob)
    if band is not None and plant in ("halo_lower_dropped", "halo_counted"):
        halo = ((ay + 1) % band == 0) & (ay + 1 < h)       # rows anchored at r0 - 1 of a band that is not the first
        if plant == "halo_counted":
            bands.index_add_(2, (ay[halo] + 1) // band, loss[:, :, halo].sum(-1))
        else:
            lower, hi = torch.zeros_like(My), halo.nonzero().flatten()
            lower[hi, ay[hi] + 1] = My[hi, ay[hi] + 1]
            dlow = dlow - back(dprob) + (My - lower).t() @ dprob @ Mx
    return dict(bands=bands, dlow=dlow, A=back(absd), dprob=dprob, absd=absd,
                npx=torch.bincount(bidx, minlength=nb).to(F64) * W, applies=_p2_applies(inp, h, w, H, band, plant, ay))


def _p2_applies(inp, h, w, H, band, plant, ay):
    """whether the planted error can show on this row at all"""
    if plant in ("ignore_inverted", "soft_as_one"):
        return bool((inp["gt"] == -1).any() if plant == "ignore_inverted" else ((inp["gt"] > 0) & (inp["gt"] < 1)).any())
    if plant == "no_eps":
        return bool(((inp["low"] == 0) | (inp["low"] == 1)).any())
    if plant in ("halo_lower_dropped", "halo_counted"):
        return band is not None and h > band
    if plant in ("row5", "row6"):
        return int(np.bincount(ay.numpy()).max()) > (4 if plant == "row5" else 5)
    return True


def p2_pixel_loop(inp, h, w, H, W):
    """the dumber reference: a loop over planes and pixels in Python floats, for maps of a few cells"""
    low, gs = inp["low"].astype(np.float64), inp["gs"]
    B, S = low.shape[:2]
    y, valid = p2_labels(inp["gt"], inp["idx"], inp["ov"], S)
    sh = float(np.float32(h - 1) / np.float32(H - 1)) if H > 1 else 0.0
    sw = float(np.float32(w - 1) / np.float32(W - 1)) if W > 1 else 0.0
    sums, dlow = np.zeros((B, S, h)), np.zeros_like(low)
    for b in range(B):
        for s in range(S):
            for Y in range(H):
                ty = float(np.float32(sh) * np.float32(Y))
                y0 = min(int(ty), h - 1)
                y1, ly = min(y0 + 1, h - 1), ty - y0
                for X in range(W):
                    tx = float(np.float32(sw) * np.float32(X))
                    x0 = min(int(tx), w - 1)
                    x1, lx = min(x0 + 1, w - 1), tx - x0
                    p = (1 - ly) * ((1 - lx) * low[b, s, y0, x0] + lx * low[b, s, y0, x1]) + ly * ((1 - lx) * low[b, s, y1, x0] + lx * low[b, s, y1, x1])
                    if not valid[b, s, Y, X]:
                        continue
                    t = float(y[b, s, Y, X])
                    sums[b, s, y0] += -(np.log(p + 1e-12) * t + np.log(1 - p + 1e-12) * (1 - t))
                    g = gs * (-(t / (p + 1e-12)) + (1 - t) / (1 - p + 1e-12))
                    dlow[b, s, y0, x0] += g * (1 - ly) * (1 - lx)
                    dlow[b, s, y0, x1] += g * (1 - ly) * lx
                    dlow[b, s, y1, x0] += g * ly * (1 - lx)
                    dlow[b, s, y1, x1] += g * ly * lx
    return torch.from_numpy(sums), torch.from_numpy(dlow)


def p2_worst(got_bands, got_dlow, ref, saturated):
    """(ratio of the band sums to their bound's coefficient 1e-5, the same of the gradient to 3e-5), each <= 1 when in bound"""
    scale = ref["bands"].abs() + (SAT_PIXEL * ref["npx"].view(1, 1, -1) if saturated else 0.0)
    a = worst(got_bands.reshape(ref["bands"].shape), ref["bands"], scale) / LOSS_COEF
    b = 0.0 if got_dlow is None else worst(got_dlow, ref["dlow"], ref["A"]) / GRAD_COEF
    return a, b


# ------------------------------------------------------------------------------------------------ NFL + Dice
def nfl_inputs(c):
    """logits and labels [B, HW].  "mixed": 0 / 1 labels with soft (0.3), ignore (-1) and -0.0 pixels, logits N(0, 3) clamped to
    +-20; "one_ignored": the same with every label of sample B // 2 (sample 0 of a batch of one) ignored; "all0" / "all1";
    "pm20": every logit +20 or -20.  A logit on the wrong side of a 0 / 1 label stops at 5 (module docstring)."""
    s, r = c.shape, rng(c)
    B, HW = s["B"], s["HW"]
    t = (r.rand(B, HW) > 0.5).astype(np.float32)
    k = r.rand(B, HW)
    if c.regime in ("mixed", "one_ignored", "pm20"):
        t[k < 0.1] = 0.3
        t[(k >= 0.1) & (k < 0.2)] = -1.0
        t[(t == 0) & (k > 0.9)] = -0.0
        t[:, :4] = np.array([1.0, 0.0, 0.3, -1.0], np.float32)
    if c.regime == "one_ignored":
        t[B // 2] = -1.0
    if c.regime in ("all0", "all1"):
        t[:] = float(c.regime == "all1")
    x = np.clip(r.randn(B, HW) * 3.0, -20.0, 20.0).astype(np.float32)
    if c.regime == "pm20":
        x = np.where(r.rand(B, HW) > 0.5, 20.0, -20.0).astype(np.float32)
    x = np.where(t == 0, np.minimum(x, 5.0), x)
    x = np.where(t == 1, np.maximum(x, -5.0), x).astype(np.float32)
    return dict(logits=x, gt=t, w_nfl=1.0 / B, w_dice=0.7 / B)


def nfl_ref(inp, plant=None):
    """float64 per-sample NFL and Dice (losses.py:11-89, 227-363), d (w_nfl sum NFL + w_dice sum Dice) / d logits and its A
    (|NFL part| + |Dice part|)"""
    x = torch.from_numpy(inp["logits"]).to(F64).requires_grad_(True)
    t = torch.from_numpy(inp["gt"]).to(F64)
    HW = x.shape[1]
    w = (t != -1).to(F64)
    p = torch.sigmoid(x)
    pt = torch.where(w > 0, 1.0 - (t - p).abs(), torch.ones_like(p))
    beta = (1.0 - pt) ** 2
    # (sum w itself cancels between mult and the size average, up to the 1e-12 terms: an error in it alone changes nothing.  What
    # a sums pass that takes an ignore pixel for a valid one gets wrong is sum beta, with pt = 1 - |-1 - p|.)
    ws = torch.ones_like(w) if plant == "ignore_counted" else w
    sw = ws.sum(1, keepdim=True)
    bsum = torch.where(ws > 0, (t - p).abs() ** 2, torch.zeros_like(p)).sum(1, keepdim=True)
    stale = 0.25 * nfl_plan(HW)["empty"] if plant == "stale_chunk" else 0.0      # every empty chunk block adds what was there before
    sw, bsum = sw + stale, bsum + stale
    mult = sw / (bsum + 1e-12)
    if plant != "mult_attached":
        mult = mult.detach()
    nfl = (-0.5 * w * beta * mult * torch.log((pt + 1e-12).clamp_max(1.0)) * w).sum(1) / (sw[:, 0] + 1e-12)
    de = 0.0 if plant == "dice_eps_dropped" else 1e-3
    dice = 1.0 - (2.0 * ((p * t).sum(1) + stale) + de) / (p.sum(1) + t.sum(1) + 2.0 * stale + de)
    gn, = torch.autograd.grad(nfl.sum() * inp["w_nfl"], x, retain_graph=True)
    gd, = torch.autograd.grad(dice.sum() * inp["w_dice"], x)
    applies = dict(ignore_counted=bool((inp["gt"] == -1).any()), stale_chunk=nfl_plan(HW)["empty"] > 0).get(plant, True)
    return dict(nfl=nfl.detach(), dice=dice.detach(), g=gn + gd, A=gn.abs() + gd.abs(), applies=applies)


def nfl_worst(out, dl, ref):
    a = max(worst(out[:, 0], ref["nfl"], ref["nfl"].abs()), worst(out[:, 1], ref["dice"], ref["dice"].abs())) / LOSS_COEF
    b = 0.0 if dl is None else worst(dl, ref["g"], ref["A"], atol=NFL_GRAD_ABS * float(ref["A"].max())) / GRAD_COEF
    return a, b


# ------------------------------------------------------------------------------------------------ loss_finalize
def finalize_inputs(c):
    r = rng(c)
    B, npart = c.shape["B"], c.shape["npart"]
    out = r.rand(B, 2).astype(np.float32)
    part = (r.rand(npart) * 10.0 ** r.randint(-2, 4, npart)).astype(np.float32)
    return dict(out=out, part=part, inv=1.0 / (B * 48 * 448 * 448), w=(1.0, 1.0, 2.0, 0.8))


def finalize_ref(inp):
    o, part = inp["out"].astype(np.float64), inp["part"].astype(np.float64)
    w_nfl, w_dice, w_pcl, iw = inp["w"]
    nfl, dice, pcl = o[:, 0].mean(), o[:, 1].mean(), part.sum() * inp["inv"]
    return torch.tensor([(w_nfl * nfl + w_dice * dice + w_pcl * pcl) * iw, nfl, dice, pcl], dtype=F64)


# ------------------------------------------------------------------------------------------------ Adam
def adam_inputs(c):
    """p, g, m, v fp32 [n], the fp32 scalars, the segment tables (or None) and, for the hyper entry, hyper[0..3].  g has a random
    sign and m, p share it; v >= 0.  Padding between tensors is zero in all four.  Regimes: tail_cases / ISSUE: "unit" |g| in
    [0.05, 0.15], "tiny" |g| in [1e-12, 1e-7] log-uniform with m, v of that size, "zero", "small_p" |p| <= 1e-3."""
    r, n, o = rng(c), c.shape["n"], c.opt
    sign = np.where(r.rand(n) > 0.5, 1.0, -1.0)
    gabs = dict(unit=r.rand(n) * 0.1 + 0.05, small_p=r.rand(n) * 0.1 + 0.05, tiny=10.0 ** (r.rand(n) * 5.0 - 12.0), zero=np.zeros(n))[c.regime]
    g = (sign * gabs).astype(np.float32)
    first = o["step"] == 1
    m = np.zeros(n, np.float32) if first else (g * (r.rand(n) * 0.5 + 0.25)).astype(np.float32)
    v = np.zeros(n, np.float32) if first else (g.astype(np.float64) ** 2 * (r.rand(n) * 0.5 + 0.01)).astype(np.float32)
    # ("tiny": |p| <= |g| as well, or a coupled decay term wd * p would be the gradient)
    p = (sign * r.rand(n) * (gabs if c.regime == "tiny" else 1e-3 if c.regime == "small_p" else 1.0)).astype(np.float32)
    seg = None
    if o["layout"] not in (None, "none"):
        if o["layout"] == "one":
            seg_end, pad = [n], np.zeros(n, bool)
        else:
            _, seg_end, sizes, starts = seg_layout(o["layout"])
            pad = np.ones(n, bool)
            for s0, sz in zip(starts, sizes):
                pad[s0:s0 + sz] = False
            for a in (p, g, m, v):
                a[pad] = 0.0
        k = len(seg_end)
        lr = (LR * 0.75 ** (np.arange(k) % 5)).astype(np.float32) if c.entry == "adam_groups" else (0.75 ** (np.arange(k) % 5)).astype(np.float32)
        wd = np.where(np.arange(k) % 3 == 1, 0.0, o["wd"]).astype(np.float32)
        seg = dict(end=np.array(seg_end, np.int64), lr=lr, wd=wd, pad=pad)
    f = np.float32
    t = o["step"]
    b1, b2 = float(f(B1)), float(f(B2))
    hyper = np.array([LR, 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t), o["gs"]], np.float32) if c.entry == "adam_hyper" else None
    return dict(p=p, g=g, m=m, v=v, seg=seg, hyper=hyper, lr=float(f(LR)), b1=b1, b2=b2, eps=float(f(EPS)), wd=float(f(o["wd"])),
                gs=float(f(o["gs"])), step=t, decoupled=bool(o["decoupled"]))


def adam_ref(c, inp, plant=None):
    """adam_kernel's formula in float64 from the fp32 values of every input; bc1 = 1 - b1^t and bc2s = sqrt(1 - b2^t) in float64
    from the fp32 betas, or the very hyper[1], hyper[2] floats.  Returns p', m', v', the update, T_m, T_v, bc1, bc2."""
    p, g, m, v = (inp[k].astype(np.float64) for k in "pgmv")
    n, b1, b2, eps, t = p.size, inp["b1"], inp["b2"], inp["eps"], inp["step"]
    if inp["hyper"] is not None:
        lr0, bc1, bc2s, gs = (float(x) for x in inp["hyper"])
    else:
        lr0, bc1, bc2s, gs = inp["lr"], 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t), inp["gs"]
    lr, wd = np.full(n, lr0), np.full(n, inp["wd"])
    seg = inp["seg"]
    if seg is not None:
        base = np.arange(n) // 4 * 4
        k = np.searchsorted(seg["end"], base, side="right")
        if plant == "next_segment":                    # the search asks for the group's last element + 1 instead of its first
            k = np.minimum(np.searchsorted(seg["end"], base + 4, side="right"), len(seg["end"]) - 1)
        slr = seg["lr"].astype(np.float64)[k]
        lr, wd = (lr0 * slr if inp["hyper"] is not None else slr), seg["wd"].astype(np.float64)[k]
    dec = inp["decoupled"] if plant != "coupled_for_decoupled" else False
    gg, gabs = g * gs, np.abs(g * gs)
    if plant == "gs_after_decay":
        gg = (g + np.where(dec, 0.0, wd * p)) * gs
    elif not dec:
        gg = gg + wd * p
    if not dec:
        gabs = gabs + np.abs(wd * p)
    p1 = p * (1.0 - lr * wd) if dec else p
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    if plant == "no_bc2":
        bc2s = 1.0
    denom = np.sqrt(v1) / bc2s + eps
    if plant == "eps_in_sqrt":
        denom = np.sqrt(v1 + eps) / bc2s
    if plant == "eps_before_bc2":
        denom = (np.sqrt(v1) + eps) / bc2s
    upd = (lr / bc1) * (m1 / denom)
    p2 = p1 - upd
    if plant == "tail_skipped" and n % 4:
        q = n - n % 4
        p2[q:], m1[q:], v1[q:] = p[q:], m[q:], v[q:]
    applies = dict(next_segment=seg is not None and len(seg["end"]) > 1, coupled_for_decoupled=inp["decoupled"],
                   gs_after_decay=gs != 1.0, tail_skipped=n % 4 != 0, no_bc2=True).get(plant, True)
    return dict(p=p2, m=m1, v=v1, upd=upd, Tm=b1 * np.abs(m) + (1.0 - b1) * gabs, Tv=b2 * np.abs(v) + (1.0 - b2) * gabs * gabs,
                bc1=bc1, bc2=bc2s * bc2s, dec=dec and bool(np.any(wd != 0)), applies=applies)


K_M, K_V, K_P = 6, 10, 19


def adam_bounds(c, ref):
    """Element-wise bounds of |got - ref| for m', v', p', u = 2^-24 the relative error of one fp32 rounding, counted from
    adam_kernel (a contraction into an fma only removes roundings):
      m'  K_M = 6:  g * gs, wd * p, their sum; b1 * m, (1 - b1) * gg, their sum ((1 - b1) is exact: b1 >= 0.5) -- each on a
          quantity <= T_m = b1 |m| + (1 - b1)(|g gs| + |wd p|).
      v'  K_V = 10: the three of gg count twice (gg is squared); (1 - b2) * gg, * gg, b2 * v, the sum -- on T_v = b2 |v| +
          (1 - b2)(|g gs| + |wd p|)^2.
      p'  u |p_ref| for the final subtraction, and the update's relative error K_P u + d_bc: m' 6 (no cancellation: inputs), the
          denominator 5 (half of v's 10) + sqrtf + the division by bc2s + the sum with eps = 8, lr / bc1, m' / denom, their
          product, and for the hyper entry lr * scale = 4, and 1 for sqrtf and the divisions being good to 1 ulp rather than
          half: K_P = 19.  d_bc = 2u / bc1 + u / bc2 is what the launcher's fp32 1 - powf(b, t) and its square root can be off
          by after the cancellation (0 for the hyper entry, whose floats the reference reads).  With decoupled decay p is first
          multiplied by fl(1 - fl(lr * wd)): two more roundings of |p| (the product's error is far below u), 3 u |p_ref|."""
    d_bc = 0.0 if c.entry == "adam_hyper" else 2.0 * U / ref["bc1"] + U / ref["bc2"]
    return dict(m=K_M * U * ref["Tm"], v=K_V * U * ref["Tv"],
                p=(3.0 if ref["dec"] else 1.0) * U * np.abs(ref["p"]) + np.abs(ref["upd"]) * (K_P * U + d_bc))


def adam_worst(c, got, ref):
    """the largest |got - ref| / bound over p', m', v' (<= 1 when in bound)"""
    bd = adam_bounds(c, ref)
    return {k: worst(torch.from_numpy(np.asarray(got[k], np.float64)), torch.from_numpy(ref[k]), torch.from_numpy(bd[k])) for k in "pmv"}


def bf16_bits(p32, plant=None):
    """the bits of fp32 -> bf16, rounded to nearest even (torch), or truncated"""
    t = torch.from_numpy(np.ascontiguousarray(p32, np.float32))
    if plant == "shadow_truncated":
        return (t.view(torch.int32) >> 16).to(torch.int16).numpy()
    return t.to(torch.bfloat16).view(torch.int16).numpy()


# ------------------------------------------------------------------------------------------------ dropout
M64 = (1 << 64) - 1


def dropout_ref(n, keep, seed, word, call):
    """vpu_dropout_mask: splitmix64 of (seed ^ state[1]) + call * golden + (i + 1) * 0xD1B54A32D192ED03, the top 24 bits against
    keep in fp32; kept channels hold fl(1 / keep)"""
    keep32, out = np.float32(keep), np.zeros(n, np.float32)
    inv = np.float32(1.0) / keep32
    for i in range(n):
        x = ((seed ^ word) + call * 0x9E3779B97F4A7C15 + (i + 1) * 0xD1B54A32D192ED03) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        x ^= x >> 31
        if np.float32(x >> 40) * np.float32(1.0 / 16777216.0) < keep32:
            out[i] = inv
    return out
