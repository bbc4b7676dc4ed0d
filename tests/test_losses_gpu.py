"""The loss-path kernels against float64 references at the shapes the training step runs: p2cl_up (upsample + P2CL + both
backward passes, persistent over (plane, band) items), p2cl_fwd_bwd with upsample_ac_fwd / upsample_ac_bwd, nfl_dice_fwd_bwd,
loss_finalize and vpu_step_losses end to end, head_grad_fused and sigmoid_to_channel.

References are the oracle's own loss functions (vpu_oracle) on float64 tensors, float64 autograd for the gradients.  The bilinear
align_corners=True upsample of the reference samples each full-resolution row / column at the position the kernels -- and torch's
own fp32 interpolate -- compute, t = fl32(fl32((n - 1) / (N - 1)) * Y), and interpolates in float64 from there: float64 positions
would differ from those by up to ~1e-5 cells at 448 pixels, which 1 / (1 - p) turns into gradient differences far above the
kernels' own rounding (the positions themselves are checked against F.interpolate in float64 in test_reference_interpolation).

Bounds (every check prints the measured value beside its bound):
  loss sums (per band, per plane, per sample)   |got - ref| <= 1e-5 |ref|
  gradients, per element                        |got - ref| <= 3e-5 A_i, A_i = the float64 backward of |d loss / d prob| (the
                                                sum of absolute contributions: cancellation cannot hide an error)
  bf16 outputs                                  2^-8 relative to float64 of the same formula, plus the absolute term at the assert
Low-resolution probabilities are drawn from [0.02, 0.98], where 1 / (1 - p) amplifies the fp32 interpolation error at most 50x;
saturated planes (exactly 0 or 1) are tested on their own."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

VPU_ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def vo():
    import vpu_oracle
    return vpu_oracle


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _within(tag, got, ref, scale, coef, atol=0.0):
    """|got - ref| <= coef * scale + atol element-wise; prints the smallest coefficient that would have passed."""
    err = (got.double() - ref).abs()
    scale = scale.double()
    over = (err - atol).clamp_min(0.0)
    need = torch.where(scale > 0, over / scale.clamp_min(1e-300), torch.where(over > 0, math.inf, 0.0))
    m = need.max().item()
    print(f"[losses] {tag}: {m:.2e} (bound {coef:.0e}{f', atol {atol:.1e}' if atol else ''})")
    bad = err > coef * scale + atol
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} elements out of bound, first at {i}: got {got[i].item()!r}, "
                             f"ref {ref[i].item()!r}, scale {scale[i].item()!r}")


# ------------------------------------------------------------------------------------------------ inputs and references
def _labels(n, H, W, seed):
    """[n, 1, H, W] labels: blocks of 0 / 1 with pixel noise, -0.0 among the zeros, and every fourth strip of 8 rows with soft
    (0.3) and ignore (-1) pixels -- so that some threads of p2cl_up take the all-0/1 ("plain") path and others the general one."""
    g = _gen(seed)
    blk = (torch.rand(n, 1, (H + 15) // 16, (W + 15) // 16, device="cuda", generator=g) > 0.5).float()
    lab = blk.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :H, :W].contiguous()
    r = torch.rand(n, 1, H, W, device="cuda", generator=g)
    lab = torch.where(r < 0.08, 1.0 - lab, lab)
    lab = torch.where((lab == 0) & (r > 0.9), torch.full_like(lab, -0.0), lab)
    strip = ((torch.arange(H, device="cuda") // 8) % 4 == 1).view(1, 1, H, 1)
    k = torch.rand(n, 1, H, W, device="cuda", generator=g)
    lab = torch.where(strip & (k < 0.25), torch.full_like(lab, 0.3), lab)
    lab = torch.where(strip & (k >= 0.25) & (k < 0.5), torch.full_like(lab, -1.0), lab)
    return lab


def _p2_inputs(B, S, h, w, H, W, seed, slots=True):
    g = _gen(seed)
    low = torch.rand(B, S, h, w, device="cuda", generator=g) * 0.96 + 0.02
    gt = _labels(B, H, W, seed + 1)
    if not slots:
        return low, gt, None, None
    ov = _labels(4, H, W, seed + 2)[:, 0].contiguous()
    idx = -torch.ones(B, S, dtype=torch.int32)
    idx[0, 0] = 0                 # first slot (positive half)
    idx[0, S - 1] = 1             # last slot (inverted half)
    idx[B - 1, S // 2 - 1] = 2    # last slot of the positive half
    idx[B - 1, S // 2] = 3        # first slot of the inverted half
    return low, gt, ov, idx.cuda()


def _interp_matrix(n, N):
    """[N, n] float64 align_corners=True weights: row Y samples t = fl32(fl32((n-1)/(N-1)) * Y), anchor i0 = min(int(t), n-1),
    weights 1 - (t - i0) and t - i0 (the right one on min(i0 + 1, n - 1))."""
    s = torch.tensor(float(n - 1), dtype=torch.float32) / torch.tensor(float(N - 1), dtype=torch.float32)
    t = s * torch.arange(N, dtype=torch.float32)
    i0 = t.long().clamp_max(n - 1)
    l1 = t.double() - i0.double()
    i1 = (i0 + 1).clamp_max(n - 1)
    M = torch.zeros(N, n, dtype=torch.float64)
    Y = torch.arange(N)
    M.index_put_((Y, i0), 1.0 - l1, accumulate=True)
    M.index_put_((Y, i1), l1, accumulate=True)
    return M.cuda(), i0.cuda()


def _ed_labels(vo, gt, S, idx, ov, b):
    """float64 [S, H, W] P2CL labels of sample b: ed_mask_label (trainer.py:329-331), then label[b, s] = override[slot_idx[b, s]]
    (trainer.py:756,764)."""
    lab = vo.ed_mask_label(gt[b:b + 1].double(), S // 2)[0]
    if idx is not None:
        for s in (idx[b] >= 0).nonzero().flatten().tolist():
            lab[s] = ov[int(idx[b, s])].double()
    return lab


def _p2cl_ref(vo, low, gt, idx, ov, H, W, gs, band=None, want_up=False):
    """float64 P2CL of the upsampled planes, per sample: per-band loss sums (bands of ``band`` anchor rows; per-plane sums if
    None), d loss / d low, and A = the backward of the absolute contributions to d loss / d prob, gs (|y| / (p + 1e-12) +
    |1 - y| / (1 - p + 1e-12)) on valid pixels (|d loss / d prob| itself for 0 / 1 labels; a soft label's two terms cancel at
    p = y).  ``want_up``: also the upsampled planes, d loss / d prob and its absolute contributions."""
    B, S, h, w = low.shape
    My, ay = _interp_matrix(h, H)
    Mx, _ = _interp_matrix(w, W)
    nb = 1 if band is None else (h + band - 1) // band
    bidx = torch.zeros(H, dtype=torch.long, device="cuda") if band is None else ay // band
    out = {"bands": [], "dlow": [], "A": [], "up": [], "dprob": [], "absd": []}
    for b in range(B):
        lo = low[b].double().requires_grad_(True)
        up = My @ lo @ Mx.t()
        lab = _ed_labels(vo, gt, S, idx, ov, b)
        rows = vo.bce_from_sigmoid(up.reshape(S * H, W), lab.reshape(S * H, W)) * W       # per-row loss sums
        dprob, = torch.autograd.grad(rows.sum() * gs, up, retain_graph=True)
        dl, = torch.autograd.grad(up, lo, dprob, retain_graph=True)
        valid = lab != -1
        y = torch.where(valid, lab, torch.zeros_like(lab))
        p = up.detach()
        absd = gs * valid * (y.abs() / (p + 1e-12) + (1.0 - y).abs() / (1.0 - p + 1e-12))
        A, = torch.autograd.grad(up, lo, absd)
        bs = torch.zeros(S, nb, dtype=torch.float64, device="cuda")
        bs.index_add_(1, bidx, rows.detach().view(S, H))
        out["bands"].append(bs)
        out["dlow"].append(dl)
        out["A"].append(A)
        if want_up:
            out["up"].append(up.detach())
            out["dprob"].append(dprob)
            out["absd"].append(absd)
    return {k: torch.stack(v) for k, v in out.items() if v}


def _band_rows(w):
    return min(8, 1024 // w - 1)      # anchor rows per p2cl_up item (loss.hip: p2cl_band)


def _p2cl_up(ops, low, gt, idx, ov, dlow, gs, H, W):
    B, S, h, w = low.shape
    return ops.p2cl_up_fwd_bwd(low, gt, idx, ov, None, dlow, gs, B, S, h, w, H, W)


# ------------------------------------------------------------------------------------------------ p2cl_up
def _cus_plus_shape():
    """(B, S, h, w, H, W) with just over one item per CU: B * S * nband = CUs + 2 (B * S is even), non-square, 2x / 4x."""
    target = _ncu() + 2
    for B in range(1, 64):
        if target % (2 * B) == 0 and target // (2 * B) <= 64:
            nb = target // (2 * B)
            h = 8 * (nb - 1) + 4 if nb > 1 else 4       # a short last band
            return B, 2, h, 96, 2 * h, 384
    pytest.fail(f"no (B, h) gives {target} items")


P2_CASES = {
    "bench": (12, 48, 112, 112, 448, 448),      # 8064 items, ~31 per workgroup
    "vith": (2, 8, 128, 128, 448, 448),         # bands of 7 rows, a short last band; no override slots
    "cus_plus_2": None,                         # _cus_plus_shape()
    "nonsquare": (2, 6, 56, 84, 224, 336),
    "span5": (2, 4, 12, 12, 52, 52),            # (H-1)/(h-1) = 4.64: 5 full-resolution rows / columns per cell
    "wide": (2, 4, 256, 256, 1024, 1024),       # bands of 3 rows
}


@pytest.mark.parametrize("case", list(P2_CASES))
def test_p2cl_up_matches_float64(ops, vo, case):
    """Per-band loss sums and d loss / d low of the persistent p2cl_up against float64; every element written and finite
    (dlow starts as NaN); the same bits with CUs reserved (another walk over the items), for one sample run alone, and for the
    loss-only call."""
    from pvpuformer_amd import _lib
    B, S, h, w, H, W = P2_CASES[case] or _cus_plus_shape()
    band = _band_rows(w)
    nband = _lib.load().vpu_p2cl_up_nband(h, w)
    assert nband == (h + band - 1) // band
    nitems, ncu = B * S * nband, _ncu()
    print(f"[losses] p2cl_up {case}: B {B} S {S} {h}x{w} -> {H}x{W}, band {band}, {nitems} items on {ncu} CUs")
    if case == "bench":
        assert nitems > ncu
    if case == "cus_plus_2":
        assert ncu < nitems <= ncu + 2
    low, gt, ov, idx = _p2_inputs(B, S, h, w, H, W, seed=100 + h + w, slots=case != "vith")
    gs = 2.0 / (B * S * H * W)
    dlow = torch.full_like(low, float("nan"))
    bands = _p2cl_up(ops, low, gt, idx, ov, dlow, gs, H, W)
    torch.cuda.synchronize()
    assert torch.isfinite(dlow).all() and torch.isfinite(bands).all()
    ref = _p2cl_ref(vo, low, gt, idx, ov, H, W, gs, band)
    _within(f"p2cl_up {case} band sums", bands.view(B, S, nband), ref["bands"], ref["bands"].abs(), 1e-5)
    _within(f"p2cl_up {case} dlow", dlow, ref["dlow"], ref["A"], 3e-5)
    lo = _p2cl_up(ops, low, gt, idx, ov, None, gs, H, W)
    assert torch.equal(lo, bands)
    try:
        for r in (16, 128):
            ops.gemm_set_option("reserve_cus", r)
            d2 = torch.full_like(low, float("nan"))
            b2 = _p2cl_up(ops, low, gt, idx, ov, d2, gs, H, W)
            assert torch.equal(b2, bands) and torch.equal(d2, dlow), r
    finally:
        ops.gemm_set_option("reserve_cus", 0)
    b = B - 1
    d1 = torch.full_like(low[b:b + 1], float("nan"))
    b1 = _p2cl_up(ops, low[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), None if idx is None else idx[b:b + 1].contiguous(),
                  ov, d1, gs, H, W)
    assert torch.equal(b1, bands[b * S:(b + 1) * S]) and torch.equal(d1[0], dlow[b])


def test_p2cl_up_ignore_label_in_both_halves(ops, vo):
    """A -1 label is ignored where the P2CL label is the ground truth itself (the positive half, override slots) and is a valid
    label 0 in the inverted half, logical_not(-1) = 0 (trainer.py:330): a map of -1 only gives zero loss and gradient on the
    positive planes and the loss of label 0 on the inverted ones."""
    B, S, h, H = 1, 4, 28, 112
    low = torch.rand(B, S, h, h, device="cuda", generator=_gen(7)) * 0.96 + 0.02
    gt = torch.full((B, 1, H, H), -1.0, device="cuda")
    gs = 1.0 / (B * S * H * H)
    for fused in (True, False):
        if fused:
            dlow = torch.full_like(low, float("nan"))
            part = _p2cl_up(ops, low, gt, None, None, dlow, gs, H, H).view(S, -1).sum(1)
        else:
            up = torch.empty(B, S, H, H, device="cuda")
            ops.upsample_ac_fwd(low, up, B * S, h, h, H, H)
            part, dprob, dlow = torch.empty(B, S, device="cuda"), torch.empty_like(up), torch.empty_like(low)
            ops.p2cl_fwd_bwd(up, gt, None, None, part, dprob, gs, B, S, H, H)
            ops.upsample_ac_bwd(dprob, dlow, B * S, h, h, H, H)
            part = part.view(S)
        ref = _p2cl_ref(vo, low, gt, None, None, H, H, gs)
        assert torch.equal(part[:S // 2], torch.zeros_like(part[:S // 2])) and torch.equal(dlow[0, :S // 2], torch.zeros_like(dlow[0, :S // 2]))
        assert (part[S // 2:] > 0).all() and (dlow[0, S // 2:] > 0).all(), fused
        _within(f"ignore labels ({'p2cl_up' if fused else 'p2cl'}) plane sums", part, ref["bands"].view(S), ref["bands"].view(S), 1e-5)
        _within(f"ignore labels ({'p2cl_up' if fused else 'p2cl'}) dlow", dlow, ref["dlow"], ref["A"], 3e-5)


def test_p2cl_up_saturated_planes(ops, vo):
    """Planes of exactly 0.0 or 1.0 (they interpolate exactly) against labels that match them (loss ~ 0) and labels opposite to
    them (loss -log(1e-12) per pixel, gradient 1e12 * grad_scale per pixel): finite and within the same bounds.  Loss sums get an
    absolute term of 2e-12 per pixel: fp32 1 + 1e-12 == 1, so a matching pixel costs 0 in the kernel and -log(1 + 1e-12) =
    -1.0000889e-12 in float64."""
    B, S, h, H = 2, 4, 28, 112
    low = torch.zeros(B, S, h, h, device="cuda")
    low[:, 0::2] = 1.0
    gt = torch.zeros(B, 1, H, H, device="cuda")
    gt[0] = 1.0
    gt[1, :, :, H // 2:] = 1.0
    gs = 2.0 / (B * S * H * H)
    band = _band_rows(h)
    dlow = torch.full_like(low, float("nan"))
    bands = _p2cl_up(ops, low, gt, None, None, dlow, gs, H, H)
    torch.cuda.synchronize()
    assert torch.isfinite(dlow).all() and torch.isfinite(bands).all()
    assert dlow.abs().max().item() > 1e11 * gs        # the opposite planes' gradient is there
    ref = _p2cl_ref(vo, low, gt, None, None, H, H, gs, band)
    _, ay = _interp_matrix(h, H)
    npx = torch.bincount(ay // band, minlength=bands.shape[1]).double() * H
    _within("saturated band sums", bands.view(B, S, -1), ref["bands"], ref["bands"].abs() + 2e-7 * npx.view(1, 1, -1), 1e-5)
    _within("saturated dlow", dlow, ref["dlow"], ref["A"], 3e-5)


def test_p2cl_up_refuses_ratio_5(ops):
    """(H - 1) / (h - 1) >= 5 (more than P2_SPAN = 5 pixels per cell) is refused in either axis before any launch."""
    from pvpuformer_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    sentinel = torch.full((4096,), 7.0, device="cuda")
    p = sentinel.data_ptr()
    for (h, w, H, W) in ((12, 12, 56, 52), (12, 12, 52, 56)):
        rc = lib.vpu_p2cl_up_fwd_bwd(p, p, None, None, p, p, 1.0, 1, 2, h, w, H, W, st)
        assert rc == VPU_ERR_ARG, (h, w, H, W, rc)
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)


# ------------------------------------------------------------------------------------------------ p2cl with aux materialised
def test_reference_interpolation(ops):
    """The reference's sampling positions: upsample_ac_fwd reproduces the float64 interpolation at the fp32 positions within
    fp32 rounding, and those positions differ from float64 F.interpolate by less than 2e-5 (cells) times the map's range."""
    import torch.nn.functional as F
    for (h, w, H, W) in ((112, 112, 448, 448), (56, 84, 224, 336)):
        low = torch.rand(4, 6, h, w, device="cuda", generator=_gen(h + w)) * 0.96 + 0.02
        My, _ = _interp_matrix(h, H)
        Mx, _ = _interp_matrix(w, W)
        ref = My @ low.double() @ Mx.t()
        up = torch.empty(4, 6, H, W, device="cuda")
        ops.upsample_ac_fwd(low, up, 24, h, w, H, W)
        _within(f"upsample_ac_fwd {h}x{w}", up, ref, torch.ones_like(ref), 5e-7)
        f64 = F.interpolate(low.double(), size=(H, W), mode="bilinear", align_corners=True)
        _within(f"fp32 positions vs F.interpolate float64 {h}x{w}", ref, f64, torch.ones_like(ref), 2e-5)


@pytest.mark.parametrize("shape", [(12, 48, 112, 112, 448, 448), (2, 6, 56, 84, 224, 336)])
def test_p2cl_with_aux_matches_float64(ops, vo, shape):
    """upsample_ac_fwd -> p2cl_fwd_bwd -> upsample_ac_bwd (the path with the full-resolution aux map): per-plane loss sums,
    d loss / d prob and d loss / d low against float64, with the same labels and override slots as p2cl_up."""
    B, S, h, w, H, W = shape
    low, gt, ov, idx = _p2_inputs(B, S, h, w, H, W, seed=300 + h + w)
    gs = 2.0 / (B * S * H * W)
    up = torch.full((B, S, H, W), float("nan"), device="cuda")
    ops.upsample_ac_fwd(low, up, B * S, h, w, H, W)
    part, dprob = torch.full((B, S), float("nan"), device="cuda"), torch.full_like(up, float("nan"))
    ops.p2cl_fwd_bwd(up, gt, idx, ov, part, dprob, gs, B, S, H, W)
    dlow = torch.full_like(low, float("nan"))
    ops.upsample_ac_bwd(dprob, dlow, B * S, h, w, H, W)
    torch.cuda.synchronize()
    assert torch.isfinite(dprob).all() and torch.isfinite(dlow).all()
    ref = _p2cl_ref(vo, low, gt, idx, ov, H, W, gs, want_up=True)
    _within(f"upsample_ac_fwd {h}x{w}", up, ref["up"], torch.ones_like(ref["up"]), 5e-7)
    _within(f"p2cl {h}x{w} plane sums", part, ref["bands"].view(B, S), ref["bands"].view(B, S).abs(), 1e-5)
    _within(f"p2cl {h}x{w} dprob", dprob, ref["dprob"], ref["absd"], 3e-5)
    _within(f"p2cl + upsample_ac_bwd {h}x{w} dlow", dlow, ref["dlow"], ref["A"], 3e-5)


# ------------------------------------------------------------------------------------------------ NFL + Dice
def _logits(gt, seed):
    """Logits in [-20, 20] (the sigmoid saturates), but not beyond 6 on the wrong side of a 0 / 1 label: NFL takes pt = 1 - |t - p|,
    and in fp32 that difference holds pt to 2^-24 absolute only, whatever the kernel does (torch's fp32 evaluation of the formula
    included) -- for t = 1 at x = -16 one ulp moves log(pt) by 0.4, from x = -17 on pt rounds to 0 and the loss to log(1e-12), and at
    x = -8 the gradient om^2 / pt is off by ~1e-4.  At |x| <= 6, pt >= 2.5e-3.  Soft (0.3) and ignore (-1) pixels take the whole
    range."""
    x = (torch.randn(gt.shape, device="cuda", generator=_gen(seed)) * 6.0).clamp(-20.0, 20.0)
    x[:, :, 0, :8] = torch.tensor([20.0, -20.0, 0.0, 15.0, -15.0, 9.0, -9.0, 1e-3], device="cuda")
    x = torch.where(gt == 0, x.clamp_max(6.0), x)
    return torch.where(gt == 1, x.clamp_min(-6.0), x)


def _nfl_dice_ref(vo, logits, gt, w_nfl, w_dice):
    """float64 per-sample NFL and Dice, and the gradient of w_nfl * sum NFL + w_dice * sum Dice with its A (|NFL part| +
    |Dice part|)."""
    B = logits.shape[0]
    x = logits.double().requires_grad_(True)
    t = gt.double()
    nfl = vo.nfl_loss(x, t)
    dice = torch.stack([vo.dice_loss_naive(x[b:b + 1], t[b:b + 1]) for b in range(B)])
    gn, = torch.autograd.grad(nfl.sum() * w_nfl, x)
    gd, = torch.autograd.grad(dice.sum() * w_dice, x)
    return nfl.detach(), dice.detach(), gn + gd, gn.abs() + gd.abs()


@pytest.mark.parametrize("H", [448, 672])
def test_nfl_dice_matches_float64(ops, vo, H):
    """NFL + Dice at B 12 with ignore (-1), soft (0.3) and -0.0 labels and logits up to +-20 (saturated sigmoid): per-sample
    losses and the logit gradient against float64; a sample's bits do not depend on the other samples.  The gradient bound has
    an absolute term of 1e-6 of its largest A: fp32 p = sigmoid(x) is exact to 6e-8 absolute, so p (1 - p) of a saturated pixel
    (x = 20: 2e-9 in float64, 0 in fp32) differs by that much from float64 whatever the kernel does."""
    B = 12
    gt = _labels(B, H, H, seed=401 + H)
    logits = _logits(gt, seed=400 + H)
    w_nfl, w_dice = 1.0 / B, 1.0 / B
    out = torch.full((B, 2), float("nan"), device="cuda")
    dl = torch.full((B, H * H), float("nan"), device="cuda")
    ops.nfl_dice_fwd_bwd(logits, gt, None, out, dl, w_nfl, w_dice, B, H * H)
    torch.cuda.synchronize()
    assert torch.isfinite(dl).all()
    nfl, dice, g, A = _nfl_dice_ref(vo, logits, gt, w_nfl, w_dice)
    _within(f"nfl {H}", out[:, 0], nfl, nfl.abs(), 1e-5)
    _within(f"dice {H}", out[:, 1], dice, dice.abs(), 1e-5)
    _within(f"nfl + dice d logits {H}", dl.view_as(logits), g, A, 3e-5, atol=1e-6 * A.max().item())
    b = 5
    o1, d1 = torch.empty(1, 2, device="cuda"), torch.empty(1, H * H, device="cuda")
    ops.nfl_dice_fwd_bwd(logits[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), None, o1, d1, w_nfl, w_dice, 1, H * H)
    assert torch.equal(o1[0], out[b]) and torch.equal(d1[0], dl[b])


# ------------------------------------------------------------------------------------------------ loss_finalize, vpu_step_losses
def test_loss_finalize_matches_float64(ops):
    """loss_finalize alone: the means of 12 per-sample NFL / Dice values and the sum of 8064 band partials (magnitudes over
    six decades) against float64; the fp32 results are within 1e-6."""
    B, npart = 12, 8064
    g = _gen(500)
    out = torch.rand(B, 2, device="cuda", generator=g)
    part = torch.rand(npart, device="cuda", generator=g) * 10.0 ** torch.randint(-2, 4, (npart,), device="cuda", generator=g)
    inv = 1.0 / (B * 48 * 448 * 448)
    res = torch.full((4,), float("nan"), device="cuda")
    ops.loss_finalize(out, part, B, npart, inv, 1.0, 1.0, 2.0, 0.8, res)
    o = out.double()
    nfl, dice, pcl = o[:, 0].mean(), o[:, 1].mean(), part.double().sum() * inv
    ref = torch.stack([(nfl + dice + 2.0 * pcl) * 0.8, nfl, dice, pcl])
    _within("loss_finalize", res, ref, ref.abs(), 1e-6)


def test_step_losses_bench_shape_matches_float64(ops, vo):
    """vpu_step_losses with the fused P2CL at the bench shape (B 12, 48 slots, 112 -> 448) with override slots and
    iter_weight 0.8: total / nfl / dice / p2cl against float64 vo.step_loss, d_inst and d_sim_low against float64 gradients."""
    from pvpuformer_amd.isegm.engine.trainer import vpu_step_losses
    B, S, h, H = 12, 48, 112, 448
    iw = 0.8
    low, gt, ov, idx = _p2_inputs(B, S, h, h, H, H, seed=600)
    inst = _logits(gt, seed=601)
    losses, d_inst, d_low = vpu_step_losses(inst, None, gt, idx, ov, iter_weight=iw, sim_low=low)
    torch.cuda.synchronize()
    assert torch.isfinite(d_inst).all() and torch.isfinite(d_low).all()
    My, _ = _interp_matrix(h, H)
    with torch.no_grad():
        aux = My @ low.double() @ My.t()
        ed = torch.stack([_ed_labels(vo, gt, S, idx, ov, b) for b in range(B)])
        total, parts = vo.step_loss({"instances": inst.double(), "instances_aux": aux}, gt.double(), ed, iter_weight=iw)
        del aux, ed
    for k, r in (("total", total), ("nfl", parts["nfl"]), ("dice", parts["dice"]), ("p2cl", parts["p2cl"])):
        _within(f"step_losses {k}", losses[k].view(1), r.view(1), r.abs().view(1), 1e-5)
    _, _, g, A = _nfl_dice_ref(vo, inst, gt, iw / B, iw / B)
    _within("step_losses d_inst", d_inst, g, A, 3e-5, atol=1e-6 * A.max().item())
    ref = _p2cl_ref(vo, low, gt, idx, ov, H, H, 2.0 * iw / (B * S * H * H))
    _within("step_losses d_sim_low", d_low, ref["dlow"], ref["A"], 3e-5)


# ------------------------------------------------------------------------------------------------ head_grad_fused
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("layout", ["bench", "hw97"])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_head_grad_fused_matches_float64(ops, C, layout, masked):
    """head_grad_fused at 12 x 112^2 rows (512 blocks, image boundaries inside blocks) and with 97-row images (boundaries inside
    blocks and waves), with and without the Dropout2d mask: dx against float64 of the kernel's formula (spatial.hip)
        dx[r][c] = [x > 0] * (inv[r] * (dfn[r][c] - y[r][c] * sum_c' dfn[r][c'] y[r][c']) + dout[r] * w[c] * mask[b][c]),
    conv_seg's weight / bias gradients (the partials summed) against float64; one image run alone gives the same dx bits."""
    B, HW = (12, 112 * 112) if layout == "bench" else (600, 97)
    rows = B * HW
    g = _gen(700 + C)
    bf = torch.bfloat16
    x = torch.randn(rows, C, device="cuda", generator=g).clamp_min(0.0).to(bf)          # a ReLU output: exact zeros
    v = torch.randn(rows, C, device="cuda", generator=g)
    y = (v / v.norm(dim=1, keepdim=True)).to(bf)
    dfn = (torch.randn(rows, C, device="cuda", generator=g) * 0.1).to(bf)
    inv = torch.rand(rows, device="cuda", generator=g) * 2.0 + 0.5
    dout = torch.randn(rows, device="cuda", generator=g) * 1e-3
    w = torch.randn(C, device="cuda", generator=g) * 0.1
    mask = (torch.rand(B, C, device="cuda", generator=g) > 0.1).float() / 0.9 if masked else None
    nb = ops.convseg_bwd_nblk(rows)
    dx = torch.full((rows, C), float("nan"), device="cuda", dtype=bf)
    part, part_b = torch.full((nb, C), float("nan"), device="cuda"), torch.full((nb,), float("nan"), device="cuda")
    ops.head_grad_fused(dfn, y, inv, dout, x, w, mask, dx, part, part_b, rows, HW, C)
    torch.cuda.synchronize()
    assert torch.isfinite(dx.float()).all()
    gd, yd, xd, ivd, dd, wd = dfn.double(), y.double(), x.double(), inv.double(), dout.double(), w.double()
    mk = torch.ones(rows, C, dtype=torch.float64, device="cuda") if mask is None else mask.double().repeat_interleave(HW, 0)
    sdot = (gd * yd).sum(1, keepdim=True)
    pos = xd > 0
    ref = torch.where(pos, ivd[:, None] * (gd - yd * sdot) + dd[:, None] * wd[None] * mk, 0.0)
    A = torch.where(pos, ivd[:, None] * (gd.abs() + yd.abs() * (gd * yd).abs().sum(1, keepdim=True)) + (dd[:, None] * wd[None] * mk).abs(), 0.0)
    # bf16 output: 2^-8 of |ref| (the rounding), plus 1e-5 of A for the fp32 arithmetic before it
    err = (dx.double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + 1e-5 * A
    excess = ((err - 2.0 ** -8 * ref.abs()).clamp_min(0.0) / A.clamp_min(1e-300)).max().item()
    print(f"[losses] head_grad_fused C {C} {layout} mask {masked}: max |dx - ref| / (2^-8 |ref| + 1e-5 A) = "
          f"{(err / lim.clamp_min(1e-300)).max().item():.3f} (bound 1); beyond the bf16 rounding {excess:.2e} A (bound 1e-5)")
    assert (err <= lim).all(), (C, layout, masked, int((err > lim).sum()))
    dw_ref = (dd[:, None] * xd * mk).sum(0)
    dw_abs = (dd[:, None] * xd * mk).abs().sum(0)
    _within(f"head_grad_fused C {C} {layout} mask {masked} d conv_seg.weight", part.sum(0), dw_ref, dw_abs, 1e-5)
    _within(f"head_grad_fused C {C} {layout} mask {masked} d conv_seg.bias", part_b.sum().view(1), dd.sum().view(1),
            dd.abs().sum().view(1), 1e-5)
    k = 7
    rs = slice(k * HW, (k + 1) * HW)
    d1 = torch.full((HW, C), float("nan"), device="cuda", dtype=bf)
    nb1 = ops.convseg_bwd_nblk(HW)
    p1, pb1 = torch.empty(nb1, C, device="cuda"), torch.empty(nb1, device="cuda")
    ops.head_grad_fused(dfn[rs], y[rs], inv[rs], dout[rs], x[rs], w, None if mask is None else mask[k:k + 1], d1, p1, pb1, HW, HW, C)
    assert torch.equal(d1, dx[rs])


# ------------------------------------------------------------------------------------------------ sigmoid_to_channel
@pytest.mark.parametrize("HW", [448 * 448, 97 * 101])
def test_sigmoid_to_channel(ops, HW):
    """prev_mask = sigmoid(logits) into channel 3 of a [B, 5, HW] input: within 3 ulp of float64 (expf's 1 ulp, then the rounded
    sum and quotient); the other channels keep their bits."""
    B, Cn, ch = 3, 5, 3
    g = _gen(800)
    logits = torch.randn(B, HW, device="cuda", generator=g) * 8.0
    logits[0, :9] = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 30.0, -30.0, 80.0], device="cuda")
    out = torch.randn(B, Cn, HW, device="cuda", generator=g)
    before = out.clone()
    ops.sigmoid_to_channel(logits, out, B, HW, Cn, ch)
    torch.cuda.synchronize()
    ref = torch.sigmoid(logits.double())
    r32 = ref.float()
    ulp = (torch.nextafter(r32, torch.full_like(r32, math.inf)) - r32).double()
    _within(f"sigmoid_to_channel HW {HW} (ulp)", out[:, ch], ref, ulp, 3.0)
    keep = [c for c in range(Cn) if c != ch]
    assert torch.equal(out[:, keep], before[:, keep])
