"""The tail of the training step -- csrc/loss.hip (p2cl_up, p2cl, nfl_dice, loss_finalize) and csrc/optim.hip (the three Adam
entries) -- against float64 references at the launchers' edges, and vpu_dropout_mask against a Python splitmix64, bit for bit.

The module walks tests/tail_cases.py, one parametrised test per entry, through the product library (its launchers read
VPU_P2CL_BAND and VPU_ADAM_GRID as unset: the band count the library reports is the table's).  tests/test_tail_cases_cpu.py checks
that the table reaches every launcher branch, sweeps the invariants p2cl_up_kernel relies on, checks the references of
tests/tail_ref.py against a second one and proves that the bounds below tell each of 20 planted errors.

Bounds (tail_ref.py; every check prints the largest measured error in units of its bound, so <= 1 passes):
  loss sums 1e-5 |ref|; gradients 3e-5 A_i; + 2e-7 per pixel on the sums of saturated planes; + 1e-6 max A on the NFL / Dice
  gradient; loss_finalize 1e-6 |ref| (test_losses_gpu.py); Adam m' 6 u T_m, v' 10 u T_v, p' u |p_ref| + |upd_ref| (19 u + d_bc)
  (3 u |p_ref| with decoupled decay), the roundings counted in tail_ref.adam_bounds; the bf16 shadow and the dropout mask bit
  for bit.
Memory: every output is the middle of a larger buffer whose guards must keep their canary bytes; float outputs start as NaN and
must come back finite and fully written; the NFL scratch starts as NaN too (an empty chunk block has to write its zeros).

Rows: p2cl_up 102, p2cl_up_items 1, p2cl 12, nfl_dice 60, finalize 4, adam 32, adam_groups 80, adam_hyper 80, dropout 10,
refuse 30.  What an MI355X measured is in RECORD below."""
import numpy as np
import pytest
import torch

import tail_ref as tr
from tail_cases import case_id, p2cl_band, p2cl_up_plan, rows

pytestmark = pytest.mark.gpu

VPU_ERR_ARG = -1
CANARY = 0x5A
GUARD = 256                 # elements on either side (a multiple of 16 bytes for every dtype: vector accesses stay aligned)

RECORD = """largest measured error per entry on an MI355X, in units of its bound (all 222 tests pass, no kernel or launcher change):
  p2cl_up        sums 0.016 (12x12 -> 52x52, saturated), dlow 0.071 (8x146 -> 17x148); the downsampling rows (9x8 -> 5x4) 0.014 / 0.021,
                 the nrp == 0 rows 0.016 / 0.050: no shape needed explaining, H < h and W < w are computed right
  p2cl_up_items  sums 0.018, dlow 0.044; the same bits with 0, 16 and 128 CUs reserved
  p2cl           sums 0.5 (HW 4, saturated: the 2e-7 per pixel term -- fp32 1 + 1e-12 == 1), dprob 0.005
  nfl_dice       losses 0.27 (B 65, HW 4, one sample ignored), dlogits 0.11
  finalize       0.13
  adam           p' 0.98, m' 0.27, v' 0.35;  adam_groups 0.99, 0.30, 0.37;  adam_hyper 1.00 (0.998), 0.30, 0.34 -- p' comes that
                 close wherever the update is far below an ulp of p: the bound is then u |p_ref|, the rounding of the final
                 subtraction itself, which round-to-nearest cannot exceed
  dropout, the bf16 shadow, the refusals: exact"""


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import _lib
    return _lib.load()


class Guarded:
    """allocations with a canary-filled guard before and after; float buffers start as NaN"""

    def __init__(self):
        self.bufs = []

    def alloc(self, shape, dtype=torch.float32, init=None, scratch=False):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        numel = int(np.prod(shape, dtype=np.int64))
        raw = torch.empty(numel + 2 * GUARD, device="cuda", dtype=dtype)
        raw.view(torch.uint8).fill_(CANARY)
        t = raw[GUARD:GUARD + numel].view(shape)
        if init is not None:
            t.copy_(torch.as_tensor(init).reshape(shape))
        elif dtype.is_floating_point and dtype != torch.bfloat16:
            t.fill_(float("nan"))
        self.bufs.append((raw, numel, t, init is None and not scratch and dtype.is_floating_point and dtype != torch.bfloat16))
        return t

    def check(self, tag):
        torch.cuda.synchronize()
        for raw, numel, t, must_fill in self.bufs:
            lo, hi = raw[:GUARD].view(torch.uint8), raw[GUARD + numel:].view(torch.uint8)
            assert bool((lo == CANARY).all()) and bool((hi == CANARY).all()), f"{tag}: written outside a buffer of {numel} elements"
            if must_fill:
                assert bool(torch.isfinite(t).all()), f"{tag}: an output of {numel} elements is not finite / not fully written"


@pytest.fixture
def guard():
    return Guarded()


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _ids(entry):
    return dict(argvalues=rows(entry), ids=[case_id(c) for c in rows(entry)])


def report(tag, **ratios):
    print(f"[tail] {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + " (of its bound; <= 1)")
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------ P2CL
def _p2cl_up(lib, guard, c, inp, with_grad=True):
    s = c.shape
    B, S, h, w, H, W = (s[k] for k in "BShwHW")
    nband = lib.vpu_p2cl_up_nband(h, w)
    plan = p2cl_up_plan(h, w, H, W, S)
    assert plan["admitted"] and nband == plan["nband"] and plan["max_block_rows"] <= plan["max_rows"] and plan["tables_exact"]
    low, gt, ov, idx = cu(inp["low"]), cu(inp["gt"]), cu(inp["ov"]), cu(inp["idx"])
    bands = guard.alloc((B * S, nband))
    dlow = guard.alloc((B, S, h, w)) if with_grad else None
    rc = lib.vpu_p2cl_up_fwd_bwd(ptr(low), ptr(gt), ptr(idx), ptr(ov), ptr(bands), ptr(dlow), inp["gs"], B, S, h, w, H, W, stream())
    assert rc == 0, rc
    guard.check(case_id(c))
    return bands, dlow


@pytest.mark.parametrize("c", **_ids("p2cl_up"))
def test_p2cl_up(lib, guard, c):
    """per-band loss sums and d loss / d low against float64; the loss-only call gives the same bits"""
    s, inp = c.shape, tr.p2_inputs(c)
    bands, dlow = _p2cl_up(lib, guard, c, inp)
    ref = tr.p2_ref(inp, s["h"], s["w"], s["H"], s["W"], p2cl_band(s["w"]))
    a, b = tr.p2_worst(bands.cpu(), dlow.cpu(), ref, c.regime == "saturated")
    report(case_id(c), sums=a, dlow=b)
    if c.regime == "saturated":
        assert dlow.abs().max().item() > 1e11 * inp["gs"]          # the opposite planes' gradient is there
    only, _ = _p2cl_up(lib, guard, c, inp, with_grad=False)
    assert torch.equal(only.view(torch.int32), bands.view(torch.int32))


@pytest.mark.parametrize("c", **_ids("p2cl_up_items"))
def test_p2cl_up_more_items_than_workgroups(lib, guard, c):
    """576 items, a little over two per CU: every workgroup prefetches across item and plane boundaries, override slots on
    consecutive planes among them; reserving CUs moves every boundary and must not move a bit"""
    from pvpuformer_amd import ops
    s, inp = c.shape, tr.p2_inputs(c)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * ncu < s["B"] * s["S"] * lib.vpu_p2cl_up_nband(s["h"], s["w"]) <= 3 * ncu
    bands, dlow = _p2cl_up(lib, guard, c, inp)
    ref = tr.p2_ref(inp, s["h"], s["w"], s["H"], s["W"], p2cl_band(s["w"]))
    a, b = tr.p2_worst(bands.cpu(), dlow.cpu(), ref, False)
    report(case_id(c), sums=a, dlow=b)
    try:
        for r in (16, 128):
            ops.gemm_set_option("reserve_cus", r)
            b2, d2 = _p2cl_up(lib, guard, c, inp)
            assert torch.equal(b2.view(torch.int32), bands.view(torch.int32)) and torch.equal(d2.view(torch.int32), dlow.view(torch.int32)), r
    finally:
        ops.gemm_set_option("reserve_cus", 0)


@pytest.mark.parametrize("c", **_ids("p2cl"))
def test_p2cl_unfused(lib, guard, c):
    """per-plane loss sums and d loss / d prob of p2cl_kernel under, at and over one trip of its 1024 threads"""
    s, inp = c.shape, tr.p2_inputs(c)
    B, S, HW = s["B"], s["S"], s["HW"]
    prob, gt, ov, idx = cu(inp["low"]), cu(inp["gt"]), cu(inp["ov"]), cu(inp["idx"])
    part, dprob = guard.alloc((B * S, 1)), guard.alloc((B, S, 1, HW))
    rc = lib.vpu_p2cl_fwd_bwd(ptr(prob), ptr(gt), ptr(idx), ptr(ov), ptr(part), ptr(dprob), inp["gs"], B, S, 1, HW, stream())
    assert rc == 0, rc
    guard.check(case_id(c))
    ref = tr.p2_ref(inp, 1, HW, 1, HW)
    a, b = tr.p2_worst(part.cpu(), dprob.cpu(), ref, c.regime == "saturated")
    report(case_id(c), sums=a, dprob=b)
    only = guard.alloc((B * S, 1))
    assert lib.vpu_p2cl_fwd_bwd(ptr(prob), ptr(gt), ptr(idx), ptr(ov), ptr(only), None, inp["gs"], B, S, 1, HW, stream()) == 0
    guard.check(case_id(c))
    assert torch.equal(only.view(torch.int32), part.view(torch.int32))


# ------------------------------------------------------------------------------------------------ NFL + Dice, loss_finalize
@pytest.mark.parametrize("c", **_ids("nfl_dice"))
def test_nfl_dice(lib, guard, c):
    """per-sample NFL and Dice and the logit gradient against float64; the call without a gradient buffer gives the same losses"""
    inp = tr.nfl_inputs(c)
    B, HW = inp["logits"].shape
    x, t = cu(inp["logits"]), cu(inp["gt"])
    nd = lib.vpu_nfl_dice_scratch_doubles(B)
    out, dl, sums = guard.alloc((B, 2)), guard.alloc((B, HW)), guard.alloc((nd,), torch.float64, scratch=True)
    rc = lib.vpu_nfl_dice_fwd_bwd(ptr(x), ptr(t), ptr(sums), ptr(out), ptr(dl), inp["w_nfl"], inp["w_dice"], B, HW, stream())
    assert rc == 0, rc
    # (of the scratch, row 0 and words 6, 7 of each row are never written: it is not an output, only its guards are checked)
    guard.check(case_id(c))
    ref = tr.nfl_ref(inp)
    a, b = tr.nfl_worst(out.cpu(), dl.cpu(), ref)
    report(case_id(c), losses=a, dlogits=b)
    o2, s2 = guard.alloc((B, 2)), torch.full((nd,), float("nan"), device="cuda", dtype=torch.float64)
    assert lib.vpu_nfl_dice_fwd_bwd(ptr(x), ptr(t), ptr(s2), ptr(o2), None, inp["w_nfl"], inp["w_dice"], B, HW, stream()) == 0
    guard.check(case_id(c))
    assert torch.equal(o2.view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("c", **_ids("finalize"))
def test_loss_finalize(lib, guard, c):
    inp = tr.finalize_inputs(c)
    B, npart = c.shape["B"], c.shape["npart"]
    out, part, res = cu(inp["out"]), cu(inp["part"]), guard.alloc((4,))
    assert lib.vpu_loss_finalize(ptr(out), ptr(part), B, npart, inp["inv"], *inp["w"], ptr(res), stream()) == 0
    guard.check(case_id(c))
    ref = tr.finalize_ref(inp)
    report(case_id(c), res=tr.worst(res.cpu(), ref, ref.abs()) / 1e-6)


# ------------------------------------------------------------------------------------------------ Adam
def _adam(lib, guard, c):
    inp = tr.adam_inputs(c)
    n, o, seg = c.shape["n"], c.opt, inp["seg"]
    p, m, v = (guard.alloc((n,), init=inp[k]) for k in "pmv")
    g = cu(inp["g"])
    sh = guard.alloc((n,), torch.bfloat16) if o["shadow"] else None
    se, sl, sw = (cu(seg[k]) for k in ("end", "lr", "wd")) if seg is not None else (None, None, None)
    nseg = 0 if seg is None else len(seg["end"])
    f = lambda k: inp[k]
    if c.entry == "adam":
        rc = lib.vpu_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), n, f("lr"), f("b1"), f("b2"), f("eps"), f("wd"), f("step"), f("gs"), stream())
    elif c.entry == "adam_groups":
        rc = lib.vpu_adam_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), n, ptr(se), ptr(sl), ptr(sw), nseg, f("b1"), f("b2"),
                                      f("eps"), int(f("decoupled")), f("step"), f("gs"), stream())
    else:
        hyper = cu(inp["hyper"])
        rc = lib.vpu_adam_step_hyper(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), n, ptr(hyper), ptr(se), ptr(sl), ptr(sw), nseg, f("b1"),
                                     f("b2"), f("eps"), f("wd"), int(f("decoupled")), stream())
    assert rc == 0, rc
    guard.check(case_id(c))
    return inp, dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy()), sh


@pytest.mark.parametrize("entry", ["adam", "adam_groups", "adam_hyper"])
def test_adam(lib, guard, entry):
    """p', m' and v' of one launch per row against the kernel's formula in float64 (bounds: tail_ref.adam_bounds); the bf16
    shadow, where the row has one, is p' rounded to nearest even, bit for bit; the zero padding between tensors keeps its bits"""
    top = dict(p=0.0, m=0.0, v=0.0)
    for c in rows(entry):
        inp, got, sh = _adam(lib, guard, c)
        ref = tr.adam_ref(c, inp)
        w = tr.adam_worst(c, got, ref)
        for k in top:
            top[k] = max(top[k], w[k])
        assert max(w.values()) <= 1.0, (case_id(c), w)
        if sh is not None:
            assert np.array_equal(sh.view(torch.int16).cpu().numpy(), tr.bf16_bits(got["p"])), case_id(c)
        if inp["seg"] is not None and inp["seg"]["pad"].any():
            pad = inp["seg"]["pad"]
            assert all((got[k][pad].view(np.int32) == 0).all() for k in "pmv"), case_id(c)
            assert sh is None or (sh.view(torch.int16).cpu().numpy()[pad] == 0).all()
        guard.bufs.clear()
    report(f"{entry}: {len(rows(entry))} rows", **top)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("c", **_ids("dropout"))
def test_dropout_mask_is_splitmix64(lib, guard, c):
    """three consecutive calls from a given (call number, seed word): every mask equals the Python splitmix64 of
    (seed ^ state[1], call, i + 1) bit for bit, state[0] advances by one per call, state[1] stays"""
    n, keep = c.shape["n"], c.opt["keep"]
    seed, word, call0 = 0x1234567, 0x0F1E2D3C4B5A6978, 41
    state = torch.tensor([call0, word], dtype=torch.int64, device="cuda")
    for k in range(3):
        out = guard.alloc((n,))
        assert lib.vpu_dropout_mask(ptr(out), n, keep, seed, ptr(state), stream()) == 0
        guard.check(case_id(c))
        want = tr.dropout_ref(n, keep, seed, word, call0 + k)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (case_id(c), k)
        assert state.tolist() == [call0 + k + 1, word]


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_call(lib, c, p):
    """the launcher call of a refuse row: every pointer is the sentinel buffer (large enough for the launch, were it made)"""
    s, fn, bad, st = c.shape, c.opt["fn"], c.regime, stream()
    if fn == "p2cl_up":
        return lib.vpu_p2cl_up_fwd_bwd(p, p, None, None, p, p, 1.0, 1, s["S"], s["h"], s["w"], s["H"], s["W"], st)
    if fn == "p2cl":
        return lib.vpu_p2cl_fwd_bwd(p, p, None, None, p, p, 1.0, 1, s["S"], s["H"], s["W"], st)
    if fn == "nfl_dice":
        return lib.vpu_nfl_dice_fwd_bwd(p, p, p, p, p, 1.0, 1.0, 1, s["HW"], st)
    if fn == "finalize":
        return lib.vpu_loss_finalize(None if bad == "out null" else p, None if bad == "part null" else p, 0 if bad == "B 0" else 4,
                                     0 if bad == "npart 0" else 4, 1.0, 1.0, 1.0, 1.0, 1.0, None if bad == "res null" else p, st)
    n, step = (0 if bad == "n 0" else 8), (0 if bad == "step 0" else 1)
    null = lambda name: None if bad == f"{name} null" else p
    if fn == "adam":
        return lib.vpu_adam_step(p, p, p, p, p, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, 1.0, st)
    if fn == "adam_groups":
        return lib.vpu_adam_step_groups(p, p, p, p, p, n, null("seg_end"), null("seg_lr"), null("seg_wd"), 0 if bad == "nseg 0" else 1,
                                        0.9, 0.999, 1e-8, 0, step, 1.0, st)
    assert fn == "adam_hyper"
    return lib.vpu_adam_step_hyper(p, p, p, p, p, n, null("hyper"), null("seg_end"), null("seg_scale"), null("seg_wd"), 1, 0.9, 0.999,
                                   1e-8, 0.0, 0, st)


@pytest.mark.parametrize("c", **_ids("refuse"))
def test_refusals_answer_before_any_launch(lib, c):
    sentinel = torch.full((1 << 18,), 7.0, device="cuda")
    assert _refusal_call(lib, c, sentinel.data_ptr()) == VPU_ERR_ARG, case_id(c)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
