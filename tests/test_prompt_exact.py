"""The prompt and click-bookkeeping kernels of csrc/prompt.hip against references that share nothing with them, bit for bit, at the
launchers' edges: the exact and the 5 x 5 chamfer distance transforms, the 8-connected components and their table, the disk maps
and the thick-line rasteriser, the PuE rows, mask_bbox / masked_argmax / error_masks, and the arguments the launchers turn down.

The module walks tests/prompt_cases.py, one parametrised test per entry (tests/test_prompt_cases_cpu.py checks that the table
reaches every launcher branch, that the references of tests/prompt_ref.py agree with a second one, and that they tell a planted
error).  Everything integer, mask, index or key is compared with array_equal; the f32 PuE click rows and out64 are bit-equal to
the reference, the bf16 rows bit-equal to the f32 launch rounded once by torch; the box rows (the only expf) have the reference's
support and its values within the tolerances of test_ops_gpu.py::test_pue_and_disks_bit_exact: 2e-7 against the oracle, 3e-7
against what the reference model recorded (tests/golden/prompt_edges.npz).

Memory: every output -- those the ops wrappers allocate too, through a stand-in for their torch.empty -- is the middle of a
larger buffer filled with a canary byte, and the guard on either side must come out untouched; an output the kernel has to write
in full starts as canary as well, so a pixel left out cannot pass as a zero.

Rows: edt 70, chamfer5 74, cc 150 and cc_table 4 (roots and table in one test), disk 108, pue 48, line 52, bbox 72, argmax 70,
errmask 5, refuse 9.  On an MI355X every row passes; against the kernels as they were before this table, three rows failed, all
of them edt without border and with a single zero in row 0: 16385 x 1 (1 pixel), 20000 x 3 (10848 pixels) and 32767 x 1 (16383
pixels) came out +inf from row 16384 on, where the squared distance reaches the 2^28 the row pass used both as "no zero pixel" and
as the start of its search; 16383 x 1, 16384 x 1 and 20000 x 3 with the border were right.  The row pass is unsigned now."""
import os

import numpy as np
import pytest
import torch

import prompt_ref as pr
import vpu_oracle as vo
from prompt_cases import case_id, rows

pytestmark = pytest.mark.gpu

CANARY = 0x5A
GUARD = 256                 # elements on either side


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, pr.GOLDEN_FILE))


class Guarded:
    """allocations with a canary-filled guard before and after"""

    def __init__(self):
        self.bufs = []

    def alloc(self, shape, dtype, zero=False):
        shape = tuple(int(s) for s in (shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape))
        numel = int(np.prod(shape, dtype=np.int64))
        raw = torch.empty(numel + 2 * GUARD, device="cuda", dtype=dtype)
        raw.view(torch.uint8).fill_(CANARY)
        t = raw[GUARD:GUARD + numel].view(shape)
        if zero:
            t.zero_()
        self.bufs.append((raw, numel))
        return t

    def check(self, tag, untouched=False):
        torch.cuda.synchronize()
        for raw, numel in self.bufs:
            lo, hi = raw[:GUARD].view(torch.uint8), raw[GUARD + numel:].view(torch.uint8)
            assert bool((lo == CANARY).all()) and bool((hi == CANARY).all()), f"{tag}: written outside an output of {numel} elements"
            if untouched:
                assert bool((raw.view(torch.uint8) == CANARY).all()), f"{tag}: an output was written to"


class _TorchWithGuardedEmpty:
    """what pvpuformer_amd.ops sees as ``torch`` during a test: its torch.empty comes from a Guarded"""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, device=None, dtype=None):
        assert str(device).startswith("cuda")
        return self._guard.alloc(shape, dtype)


@pytest.fixture
def guard(ops, monkeypatch):
    g = Guarded()
    monkeypatch.setattr(ops, "torch", _TorchWithGuardedEmpty(g))
    return g


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, tag):
    """array_equal with the first difference in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        bad = got.view(f"u{got.dtype.itemsize}") != want.view(f"u{want.dtype.itemsize}")
        bad &= ~((got == 0) & (want == 0))                      # (no kernel here writes a negative zero; the sign is not the point)
    else:
        bad = got != want
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}")


def _ids(entry):
    return dict(argvalues=rows(entry), ids=[case_id(c) for c in rows(entry)])


# ------------------------------------------------------------------------------------------------ distance transforms
@pytest.mark.parametrize("c", **_ids("edt"))
def test_edt(ops, guard, c):
    inp, ref = pr.case_data(c)
    got = ops.edt(cu(inp["mask"]), zero_border=c.opt["border"])
    guard.check(case_id(c))
    same(got.cpu().numpy(), ref["dist"], case_id(c))


@pytest.mark.parametrize("c", **_ids("chamfer5"))
def test_chamfer5(ops, guard, c):
    inp, ref = pr.case_data(c)
    got = ops.chamfer5(cu(inp["mask"]), zero_border=c.opt["border"])
    guard.check(case_id(c))
    same(got.cpu().numpy(), ref["dist"], case_id(c))


# ------------------------------------------------------------------------------------------------ components
@pytest.mark.parametrize("c", rows("cc") + rows("cc_table"), ids=[case_id(c) for c in rows("cc") + rows("cc_table")])
def test_cc_roots_and_table(ops, guard, c):
    inp, ref = pr.case_data(c)
    tag, kmax = case_id(c), c.opt["kmax"]
    roots = ops.cc_roots(cu(inp["mask"]))
    flat = ops.cc_table(roots, kmax)
    guard.check(tag)
    same(roots.cpu().numpy(), ref["roots"], tag)
    flat = flat.cpu().numpy().astype(np.int64)
    want = ref["table"]
    assert flat[-1] == len(want), (tag, "component count", flat[-1], len(want))
    table = flat[:6 * min(len(want), kmax)].reshape(-1, 6)
    table = table[np.argsort(table[:, 0])]
    if len(want) <= kmax:
        same(table, want, tag + " table")
    else:                                  # more components than rows: kmax of them, each one whole, and the count says so
        assert len(np.unique(table[:, 0])) == kmax, tag
        by_root = {int(r[0]): r for r in want}
        for r in table:
            assert int(r[0]) in by_root and np.array_equal(r, by_root[int(r[0])]), (tag, r)


# ------------------------------------------------------------------------------------------------ disk maps and the rasteriser
@pytest.mark.parametrize("c", **_ids("disk"))
def test_disk_maps(ops, guard, golden, c):
    inp, ref = pr.case_data(c)
    s, tag = c.shape, case_id(c)
    out = guard.alloc((s["B"], 2, s["H"], s["W"]), torch.float32)
    boxes = cu(inp["boxes"]) if "boxes" in inp else None
    ops.disk_maps(cu(inp["points"]), boxes, out, s["B"], s["n"], s["H"], s["W"], float(c.opt["radius"]))
    guard.check(tag)
    got = out.cpu().numpy()
    same(got, ref["disks"], tag)
    key = pr.golden_key(c)
    if key is not None:
        assert np.array_equal(golden[key + "_points"], inp["points"]), tag
        rec = np.unpackbits(golden[key + "_out"])[:got.size].reshape(got.shape).astype(np.float32)
        same(got, rec, tag + " (recorded)")


@pytest.mark.parametrize("c", **_ids("line"))
def test_thick_lines(ops, guard, c):
    inp, ref = pr.case_data(c)
    s, tag = c.shape, case_id(c)
    if c.opt["kind"] == "box":             # the outline alone: no click in any slot
        n = int(inp["n"])
        out = guard.alloc((s["B"], 2, s["H"], s["W"]), torch.float32)
        ops.disk_maps(-torch.ones(s["B"], 2 * n, 3, device="cuda"), cu(inp["boxes"]), out, s["B"], n, s["H"], s["W"], 5.0)
    else:
        out = guard.alloc((s["B"], 2, s["H"], s["W"]), torch.float32, zero=True)
        ops.draw_polyline(cu(inp["curve"]), out, s["B"], s["P"], s["H"], s["W"])
    guard.check(tag)
    same(out.cpu().numpy(), ref["disks"], tag)


# ------------------------------------------------------------------------------------------------ PuE rows
def _pue_launch(ops, guard, inp, s, dtype, out64):
    B, R, E = inp["points"].shape[0], 2 * s["num_max"], 2 * s["img"] + 3
    out = guard.alloc((B, R, s["ld"]), dtype)
    o64 = guard.alloc((B, R, E), torch.float64) if out64 else None
    boxes = cu(inp["boxes"]) if "boxes" in inp else None
    ops.pue_encode(cu(inp["points"]), boxes, cu(vo.click_lut()), out, o64, B, s["n"], s["num_max"], s["img"], s["ld"])
    return out, o64


@pytest.mark.parametrize("c", **_ids("pue"))
def test_pue_rows(ops, guard, golden, c):
    inp, ref = pr.case_data(c)
    s, tag = c.shape, case_id(c)
    E = 2 * s["img"] + 3
    want, box_rows = ref["rows"], ref["box_rows"]
    if c.dtype == "f32":
        (out, o64), outb = _pue_launch(ops, guard, inp, s, torch.float32, c.opt["out64"]), None
    else:                                  # the bf16 launch writes out64 (the f32 value, widened); an f32 launch to round from
        out = _pue_launch(ops, guard, inp, s, torch.float32, False)[0]
        outb, o64 = _pue_launch(ops, guard, inp, s, torch.bfloat16, c.opt["out64"])
    guard.check(tag)
    key = pr.golden_key(c)
    rec = None
    if key is not None:
        assert np.array_equal(golden[key + "_points"], inp["points"]), tag
        assert "boxes" not in inp or np.array_equal(golden[key + "_boxes"], inp["boxes"]), tag
        rec = golden[key + "_out"]
    assert bool((out[:, :, E:] == 0).all()), f"{tag}: padding columns"
    f32 = out[:, :, :E].cpu().numpy()
    views = [("out", f32.astype(np.float64))] + ([("out64", o64.cpu().numpy())] if o64 is not None else [])
    if o64 is not None:
        same(views[1][1], views[0][1], tag + ": out64 against out")
    for name, got in views:
        same(got[~box_rows], want[~box_rows], f"{tag} {name} click rows")
        if rec is not None:
            same(got[~box_rows], rec[~box_rows], f"{tag} {name} click rows (recorded)")
        if box_rows.any():
            assert np.array_equal(got[box_rows] != 0, want[box_rows] != 0), f"{tag} {name}: support of the box rows"
            np.testing.assert_allclose(got[box_rows], want[box_rows], atol=2e-7, rtol=0, err_msg=f"{tag} {name}")
            if rec is not None:
                assert np.array_equal(got[box_rows] != 0, rec[box_rows] != 0), f"{tag} {name}: support of the box rows (recorded)"
                np.testing.assert_allclose(got[box_rows], rec[box_rows], atol=3e-7, rtol=0, err_msg=f"{tag} {name} (recorded)")
    if outb is not None:                   # the same f32 value, rounded once
        assert torch.equal(outb.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), f"{tag}: bf16 rows"


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("c", **_ids("bbox"))
def test_mask_bbox(ops, guard, c):
    inp, ref = pr.case_data(c)
    got = ops.mask_bbox(cu(inp["prob"]), float(inp["thr"]), cu(inp["clicks"]) if "clicks" in inp else None)
    guard.check(case_id(c))
    same(got.cpu().numpy(), ref["box"], case_id(c))


@pytest.mark.parametrize("c", **_ids("argmax"))
def test_masked_argmax(ops, guard, c):
    inp, ref = pr.case_data(c)
    got = ops.masked_argmax(cu(inp["dist"]), cu(inp["keep"]))
    guard.check(case_id(c))
    same(got.cpu().numpy().view(np.uint64), ref["key"], case_id(c))


@pytest.mark.parametrize("c", **_ids("errmask"))
def test_error_masks(ops, guard, c):
    inp, ref = pr.case_data(c)
    got = ops.error_masks(cu(inp["pred"]), cu(inp["gt"]), cu(inp["valid"]))
    guard.check(case_id(c))
    same(got.cpu().numpy(), ref["masks"], case_id(c))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("c", **_ids("refuse"))
def test_refusals_answer_before_any_launch(ops, guard, c):
    """as test_ops_gpu.py::test_argument_errors_answer_before_any_launch: a VpuError that names the rule, nothing launched (every
    output the call was given or allocated still holds the canary, no error is pending), and the library still works"""
    from pvpuformer_amd import _lib
    s, tag = c.shape, case_id(c)
    z = lambda *shape, dt=torch.uint8: torch.zeros(*shape, device="cuda", dtype=dt)
    with pytest.raises(_lib.VpuError) as e:
        if c.regime == "edt":
            ops.edt(z(s["B"], s["H"], s["W"]), zero_border=False)
        elif c.regime == "chamfer5":
            ops.chamfer5(z(s["B"], s["H"], s["W"]), zero_border=c.opt["border"])
        elif c.regime == "bbox":
            ops.mask_bbox(z(s["B"], s["H"], s["W"], dt=torch.float32), 0.49)
        elif c.regime == "disk":
            ops.disk_maps(-torch.ones(s["B"], 2 * s["n"], 3, device="cuda"), None, guard.alloc((s["B"], 2, s["H"], s["W"]), torch.float32),
                          s["B"], s["n"], s["H"], s["W"], 5.0)
        else:
            assert c.regime == "pue", c.regime
            ops.pue_encode(-torch.ones(s["B"], 2 * s["n"], 3, device="cuda"), None, cu(vo.click_lut()),
                           guard.alloc((s["B"], 2 * s["num_max"], max(s["ld"], 2 * s["img"] + 3)), torch.float32), None,
                           s["B"], s["n"], s["num_max"], s["img"], s["ld"])
    assert "failed (-" in str(e.value) and len(str(e.value).split(": ", 1)[1]) > 8, (tag, str(e.value))
    assert guard.bufs, tag
    guard.check(tag, untouched=True)
    got = ops.edt(torch.tensor([[[0, 1, 1]]], device="cuda", dtype=torch.uint8), zero_border=False)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [[[0.0, 1.0, 2.0]]]
