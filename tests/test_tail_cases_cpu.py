"""CPU checks of the loss / optimizer test table (tests/tail_cases.py) and of its references (tests/tail_ref.py):
1. the table reaches every branch and edge of the launchers' arithmetic, asserted through the plan functions;
2. the invariants p2cl_up_kernel relies on without checking them hold over the whole admitted space, in np.float32 as the kernel
   computes them: the anchor index is monotone, the kernel's table of first rows is the true one, no cell owns more than P2_SPAN
   rows, no (band, halo) item owns more than max_rows pixel rows (max_rows - 1 is reached, max_rows never exceeded -- the
   kernel would write past its LDS), and the LDS refusal cannot be reached once the other checks pass;
3. the references agree with a second, dumber one: a per-pixel loop, torch.optim.Adam / AdamW, the oracle's loss functions;
4. each table discriminates: a reference with one error planted leaves the bounds of tests/test_tail_f64.py on at least one
   row of its entry (the rows an error applies to are counted: the check is not vacuous)."""
import numpy as np
import pytest
import torch

import tail_ref as tr
from tail_cases import (ADAM_N, ADAM_REGIMES, ADAM_STEPS, CASES, DROPOUT_N, ENTRIES, FINALIZE, NFL_B, NFL_HW, NFL_REGIMES,
                        P2_LDS_LIMIT, P2_REGIMES, P2_SHAPES, P2_SPAN, P2CL_HW, Case, adam_plan, block_rows, case_id, finalize_plan,
                        first_rows, max_rows_of, nfl_final_blocks, nfl_plan, p2cl_band, p2cl_up_plan, rows, seg_layout)


def _hw(c):
    s = c.shape
    return s["h"], s["w"], s["H"], s["W"]


# ------------------------------------------------------------------------------------------------ 1. coverage
def test_table_is_well_formed():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c.entry for c in CASES} == set(ENTRIES)
    assert all(rows(e) for e in ENTRIES)


def test_table_p2cl_up():
    up = rows("p2cl_up")
    issue = [(2, 2, 2, 4), (512, 2, 512, 4), (9, 3, 9, 4), (17, 5, 17, 8), (16, 128, 16, 128), (9, 8, 5, 4), (10, 342, 12, 344),
             (10, 341, 12, 344), (2, 512, 4, 1028), (7, 300, 14, 1200), (9, 113, 33, 452), (12, 12, 52, 52), (6, 7, 25, 28)]
    assert {_hw(c) for c in up} == set(P2_SHAPES) >= set(issue)
    for shp in P2_SHAPES:                                   # every shape with every label regime, with and without slots
        mine = [c for c in up if _hw(c) == shp]
        assert {(c.regime, c.opt["slots"]) for c in mine} == {(r, s) for r in P2_REGIMES for s in (False, True)}
    plans = {shp: p2cl_up_plan(*shp) for shp in P2_SHAPES}
    assert all(p["admitted"] and p["tables_exact"] and p["monotone"] for p in plans.values())
    assert all(p["max_cell_rows"] <= P2_SPAN and p["max_cell_cols"] <= P2_SPAN and p["max_block_rows"] <= p["max_rows"]
               and p["shmem"] <= P2_LDS_LIMIT for p in plans.values())
    assert {p["band"] for p in plans.values()} == set(range(1, 9))
    assert plans[(10, 342, 12, 344)]["band"] == 1 and plans[(10, 341, 12, 344)]["band"] == 2
    assert {min(p["nrp"], 2) for p in plans.values()} == {0, 1, 2}
    assert plans[(2, 512, 4, 1028)]["nrp"] == 0 and plans[(7, 300, 14, 1200)]["nrp"] == 0
    assert {p["wide_quads"] for p in plans.values()} == {True, False} and plans[(12, 12, 52, 52)]["wide_quads"]
    assert sum(p["last_band_rows"] == 1 and p["nband"] > 1 for p in plans.values()) >= 4
    assert plans[(16, 128, 16, 128)]["ratio_one"] and plans[(9, 8, 5, 4)]["down"] == (True, True)
    assert plans[(2, 2, 2, 4)]["all_edge"] and plans[(512, 2, 512, 4)]["nband"] == 64
    assert plans[(9, 113, 33, 452)]["rounded_up"] and plans[(9, 113, 33, 452)]["nthr"] == 1024
    assert any(p["launch_threads"] == 64 for p in plans.values())
    h, w, H, W = 6, 7, 25, 28
    # the last admitted H; the last admitted W that is a multiple of 4 (W - 1 == 5 (w - 1) - 1 would be W 30)
    assert H - 1 == 5 * (h - 1) - 1 and W - 1 < 5 * (w - 1) <= W + 4 - 1
    assert plans[(6, 7, 25, 28)]["max_cell_rows"] == 5 == plans[(6, 7, 25, 28)]["max_cell_cols"] == plans[(12, 12, 52, 52)]["max_cell_rows"]
    items, = rows("p2cl_up_items")
    s = items.shape
    assert s["B"] * s["S"] * p2cl_up_plan(*_hw(items), S=s["S"])["nband"] == 576 > 2 * 256
    idx = tr.p2_inputs(items)["idx"].ravel()
    assert idx[10] >= 0 and idx[11] >= 0 and idx[9] < 0 and idx[12] < 0            # slots on consecutive planes, none around them
    assert {c.shape["HW"] for c in rows("p2cl")} == set(P2CL_HW) and {c.regime for c in rows("p2cl")} == set(P2_REGIMES)
    assert [(HW // 4 + 1023) // 1024 for HW in P2CL_HW] == [1, 1, 1, 2] and 4096 // 4 == 1024


def test_table_refusals():
    ref = rows("refuse")
    up = [c for c in ref if c.opt["fn"] == "p2cl_up"]
    plans = [(c, p2cl_up_plan(c.shape["h"], c.shape["w"], c.shape["H"], c.shape["W"], c.shape["S"])) for c in up]
    assert all(not p["admitted"] for _, p in plans)
    assert {p["refusal"] for _, p in plans} == {"args", "block"}        # (the third, "lds", cannot be reached: see the sweep)
    assert [c.regime for c, p in plans if p["refusal"] == "block"] == ["block"]
    assert {c.regime for c in up} >= {"S odd", "W % 4", "h 1", "h 513", "w 1", "w 513", "ratio 5 in H", "ratio 5 in W"}
    for c, p in plans:      # each row is turned down by the one check it names: mending that argument alone admits it
        s = dict(c.shape)
        fix = {"S odd": dict(S=2), "W % 4": dict(W=48), "h 1": dict(h=2), "h 513": dict(h=512, H=512), "w 1": dict(w=2),
               "w 513": dict(w=512), "ratio 5 in H": dict(H=55), "ratio 5 in W": dict(W=52), "block": dict(W=452)}[c.regime]
        s.update(fix)
        assert p2cl_up_plan(s["h"], s["w"], s["H"], s["W"], s["S"])["admitted"], c
    assert {c.opt["fn"] for c in ref} == {"p2cl_up", "p2cl", "nfl_dice", "finalize", "adam", "adam_groups", "adam_hyper"}
    assert not nfl_plan(6)["admitted"] and not finalize_plan(0, 1)["admitted"] and not finalize_plan(1, 0)["admitted"]
    assert not adam_plan(0)["admitted"]


def test_table_nfl_finalize_dropout():
    n = rows("nfl_dice")
    assert {(c.shape["HW"], c.shape["B"], c.regime) for c in n} == {(a, b, r) for a in NFL_HW for b in NFL_B for r in NFL_REGIMES}
    plans = {HW: nfl_plan(HW) for HW in NFL_HW}
    assert plans[4]["empty"] == 31 and plans[124]["empty"] == 1 and plans[128]["empty"] == 0 and plans[132]["empty"] == 15
    assert plans[132]["last_partial"] and not plans[128]["last_partial"]
    assert plans[4 * 32 * 256]["trips"] == 1 and plans[4 * 32 * 256]["per"] == 256 and plans[4 * 32 * 256 + 4]["trips"] == 2
    assert plans[4 * 32 * 256 + 4]["last_partial"] and plans[4 * 32 * 256 + 4]["empty"] == 0
    assert {nfl_final_blocks(B) for B in NFL_B} == {1, 2}
    for c in n:
        t = tr.nfl_inputs(c)["gt"]
        if c.regime == "one_ignored":
            assert (t[c.shape["B"] // 2] == -1).all() and (c.shape["B"] == 1 or (t != -1).any())
        if c.regime in ("all0", "all1"):
            assert (t == float(c.regime == "all1")).all()
        if c.regime == "pm20":
            assert (np.abs(tr.nfl_inputs(c)["logits"]) == 20).any()
    f = {(c.shape["B"], c.shape["npart"]) for c in rows("finalize")}
    assert f == set(FINALIZE)
    plans = [finalize_plan(*k) for k in FINALIZE]
    assert {p["trips_out"] for p in plans} == {1, 2} and {p["trips_part"] for p in plans} >= {1, 32}
    assert any(p["idle_threads"] == 255 for p in plans) and any(p["idle_part"] == 1 for p in plans)
    assert finalize_plan(257, 256)["idle_part"] == 0 and finalize_plan(257, 256)["trips_out"] == 2
    assert {(c.shape["n"], c.opt["keep"]) for c in rows("dropout")} == {(n, k) for n in DROPOUT_N for k in (1.0, 0.9)}


def test_table_adam():
    for entry in ("adam", "adam_groups", "adam_hyper"):
        mine = rows(entry)
        assert {c.shape["n"] for c in mine} >= set(ADAM_N)
        assert {c.regime for c in mine} == set(ADAM_REGIMES) and {c.opt["step"] for c in mine} == set(ADAM_STEPS)
        assert {c.opt["gs"] for c in mine} == {1.0, 0.5} and {c.opt["shadow"] for c in mine} == {True, False}
        assert {c.opt["wd"] for c in mine} == {0.0, 0.02}
        if entry != "adam":
            assert {(c.opt["decoupled"], c.opt["wd"] != 0) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}
        for r in ADAM_REGIMES:                 # every regime meets a first step, a later one and both grad scales
            assert {c.opt["step"] == 1 for c in mine if c.regime == r} == {True, False}
            assert {c.opt["gs"] for c in mine if c.regime == r} == {1.0, 0.5}
    assert {c.opt["layout"] for c in rows("adam_groups")} == {"one", "two8", "three", "thousand"}
    assert {c.opt["layout"] for c in rows("adam_hyper")} == {"none", "two8", "three", "thousand"}
    plans = [adam_plan(c.shape["n"], () if c.opt["layout"] in (None, "none") else [c.shape["n"]] if c.opt["layout"] == "one"
                       else seg_layout(c.opt["layout"])[1]) for c in rows("adam_groups") + rows("adam_hyper")]
    assert {p["tail"] for p in plans} == {0, 1, 2, 3} and {adam_plan(n)["tail"] for n in ADAM_N} == {0, 1, 3}
    assert {p["nseg"] for p in plans} == {0, 1, 2, 3, 1000} and max(p["depth"] for p in plans) == 10
    assert any(p["groups_at_segment_end"] for p in plans)
    assert {p["blocks"] for p in plans} >= {1, 2}
    n, seg_end, sizes, starts = seg_layout("two8")
    assert (n, seg_end, sizes) == (16, [8, 16], [8, 8]) and adam_plan(n, seg_end)["groups_at_segment_end"] == [4, 12]
    n, seg_end, sizes, starts = seg_layout("thousand")
    assert all(s % 8 == 0 for s in starts) and 8 in sizes and any(s % 8 for s in sizes) and n == seg_end[-1]
    inp = tr.adam_inputs([c for c in rows("adam_groups") if c.opt["layout"] == "thousand" and c.regime == "unit"][0])
    pad = inp["seg"]["pad"]
    assert pad.any() and all((inp[k][pad] == 0).all() for k in "pgmv") and (inp["g"][~pad] != 0).all()
    tiny = tr.adam_inputs([c for c in rows("adam") if c.regime == "tiny" and c.shape["n"] == 1027][0])
    assert 1e-12 <= np.abs(tiny["g"]).min() and np.abs(tiny["g"]).max() <= 1e-7 and np.sqrt(tiny["v"].max()) < tr.EPS * 10


# ------------------------------------------------------------------------------------------------ 2. launcher invariants
_H_LIST = lambda h: {1, 2, h - 1, h, h + 1, 2 * h, 3 * h + 1, 4 * h, 4 * (h - 1) + 1, 5 * (h - 1) - 3, 5 * (h - 1) - 1, 5 * (h - 1)}


def test_anchor_tables_and_max_rows_over_the_admitted_space():
    """every (h, H) with 2 <= h <= 64 and H admitted ((H - 1) < 5 (h - 1)), and the edge list of H for h up to 512; the same
    function serves rows and columns, so (w, W) is covered with it"""
    slack = {b: 10 ** 9 for b in range(1, 9)}
    npairs = 0
    for h in range(2, 513):
        Hs = range(1, 5 * (h - 1) + 1) if h <= 64 else sorted(H for H in _H_LIST(h) if 1 <= H <= 5 * (h - 1))
        assert 5 * (h - 1) in Hs and 5 * (h - 1) + 1 not in Hs
        for H in Hs:
            t, true, a = first_rows(h, H)
            assert (np.diff(a) >= 0).all() and a[0] == 0 and a[-1] <= h - 1, (h, H)
            assert (t == true).all(), (h, H)                           # the walk's start never lies beyond the row it looks for
            assert t[0] == 0 and t[1] == 0 and t[h + 1] == H and t[h + 2] == H
            assert np.diff(t).max() <= P2_SPAN and np.bincount(a).max() <= P2_SPAN, (h, H)
            for band in range(1, 9):
                s = max_rows_of(band, h, H) - int(block_rows(t, h, band).max())
                assert s >= 0, (h, H, band)
                slack[band] = min(slack[band], s)
            npairs += 1
    print(f"[tail] {npairs} (h, H) pairs; least max_rows - pixel rows per band: {slack}")
    # (never exceeded; and tight: of the launcher's "+ 2 for rounding" exactly one row is spare at every band, no more)
    assert all(v == 1 for v in slack.values())


def test_lds_refusal_cannot_be_reached():
    """shmem grows with W and with max_rows, max_rows with H: at every w and h, the largest W the other checks admit and the
    largest H stay below the LDS limit, so the `shmem >` test of the launcher never decides"""
    top = 0
    for w in range(2, 513):
        band = p2cl_band(w)
        W = min(5 * (w - 1), 4 * (1024 // (band + 1)) + 3) // 4 * 4
        assert (band + 1) * (W // 4) <= 1024 and W - 1 < 5 * (w - 1)
        assert (band + 1) * ((W + 4) // 4) > 1024 or W + 4 - 1 >= 5 * (w - 1)
        h = np.arange(2, 513)
        max_rows = ((band + 1) * (5 * (h - 1) - 1)) // (h - 1) + 2
        shmem = ((2 * band + 2) * w + (band + 2 + max_rows) * W) * 4
        top = max(top, int(shmem.max()))
    print(f"[tail] largest admitted p2cl_up LDS request {top} of {P2_LDS_LIMIT} bytes")
    assert top <= P2_LDS_LIMIT


# ------------------------------------------------------------------------------------------------ 3. references against a second one
@pytest.mark.parametrize("shape", [(2, 2, 2, 4), (3, 4, 11, 16), (6, 5, 5, 4), (6, 6, 25, 24), (4, 3, 4, 4)])
def test_p2cl_reference_against_a_pixel_loop(shape):
    h, w, H, W = shape
    for regime in P2_REGIMES[:2]:
        c = Case("p2cl_up", "f32", dict(B=1, S=4, h=h, w=w, H=H, W=W), dict(slots=True), regime)
        inp = tr.p2_inputs(c)
        ref = tr.p2_ref(inp, h, w, H, W, band=1)
        sums, dlow = tr.p2_pixel_loop(inp, h, w, H, W)
        assert tr.worst(ref["bands"], sums, sums.abs()) < 1e-12 and tr.worst(ref["dlow"], dlow, ref["A"]) < 1e-12
        coarse = tr.p2_ref(inp, h, w, H, W, band=4)["bands"]
        assert tr.worst(coarse.sum(-1), sums.sum(-1), sums.sum(-1).abs()) < 1e-12


def test_adam_reference_against_torch_optim():
    r = np.random.RandomState(5)
    n = 37
    f32 = lambda a: np.asarray(a, np.float32)
    for decoupled in (False, True):
        for wd in (0.0, 0.02):
            p0, gs = f32(r.randn(n)), [f32(r.randn(n) * 0.1) for _ in range(3)]
            q = torch.nn.Parameter(torch.from_numpy(p0).double())
            b1, b2, eps, lr = (float(np.float32(x)) for x in (tr.B1, tr.B2, tr.EPS, tr.LR))
            opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=float(np.float32(wd)))
            p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
            for t, g in enumerate(gs, 1):
                q.grad = torch.from_numpy(g).double()
                opt.step()
                inp = dict(p=p, g=g, m=m, v=v, seg=None, hyper=None, lr=lr, b1=b1, b2=b2, eps=eps, wd=float(np.float32(wd)), gs=1.0,
                           step=t, decoupled=decoupled)
                ref = tr.adam_ref(None, inp)
                p, m, v = ref["p"], ref["m"], ref["v"]
            st = opt.state[q]
            np.testing.assert_allclose(p, q.detach().numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_nfl_dice_reference_against_the_oracle():
    import vpu_oracle as vo
    for c in [c for c in rows("nfl_dice") if c.shape["HW"] in (4, 132) and c.shape["B"] == 65 or c.shape["HW"] == 4 * 32 * 256 + 4 and c.shape["B"] == 1]:
        inp = tr.nfl_inputs(c)
        ref = tr.nfl_ref(inp)
        B, HW = inp["logits"].shape
        x = torch.from_numpy(inp["logits"]).double().view(B, 1, 1, HW).requires_grad_(True)
        t = torch.from_numpy(inp["gt"]).double().view(B, 1, 1, HW)
        nfl = vo.nfl_loss(x, t)
        dice = torch.stack([vo.dice_loss_naive(x[b:b + 1], t[b:b + 1].double()) for b in range(B)])
        g, = torch.autograd.grad(nfl.sum() * inp["w_nfl"] + dice.sum() * inp["w_dice"], x)
        # (dice_loss_naive casts its target to fp32 and sums it there: exact for -1, 0 and 1, ~1e-7 of the sum with soft labels)
        tol = 1e-12 if c.regime in ("all0", "all1") else 1e-5
        assert tr.worst(ref["nfl"], nfl.detach(), nfl.detach().abs()) < 1e-12, case_id(c)
        assert tr.worst(ref["dice"], dice.detach(), dice.detach().abs()) < tol, case_id(c)
        assert tr.worst(ref["g"], g.view(B, HW), ref["A"]) < tol, case_id(c)


def test_dropout_reference_is_splitmix64():
    """the first outputs of the published splitmix64 from state 0, whose finaliser the mask uses, and the mask's own arithmetic:
    counters that wrap at 2^64, keep 1.0 keeps everything, the kept fraction at 0.9"""
    def splitmix(x):
        x = (x + 0x9E3779B97F4A7C15) & tr.M64
        z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & tr.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & tr.M64
        return z ^ (z >> 31)
    assert splitmix(0) == 0xE220A8397B1DCDAF and splitmix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert (tr.dropout_ref(300, 1.0, 5, 9, 2) == 1.0).all()
    m = tr.dropout_ref(3072, 0.9, 2 ** 63 - 1, 12345, 2 ** 40)
    assert set(np.unique(m)) == {np.float32(0), np.float32(1) / np.float32(0.9)} and abs((m != 0).mean() - 0.9) < 0.02
    assert not np.array_equal(m, tr.dropout_ref(3072, 0.9, 2 ** 63 - 1, 12345, 2 ** 40 + 1))
    assert np.array_equal(tr.dropout_ref(64, 0.9, 6, 3, 0), tr.dropout_ref(64, 0.9, 5, 0, 0))        # seed ^ state[1]


# ------------------------------------------------------------------------------------------------ 4. discrimination
P2_PLANTS = ("ignore_inverted", "no_eps", "halo_lower_dropped", "halo_counted", "soft_as_one", "last_col_clamp", "row5", "row6")


@pytest.mark.parametrize("plant", P2_PLANTS)
def test_p2cl_table_tells_a_planted_error(plant):
    """"row6" (a sixth pixel row per cell ignored) is the one plant no admitted row can tell, and must not: no cell owns a sixth
    row (the sweep above), so it applies to no row and changes none -- its neighbour "row5" (P2_SPAN one too small) is the
    error the table has to catch, at the two shapes whose cells own five rows."""
    applies = caught = 0
    for c in rows("p2cl_up") + rows("p2cl_up_items") + rows("p2cl"):
        if c.entry == "p2cl":
            h, w, H, W, band = 1, c.shape["HW"], 1, c.shape["HW"], None
        else:
            (h, w, H, W), band = _hw(c), p2cl_band(c.shape["w"])
        if (plant in ("halo_lower_dropped", "halo_counted", "last_col_clamp", "row5", "row6")) and c.entry == "p2cl":
            continue
        inp = tr.p2_inputs(c)
        bad = tr.p2_ref(inp, h, w, H, W, band, plant)
        if not bad["applies"]:
            continue
        applies += 1
        ref = tr.p2_ref(inp, h, w, H, W, band)
        a, b = tr.p2_worst(bad["bands"], bad["dlow"], ref, c.regime == "saturated")
        caught += max(a, b) > 1.0
    print(f"[tail] p2cl plant {plant}: applies to {applies} rows, out of bound on {caught}")
    if plant == "row6":
        assert applies == 0
    else:
        assert applies >= 2 and caught >= 1


NFL_PLANTS = ("ignore_counted", "mult_attached", "dice_eps_dropped", "stale_chunk")


@pytest.mark.parametrize("plant", NFL_PLANTS)
def test_nfl_dice_table_tells_a_planted_error(plant):
    applies = caught = 0
    for c in rows("nfl_dice"):
        if c.shape["B"] == 65 and c.shape["HW"] > 132:
            continue                                      # (the small maps and the batch of one decide; this keeps the test quick)
        inp = tr.nfl_inputs(c)
        bad = tr.nfl_ref(inp, plant)
        if not bad["applies"]:
            continue
        applies += 1
        ref = tr.nfl_ref(inp)
        a, b = tr.nfl_worst(torch.stack([bad["nfl"], bad["dice"]], 1), bad["g"], ref)
        caught += max(a, b) > 1.0
    print(f"[tail] nfl_dice plant {plant}: applies to {applies} rows, out of bound on {caught}")
    assert applies >= 2 and caught >= 1


ADAM_PLANTS = ("eps_in_sqrt", "eps_before_bc2", "no_bc2", "coupled_for_decoupled", "gs_after_decay", "next_segment", "tail_skipped")


@pytest.mark.parametrize("plant", ADAM_PLANTS)
def test_adam_tables_tell_a_planted_error(plant):
    """per entry: wherever the error applies to a row of an entry, one of that entry's rows leaves the bounds"""
    seen = 0
    for entry in ("adam", "adam_groups", "adam_hyper"):
        applies = caught = 0
        for c in rows(entry):
            inp = tr.adam_inputs(c)
            bad = tr.adam_ref(c, inp, plant)
            if not bad["applies"]:
                continue
            applies += 1
            w = tr.adam_worst(c, bad, tr.adam_ref(c, inp))
            caught += max(w.values()) > 1.0
        print(f"[tail] {entry} plant {plant}: applies to {applies} rows, out of bound on {caught}")
        assert caught >= 1 or applies == 0, entry
        seen += applies
    assert seen >= 2
    if plant in ("eps_in_sqrt", "eps_before_bc2"):        # where eps decides the update, every row tells where it is added
        for c in [c for c in rows("adam") if c.regime == "tiny"]:
            inp = tr.adam_inputs(c)
            w = max(tr.adam_worst(c, tr.adam_ref(c, inp, plant), tr.adam_ref(c, inp)).values())
            assert w > 1.0, (case_id(c), w)


def test_shadow_check_tells_truncation():
    applies = 0
    for c in rows("adam"):
        p = tr.adam_ref(c, tr.adam_inputs(c))["p"].astype(np.float32)
        applies += not np.array_equal(tr.bf16_bits(p), tr.bf16_bits(p, "shadow_truncated"))
    assert applies >= len(rows("adam")) // 2
    one = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20)], np.float32)       # ties to even, above half
    assert tr.bf16_bits(one).tolist() == [0x3F80, 0x3F82, 0xBF81 - 0x10000]


def test_bounds_pass_a_reference_rounded_to_fp32():
    """the other direction: the float64 reference rounded once to fp32 -- the best any fp32 kernel can return -- is inside
    every bound, with room"""
    for c in rows("adam") + rows("adam_groups")[::5] + rows("adam_hyper")[::5]:
        ref = tr.adam_ref(c, tr.adam_inputs(c))
        w = tr.adam_worst(c, {k: ref[k].astype(np.float32) for k in "pmv"}, ref)
        assert max(w.values()) <= 1.0, (case_id(c), w)
