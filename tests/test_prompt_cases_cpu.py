"""CPU checks of the prompt-kernel test table (tests/prompt_cases.py) and of its references (tests/prompt_ref.py):
1. the table reaches every branch and edge of the launchers' arithmetic, asserted through the plan functions;
2. the references agree with a second, dumber one at small sizes, and with what the reference model recorded;
3. each table discriminates: a reference with an error planted differs from the true one on at least one row of its entry (the
   rows an error applies to are counted: the check is not vacuous);
4. no row can be skipped: every row has inputs and a reference, and an entry nobody knows fails."""
import os

import numpy as np
import pytest

import prompt_ref as pr
from prompt_cases import (CASES, CC_KMAX, CC_W, CHAMFER_WP, DISK_N, EDT_LEGACY_SENTINEL, ENTRIES, INT_MAX, PUE_BOX_SIDES, Case,
                          case_id, cc_plan, chamfer_plan, disk_grid, disk_plan, edt_plan, pue_plan, pue_sweep, reduce_plan, rows)


# ------------------------------------------------------------------------------------------------ 1. coverage
def test_table_is_well_formed():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c.entry for c in CASES} == set(ENTRIES)
    assert all(rows(e) for e in ENTRIES)


def test_table_disks():
    d = rows("disk")
    assert {c.shape["n"] for c in d} == set(DISK_N) and {32, 33} <= set(DISK_N)
    plans = {n: disk_plan(n) for n in DISK_N}
    assert {p["form"] for p in plans.values()} == {"compact", "fallback"}
    assert plans[32]["form"] == "compact" and plans[32]["top_lane"] and plans[33]["form"] == "fallback"      # 1ull << 63
    assert plans[1]["live_lanes"] == 2 and not plans[24]["top_lane"]
    assert all(p["lds"] <= 64 << 10 for p in plans.values()) and disk_plan(1024)["lds"] == 16392
    grids = [disk_grid(c.shape["H"], c.shape["W"]) for c in d]
    assert any(g["under_one_block"] for g in grids) and any(g["blocks"] > 1 and g["part_block"] for g in grids)
    assert any(g["blocks"] > 1 and not g["part_block"] or g["blocks"] == 1 and not g["part_block"] for g in grids)   # 16 x 16
    assert {c.opt["radius"] for c in d} == {3, 5} and {c.opt["box"] for c in d} == {True, False}
    for n in DISK_N:                                   # both forms see a box, both radii and a canvas below one block
        mine = [c for c in d if c.shape["n"] == n]
        assert any(c.opt["box"] for c in mine) and any(c.opt["radius"] == 3 for c in mine)
        assert any(c.shape["H"] * c.shape["W"] == 1 for c in mine)


def test_table_chamfer():
    ch = rows("chamfer5")
    plans = [(c, chamfer_plan(c.shape["W"], c.opt["border"], c.shape["H"])) for c in ch]
    assert all(p["admitted"] for _, p in plans)
    assert {p["Wp"] for _, p in plans} == set(CHAMFER_WP)
    assert {p["waves"] for _, p in plans} >= {1, 2, 3, 16}
    assert any(p["waves"] == 1 and p["idle_lanes"] == 0 for _, p in plans)              # Wp = 64
    assert any(p["waves"] == 16 and p["idle_lanes"] == 0 for _, p in plans)             # Wp = 1024: every scan slot live
    assert any(p["waves"] == 16 and p["idle_lanes"] == 1 for _, p in plans)
    assert any(p["taps2_in_guard"] for _, p in plans) and sum(p["taps2_reach_guard_everywhere"] for _, p in plans) >= 12
    for wp in CHAMFER_WP:
        mine = [(c, p) for c, p in plans if p["Wp"] == wp and c.shape["H"] <= 7]
        assert {c.shape["H"] for c, _ in mine} == {1, 2, 3, 7}
        assert {c.opt["border"] for c, _ in mine} == ({False, True} if wp >= 3 else {False})
    tall = [(c, p) for c, p in plans if c.shape["H"] == 16000]
    assert {c.opt["border"] for c, _ in tall} == {False, True} and all("ones" in c.regime and "corner0" in c.regime for c, _ in tall)
    walk = [p["walk_max"] for c, p in tall if not c.opt["border"]][0]
    assert walk == 2122461799 and walk < INT_MAX and not chamfer_plan(1, False, 16001)["admitted"]
    assert not chamfer_plan(1023, True)["admitted"] and not chamfer_plan(1025, False)["admitted"]


def test_table_edt():
    e = rows("edt")
    plans = [(c, edt_plan(c.shape["H"], c.shape["W"], c.opt["border"])) for c in e]
    assert all(p["admitted"] and p["sum_max"] < 1 << 32 for _, p in plans)
    top = edt_plan(32767, 8192, False)
    assert top["admitted"] and top["d2_bound"] <= top["d2_max_representable"] and top["sum_max"] < 1 << 32
    assert not edt_plan(32768, 1, False)["admitted"] and not edt_plan(1, 8193, False)["admitted"]
    assert any(p["lds"] == 32 << 10 for _, p in plans)                                   # the widest row
    assert {p["col_blocks"] for _, p in plans} >= {1, 2, 32}
    # rows whose TRUE largest d^2 (not only the shape's bound) is at or beyond the sentinel of the earlier row pass, on both sides
    # of the edge and with the border, where the bound stays small
    d2max = {}
    for c, p in plans:
        if c.regime == "corner0":
            d2 = pr.edt_d2(pr.inputs(c)["mask"], c.opt["border"])
            d2max[(c.shape["H"], c.shape["W"], c.opt["border"])] = int(d2.max())
    assert d2max[(16383, 1, False)] == 16382 ** 2 < EDT_LEGACY_SENTINEL
    assert d2max[(16384, 1, False)] == 16383 ** 2 < EDT_LEGACY_SENTINEL
    assert d2max[(16385, 1, False)] == 16384 ** 2 == EDT_LEGACY_SENTINEL
    assert d2max[(20000, 3, False)] == 19999 ** 2 + 4 and d2max[(32767, 1, False)] == 32766 ** 2
    assert d2max[(20000, 3, True)] == 4
    assert sum(v >= EDT_LEGACY_SENTINEL for v in d2max.values()) == 3
    assert all(v <= edt_plan(*k)["d2_max_representable"] and v <= edt_plan(*k)["d2_bound"] for k, v in d2max.items())
    small = [c for c in e if c.regime != "corner0"]
    assert {c.regime for c in small} == {"corner", "sparse", "line2", "ones", "zeros"}
    assert {c.opt["border"] for c in small} == {True, False}
    assert {(c.shape["B"], c.shape["H"], c.shape["W"]) for c in small} >= {(1, 1, 1), (2, 3, 255), (2, 3, 256), (2, 3, 257), (1, 2, 8192)}


def test_table_reductions():
    for entry in ("bbox", "argmax"):
        plans = [(c, reduce_plan(c.shape["H"], c.shape["W"])) for c in rows(entry)]
        assert any(p["capped"] and p["trips"] > 8 for _, p in plans) and any(not p["capped"] and p["blocks"] > 1 for _, p in plans)
        assert any(p["blocks"] == 1 and p["idle_threads"] == 255 for _, p in plans)                    # one pixel
        assert any(p["blocks"] == 1 and not p["last_trip_partial"] and p["trips"] == 8 for _, p in plans)   # 2048: one full block
        assert any(p["blocks"] == 1 and p["trips"] == 8 and p["last_trip_partial"] for _, p in plans)   # 2025
        assert any(p["blocks"] == 2 for _, p in plans)
    assert reduce_plan(512, 512)["capped"] is False and reduce_plan(513, 512)["nb"] == 129
    assert {c.shape["B"] for c in rows("bbox")} == {1, 2, 64}
    assert any(c.shape["B"] == 64 and reduce_plan(c.shape["H"], c.shape["W"])["capped"] for c in rows("bbox"))
    assert {c.shape["P"] for c in rows("argmax")} == {1, 5}
    for H, W in {(c.shape["H"], c.shape["W"]) for c in rows("bbox")}:               # a single pixel in each corner, on every plane
        c = [c for c in rows("bbox") if c.regime == "corners" and (c.shape["H"], c.shape["W"], c.shape["B"]) == (H, W, 64)][0]
        prob = pr.inputs(c)["prob"]
        assert ((prob > pr.BBOX_THR).sum(axis=(1, 2)) == 1).all()
        assert {tuple(np.argwhere(p > pr.BBOX_THR)[0]) for p in prob} == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    # the planted ties fall where their names say: one wave, two waves of one block, two blocks
    for c in rows("argmax"):
        p = reduce_plan(c.shape["H"], c.shape["W"])
        if c.regime in ("tie_wave", "tie_waves", "tie_blocks") and p["blocks"] > 1 and c.shape["P"] == 1:
            inp = pr.inputs(c)
            i0, i1 = np.flatnonzero(inp["dist"].ravel() == 99.0)
            where = lambda i: ((i // 256) % p["blocks"], (i % 256) // 64)
            same_block, same_wave = where(i0)[0] == where(i1)[0], where(i0) == where(i1)
            assert (same_block, same_wave) == dict(tie_wave=(True, True), tie_waves=(True, False), tie_blocks=(False, False))[c.regime]
    seen = set()
    for c in rows("errmask"):
        inp = pr.inputs(c)
        seen |= set(zip(*(inp[k].ravel() != 0 for k in ("pred", "gt", "valid"))))
        if c.shape["H"] * c.shape["W"] >= 8:
            assert len(set(zip(*(inp[k].ravel() != 0 for k in ("pred", "gt", "valid"))))) == 8
    assert len(seen) == 8
    thr = [pr.inputs(c) for c in rows("bbox") if c.regime == "thr" and c.shape["H"] * c.shape["W"] > 100 and c.shape["B"] == 1]
    for inp in thr:
        assert (inp["prob"] == inp["thr"]).any() and (inp["prob"] < inp["thr"]).any() and (inp["prob"] > inp["thr"]).any()


def test_table_components():
    cc = rows("cc")
    assert {c.shape["W"] for c in cc} == set(CC_W) and {c.shape["H"] for c in cc} == {1, 2, 9} and {c.shape["B"] for c in cc} == {3}
    plans = {W: cc_plan(W) for W in CC_W}
    assert plans[255]["chunks"] == 1 and plans[255]["last_partial"] and plans[256]["chunks"] == 1 and not plans[256]["last_partial"]
    assert plans[257]["chunks"] == 2 and plans[257]["carry"] and plans[513]["chunks"] == 3 and not plans[1]["carry"]
    for W in (257, 513):
        m = pr.inputs([c for c in cc if c.regime == "run256" and c.shape["W"] == W and c.shape["H"] == 2][0])["mask"]
        assert m[0, 0, 256] and not m[0, 0, 255]                      # a run that starts exactly at column 256
        assert m[1, 0, 255] and m[1, 0, 256] and not m[1, 0, 249]     # and one that crosses it
    edge = pr.inputs([c for c in cc if c.regime == "plane_edge" and c.shape["W"] == 257 and c.shape["H"] == 9][0])["mask"]
    assert edge[0, -1].all() and edge[1, 0].all() and not edge[0, 1].any()
    table = rows("cc_table")
    counts = {c.regime: len(pr.case_data(c)[1]["table"]) for c in table}
    assert counts["k_exact"] == CC_KMAX and counts["k_plus1"] == CC_KMAX + 1
    m = pr.inputs([c for c in table if c.regime == "two_in_wave"][0])["mask"]
    lab = pr.case_data([c for c in table if c.regime == "two_in_wave"][0])[1]["roots"]
    assert len(set(lab[0, 0, :64][m[0, 0, :64] != 0])) == 2              # the non-uniform path of the table's wave
    m = pr.inputs([c for c in table if c.regime == "cross_wave"][0])["mask"]
    assert m[0, 0, 63] and m[0, 0, 64] and m[1, 2, 127] and m[1, 2, 128]


def test_table_pue_and_lines():
    p = rows("pue")
    shapes = {(c.shape["n"], c.shape["num_max"], c.shape["img"], c.shape["ld"]) for c in p}
    assert shapes == {(24, 24, 448, 904), (3, 24, 448, 899), (1, 24, 448, 904), (5, 8, 32, 67), (5, 8, 32, 72)}
    plans = [pue_plan(*s) for s in shapes]
    assert all(q["admitted"] for q in plans) and {q["pad_cols"] for q in plans} == {0, 5}
    assert any(q["nap_rows"] == 0 for q in plans) and any(q["nap_rows"] > 0 for q in plans) and {q["trips"] for q in plans} == {1, 4}
    for s in shapes:
        mine = [c for c in p if (c.shape["n"], c.shape["num_max"], c.shape["img"], c.shape["ld"]) == s]
        assert {(c.dtype, c.opt["out64"]) for c in mine} == {("f32", True), ("f32", False), ("bf16", True), ("bf16", False)}
        assert any(c.regime == "axes" for c in mine) and any(c.regime.startswith("boxes") for c in mine)
    for img in (32, 448):
        sw = np.array(pue_sweep(img), np.float32)
        c = [c for c in p if c.shape["img"] == img and c.regime == "corners"][0]
        pts = pr.inputs(c)["points"].reshape(-1, 3)
        assert {(float(a), float(b)) for a in sw for b in sw} <= {(float(a), float(b)) for a, b, _ in pts}
        c = [c for c in p if c.shape["img"] == img and c.regime == "boxes"][0]
        inp = pr.inputs(c)
        bx, n = inp["boxes"], c.shape["n"]
        assert {(w, h) for w in PUE_BOX_SIDES for h in PUE_BOX_SIDES} <= {(int(b[2]), int(b[3])) for b in bx}
        assert {0, img // 2, img - 1} <= set(bx[:, 0].tolist()) and (bx[:, :4].sum(1) == 0).any()
        sl = bx[:, 4]
        assert (sl == -1).any() and (sl >= 2 * n).any() and ((sl >= 0) & (sl < n)).any() and ((sl >= n) & (sl < 2 * n)).any()
    ax = pr.inputs([c for c in p if c.regime == "axes" and c.shape["n"] == 24][0])["points"].reshape(-1, 3)
    assert ((ax[:, 2] == -1) & (ax[:, 0] > 0)).any() and ((ax[:, 2] != -1) & (ax[:, 0] == -1)).any()
    ln = rows("line")
    assert {c.shape["P"] for c in ln if c.opt["kind"] == "polyline"} == {2, 3, 64}
    assert {(c.shape["H"], c.shape["W"]) for c in ln} == {(97, 131), (1, 1), (1, 40), (40, 1)}
    assert {c.opt["kind"] for c in ln} == {"polyline", "box"}
    for c in ln:
        if c.opt["kind"] != "polyline" or c.shape["P"] != 64:
            continue
        cur = pr.inputs(c)["curve"].astype(np.int64)
        d = np.abs(np.diff(cur, axis=1))
        if c.regime == "far":
            assert np.abs(cur).max() == 5000
        if c.regime == "slope45":
            assert (d[..., 0] == d[..., 1]).any() and (d[..., 0] == d[..., 1] + 1).any() and (d[..., 0] + 1 == d[..., 1]).any()
        if c.regime == "zero_len":
            assert (d[:, 31] == 0).all()
        if c.regime == "border":
            assert ((d[..., 0] == 0) | (d[..., 1] == 0)).all()


# ------------------------------------------------------------------------------------------------ 2. the references against others
def _same(entry, a, b):
    """does reference ``a`` (the layout of prompt_ref.reference) equal ``b`` (what ``dumb`` / ``planted`` give) where b speaks"""
    if entry == "disk":
        return all(np.array_equal(a["disks"][i], d) for i, d in enumerate(b["disks"]) if d is not None)
    return all(np.array_equal(a[k], v) for k, v in b.items())


def test_references_agree_with_a_second_one():
    seen = {}
    for c in CASES:
        inp, ref = pr.case_data(c)
        other = pr.dumb(c, inp)
        if other is None:
            continue
        if c.entry == "disk":
            seen["disk"] = seen.get("disk", 0) + sum(d is not None for d in other["disks"])
        else:
            seen[c.entry] = seen.get(c.entry, 0) + 1
        assert _same(c.entry, ref, other), case_id(c)
    assert seen["edt"] >= 40 and seen["cc"] >= 80 and seen["cc_table"] == 4 and seen["disk"] >= 120, seen


def test_golden_rows_equal_the_oracle(golden_dir):
    """what the reference model recorded for the table's own inputs (oracle/make_golden.py::prompt_edge_fixtures): the inputs
    are still the ones the table draws, the click rows and the disk maps equal the oracle bit for bit, the box rows have its
    support and its values within the tolerance tests/test_ops_gpu.py::test_pue_and_disks_bit_exact uses against the oracle"""
    fx = np.load(os.path.join(golden_dir, pr.GOLDEN_FILE))
    used = set()
    for c in CASES:
        key = pr.golden_key(c)
        if key is None:
            continue
        inp, ref = pr.case_data(c)
        assert np.array_equal(fx[key + "_points"], inp["points"]), key
        used |= {key + "_points", key + "_out"}
        if c.entry == "disk":
            want = np.unpackbits(fx[key + "_out"])[:ref["disks"].size].reshape(ref["disks"].shape)
            assert np.array_equal(want.astype(np.float32), ref["disks"]), key
            continue
        if "boxes" in inp:
            assert np.array_equal(fx[key + "_boxes"], inp["boxes"]), key
            used.add(key + "_boxes")
        out, clicks = fx[key + "_out"], ~ref["box_rows"]
        assert np.array_equal(out[clicks], ref["rows"][clicks]), key
        assert np.array_equal(out != 0, ref["rows"] != 0), key
        np.testing.assert_allclose(out, ref["rows"], atol=2e-7, rtol=0)
    assert used == set(fx.files) and len(used) >= 80


# ------------------------------------------------------------------------------------------------ 3. the tables discriminate
@pytest.mark.parametrize("entry,kind", [(e, k) for e, kinds in pr.PLANTED.items() for k in kinds])
def test_planted_error_is_noticed(entry, kind):
    applies, noticed = 0, []
    for c in rows(entry):
        inp, ref = pr.case_data(c)
        wrong = pr.planted(c, inp, kind)
        if wrong is None:
            continue
        applies += 1
        if not _same(entry, ref, wrong):
            noticed.append(case_id(c))
    assert applies >= 4 and noticed, (entry, kind, applies)
    print(f"[planted] {entry}/{kind}: noticed on {len(noticed)} of {applies} rows")
    if kind == "sat28":                    # exactly the rows past the old sentinel
        assert len(noticed) == 3


# ------------------------------------------------------------------------------------------------ 4. no row without a reference
def test_every_row_has_inputs_and_a_reference():
    for c in CASES:
        inp, ref = pr.case_data(c)
        assert isinstance(inp, dict) and isinstance(ref, dict) and ref, case_id(c)
        if c.entry != "refuse":
            assert inp and all(isinstance(v, (np.ndarray, np.generic, int)) for v in inp.values()), case_id(c)
    stranger = Case("no_such_entry", "f32", {}, {}, "x")
    with pytest.raises(KeyError):
        pr.inputs(stranger)
    with pytest.raises(KeyError):
        pr.reference(stranger, {})
