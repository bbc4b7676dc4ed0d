"""tests/gemm_cases.py and tests/gemm_ref.py without a GPU: (1) the table reaches every product instantiation of the GEMM dispatch
and every value of every plan field, within the memory and K limits of the suite; (2) the bounds accept an honest fp32
implementation at the committed constants; (3) the bounds reject wrong float64 answers."""
import pytest
import torch

import gemm_cases as gc
import gemm_ref as gr
from gemm_cases import CASES, F_B, F_BR, F_G, F_BL, F_M, F_D, ACCUM, RESID, plan

# every NOTE_KERNEL instantiation of the product library (csrc/gemm.hip, csrc/gemm_k5.hip); the laboratory-only kernels -- the
# three-stage ring and 256 x 128 three-stage forms, K3 forward and grouped, the non-pipelined K4, the K2 grouped weight gradient,
# the LDS-transposed K2 epilogue -- are not in it
K2SETS = ((0, F_B), (0, F_BR), (0, F_G), (0, 0), (1, 0), (1, F_M))
PRODUCT_KERNELS = (
    [f"gemm_f32_kernel<{a}, {b}>" for a in (0, 1) for b in (0, 1)] +
    [f"gemm_bf16_kernel<{a}, {b}, true, false, -1, 0>" for a in (0, 1) for b in (0, 1)] +
    [f"gemm_bf16_kernel<0, 0, true, false, {f}, 0>" for f in (F_B, F_BR, F_G, F_BL, 0)] +
    [f"gemm_bf16_kernel<0, 1, true, false, {f}, 0>" for f in (F_D, 0, F_M, ACCUM)] +
    [f"gemm_bf16_kernel<{a}, {b}, true, false, 65536, 0>" for a, b in ((0, 0), (0, 1), (1, 1))] +
    ["gemm_bf16_kernel<1, 1, true, true, 65536, 0>", "gemm_bf16_kernel<1, 1, true, true, -1, 0>",
     "gemm_bf16_kernel<1, 0, true, true, -1, 0>"] +
    [f"gemm_bf16_k3s_kernel<0, 0, {f}>" for f in (F_B, F_BR, F_G, F_BL, 0)] +
    [f"gemm_bf16_k3s_kernel<0, 1, {f}>" for f in (F_D, 0, F_M, RESID)] +
    ["gemm_bf16_skinny_kernel<0>", "gemm_bf16_skinny_kernel<1>"] +
    [f"gemm_bf16_k2_kernel<0, {b}, 2, {f}, {rb}, 1>" for b, f in K2SETS for rb in (5, 6, 7, 8)] +
    [f"gemm_bf16_k2_kernel<0, {b}, 4, {f}, {rb}, 1>" for b, f in K2SETS for rb in (7, 8)] +
    [f"gemm_bf16_k5_kernel<{b}, {f}, {rb}, 12>" for b, f in K2SETS for rb in (6, 7, 8)] +
    [f"gemm_bf16_k5_kernel<{b}, {f}, {rb}, 6>" for b, f in K2SETS for rb in (6, 7)] +
    ["gemm_bf16_skinny_grouped_kernel<0, 0>", "gemm_bf16_skinny_grouped_kernel<0, 1>", "gemm_bf16_skinny_grouped_kernel<1, 1>",
     "gemm_bf16_k2_grouped_fl_kernel<0, 0, 1>", "gemm_bf16_k2_grouped_fl_kernel<0, 1, 0>",
     "gemm_bf16_k2_grouped_kernel<0, 0, false>", "gemm_bf16_k2_grouped_kernel<0, 1, false>",
     "gemm_bf16_k4p_grouped_kernel<1, 1, true, true>", "gemm_bf16_k4p_grouped_kernel<1, 1, true>"] +
    [f"gemm_bf16_grouped_kernel<{a}, {b}, {'true' if a and b else 'false'}>" for a in (0, 1) for b in (0, 1)])

PLANS = {c.name: plan(c, 256) for c in CASES}
RUNNABLE = [c for c in CASES if not PLANS[c.name].err]


def test_names_are_unique():
    assert len({c.name for c in CASES}) == len(CASES)


def test_table_reaches_every_product_kernel():
    got = {pl.kernel for pl in PLANS.values() if not pl.err}
    want = set(PRODUCT_KERNELS)
    assert len(want) == len(PRODUCT_KERNELS)
    assert got == want, f"never reached: {sorted(want - got)}; not a product kernel: {sorted(got - want)}"


def test_every_case_plans_to_its_family():
    bad = [(c.name, c.family, PLANS[c.name].family) for c in RUNNABLE if PLANS[c.name].family != c.family]
    assert not bad, bad


def test_the_gpu_rows_alone_reach_every_kernel_but_the_cpu_only_branches():
    """what only the CPU test reaches is branches (the default rule's wide form, the GELU rule, the refusals), not kernels"""
    got = {PLANS[c.name].kernel for c in RUNNABLE if c.gpu}
    assert got == set(PRODUCT_KERNELS)


def test_every_plan_field_takes_each_value():
    pls = [PLANS[c.name] for c in RUNNABLE]
    by = lambda fam: [pl for pl in pls if pl.family == fam]
    assert {pl.vec for pl in by("k128")} == {True, False} and {pl.vec for pl in by("skinny")} == {True, False}
    assert {pl.vec for pl in by("grouped")} == {True, False} and {pl.vec for pl in by("splitk")} == {True, False}
    assert {pl.vec8 for pl in by("splitk")} == {-1, 0, 1, 2}
    assert {pl.inlaunch for pl in by("splitk")} == {True, False}
    assert {pl.splitk for pl in by("splitk")} >= {3, 4, 10, 16} and all(pl.splitk == 1 for pl in pls if pl.family != "splitk")
    # slice lengths: K a multiple of the slice, and a short last slice (1000 = 2 x 384 + 232, 4096 = 9 x 448 + 64)
    assert {pl.kchunk for pl in by("splitk")} == {256, 384, 448}
    assert {pl.k5 for pl in by("k5")} == {True} and not any(pl.k5 for pl in pls if pl.family != "k5")
    # 128 x 128 tiles of the bf16 kernels: one tile, several in each direction, and a launch of many
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("k128")} >= {(1, 1), (2, 1), (1, 2), (2, 2), (3, 3)}
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("splitk")} >= {(1, 1), (2, 1), (2, 2), (5, 8)}
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("k3s")} >= {(3, 3), (2, 1)}
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("k2") + by("k5")} >= {(13, 13), (15, 12), (4, 128)}
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("skinny")} >= {(1, 2), (2, 3), (2, 2)}          # 64 x 64 tiles
    assert {(pl.wide, pl.rb) for pl in by("k2")} == {(False, 5), (False, 6), (False, 7), (False, 8), (True, 7), (True, 8)}
    assert {pl.rb for pl in by("k5")} == {6, 7, 8}
    assert {pl.acc_as_res for pl in by("k3s")} == {True, False}
    assert {pl.wide for pl in by("k4p")} == {True, False}                 # direct / LDS-transposed epilogue
    assert {pl.err for pl in PLANS.values()} == {None, "2GiB"}
    assert sum(pl.err == "2GiB" for pl in PLANS.values()) == 2            # vpu_gemm and vpu_gemm_grouped
    # transposes of the fp32 and run-time kernels, tile counts of the fp32 kernel
    assert {(pl.tiles_m, pl.tiles_n) for pl in by("f32")} >= {(1, 1), (2, 3)}


def test_branches_only_the_cpu_reaches():
    name = {c.name: c for c in CASES}
    # the default rule's wide branch: 384 tiles of 256 x 256
    for n in ("k2-wide-default", "k2-wide-default-rb7"):
        assert not name[n].opts and PLANS[n].wide and not name[n].gpu
    assert {PLANS["k2-wide-default"].rb, PLANS["k2-wide-default-rb7"].rb} <= {7, 8}
    # the M > 6272 GELU rule: K2 by default, K5 with k5 = 2
    assert PLANS["k5-gelu5-rule"].family == "k2" and PLANS["k5-gelu-k5eq2-large"].family == "k5"
    p = dict(name["k5-gelu5-rule"].probs[0], M=6272)
    assert gc.plan_gemm(p, 256, None).family == "k5"
    # K = 576: the residual and aux forms fall through to K2, the others stay on K5
    assert PLANS["k5-k576-resid-falls-to-k2"].family == "k2" and PLANS["k5-k576-aux-falls-to-k2"].family == "k2"
    # ncu is a parameter: fewer CUs, other tile heights
    assert any(plan(c, 104) != PLANS[c.name] for c in RUNNABLE if c.family in ("k2", "k5"))
    assert all(plan(c, 104) == PLANS[c.name] for c in RUNNABLE if c.family in ("f32", "skinny", "k3s"))


def test_k2_and_k5_rows_are_ragged():
    """every K2 / K5 row that runs on the GPU ends in a partial row tile and a partial column tile (256-column tiles of the wide
    form: N has to be a multiple of 256 there, so only M is ragged)"""
    for c in RUNNABLE:
        pl = PLANS[c.name]
        if c.gpu and pl.family in ("k2", "k5"):
            p = c.probs[0]
            assert p["M"] % (32 * pl.rb), c.name
            assert pl.wide or p["N"] % 128, c.name


def test_sizes_stay_small():
    for c in RUNNABLE:
        for p in c.probs:
            assert p["K"] <= 4096, c.name
            if c.gpu:
                big = max(p["batch"] * p["M"] * p["N"], p["batch"] * p["M"] * p["K"], p["batch"] * p["K"] * p["N"]) * 8
                assert big < 256 << 20, (c.name, big)
    assert max(p["K"] for c in RUNNABLE for p in c.probs) == 4096


# ------------------------------------------------------------------------------------------------ (2) an honest implementation passes
SHRINK = (200, 144)


def _shrink(c):
    return SHRINK if any(p["batch"] * p["M"] * p["N"] > 60000 for p in c.probs) else None


@pytest.mark.parametrize("case", RUNNABLE, ids=lambda c: c.name)
def test_bounds_accept_honest_fp32(case):
    gr.verify(case, PLANS[case.name], lambda c, pts: [gr.honest(p, t) for p, t in pts], "cpu", _shrink(case))


# ------------------------------------------------------------------------------------------------ (3) wrong answers are rejected
@pytest.mark.parametrize("perturb", gr.PERTURBATIONS)
def test_bounds_reject(perturb):
    """each wrong float64 answer fails on at least one row of every family that carries it"""
    carried, rejected = set(), set()
    for c in RUNNABLE:
        pl = PLANS[c.name]
        for p, t in gr.inputs(c, "cpu", _shrink(c)):
            if not gr.carries(perturb, c, p, pl) or c.family in rejected:
                continue
            carried.add(c.family)
            if gr.rejects(c.family, gr.reference(p, t), gr.reference(p, t, perturb, pl)):
                rejected.add(c.family)
    print(f"{perturb}: carried by {sorted(carried)}")
    assert carried and carried == rejected, f"{perturb}: not rejected in {sorted(carried - rejected)}"
