"""The table of GEMM problems that tests/test_gemm_f64.py runs on the GPU, and the dispatch of vpu_gemm / vpu_gemm_grouped
(csrc/gemm.hip, csrc/gemm_k5.hip) restated for the PRODUCT library: every laboratory environment knob reads as unset and the
laboratory bits of the k3 option are masked.  Pure Python, importable without a GPU: tests/test_gemm_cases_cpu.py checks that the
table reaches every product instantiation and every value of every plan field.

A problem is a dict (see ``P``): sizes, transposes, flags, leading-dimension pads, the element shift of the C base (2-byte
alignment = the non-vector epilogue), batch / inner, scalars, workspace, colsum.  A case is one vpu_gemm call or one
vpu_gemm_grouped call over several problems, the options it is launched under and the input regime.

plan_gemm / plan_grouped return the kernel name exactly as vpu_gemm_last_kernel() prints it, and the quantities that decide it.
``ncu`` is a parameter: the sizes of the table were found by searching the plan at 256 CUs."""
from collections import namedtuple

BIAS, PREACT, GELU, RELU, DGELU, DRELU, RESID, AFFINE, ACCUM, OUT_F32, SAVE_DGELU, MULAUX = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
F_B, F_BR, F_G, F_BL, F_M, F_D = BIAS, BIAS | RESID, BIAS | GELU | SAVE_DGELU, BIAS | RELU, MULAUX, DRELU
AUXF = DGELU | DRELU | MULAUX
CNT_BYTES = 256 << 10
WS_BYTES = 24 << 20                  # the split-K workspace the GPU test passes (zeroed; its tail holds the tile counters)
BK = 64
LIM31 = 0x7FFFFFF0
DEFAULT_OPTS = dict(k2=2, k3=28, k5=1, k5_grid=0, k5_split=-1, skinny=1, skinny_group=1, splitk_inlaunch=0)

Plan = namedtuple("Plan", "kernel err family vec tiles_m tiles_n splitk kchunk vec8 inlaunch rb wide k5 acc_as_res")
Case = namedtuple("Case", "name entry family dtype probs opts regime gpu")


def cdiv(a, b):
    return (a + b - 1) // b


def up(a, b):
    return cdiv(a, b) * b


def P(M, N, K, tA=0, tB=0, flags=0, pad_a=0, pad_b=0, pad_c=0, pad_r=0, pad_aux=0, shift_c=0, batch=1, inner=1, alpha=1.0,
      post_mul=1.0, post_add=0.0, period=0, ws=True, colsum=False, cs_tn=0, cs_t0=0, dtype="bf16"):
    """One problem.  Leading dimensions: the row length rounded up to 16 bytes plus the pad (A, B), the row length plus the pad
    (C and preact, resid, aux)."""
    q = 8 if dtype == "bf16" else 4
    d = dict(M=M, N=N, K=K, tA=tA, tB=tB, flags=flags, shift_c=shift_c, batch=batch, inner=inner, alpha=alpha, post_mul=post_mul,
             post_add=post_add, period=period, ws=ws, colsum=colsum, cs_tn=cs_tn, cs_t0=cs_t0, dtype=dtype)
    d["lda"] = up(M if tA else K, q) + pad_a
    d["ldb"] = up(N if tB else K, q) + pad_b
    d["ldc"] = N + pad_c
    d["ldr"] = N + pad_r
    d["ldaux"] = d["ldc"] if batch > 1 else N + pad_aux
    # batch entry z = zo * inner + zi: A, B, C (and preact, aux) and resid are stacked along their rows
    ra, rb = (K if tA else M), (K if tB else N)
    d["sA"] = (inner * ra * d["lda"], ra * d["lda"])
    d["sB"] = (inner * rb * d["ldb"], rb * d["ldb"])
    d["sC"] = (inner * M * d["ldc"], M * d["ldc"])
    d["sR"] = (inner * M * d["ldr"], M * d["ldr"])
    return d


def opts_of(opts):
    o = dict(DEFAULT_OPTS)
    for k, v in (opts or {}).items():
        assert k in o, k
        if v >= 0 or k == "k5_split":
            o[k] = v
    if o["k3"] >= 0:                       # product library: k3 bits 0-1 read as off, bit 3 implies bit 4
        o["k3"] &= ~3
        if o["k3"] & 8:
            o["k3"] |= 16
    return o


def vec_of(p):
    """the vector epilogue: everything the epilogue touches addressable in 16 / 32-byte units (the test's buffers are 32-byte
    aligned apart from the shift of C)"""
    f = p["flags"]
    v = p["ldc"] % 8 == 0 and p["sC"][0] % 8 == 0 and p["sC"][1] % 8 == 0 and p["shift_c"] % 8 == 0
    if f & AUXF:
        v = v and p["ldaux"] % 8 == 0
    if f & RESID:
        v = v and p["ldr"] % 8 == 0 and p["sR"][0] % 8 == 0 and p["sR"][1] % 8 == 0
    return v


def _span_err(p):
    ea = (p["K"] if p["tA"] else p["M"]) * p["lda"]
    eb = (p["K"] if p["tB"] else p["N"]) * p["ldb"]
    return ea * 2 >= LIM31 or eb * 2 >= LIM31


def _mk(kernel, family, err=None, vec=False, tiles_m=0, tiles_n=0, splitk=1, kchunk=0, vec8=-1, inlaunch=False, rb=0, wide=False,
        k5=False, acc_as_res=False):
    return Plan(kernel, err, family, vec, tiles_m, tiles_n, splitk, kchunk, vec8, inlaunch, rb, wide, k5, acc_as_res)


def _k5_name(p, rb, o):
    """vpu_k5_launch: the instantiation, or None where the form has none (the caller falls through to K2)"""
    f, K = p["flags"], p["K"]
    if p["tA"] or K < 9 * BK or K % BK:
        return None
    if (f & (RESID | MULAUX)) and K < 10 * BK:
        return None
    if f not in ((0, F_M) if p["tB"] else (F_B, F_BR, F_G, 0)):
        return None
    if rb not in (6, 7, 8):
        return None
    pwp = 6 if rb < 8 and max(o["k5_split"], 0) == 1 else 12
    return f"gemm_bf16_k5_kernel<{p['tB']}, {f}, {rb}, {pwp}>"


def plan_gemm(p, ncu=256, opts=None):
    o = opts_of(opts)
    M, N, K, f, batch = p["M"], p["N"], p["K"], p["flags"], p["batch"]
    key = 2 * p["tA"] + p["tB"]
    if p["colsum"] and p["cs_tn"] > 1:
        return _mk("", "", err="cs_tn")
    if p["dtype"] == "f32":
        return _mk(f"gemm_f32_kernel<{p['tA']}, {p['tB']}>", "f32", tiles_m=cdiv(M, 64), tiles_n=cdiv(N, 64), kchunk=K)
    if p["colsum"] and (not p["tA"] or batch != 1):
        return _mk("", "", err="colsum")
    if _span_err(p):
        return _mk("", "", err="2GiB")
    tiles_m, tiles_n = cdiv(M, 128), cdiv(N, 128)
    vec = vec_of(p)
    tiles = tiles_m * tiles_n * batch
    splitk, kchunk = 1, up(K, BK)
    if p["ws"] and (tiles < 192 or (tiles <= 256 and K >= 32 * BK)) and K >= 8 * BK:
        want = min(cdiv(384, tiles), K // (4 * BK), (WS_BYTES - CNT_BYTES) // (batch * M * (N + 1) * 4), 128)
        if want > 1:
            kchunk = up(cdiv(K, want), BK)
            splitk = cdiv(K, kchunk)
    common = dict(vec=vec, tiles_m=tiles_m, tiles_n=tiles_n)
    fits31 = M * p["ldc"] * 2 < LIM31 and M * max(p["ldr"], p["ldaux"]) * 2 < LIM31
    # ---- K2 / K5
    k2 = o["k2"]
    tm2, tn2 = cdiv(M, 256), cdiv(N, 128)

    def cost(bm, bn):
        return cdiv(cdiv(M, bm) * cdiv(N, bn), ncu) * bm

    rbn, best = 8, cost(256, 128)
    for rb in (7, 6):
        c = cost(32 * rb, 128)
        if c < best:
            best, rbn = c, rb
    if cdiv(M, 32 * rbn) * tn2 < 120 and cdiv(M, 160) * tn2 >= 120:
        rbn = 5
    tiles_narrow = cdiv(M, 32 * rbn) * tn2
    if (k2 > 0 and batch == 1 and not p["colsum"] and vec and N % 8 == 0 and K % BK == 0 and K >= 256 and
            (tm2 * tn2 >= 120 or tiles_narrow >= 120) and not p["tA"] and p["alpha"] == 1.0 and fits31):
        wide = N % 256 == 0 and (k2 == 3 or (k2 == 2 and tm2 * (N // 256) >= 384))
        narrow_ok = (k2 in (1, 3) or K >= 1024 or tm2 * tn2 >= 400 or
                     (K >= 512 and (tm2 * tn2 >= 200 or tiles_narrow >= 120)))
        bn_sel = 256 if wide else 128
        short_tile = cost(224, bn_sel) < cost(256, bn_sel)
        k5 = o["k5"]
        if k5 > 0 and (k2 == 2 or k5 == 2) and K >= 9 * BK and not ((f & RESID) and p["period"] > 0):
            rb5, best5 = 8, cost(256, 128)
            for rb in (7, 6):
                c = cost(32 * rb, 128)
                if c < best5:
                    best5, rb5 = c, rb
            gelu5 = bool(f & GELU) and M > 6272
            if k5 == 2 or not gelu5:
                name = _k5_name(p, rb5, o)
                if name:
                    return _mk(name, "k5", rb=rb5, k5=True, kchunk=K, **common)
        if (key == 0 and f in (F_B, F_BR, F_G, 0)) or (key == 1 and f in (0, F_M)):
            if wide:
                rb = 7 if short_tile else 8
                return _mk(f"gemm_bf16_k2_kernel<0, {p['tB']}, 4, {f}, {rb}, 1>", "k2", rb=rb, wide=True, kchunk=K, **common)
            if narrow_ok:
                return _mk(f"gemm_bf16_k2_kernel<0, {p['tB']}, 2, {f}, {rbn}, 1>", "k2", rb=rbn, kchunk=K, **common)
    # ---- skinny
    if (o["skinny"] and not p["tA"] and batch == 1 and not p["colsum"] and M <= 4096 and N <= 4096 and 64 <= K <= 4096 and
            tiles_m * tiles_n < 192):
        return _mk(f"gemm_bf16_skinny_kernel<{p['tB']}>", "skinny", vec=vec, tiles_m=cdiv(M, 64), tiles_n=cdiv(N, 64), kchunk=K)
    spec_ok = not p["colsum"] and vec and splitk == 1 and N % 8 == 0
    # ---- K3S
    if (spec_ok and (o["k3"] & 4) and (K <= 384 or (o["k3"] & 32)) and batch == 1 and K % 32 == 0 and K >= 128 and
            p["alpha"] == 1.0 and fits31):
        acc_as_res = key == 1 and f == ACCUM
        fl = None
        if key == 0 and f in (F_B, F_BR, F_G, F_BL, 0):
            fl = f
        elif key == 1 and f in (F_D, 0, F_M):
            fl = f
        elif acc_as_res:
            fl = RESID
        if fl is not None:
            return _mk(f"gemm_bf16_k3s_kernel<0, {p['tB']}, {fl}>", "k3s", acc_as_res=acc_as_res, kchunk=K, **common)
    # ---- compile-time 128 x 128 forms
    if spec_ok and ((key == 0 and f in (F_B, F_BR, F_G, F_BL, 0)) or (key == 1 and f in (F_D, 0, F_M, ACCUM))):
        return _mk(f"gemm_bf16_kernel<0, {p['tB']}, true, false, {f}, 0>", "k128", kchunk=kchunk, **common)
    # ---- split-K slabs / the run-time kernel
    inlaunch, name = False, None
    if splitk > 1 and N % 8 == 0:
        inl = o["splitk_inlaunch"]
        slab_bytes = batch * splitk * M * N * 4
        if inl and (inl == 1 or slab_bytes <= (inl << 20)) and tiles <= CNT_BYTES // 4 and M * N * 4 < LIM31 and WS_BYTES > 2 * CNT_BYTES:
            inlaunch = True
        if p["colsum"] and key == 3:
            name = "gemm_bf16_kernel<1, 1, true, true, 65536, 0>"
        elif not p["colsum"] and key in (0, 1, 3):
            name = f"gemm_bf16_kernel<{p['tA']}, {p['tB']}, true, false, 65536, 0>"
        else:
            inlaunch = False              # only the slab forms combine in the launch: the run-time kernel keeps the reduce launch
    if name is None:
        if p["colsum"]:
            name = f"gemm_bf16_kernel<1, {1 if key == 3 else 0}, true, true, -1, 0>"
        else:
            name = f"gemm_bf16_kernel<{p['tA']}, {p['tB']}, true, false, -1, 0>"
    vec8 = -1
    if splitk > 1 and not inlaunch:
        vec8 = 1 if vec and N % 8 == 0 else 0
        if vec8 and splitk >= 16 and (M * N) // 8 <= 8 * 65535:
            vec8 = 2
    return _mk(name, "splitk" if splitk > 1 else "k128", splitk=splitk, kchunk=kchunk, vec8=vec8, inlaunch=inlaunch, **common)


def plan_grouped(ps, ncu=256, opts=None):
    o = opts_of(opts)
    n = len(ps)
    if not 1 <= n <= 16:
        return _mk("", "", err="n")
    key = 2 * ps[0]["tA"] + ps[0]["tB"]
    any_batch = False
    for p in ps:
        if p["inner"] != 1 or p["dtype"] != "bf16" or 2 * p["tA"] + p["tB"] != key:
            return _mk("", "", err="arg")
        if p["batch"] > 1:
            any_batch = True
            if key != 3:
                return _mk("", "", err="batch")
        if p["colsum"] and key != 3:
            return _mk("", "", err="colsum")
        if _span_err(p):
            return _mk("", "", err="2GiB")
    vec = all(vec_of(p) for p in ps)
    t128 = lambda p: cdiv(p["M"], 128) * cdiv(p["N"], 128)
    if not any_batch and o["skinny_group"] and (key <= 1 or (key == 3 and o["skinny_group"] >= 2)) and n >= 2:
        ok = all(p["M"] <= 2560 and p["N"] <= 4096 and 64 <= p["K"] <= 4096 and p["alpha"] == 1.0 and t128(p) < 192 for p in ps)
        if ok and sum(cdiv(p["M"], 64) * cdiv(p["N"], 64) for p in ps) <= 2048:
            return _mk(f"gemm_bf16_skinny_grouped_kernel<{key >> 1}, {key & 1}>", "grouped", vec=vec)
    if key <= 1 and o["k2"] > 0 and vec:
        ok = all(p["K"] % BK == 0 and p["K"] >= 512 and p["N"] % 8 == 0 and p["alpha"] == 1.0 and not p["colsum"] and
                 p["M"] * p["ldc"] * 2 < LIM31 for p in ps)
        total2 = sum(cdiv(p["M"], 256) * cdiv(p["N"], 128) for p in ps)
        same_fl = ok and all(p["flags"] == (BIAS if key == 0 else 0) for p in ps)
        if ok and total2 >= 100 and same_fl:
            return _mk("gemm_bf16_k2_grouped_fl_kernel<0, 0, 1>" if key == 0 else "gemm_bf16_k2_grouped_fl_kernel<0, 1, 0>",
                       "grouped", vec=vec, tiles_m=total2)
        if ok and total2 >= 192:
            return _mk(f"gemm_bf16_k2_grouped_kernel<0, {key}, false>", "grouped", vec=vec, tiles_m=total2)
    if key == 3 and o["k2"] > 0 and vec:
        ok = all(p["K"] % BK == 0 and p["K"] >= 2048 and p["N"] % 8 == 0 and p["M"] % 8 == 0 for p in ps)
        any_dcs = any(p["colsum"] and p["cs_tn"] > 1 for p in ps)
        if any_dcs and not (ok and (o["k3"] & 8)):
            return _mk("", "", err="cs_tn")
        if ok and (o["k3"] & 8):
            direct = all((p["flags"] & ~(OUT_F32 | ACCUM)) == 0 and (p["flags"] & OUT_F32) and p["alpha"] == 1.0 and
                         p["ldc"] % 4 == 0 and p["N"] % 4 == 0 and p["sC"][0] % 4 == 0 and p["shift_c"] % 4 == 0 and
                         p["M"] * p["ldc"] * 4 < LIM31 for p in ps)
            total4 = sum(cdiv(p["M"], 256) * cdiv(p["N"], 256) * p["batch"] for p in ps)
            return _mk("gemm_bf16_k4p_grouped_kernel<1, 1, true%s>" % (", true" if direct else ""), "k4p", vec=vec,
                       tiles_m=total4, wide=direct)
        if any_batch and not ok:
            return _mk("", "", err="batch")
    if any_batch:
        return _mk("", "", err="batch")
    return _mk(f"gemm_bf16_grouped_kernel<{key >> 1}, {key & 1}, {'true' if key == 3 else 'false'}>", "grouped", vec=vec,
               tiles_m=sum(t128(p) for p in ps))


def plan(case, ncu=256):
    return plan_gemm(case.probs[0], ncu, case.opts) if case.entry == "gemm" else plan_grouped(case.probs, ncu, case.opts)


# ------------------------------------------------------------------------------------------------ the table
CASES = []


def _add(name, family, probs, opts=None, regime="ord", entry=None, gpu=True):
    probs = probs if isinstance(probs, list) else [probs]
    entry = entry or ("gemm" if len(probs) == 1 else "grouped")
    CASES.append(Case(name, entry, family, probs[0]["dtype"], probs, dict(opts or {}), regime, gpu))


SK0 = dict(skinny=0)

# ---- fp32 kernel (64 x 64 tiles): all transposes, one tile and 2 x 3 ragged tiles, K % 16 != 0, every flag
for _ta in (0, 1):
    for _tb in (0, 1):
        _add(f"f32-1tile-{_ta}{_tb}", "f32", P(37, 29, 20, _ta, _tb, BIAS, dtype="f32"))
        _add(f"f32-2x3-{_ta}{_tb}", "f32", P(100, 150, 52, _ta, _tb, BIAS | RESID, pad_c=4, pad_r=8, dtype="f32"), regime="offset")
_add("f32-attn-layout", "f32", P(50, 70, 36, 0, 1, 0, batch=6, inner=3, alpha=0.125, pad_c=2, dtype="f32"))
_add("f32-attn-layout-ta", "f32", P(50, 70, 36, 1, 0, RESID, batch=4, inner=2, dtype="f32"), regime="cancel")
_add("f32-preact-gelu", "f32", P(70, 66, 24, 0, 0, BIAS | PREACT | GELU, dtype="f32"), regime="tails")
_add("f32-save-dgelu", "f32", P(70, 66, 24, 0, 0, F_G, dtype="f32"), regime="tails")
_add("f32-relu", "f32", P(70, 66, 24, 0, 0, F_BL, dtype="f32"), regime="sign")
_add("f32-dgelu", "f32", P(70, 66, 24, 0, 1, DGELU, pad_aux=4, dtype="f32"), regime="tails")
_add("f32-drelu", "f32", P(70, 66, 24, 0, 1, DRELU, dtype="f32"), regime="sign")
_add("f32-mulaux-affine", "f32", P(70, 66, 24, 0, 1, MULAUX | RESID | AFFINE, alpha=0.5, post_mul=-1.5, post_add=0.25, dtype="f32"))
_add("f32-accum", "f32", P(70, 66, 1000, 1, 1, ACCUM | OUT_F32, alpha=2.0, dtype="f32"), regime="offset")
_add("f32-period", "f32", P(70, 66, 24, 0, 0, BIAS | RESID, period=32, dtype="f32"))

# ---- 128 x 128 bf16 kernel, run-time epilogue (the skinny rule precedes it: K < 64, transA, or skinny = 0)
for _ta in (0, 1):
    for _tb in (0, 1):
        _add(f"k128-rt-nonvec-ldc-{_ta}{_tb}", "k128", P(130, 75, 72, _ta, _tb, BIAS | RESID, pad_c=0), SK0)
        _add(f"k128-rt-vec-tail-{_ta}{_tb}", "k128", P(150, 139, 200, _ta, _tb, BIAS | PREACT | GELU | RESID, pad_c=5, pad_r=5), SK0,
             regime="tails")
_add("k128-rt-k8", "k128", P(140, 136, 8, 0, 0, BIAS | AFFINE, alpha=0.5, post_mul=2.5, post_add=-0.75))
_add("k128-rt-shift", "k128", P(129, 136, 72, 0, 1, RESID | AFFINE, shift_c=1, post_mul=0.5, post_add=0.5), SK0)
_add("k128-rt-batch", "k128", P(70, 136, 72, 0, 1, MULAUX, batch=6, inner=3, alpha=0.125, pad_c=8), SK0)
_add("k128-rt-batch-rt", "k128", P(70, 136, 72, 0, 1, MULAUX | RESID, batch=4, inner=2, alpha=0.25), SK0)
_add("k128-rt-batch-ta", "k128", P(70, 72, 200, 1, 0, RESID, batch=4, inner=2, alpha=-0.5), regime="cancel")
_add("k128-rt-f32-accum", "k128", P(150, 136, 200, 1, 1, OUT_F32 | ACCUM | AFFINE, alpha=0.5, post_mul=0.5, post_add=0.5, ws=False),
     regime="offset")
_add("k128-rt-dgelu", "k128", P(150, 136, 72, 0, 1, DGELU, pad_aux=8), SK0, regime="tails")
_add("k128-rt-drelu", "k128", P(150, 130, 72, 0, 1, DRELU, pad_c=6), SK0, regime="sign")
_add("k128-rt-relu", "k128", P(150, 130, 72, 0, 0, BIAS | RELU | RESID, pad_c=6), SK0, regime="sign")
_add("k128-rt-period", "k128", P(150, 136, 72, 0, 0, BIAS | RESID, period=64, alpha=0.75), SK0)
_add("k128-rt-period-affine", "k128", P(150, 136, 72, 0, 0, BIAS | RESID | AFFINE, period=64, post_mul=0.5, post_add=0.25), SK0)
_add("k128-rt-save-dgelu", "k128", P(150, 136, 72, 0, 0, F_G | RESID), SK0, regime="tails")
_add("k128-rt-bf16-accum", "k128", P(150, 136, 72, 1, 0, ACCUM | BIAS), regime="offset")

# ---- compile-time 128 x 128 forms (K = 200: not a K3S length)
for _tb, _fs in ((0, (F_B, F_BR, F_G, F_BL, 0)), (1, (F_D, 0, F_M, ACCUM))):
    for _f in _fs:
        _add(f"k128-fl-{_tb}-{_f}", "k128", P(150, 136, 200, 0, _tb, _f, pad_c=8, pad_r=16, pad_aux=8), SK0,
             regime="tails" if _f == F_G else "sign" if _f in (F_BL, F_D) else "ord")
_add("k128-fl-offset", "k128", P(260, 264, 1984, 0, 0, F_B, ws=False), SK0, regime="offset")

# ---- K3S
for _K, _tb, _f, _rg in ((128, 0, F_B, "ord"), (160, 0, F_BR, "ord"), (384, 0, F_G, "tails"), (160, 0, F_BL, "sign"), (128, 0, 0, "cancel"),
                         (160, 1, F_D, "sign"), (384, 1, 0, "offset"), (128, 1, F_M, "ord"), (160, 1, ACCUM, "ord")):
    _add(f"k3s-{_K}-{_tb}-{_f}", "k3s", P(300, 264, _K, 0, _tb, _f, pad_c=8, pad_r=8, pad_aux=16), SK0, regime=_rg)
_add("k3s-bit5-k1024", "k3s", P(300, 264, 1024, 0, 0, F_BR, ws=False), dict(skinny=0, k3=60), regime="offset")
_add("k3s-bit5-k4096-gelu", "k3s", P(130, 72, 4096, 0, 0, F_G, ws=False), dict(skinny=0, k3=60), regime="tails")

# ---- split-K: reduce forms 0 / 1 / 2, the in-launch combine, the weight-gradient form with column sums, un-split controls
_add("splitk-vec8-0", "splitk", P(130, 75, 1024, 1, 1, BIAS | AFFINE, alpha=0.5, post_mul=1.5, post_add=0.1))
_add("splitk-vec8-0-key2", "splitk", P(130, 75, 1024, 1, 0, RESID))
_add("splitk-vec8-1", "splitk", P(130, 72, 1024, 0, 0, BIAS | PREACT | GELU | RESID), SK0, regime="tails")
_add("splitk-vec8-1-key1", "splitk", P(130, 72, 1024, 0, 1, MULAUX | RESID), SK0, regime="offset")
_add("splitk-vec8-2", "splitk", P(130, 72, 4096, 0, 0, BIAS | RESID | AFFINE, post_mul=-1.5, post_add=1.0), SK0)
_add("splitk-vec8-2-wgrad", "splitk", P(130, 72, 4096, 1, 1, OUT_F32 | ACCUM), regime="offset")
_add("splitk-cancel", "splitk", P(130, 72, 4096, 1, 1, OUT_F32), regime="cancel")
_add("splitk-inlaunch", "splitk", P(130, 72, 4096, 0, 0, BIAS | RESID | AFFINE, post_mul=0.5, post_add=1.0),
     dict(skinny=0, splitk_inlaunch=1), regime="offset")
_add("splitk-inlaunch-wgrad", "splitk", P(130, 72, 1024, 1, 1, OUT_F32 | ACCUM), dict(splitk_inlaunch=1))
_add("splitk-inlaunch-key2", "splitk", P(130, 72, 1024, 1, 0, BIAS | RESID), dict(splitk_inlaunch=1))
_add("splitk-inlaunch-key2-colsum", "splitk", P(136, 72, 1024, 1, 0, OUT_F32 | ACCUM, colsum=True), dict(splitk_inlaunch=1))
_add("splitk-inlaunch-ragged-n", "splitk", P(130, 75, 1024, 1, 1, OUT_F32), dict(splitk_inlaunch=1))
_add("splitk-batch", "splitk", P(70, 72, 1024, 1, 1, OUT_F32 | ACCUM, batch=4, inner=2, alpha=0.5), regime="offset")
_add("splitk-batch-key2", "splitk", P(70, 75, 1024, 1, 0, RESID, batch=4, inner=2))
_add("splitk-batch-inlaunch", "splitk", P(70, 72, 1024, 0, 1, MULAUX | RESID, batch=6, inner=3), dict(skinny=0, splitk_inlaunch=1))
_add("splitk-k1000", "splitk", P(130, 72, 1000, 1, 1, OUT_F32 | ACCUM), regime="offset")        # three slices of 384, the last short
_add("splitk-k1000-key0", "splitk", P(130, 136, 1000, 0, 0, BIAS | RESID), SK0)
_add("splitk-kchunk-448", "splitk", P(520, 1000, 4096, 1, 1, OUT_F32), regime="cancel")   # 40 tiles: ten slices, the last of 64
_add("splitk-colsum", "splitk", P(136, 72, 4096, 1, 1, OUT_F32 | ACCUM, colsum=True), regime="offset")
_add("splitk-colsum-inlaunch", "splitk", P(136, 72, 1024, 1, 1, OUT_F32, colsum=True), dict(splitk_inlaunch=1))
_add("colsum-unsplit", "k128", P(136, 72, 1024, 1, 1, OUT_F32 | ACCUM, colsum=True, ws=False), regime="offset")
_add("colsum-unsplit-key2", "k128", P(136, 72, 200, 1, 0, OUT_F32, colsum=True, ws=False))
_add("colsum-key2-ws", "splitk", P(136, 72, 1024, 1, 0, OUT_F32, colsum=True))
_add("splitk-control-nows", "k128", P(130, 72, 4096, 1, 1, OUT_F32 | ACCUM, ws=False), regime="offset")

# ---- skinny kernel: both transB, M in {1, 65, 96}, K in {64, 72, 4096}, N ragged against 64; engine.py's flag sets + run-time flags
for _i, (_M, _N, _K, _tb, _f, _rg, _kw) in enumerate((
        (1, 70, 64, 0, F_B, "ord", {}), (65, 100, 72, 0, F_BR, "ord", dict(pad_c=4, pad_r=4)), (96, 136, 4096, 0, F_G, "tails", {}),
        (65, 72, 4096, 0, F_BL, "sign", {}), (96, 130, 72, 0, 0, "cancel", dict(pad_c=6)),
        (1, 72, 72, 1, 0, "ord", {}), (65, 136, 4096, 1, F_M, "offset", dict(pad_aux=8)), (96, 100, 64, 1, F_D, "sign", dict(pad_c=4)),
        (65, 72, 72, 1, ACCUM, "ord", {}), (96, 136, 72, 1, OUT_F32 | ACCUM | AFFINE, "ord", dict(alpha=0.5, post_mul=0.5, post_add=0.5)),
        (65, 136, 72, 0, BIAS | RESID, "ord", dict(period=32, alpha=0.75)), (96, 136, 200, 0, BIAS | PREACT | GELU | RESID, "tails", {}),
        (65, 136, 72, 1, DGELU, "tails", {}), (1, 136, 4096, 1, OUT_F32, "ord", {}),
        (65, 100, 72, 0, OUT_F32 | AFFINE, "ord", dict(pad_c=4, alpha=0.25, post_mul=-2.0, post_add=0.5)), (96, 136, 72, 0, BIAS | RESID | AFFINE, "ord", dict(shift_c=1, post_mul=2.0, post_add=-1.0)))):
    _add(f"skinny-{_i}-{_M}x{_N}x{_K}-{_tb}-{_f}", "skinny", P(_M, _N, _K, 0, _tb, _f, **_kw), regime=_rg)

# ---- K2: 256 x 128 form (k2 = 1 at K = 256 / 320, the default rule at K = 512), tile heights 5 .. 8, the six flag sets
K2SETS = ((0, F_B), (0, F_BR), (0, F_G), (0, 0), (1, 0), (1, F_M))
# (every shape ragged in M and N against its tile: the last row tile and the last 128-column tile are partial)
K2SHAPES = {5: (1571, 1544), 6: (1901, 1528), 7: (440, 16376), 8: (500, 16376)}
for _rb, (_M, _N) in K2SHAPES.items():
    for _j, (_tb, _f) in enumerate(K2SETS):
        _K = (256, 320)[_j % 2] if _rb in (5, 6) else 512
        _o = dict(k2=1) if _K < 512 else dict(k5=0)
        _add(f"k2-rb{_rb}-{_tb}-{_f}-k{_K}", "k2", P(_M, _N, _K, 0, _tb, _f, pad_c=8, pad_r=8, pad_aux=8), _o,
             regime="tails" if _f == F_G else "ord")
_add("k2-default-k512-offset", "k2", P(1571, 1544, 512, 0, 0, F_BR, pad_c=8), dict(k5=0), regime="offset")
# ---- K2: 256 x 256 form (k2 = 3; the default rule's wide branch needs 384 such tiles: CPU test only)
for _j, (_tb, _f) in enumerate(K2SETS):
    _M = (1571, 1800)[_j % 2]
    _add(f"k2-wide-{_tb}-{_f}", "k2", P(_M, 1536, 256, 0, _tb, _f, pad_r=8), dict(k2=3), regime="tails" if _f == F_G else "ord")
for _tb, _f in K2SETS:
    _add(f"k2-wide-rb8-{_tb}-{_f}", "k2", P(500, 22016, 256, 0, _tb, _f, pad_c=8), dict(k2=3), regime="tails" if _f == F_G else "ord")
_add("k2-wide-default", "k2", P(256 * 96, 1024, 256, 0, 0, F_B), None, gpu=False)
_add("k2-wide-default-rb7", "k2", P(224 * 110, 1024, 256, 0, 0, 0), None, gpu=False)

# ---- K5: k5 = 2; K = 576 (no residual / aux forms), 640 and longer; tile heights 6 .. 8; k5_grid, k5_split; the six flag sets
K5SHAPES = {6: (1901, 1528), 7: (440, 16376), 8: (500, 16376)}
for _rb, (_M, _N) in K5SHAPES.items():
    for _j, (_tb, _f) in enumerate(K2SETS):
        for _sp in ((0, 1) if _rb < 8 else (_j % 2,)):
            _K = 640 if _f in (F_BR, F_M) else (576, 640)[(_j + _sp) % 2]
            _o = dict(k5=2, k5_split=_sp, k5_grid=(0, 37)[(_j // 2 + _sp) % 2])
            _add(f"k5-rb{_rb}-{_tb}-{_f}-k{_K}-s{_sp}", "k5", P(_M, _N, _K, 0, _tb, _f, pad_c=8, pad_r=8, pad_aux=8), _o,
                 regime="tails" if _f == F_G else "ord")
_add("k5-ragged-k1024", "k5", P(1901, 1528, 1024, 0, 0, F_BR, pad_c=8), dict(k5=2, k5_grid=61), regime="offset")
_add("k5-default-rule", "k5", P(1901, 1528, 640, 0, 1, F_M), None, regime="ord")
_add("k5-k576-resid-falls-to-k2", "k2", P(1901, 1528, 576, 0, 0, F_BR), dict(k5=2))
_add("k5-k576-aux-falls-to-k2", "k2", P(1901, 1528, 576, 0, 1, F_M), dict(k5=2))
_add("k5-gelu5-rule", "k2", P(6400, 1024, 640, 0, 0, F_G), None, gpu=False)
_add("k5-gelu-k5eq2-large", "k5", P(6400, 1024, 640, 0, 0, F_G), dict(k5=2), gpu=False)

# ---- vpu_gemm_grouped
_add("grp-skinny-n2-key0", "grouped", [P(65, 100, 72, 0, 0, F_B), P(96, 136, 200, 0, 0, F_BR, pad_r=8)])
_add("grp-skinny-n5-key1", "grouped", [P(65, 72, 64, 0, 1, 0), P(1, 136, 72, 0, 1, F_M), P(96, 100, 4096, 0, 1, 0, pad_c=4),
                                       P(130, 72, 136, 0, 1, F_D), P(33, 200, 72, 0, 1, ACCUM)], regime="ord")
_add("grp-skinny-n3-key3", "grouped", [P(72, 100, 200, 1, 1, OUT_F32 | ACCUM), P(136, 72, 4096, 1, 1, OUT_F32), P(8, 264, 64, 1, 1, 0)],
     dict(skinny_group=2), regime="offset")
_add("grp-k2-fl-key0", "grouped", [P(2600, 1280, 512, 0, 0, F_B), P(300, 136, 576, 0, 0, F_B, pad_c=8)], regime="offset")
_add("grp-k2-fl-key1", "grouped", [P(2600, 1280, 512, 0, 1, 0), P(300, 136, 576, 0, 1, 0)])
_add("grp-k2-rt-key0", "grouped", [P(2700, 1280, 512, 0, 0, F_BR, pad_r=8), P(2600, 1288, 576, 0, 0, F_G), P(300, 136, 512, 0, 0, 0)],
     regime="tails")
_add("grp-k2-rt-key1", "grouped", [P(2700, 1280, 512, 0, 1, F_M, pad_aux=8), P(2600, 1288, 576, 0, 1, 0), P(300, 136, 512, 0, 1, F_D)])
_add("grp-k4p-direct", "k4p", [P(264, 520, 2048, 1, 1, OUT_F32), P(520, 264, 2048, 1, 1, OUT_F32 | ACCUM, pad_c=8)], regime="offset")
_add("grp-k4p-direct-colsum", "k4p", [P(264, 520, 2048, 1, 1, OUT_F32 | ACCUM, colsum=True), P(136, 72, 2112, 1, 1, OUT_F32)])
_add("grp-k4p-lds-bf16", "k4p", [P(264, 520, 2048, 1, 1, 0), P(520, 264, 2048, 1, 1, OUT_F32 | ACCUM, colsum=True)], regime="cancel")
_add("grp-k4p-lds-alpha", "k4p", [P(264, 520, 2048, 1, 1, OUT_F32 | ACCUM, alpha=0.5, colsum=True)], entry="grouped")
_add("grp-k4p-batch2", "k4p", [P(264, 520, 2048, 1, 1, OUT_F32, batch=2, colsum=True)], entry="grouped")
_add("grp-k4p-dcs", "k4p", [P(264, 256, 2048, 1, 1, OUT_F32, colsum=True, cs_tn=3, cs_t0=0),
                            P(264, 264, 2048, 1, 1, OUT_F32 | ACCUM, colsum=True, cs_tn=3, cs_t0=1)])
_add("grp-k4p-dcs2-batch2", "k4p", [P(136, 512, 4096, 1, 1, OUT_F32, batch=2, colsum=True, cs_tn=2, cs_t0=0)], entry="grouped",
     regime="offset")
for _key in range(4):
    _fl = (F_B | RESID, MULAUX, RESID, OUT_F32 | ACCUM)[_key]
    _add(f"grp-general-key{_key}", "grouped",
         [P(130, 75, 200, _key >> 1, _key & 1, _fl), P(200, 136, 72, _key >> 1, _key & 1, 0 if _key else F_G, alpha=0.5),
          P(64, 264, 1000, _key >> 1, _key & 1, OUT_F32 | AFFINE, post_mul=0.5, post_add=1.0, colsum=_key == 3)],
         dict(skinny_group=0), regime="tails" if _key == 0 else "ord")
_add("grp-16", "grouped", [P(40 + 9 * i, 72 + 8 * (i % 3), 72 + 64 * (i % 4), 1, 1, OUT_F32 | (ACCUM if i % 2 else 0), colsum=i % 3 == 0)
                           for i in range(16)])
# ---- refusals (CPU test only)
_add("refuse-2gib", "k128", P(9, 8, 8, 0, 0, 0, pad_a=1 << 27), None, gpu=False)
_add("refuse-2gib-grouped", "grouped", [P(9, 8, 8, 0, 0, 0, pad_a=1 << 27), P(8, 8, 8)], None, gpu=False)


def case_id(c):
    return c.name
