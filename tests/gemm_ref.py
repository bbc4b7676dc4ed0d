"""Float64 reference, per-element bounds, inputs and the case walker for vpu_gemm / vpu_gemm_grouped (csrc/gemm.hip,
csrc/gemm_k5.hip).  Plain torch, importable without a GPU: tests/test_gemm_cases_cpu.py runs the walker over an honest fp32
implementation on the CPU, tests/test_gemm_f64.py over the kernels.  Sentinel buffers, bound arithmetic and Phi / phi come from
tests/rowops_ref.py.

Reference.  The operands as stored (bf16 or fp32 bits) converted to float64; v = alpha op(A) op(B) in float64; then the epilogue
flags in the order of include/vpu_hip.h, in float64: BIAS, PREACT (the side output is v), SAVE_DGELU (the side output is GELU'(v)),
GELU, RELU, DGELU / DRELU / MULAUX, RESID (row m % period of a broadcast residual), AFFINE, ACCUM.  GELU = v Phi(v) and
GELU' = Phi(v) + v phi(v) with erf in float64 on the UNROUNDED v.  colsum[m] = colsum0[m] + sum_k op(A)[m][k]; the distributed form
writes, for global column tile t of cs_tn, the sum over K-steps [t nk / cs_tn, (t + 1) nk / cs_tn) of 32.

Bound per output element:  |got - ref| <= rel |ref| + c Amp + as_term.
  rel      REL = 2^-8 where the output is bf16, 0 where it is fp32.
  Amp      the float64 sum of the magnitudes that feed the element, carried through the later steps by their Lipschitz factors:
           |alpha| sum_k |a||b|, + |bias|; GELU: 1.13 Amp + |v| (1 + |erf|) / 2 (sup |GELU'| <= 1.13; 1 + erf cancels in the left
           tail); GELU' as a side output: 0.8 Amp + (1 + |erf|) / 2 + |v| phi(v) (sup |GELU''| <= 0.8); DGELU: Amp |GELU'(a)| +
           |v| ((1 + |erf a|) / 2 + |a| phi(a)); MULAUX: Amp |aux|; DRELU / RELU: unchanged; + |resid|; AFFINE: Amp |post_mul| +
           |post_add|; ACCUM: + |C_old|.  Cancellation cannot hide an error, and an element with Amp = 0 passes only when it is exact.
  as_term  the bf16 kernels evaluate the Phi of GELU and of the saved GELU' through gelu_pair_fast / gelu_dgelu8 (Abramowitz &
           Stegun 7.1.26, |error| <= AS_ERR = 1.5e-7 on Phi, times max(1, |x|) for the fp32 evaluation of the polynomial and the
           exponential): as_term = AS_ERR max(1, |v|) times the factor that multiplies Phi -- |v| for GELU, 1 for GELU' as a side
           output -- and times |aux| / |post_mul| where those follow.  For x below about -5 GELU(x) itself is below 1e-6: the fast
           form has NO relative accuracy there, its absolute error is a few 1e-7, and this term (1.5e-7 x^2, 5.4e-6 at x = -6) is
           what admits it -- not a loose rel.  DGELU (GELU' of aux) is erff in every kernel (dgelu_f: csrc/gemm.hip epilogue_store
           and epilogue_store8) and gets no as_term; nor does anything in the fp32 kernel.  The scalar tail of the run-time
           epilogue evaluates GELU with erff as well; it shares its rows with the vector form and stays under the same term.

Exact, bit for bit: every output of a `sign` row (small-integer operands: every partial sum is exact in fp32 in any order, so the
result is the float64 one rounded once -- ReLU / DRELU zeros and the signs of zeros included), and the outputs of one descriptor
run with splitk_inlaunch 0 and 1 (tests/test_gemm_f64.py).

c per family (COEF): the next power of two at or above 4 x the worst value tests/test_gemm_f64.py measured on an MI355X (its
docstring lists them); none may exceed rowops_ref.COEF_MAX = 2^-17 -- sequential fp32 accumulation in 16-wide chunks needs at most
1.0e-6 Amp at K = 4096 with all-positive operands."""
import math
import zlib

import torch

import gemm_cases as gc
from gemm_cases import (BIAS, PREACT, GELU, RELU, DGELU, DRELU, RESID, AFFINE, ACCUM, OUT_F32, SAVE_DGELU, MULAUX, AUXF)
from rowops_ref import Guarded, O, _within, check, STATS, summary, REL, AS_ERR, COEF_MAX, Phi, phi   # noqa: F401
from rowops_ref import A_Phi, gelu_tanh, _fails

COEF = {"gemm_f32": 2.0 ** -17, "gemm_k128": 2.0 ** -17, "gemm_splitk": 2.0 ** -19, "gemm_skinny": 2.0 ** -21,
        "gemm_k3s": 2.0 ** -27, "gemm_k2": 2.0 ** -23, "gemm_k5": 2.0 ** -23, "gemm_grouped": 2.0 ** -19, "gemm_k4p": 2.0 ** -17}
assert all(v <= COEF_MAX for v in COEF.values())


def gemm_summary():
    """rowops_ref.summary restricted to the GEMM kernels"""
    lines = ["[gemm f64] worst coefficient per kernel and output:"]
    for (k, o), v in sorted(STATS.items()):
        if k.startswith("gemm_"):
            lines.append(f"  {k:44s} {o:7s} {v:.2e}")
    return "\n".join(lines)


TINY = 2.0 ** -126               # the smallest normal of bf16 and fp32
SUB16 = 2.0 ** -133              # the smallest subnormal of bf16
SPECIAL = [0.0, -0.0, TINY, -TINY, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 5.0, -5.0, 5.5, -5.5, 6.0, -6.0]
SIGNS = [0.0, -0.0, SUB16, -SUB16, 1.0, -1.0, TINY, -TINY]


def tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def out_dtype(p):
    return torch.float32 if (p["flags"] & OUT_F32) or p["dtype"] == "f32" else torch.bfloat16


def dgelu64(t):
    return Phi(t) + t * phi(t)


# ------------------------------------------------------------------------------------------------ inputs
def _gen(case, device):
    return torch.Generator(device=device).manual_seed(zlib.crc32(case.name.encode()) & 0x7FFFFFFF)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32)


def inputs(case, device, shrink=None):
    """per problem: A [Z, M, K] = op(A), B [Z, K, N] = op(B) in the stored dtype, bias [N] fp32, resid [Z, M, N] or [period, N], aux
    [Z, M, N], C0 [Z, M, N] (ACCUM), colsum0 (fp32).  ``shrink`` = (M, N) caps for the CPU run of a large row."""
    g = _gen(case, device)
    res = []
    for p in case.probs:
        if shrink:
            p = dict(p, M=min(p["M"], shrink[0]), N=min(p["N"], shrink[1]))
        td, od = tdt(p["dtype"]), out_dtype(p)
        M, N, K, Z, f, rg = p["M"], p["N"], p["K"], p["batch"], p["flags"], case.regime
        dev = g.device
        if rg == "sign":
            A = torch.randint(-2, 3, (Z, M, K), generator=g, device=dev).float()
            B = torch.randint(-2, 3, (Z, K, N), generator=g, device=dev).float()
            bias = torch.randint(-3, 4, (N,), generator=g, device=dev).float()
            if f & BIAS:
                bias = -(A[0, 0].double() @ B[0].double()).float()          # row 0: the fp32 sum with the bias is exactly 0
            resid = torch.randint(-3, 4, (Z, M, N), generator=g, device=dev).float()
            C0 = torch.randint(-3, 4, (Z, M, N), generator=g, device=dev).float()
            aux = _randn(g, Z, M, N)
            sp = torch.tensor(SIGNS, device=dev, dtype=torch.float32)
            aux[:, :, :min(8, N)] = sp[:min(8, N)]
        else:
            A, B = _randn(g, Z, M, K), _randn(g, Z, K, N) * 0.2
            bias, resid, aux, C0 = _randn(g, N), _randn(g, Z, M, N), _randn(g, Z, M, N) * 1.5, _randn(g, Z, M, N)
            if rg == "offset":
                A, B = A.abs() + 0.5, B.abs() + 0.1
                bias, resid, aux, C0 = bias.abs() + 0.5, resid.abs() + 0.5, aux.abs() + 0.5, C0.abs() + 0.5
            elif rg == "cancel":
                A = A * 16.0
                A[:, :, 1::2] = -A[:, :, 0:K - K % 2:2]
                B[:, 1::2, :] = B[:, 0:K - K % 2:2, :] + 0.002 * _randn(g, Z, K // 2, N)
            elif rg == "tails":
                # pre-activations alpha a.b + bias spread over [-9, 9] and beyond; rows m % 4 == 0 are e_0, so that their first
                # 16 columns are EXACTLY the special points (bias 0 there)
                B = _randn(g, Z, K, N) * (3.0 / math.sqrt(K)) / abs(p["alpha"])
                bias = torch.rand(N, generator=g, device=dev) * 12.0 - 6.0
                ns = min(16, N)
                sp = torch.tensor(SPECIAL, device=dev, dtype=torch.float32)
                bias[:ns] = 0.0
                A[:, 0::4, :] = 0.0
                A[:, 0::4, 0] = 1.0 / p["alpha"] if abs(p["alpha"]) in (0.5, 1.0, 2.0) else 1.0
                B[:, 0, :ns] = sp[:ns]
                aux = torch.rand(Z, M, N, generator=g, device=dev) * 18.0 - 9.0
                aux[:, 0::4, :ns] = sp[:ns]
        t = dict(A=A.to(td), B=B.to(td), bias=bias)
        if f & RESID:
            t["resid"] = (resid[0, :p["period"]] if p["period"] else resid).to(td).contiguous()
        if f & AUXF:
            t["aux"] = aux.to(td)
        if f & ACCUM:
            t["C0"] = C0.to(od)
        if p["colsum"]:
            t["colsum0"] = torch.zeros(Z * M, device=dev) if rg == "sign" else _randn(g, Z * M)
        res.append((p, t))
    return res


# ------------------------------------------------------------------------------------------------ reference
def dcs_rows(p):
    """distributed column sums: (z, global column tile, first k, last k) per slab row this descriptor writes, in slab order"""
    nk, tn = p["K"] // 32, p["cs_tn"]
    rows = []
    for z in range(p["batch"]):
        for lt in range(gc.cdiv(p["N"], 256)):
            gt = p["cs_t0"] + lt
            rows.append((z, gt, 32 * (gt * nk // tn), 32 * ((gt + 1) * nk // tn)))
    return rows


def reference(p, t, perturb=None, plan=None):
    """name -> O(ref, Amp, rel, atol) for C, preact and colsum of one problem"""
    f, bf = p["flags"], p["dtype"] == "bf16"
    A, B = t["A"].double(), t["B"].double()
    alpha = float(p["alpha"])
    K = A.shape[2]
    if perturb == "bf16-partials-64":
        acc = torch.zeros(A.shape[0], A.shape[1], B.shape[2], dtype=torch.float64, device=A.device)
        for k in range(0, K, 64):
            acc = (acc + A[:, :, k:k + 64] @ B[:, k:k + 64]).bfloat16().double()
    elif perturb == "slab-bf16":
        acc = 0.0
        for k in range(0, K, plan.kchunk):
            acc = acc + (A[:, :, k:k + plan.kchunk] @ B[:, k:k + plan.kchunk]).bfloat16().double()
    else:
        acc = A @ B
    amp = abs(alpha) * (A.abs() @ B.abs())
    bias = t["bias"].double()
    if perturb == "bias-last-group":
        bias = bias.clone()
        bias[(bias.numel() - 1) // 8 * 8:] = 0.0
    if perturb == "alpha-after-bias" and (f & BIAS):
        v = alpha * (acc + bias)
    else:
        v = alpha * acc + (bias if f & BIAS else 0.0)
    if f & BIAS:
        amp = amp + t["bias"].double().abs()
    atol = torch.zeros_like(v)
    rel_t = REL if bf else 0.0
    outs = {}
    if f & PREACT:
        outs["preact"] = O(v, amp, rel_t)
    if f & SAVE_DGELU:
        d = Phi(v) if perturb == "dgelu-no-xphi" else dgelu64(v)
        outs["preact"] = O(d, 0.8 * amp + A_Phi(v) + v.abs() * phi(v), rel_t, AS_ERR * v.abs().clamp_min(1.0) if bf else 0.0)
    if f & GELU:
        vin = v.bfloat16().double() if perturb == "gelu-rounded-preact" else v
        y = gelu_tanh(vin) if perturb == "tanh-gelu" else vin * Phi(vin)
        if bf:
            atol = AS_ERR * v.abs().clamp_min(1.0) * v.abs()
        amp = 1.13 * amp + v.abs() * A_Phi(v)
        v = y
    if f & RELU:
        v = v.clamp_min(0.0)
    if f & AUXF:
        a = t["aux"].double()
        if f & MULAUX:
            v, amp, atol = v * a, amp * a.abs(), atol * a.abs()
        elif f & DGELU:
            d = Phi(a) if perturb == "dgelu-no-xphi" else dgelu64(a)
            atol = atol * d.abs()             # (no as_term of its own: every kernel evaluates GELU'(aux) with erff, dgelu_f)
            amp = amp * dgelu64(a).abs() + v.abs() * (A_Phi(a) + a.abs() * phi(a))
            v = v * d
        else:
            v = v * (a > 0).double()
    r = None
    if f & RESID:
        r = t["resid"].double()
        if p["period"]:
            idx = torch.arange(v.shape[1], device=v.device)
            idx = (idx + 1) % p["period"] if perturb == "period-off-by-one" else idx % p["period"]
            r = r[idx].unsqueeze(0)
        if perturb != "affine-before-resid":
            v = v + r
        amp = amp + r.abs()
    if f & AFFINE:
        v = v * p["post_mul"] + p["post_add"]
        amp, atol = amp * abs(p["post_mul"]) + abs(p["post_add"]), atol * abs(p["post_mul"])
    if perturb == "affine-before-resid" and r is not None:
        v = v + r
    if f & ACCUM:
        c0 = t["C0"].double()
        if perturb != "accum-overwrite":
            v = v + c0
        amp = amp + c0.abs()
    outs["C"] = O(v, amp, REL if out_dtype(p) == torch.bfloat16 else 0.0, atol)
    if p["colsum"]:
        Kc = (gc.cdiv(K, 64) - 1) * 64 if perturb == "colsum-last-ktile" else K
        if p["cs_tn"] > 1:
            outs["colsum"] = O(torch.stack([A[z, :, k0:min(k1, Kc)].sum(1) for z, _, k0, k1 in dcs_rows(p)]),
                               torch.stack([A[z, :, k0:k1].abs().sum(1) for z, _, k0, k1 in dcs_rows(p)]))
        else:
            c0 = t["colsum0"].double()
            outs["colsum"] = O(c0 + A[:, :, :Kc].sum(2).reshape(-1), c0.abs() + A.abs().sum(2).reshape(-1))
    return outs


PERTURBATIONS = ("tanh-gelu", "dgelu-no-xphi", "gelu-rounded-preact", "bf16-partials-64", "slab-bf16", "alpha-after-bias",
                 "affine-before-resid", "period-off-by-one", "bias-last-group", "accum-overwrite", "colsum-last-ktile")


def carries(perturb, case, p, plan):
    """does problem p of the case have what the perturbation breaks"""
    f = p["flags"]
    return {"tanh-gelu": bool(f & GELU), "dgelu-no-xphi": bool(f & (SAVE_DGELU | DGELU)),
            "gelu-rounded-preact": bool(f & GELU) and p["dtype"] == "bf16", "bf16-partials-64": p["K"] > 64,
            "slab-bf16": plan.splitk > 1, "alpha-after-bias": bool(f & BIAS) and p["alpha"] != 1.0,
            "affine-before-resid": (f & (AFFINE | RESID)) == (AFFINE | RESID), "period-off-by-one": bool(f & RESID) and p["period"] > 0,
            "bias-last-group": bool(f & BIAS), "accum-overwrite": bool(f & ACCUM), "colsum-last-ktile": bool(p["colsum"])}[perturb]


def rejects(family, outs, wrong):
    """do the bounds reject the outputs ``wrong`` (name -> O whose .ref is the wrong answer)"""
    c = COEF["gemm_" + family]
    return any(_fails(wrong[n].ref, o.ref, o.A, c, o.rel, o.atol) for n, o in outs.items())


# ------------------------------------------------------------------------------------------------ an honest fp32 implementation
def honest(p, t):
    """The same operation in fp32 on the host: K accumulated in sequential chunks of 16, erff-form GELU, each output rounded once."""
    f = p["flags"]
    A, B = t["A"].float(), t["B"].float()
    K = A.shape[2]
    acc = torch.zeros(A.shape[0], A.shape[1], B.shape[2])
    cs = torch.zeros(A.shape[0], A.shape[1])
    for k in range(0, K, 16):
        acc = acc + A[:, :, k:k + 16] @ B[:, k:k + 16]
    one, half = torch.tensor(1.0), torch.tensor(0.5)
    Phi32 = lambda x: half * (one + torch.erf(x * torch.tensor(0.70710678118654752)))
    dg32 = lambda x: Phi32(x) + x * torch.tensor(0.3989422804014327) * torch.exp(-half * x * x)
    v = acc * torch.tensor(float(p["alpha"]))
    if f & BIAS:
        v = v + t["bias"]
    td, od = tdt(p["dtype"]), out_dtype(p)
    out = {}
    if f & PREACT:
        out["preact"] = v.to(td)
    if f & SAVE_DGELU:
        out["preact"] = dg32(v).to(td)
    if f & GELU:
        v = v * Phi32(v)
    if f & RELU:
        v = torch.maximum(v, torch.tensor(0.0))
    if f & AUXF:
        a = t["aux"].float()
        v = v * (a if f & MULAUX else dg32(a) if f & DGELU else (a > 0).float())
    if f & RESID:
        r = t["resid"].float()
        v = v + (r[torch.arange(v.shape[1]) % p["period"]].unsqueeze(0) if p["period"] else r)
    if f & AFFINE:
        v = v * torch.tensor(float(p["post_mul"])) + torch.tensor(float(p["post_add"]))
    if f & ACCUM:
        v = v + t["C0"].float()
    out["C"] = v.to(od)
    if p["colsum"]:
        if p["cs_tn"] > 1:
            rows = []
            for z, _, k0, k1 in dcs_rows(p):
                s = torch.zeros(A.shape[1])
                for k in range(k0, k1, 16):
                    s = s + A[z, :, k:k + 16].sum(1)
                rows.append(s)
            out["colsum"] = torch.stack(rows)
        else:
            for k in range(0, K, 16):
                cs = cs + A[:, :, k:k + 16].sum(2)
            out["colsum"] = t["colsum0"] + cs.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ the case walker
def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def verify(case, plan, run, device, shrink=None):
    """Runs the case through ``run(case, [(p, t), ...]) -> [name -> tensor, ...]`` and applies every bound and exact check."""
    pts = inputs(case, device, shrink)
    gots = run(case, pts)
    kname = plan.kernel.split("<")[0] + f" [{case.family}]"
    for i, ((p, t), got) in enumerate(zip(pts, gots)):
        outs = reference(p, t)
        tag = f"{case.name}[{i}]"
        assert set(got) == set(outs), (tag, sorted(got), sorted(outs))
        for name, o in outs.items():
            _within(f"{tag} {name}", got[name], o.ref, o.A, COEF["gemm_" + case.family], o.rel, key=(kname, name), atol=o.atol)
            if case.regime == "sign":
                want = o.ref.to(got[name].dtype)
                assert torch.equal(_bits(got[name]), _bits(want)), \
                    f"{tag} {name}: not bit-identical to the float64 result rounded once ({int((_bits(got[name]) != _bits(want)).sum())} differ)"
    return gots
