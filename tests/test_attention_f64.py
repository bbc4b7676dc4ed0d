"""Every fused-attention entry point against float64, per element, at the models' shapes and at the launchers' edges; the
unfused path's softmax kernels and Engine.sdpa the same way.

The kernels take bf16 inputs; the references take exactly those values, upcast to float64, and are computed on the GPU in
torch (per group of (batch, head) problems, so that no intermediate exceeds ~1 GB).  S = scale Q K^T, P = softmax(S), O = P V.
Every bound is built from the sum of absolute contributions A (cancellation cannot hide an error):

  O      2^-8 |O_ref| + c A_O,            A_O = P |V|
  lse    2^-18 (|lse_ref| + max_k |S_ik|), + 2^-8 for the lean forward (LSE_LEAN below)
  delta  1e-5 rowsum(|dO| |O_kernel|)     (reference rowsum(dO O_kernel): the kernel's own bf16 O; the one-pass backward
                                           forms keep delta on chip and leave the workspace alone)
  dV     2^-8 |ref| + c P^T |dO|
  dQ     2^-8 |ref| + c scale A_dS |K|,   A_dS = P (|dO| |V|^T + 2 rowsum(|dO| A_O))
  dK     2^-8 |ref| + c scale A_dS^T |Q|

2^-8 |ref| is the rounding of the bf16 result; the kernels also round P and dS to bf16 before their MFMAs, which predicts c of
2^-9 to 2^-8 (the split forms round each partial result as well).  Every check prints the smallest coefficient that would have
passed beside its bound, and the module ends with the worst one per kernel form.

Every element is written and nothing outside: the outputs are pre-filled with NaN, q / k / v / o and the gradients are column
slices of wider matrices (gap columns) with guard rows after the last batch entry, gap and guard filled with a sentinel bit
pattern that must come out unchanged (inputs: the whole buffer).  The sentinel is a large finite bf16 value, so that a kernel
reading a gap column into a product is caught by the bounds, while one that reads padding rows it then masks is not.

The rows come from tests/attention_cases.py (launcher branches and model shapes; tests/test_attention_cases_cpu.py checks the
coverage); each launch asserts the kernel vpu_attn_last_kernel() names.  A few rows also check that the bounds reject wrong
float64 answers (last key omitted, scale * (1 + 2^-7), two heads' V swapped, the last key's dK / dV zeroed)."""
import math

import pytest
import torch

from attention_cases import CASES

pytestmark = pytest.mark.gpu

# c of the bounds above, the same for every form.  Measured worst c per form on one MI355X (the module prints them):
#   forward O:  lean <32,*,32> 1.6e-3, <64,*,64> 2.8e-3, <128,*,96> 3.3e-3, <128,*,128> 1.3e-3; step forms 1.1e-3
#   backward dQ / dK / dV:  lean pairs 5.1e-4 / 1.3e-3 / 5.5e-3; step pairs 2.7e-4 / 6.1e-4 / 2.6e-3;
#     winx 2.8e-4 / 4.7e-4 / 5.1e-3, win 1.1e-4 / 1.2e-4 / 2.0e-3, winp 1.2e-4 / 3.8e-5 / 6.8e-4
#   split (+ attn_combine / sum_groups): O 1.7e-3, dQ 1.2e-4, dK 1.4e-4, dV 1.5e-3
#   lse: step forms 1.1e-7 of 2^-18 = 3.8e-6; delta 7.2e-8 of 1e-5
C_ATTN = 2.0 ** -7
REL = 2.0 ** -8          # bf16 rounding of the result
C_LSE = 2.0 ** -18
# The lean forward sums its row's probabilities with the same MFMA that forms O (l = 1 . P^T over the bf16-ROUNDED P: O is
# normalised by exactly the weights it was built from), so its lse is log sum fl(p) + m: each fl(p) is within 2^-8 of p, so
# |lse - log sum p - m| <= 2^-8 whatever the scores.  Measured worst 1.9e-3 (48 x 1024 keys, inputs x 8).  The step kernels
# sum the unrounded fp32 p: 2^-18 relative alone.
LSE_LEAN = 2.0 ** -8
ONE_PASS = ("attn_bwd_winp_kernel<1>", "attn_bwd_winx_kernel", "attn_bwd_win_kernel")   # delta stays on chip
C_DELTA = 1e-5
TINY = 2.0 ** -100       # the kernels flush subnormals: probabilities below 2^-126 are 0, so a gradient built only from such
                         # probabilities loses up to 2^-126 x nq x |dP| |q| scale -- far below 2^-100 here (seen at 48 x 1024
                         # keys, inputs x 8: dK of 6e-38 came out as 0)
GAP = 48                 # gap columns past the used width: a 128-column instantiation at head dim 80 could spill 48
GUARD = 3                # guard rows past the last batch entry
SENT16 = 0x4B5A          # bf16 1.43e7
SENT32 = 0x4B5A4B5A      # fp32 1.43e7
REF_ELEMS = 1 << 24      # elements of one [problems, nq, nk] float64 intermediate per reference chunk (128 MB)

STATS = {}               # (form, output) -> worst coefficient


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvpuformer_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if STATS:
        print("\n[attention f64] worst coefficient per kernel form and output:")
        for (form, out), v in sorted(STATS.items()):
            print(f"  {form:90s} {out:6s} {v:.2e}")


def _record(form, out, v):
    STATS[(form, out)] = max(STATS.get((form, out), 0.0), v)


def _need(got, ref, A, rel, atol=0.0):
    """smallest c with |got - ref| <= rel |ref| + atol + c A everywhere (inf where A == 0 and the error is not covered; NaN -> inf)."""
    err = (got.double() - ref).abs()
    over = (err - rel * ref.abs() - atol).clamp_min(0.0)
    need = torch.where(A > 0, over / A.clamp_min(1e-300), torch.where(over > 0, math.inf, 0.0))
    need = torch.where(torch.isnan(err), math.inf, need)
    return need


def _within(tag, got, ref, A, coef, rel=REL, form=None, out=None, atol=0.0):
    """|got - ref| <= rel |ref| + atol + coef A element-wise; prints the smallest coefficient that would have passed."""
    need = _need(got, ref, A, rel, atol)
    m = need.max().item()
    print(f"[attention f64] {tag}: {m:.2e} (bound {coef:.2e}{f', atol {atol:.1e}' if atol else ''})")
    if form is not None:
        _record(form, out, m)
    bad = ~(need <= coef)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} elements out of bound, first at {i}: got {got[i].item()!r}, "
                             f"ref {ref[i].item()!r}, A {A[i].item()!r}")


def _fails(got, ref, A, coef, rel=REL, atol=0.0):
    return bool((~(_need(got, ref, A, rel, atol) <= coef)).any())


# ------------------------------------------------------------------------------------------------ float64 reference
def _ref(q, k, v, dO, Ok, scale):
    """q [P, nq, hd], k / v [P, nk, hd], dO / Ok [P, nq, hd] (float64, on the GPU); Ok = the kernel's output.  Returns the
    float64 outputs, gradients and their absolute-contribution terms, computed over chunks of the P problems."""
    Pn, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    step = max(1, REF_ELEMS // (nq * nk))
    parts = []
    for p0 in range(0, Pn, step):
        sl = slice(p0, p0 + step)
        qc, kc, vc, dc, oc = q[sl], k[sl], v[sl], dO[sl], Ok[sl]
        S = scale * (qc @ kc.transpose(1, 2))
        lse = torch.logsumexp(S, -1)
        smax = S.abs().amax(-1)
        P = torch.exp(S - lse[..., None])
        del S
        O = P @ vc
        A_O = P @ vc.abs()
        dP = dc @ vc.transpose(1, 2)
        dS = P * (dP - (dc * O).sum(-1, keepdim=True))
        del dP
        A_dS = P * (dc.abs() @ vc.abs().transpose(1, 2) + 2 * (dc.abs() * A_O).sum(-1, keepdim=True))
        r = dict(O=O, A_O=A_O, lse=lse, smax=smax,
                 delta=(dc * oc).sum(-1), A_delta=(dc.abs() * oc.abs()).sum(-1),
                 dQ=scale * (dS @ kc), A_dQ=scale * (A_dS @ kc.abs()),
                 dK=scale * (dS.transpose(1, 2) @ qc), A_dK=scale * (A_dS.transpose(1, 2) @ qc.abs()),
                 dV=P.transpose(1, 2) @ dc, A_dV=P.transpose(1, 2) @ dc.abs())
        del P, dS, A_dS
        parts.append(r)
    return {key: torch.cat([p[key] for p in parts]) for key in parts[0]}


# ------------------------------------------------------------------------------------------------ buffers
def _sentinel(rows, ld, dtype):
    if dtype == torch.bfloat16:
        return torch.full((rows, ld), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full((rows, ld), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)


def _matrix(rows, ld):
    """[rows + GUARD, ld] bf16 filled with the sentinel (_put / _fill_nan then write the problem's cells)"""
    return _sentinel(rows + GUARD, ld, torch.bfloat16)


def _put(buf, col0, data):
    buf[:data.shape[0], col0:col0 + data.shape[1]] = data


def _fill_nan(buf, rows, col0, width):
    buf[:rows, col0:col0 + width] = float("nan")


def _vector(n):
    buf = _sentinel(1, n + 64, torch.float32).view(-1)
    buf[:n] = float("nan")
    return buf


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


class Region:
    """the cells of a buffer the launch may write; everything else must keep its bits"""

    def __init__(self, buf, rows, cols):
        self.buf, self.before = buf, _bits(buf).clone()
        self.mask = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
        self.mask[:rows, cols[0]:cols[1]] = True

    def check(self, tag):
        same = _bits(self.buf) == self.before
        bad = ~same & ~self.mask
        assert not bad.any(), f"{tag}: {int(bad.sum())} cells outside the problem changed, first at {tuple(bad.nonzero()[0].tolist())}"


def _heads(buf, nb, n, H, hd, col0):
    """[nb * n, ...] column slice -> [nb * H, n, hd] float64"""
    return buf[:nb * n, col0:col0 + H * hd].double().view(nb, n, H, hd).permute(0, 2, 1, 3).reshape(nb * H, n, hd)


# ------------------------------------------------------------------------------------------------ inputs
def _inputs(c, seed):
    """q [nb, nq, H, hd], k / v [nb, nk, H, hd], dO [nb, nq, H, hd], bf16 (drawn on the host: the same values on every box)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    q = u(c.nb, c.nq, c.H, c.hd) * 1.5
    k = u(c.nb, c.nk, c.H, c.hd) * 1.5
    v = u(c.nb, c.nk, c.H, c.hd) * 1.5
    dO = u(c.nb, c.nq, c.H, c.hd)
    if c.regime in ("x4", "x8"):
        f = 4.0 if c.regime == "x4" else 8.0
        q, k = q * f, k * f
    elif c.regime == "ramp":
        k = k * (1.0 + 0.7 * torch.arange(c.nk, dtype=torch.float32) / c.nk).view(1, c.nk, 1, 1)
    elif c.regime == "flat":
        q[:, ::5] = 0.0
        dO[:, 1::7] = 0.0
    return [t.to(torch.bfloat16).cuda() for t in (q, k, v, dO)]


def _rise_log2(q, k, scale):
    """per query row: how far (log2 units) the score maximum over all keys lies above the one over the first 32 keys"""
    S = scale * torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double())
    return ((S.amax(-1) - S[..., :32].amax(-1)) / math.log(2)).flatten()


# ------------------------------------------------------------------------------------------------ launches
def _run(ops, c):
    """Runs forward and backward of row ``c`` on the padded layouts; returns the inputs, the outputs as [nb * H, n, hd] /
    [nb * H, nq] float64, and checks names and untouched cells on the way."""
    nb, H, nq, nk, hd, S = c.nb, c.H, c.nq, c.nk, c.hd, c.S
    D = H * hd
    scale = hd ** -0.5
    q, k, v, dO = _inputs(c, seed=1000 + CASES.index(c))
    flat = lambda t: t.reshape(-1, D)
    regions = []
    if c.entry == "attn":
        ld = 3 * D + GAP
        qkv = _matrix(nb * nq, ld)
        for i, t in enumerate((q, k, v)):
            _put(qkv, i * D, flat(t))
        Q, K, V, ldq, ldk = (qkv, 0), (qkv, D), (qkv, 2 * D), ld, ld
        inputs = [qkv]
    else:
        ldq = ldk = D + GAP
        Qb, Kb, Vb = _matrix(nb * nq, ldq), _matrix(nb * nk, ldk), _matrix(nb * nk, ldk)
        _put(Qb, 0, flat(q)); _put(Kb, 0, flat(k)); _put(Vb, 0, flat(v))
        Q, K, V = Qb, Kb, Vb
        inputs = [Qb, Kb, Vb]
    ldo = D + GAP
    dOb = _matrix(nb * nq, ldo)
    _put(dOb, 0, flat(dO))
    inputs.append(dOb)
    snap = [_bits(t).clone() for t in inputs]
    O = _matrix(nb * nq, ldo); _fill_nan(O, nb * nq, 0, D)
    lse = _vector(nb * H * nq)
    delta = _vector(nb * H * nq)
    regions += [Region(O, nb * nq, (0, D)), Region(lse.view(1, -1), 1, (0, nb * H * nq)),
                Region(delta.view(1, -1), 1, (0, nb * H * nq))]
    if c.entry == "attn":
        dqkv = _matrix(nb * nq, ld); _fill_nan(dqkv, nb * nq, 0, 3 * D)
        dQ, dK, dV, ldgq, ldgk = (dqkv, 0), (dqkv, D), (dqkv, 2 * D), ld, ld
        regions.append(Region(dqkv, nb * nq, (0, 3 * D)))
        bufs = dict(dQ=dqkv, dK=dqkv, dV=dqkv)
        cols = dict(dQ=0, dK=D, dV=2 * D)
    else:
        ldgq = ldgk = D + GAP
        dQb, dKb, dVb = _matrix(nb * nq, ldgq), _matrix(nb * nk, ldgk), _matrix(nb * nk, ldgk)
        for t, n in ((dQb, nq), (dKb, nk), (dVb, nk)):
            _fill_nan(t, nb * n, 0, D)
        dQ, dK, dV = dQb, dKb, dVb
        bufs = dict(dQ=dQb, dK=dKb, dV=dVb)
        cols = dict(dQ=0, dK=0, dV=0)
        if c.entry == "split_k":
            regions.append(Region(dQb, nb * nq, (0, ldgq)))     # (vpu_sum_groups adds whole rows: the gap columns too)
            regions += [Region(dKb, nb * nk, (0, D)), Region(dVb, nb * nk, (0, D))]
        elif c.entry == "split_q":
            regions.append(Region(dQb, nb * nq, (0, D)))
            regions += [Region(dKb, nb * nk, (0, ldgk)), Region(dVb, nb * nk, (0, ldgk))]
        else:
            regions += [Region(dQb, nb * nq, (0, D)), Region(dKb, nb * nk, (0, D)), Region(dVb, nb * nk, (0, D))]
    args = (ldq, ldk, ldo)
    try:
        ops.attn_set_option("lean", c.lean)
        ops.attn_set_option("onepass", c.onepass)
        if c.entry == "attn":
            ops.attn_fwd(Q, K, V, O, lse, nb, H, nq, hd, ld, ldo, scale)
            fwd_name = ops.attn_last_kernel()
            ops.attn_bwd(Q, K, V, O, dOb, lse, delta, dQ, dK, dV, nb, H, nq, hd, ld, ldo, ld, scale)
            bwd_name = ops.attn_last_kernel()
        elif c.entry == "xattn":
            ops.xattn_fwd(Q, K, V, O, lse, nb, H, nq, nk, hd, *args, scale)
            fwd_name = ops.attn_last_kernel()
            ops.xattn_bwd(Q, K, V, O, dOb, lse, delta, dQ, dK, dV, nb, H, nq, nk, hd, *args, ldgq, ldgk, scale)
            bwd_name = ops.attn_last_kernel()
        elif c.entry == "split_k":      # long keys: S partial softmaxes merged through their log-sum-exp; dQ as S partial sums
            o_s = _matrix(nb * S * nq, ldo); _fill_nan(o_s, nb * S * nq, 0, D)
            lse_s = _vector(nb * S * H * nq)
            dqp = _matrix(nb * S * nq, ldgq); _fill_nan(dqp, nb * S * nq, 0, D)
            regions += [Region(o_s, nb * S * nq, (0, D)), Region(lse_s.view(1, -1), 1, (0, nb * S * H * nq)),
                        Region(dqp, nb * S * nq, (0, D))]
            ops.xattn_fwd_split(Q, K, V, o_s, lse_s, nb * S, H, nq, nk // S, hd, *args, scale, S, 1)
            fwd_name = ops.attn_last_kernel()
            torch.cuda.synchronize()
            assert torch.isfinite(o_s[:nb * S * nq, :D].float()).all() and torch.isfinite(lse_s[:nb * S * H * nq]).all()
            ops.attn_combine(o_s, lse_s, O, lse, nb, H, nq, hd, S, ldo, ldo)
            ops.xattn_bwd_split(Q, K, V, O, dOb, lse, delta, dqp, dK, dV, nb * S, H, nq, nk // S, hd, *args, ldgq, ldgk, scale, S, 1)
            bwd_name = ops.attn_last_kernel()
            torch.cuda.synchronize()
            assert torch.isfinite(dqp[:nb * S * nq, :D].float()).all()
            ops.sum_groups(dqp, dQ, nb, S, nq * ldgq)
        else:                           # long queries: S query ranges against the same keys; dK / dV as S partial sums
            dkp, dvp = _matrix(nb * S * nk, ldgk), _matrix(nb * S * nk, ldgk)
            for t in (dkp, dvp):
                _fill_nan(t, nb * S * nk, 0, D)
            regions += [Region(dkp, nb * S * nk, (0, D)), Region(dvp, nb * S * nk, (0, D))]
            ops.xattn_fwd_split(Q, K, V, O, lse, nb * S, H, nq // S, nk, hd, *args, scale, 1, S)
            fwd_name = ops.attn_last_kernel()
            ops.xattn_bwd_split(Q, K, V, O, dOb, lse, delta, dQ, dkp, dvp, nb * S, H, nq // S, nk, hd, *args, ldgq, ldgk, scale, 1, S)
            bwd_name = ops.attn_last_kernel()
            torch.cuda.synchronize()
            assert torch.isfinite(dkp[:nb * S * nk, :D].float()).all() and torch.isfinite(dvp[:nb * S * nk, :D].float()).all()
            ops.sum_groups(dkp, dK, nb, S, nk * ldgk)
            ops.sum_groups(dvp, dV, nb, S, nk * ldgk)
        torch.cuda.synchronize()
    finally:
        ops.attn_set_option("lean", -1)
        ops.attn_set_option("onepass", -1)
    tag = f"{c.entry} nb={nb} H={H} {nq}x{nk} hd={hd} lean={c.lean} onepass={c.onepass} {c.regime}" + (f" S={S}" if S > 1 else "")
    assert fwd_name == c.fwd, (tag, fwd_name)
    assert bwd_name == c.bwd, (tag, bwd_name)
    for t, s in zip(inputs, snap):
        assert torch.equal(_bits(t), s), f"{tag}: an input buffer changed"
    for r in regions:
        r.check(tag)
    lse_k, delta_k = lse[:nb * H * nq], delta[:nb * H * nq]
    if c.entry == "split_q":        # [nb, S, H, nq / S] -> [nb, H, nq]
        lse_k = lse_k.view(nb, S, H, nq // S).permute(0, 2, 1, 3).reshape(-1)
        delta_k = delta_k.view(nb, S, H, nq // S).permute(0, 2, 1, 3).reshape(-1)
    got = dict(O=_heads(O, nb, nq, H, hd, 0), lse=lse_k.double().view(nb * H, nq), delta=delta_k.double().view(nb * H, nq),
               dQ=_heads(bufs["dQ"], nb, nq, H, hd, cols["dQ"]), dK=_heads(bufs["dK"], nb, nk, H, hd, cols["dK"]),
               dV=_heads(bufs["dV"], nb, nk, H, hd, cols["dV"]))
    for key, t in got.items():
        if key == "delta" and c.bwd in ONE_PASS:
            continue        # (workspace the one-pass forms keep on chip: include/vpu_hip.h, vpu_attn_bwd)
        assert torch.isfinite(t).all(), f"{tag}: {key} has {int((~torch.isfinite(t)).sum())} unwritten / non-finite elements"
    x = dict(q=q.double().permute(0, 2, 1, 3).reshape(nb * H, nq, hd), k=k.double().permute(0, 2, 1, 3).reshape(nb * H, nk, hd),
             v=v.double().permute(0, 2, 1, 3).reshape(nb * H, nk, hd), dO=dO.double().permute(0, 2, 1, 3).reshape(nb * H, nq, hd))
    return tag, scale, q, k, x, got


def _checks(c, ref, got):
    """(output, got, ref, A, coef, rel, atol) of every bound of row ``c``"""
    lean = c.fwd.startswith("attn_fwd_lean_kernel")
    checks = [("O", got["O"], ref["O"], ref["A_O"], C_ATTN, REL, TINY),
              ("lse", got["lse"], ref["lse"], ref["lse"].abs() + ref["smax"], C_LSE, 0.0, LSE_LEAN if lean else 0.0),
              ("dQ", got["dQ"], ref["dQ"], ref["A_dQ"], C_ATTN, REL, TINY),
              ("dK", got["dK"], ref["dK"], ref["A_dK"], C_ATTN, REL, TINY),
              ("dV", got["dV"], ref["dV"], ref["A_dV"], C_ATTN, REL, TINY)]
    if c.bwd not in ONE_PASS:
        checks.append(("delta", got["delta"], ref["delta"], ref["A_delta"], C_DELTA, 0.0, 0.0))
    return checks


@pytest.mark.parametrize("c", CASES, ids=[f"{c.entry}-{c.nb}x{c.H}-{c.nq}x{c.nk}-hd{c.hd}-l{c.lean}o{c.onepass}-{c.regime}-S{c.S}"
                                          for c in CASES])
def test_attention_against_float64(ops, c):
    tag, scale, q, k, x, got = _run(ops, c)
    if c.regime == "ramp":
        rise = _rise_log2(q, k, scale)
        print(f"[attention f64] {tag}: the score maximum rises by up to {rise.max().item():.2f} (log2) past the first key block")
        assert 4.0 < rise.max().item() < 8.0       # the lean forward's deferred rescale: no raise, probabilities up to 2^8
    elif c.regime in ("x4", "x8"):
        rise = _rise_log2(q, k, scale)
        print(f"[attention f64] {tag}: the score maximum rises by up to {rise.max().item():.2f} (log2) past the first key block")
        assert rise.max().item() > 8.0             # the reference maximum is raised
    ref = _ref(x["q"], x["k"], x["v"], x["dO"], got["O"], scale)
    for out, g_, r_, A, coef, rel, atol in _checks(c, ref, got):
        form = c.fwd if out in ("O", "lse") else c.bwd
        if c.S > 1:
            form = f"{c.entry} S={c.S}: {form}"
        _within(f"{tag} {out}", g_, r_, A, coef, rel, form=form, out=out, atol=atol)
    if c.sens:
        _sensitivity(tag, c, scale, x, got, ref)


def _sensitivity(tag, c, scale, x, got, ref):
    """The kernel's outputs against deliberately wrong float64 answers: each one must break at least one bound."""
    nb, H = c.nb, c.H
    wrong = {}
    r = _ref(x["q"], x["k"][:, :-1], x["v"][:, :-1], x["dO"], got["O"], scale)          # the last key omitted
    for key in ("dK", "dV", "A_dK", "A_dV"):
        r[key] = torch.cat([r[key], torch.zeros_like(r[key][:, :1])], 1)
    wrong["last key omitted"] = r
    wrong["scale * (1 + 2^-7)"] = _ref(x["q"], x["k"], x["v"], x["dO"], got["O"], scale * (1 + 2.0 ** -7))
    perm = torch.arange(nb * H, device="cuda").view(nb, H)
    sw = perm.clone()
    sw[:, 0:H - 1:2], sw[:, 1:H:2] = perm[:, 1:H:2], perm[:, 0:H - 1:2]
    sw = sw.flatten()
    r = _ref(x["q"], x["k"], x["v"][sw], x["dO"], got["O"], scale)                      # heads 0 <-> 1, 2 <-> 3, ...
    r["dV"], r["A_dV"] = r["dV"][sw], r["A_dV"][sw]
    wrong["adjacent heads' V swapped"] = r
    r = dict(ref)
    r["dK"], r["dV"] = ref["dK"].clone(), ref["dV"].clone()
    r["dK"][:, -1], r["dV"][:, -1] = 0.0, 0.0
    wrong["last key's dK / dV zeroed"] = r
    for name, r in wrong.items():
        broken = [out for out, g_, r_, A, coef, rel, atol in _checks(c, r, got) if _fails(g_, r_, A, coef, rel, atol)]
        print(f"[attention f64] {tag}: against '{name}' the bounds of {broken or 'NOTHING'} are violated")
        assert broken, f"{tag}: the bounds do not tell the kernel's output from the wrong answer '{name}'"


# ------------------------------------------------------------------------------------------------ the unfused path
C_SM = 2.0 ** -17        # softmax_bwd: a fp32 row dot product over <= 4096 columns (64 in-lane, then 6 shuffle levels)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ncols", [1, 48, 63, 784, 1000, 1024, 1025, 1764, 2304, 4096])
def test_softmax_against_float64(ops, dtype, ncols):
    """vpu_softmax_fwd / _bwd (the unfused attention: fp32 mode, head dims above 128) against float64: both SM_MAX instantiations
    (ldp <= 1024: 16 columns per lane; above: 64), P's and dS's columns [ncols, ldp) exact zeros, rows past the end untouched,
    S / dP strides wider than P's, a row count that leaves idle waves in the last workgroup."""
    rows = 4 * 37 + 3
    ldp = 4096 if ncols == 4096 else (1024 if ncols == 1000 else ncols + 24)
    lds_ = ldp + 40
    g = torch.Generator().manual_seed(ncols)
    Sv = (torch.randn(rows, ncols, generator=g) * 3.0).cuda()
    dPv = torch.randn(rows, ncols, generator=g).cuda()
    Sb, dPb = _sentinel(rows + GUARD, lds_, torch.float32), _sentinel(rows + GUARD, lds_, torch.float32)
    Sb[:rows, :ncols], dPb[:rows, :ncols] = Sv, dPv
    snap = [_bits(Sb).clone(), _bits(dPb).clone()]
    P, dS = _sentinel(rows + GUARD, ldp, dtype), _sentinel(rows + GUARD, ldp, dtype)
    _fill_nan(P, rows, 0, ldp); _fill_nan(dS, rows, 0, ldp)
    regions = [Region(P, rows, (0, ldp)), Region(dS, rows, (0, ldp))]
    scale = 0.125
    ops.softmax_fwd(Sb, lds_, P, ldp, rows, ncols)
    ops.softmax_bwd(P, ldp, dPb, lds_, dS, rows, ncols, scale)
    torch.cuda.synchronize()
    tag = f"softmax {str(dtype)[6:]} ncols={ncols} ldp={ldp}"
    assert torch.equal(_bits(Sb), snap[0]) and torch.equal(_bits(dPb), snap[1]), tag
    for r in regions:
        r.check(tag)
    for t in (P, dS):
        assert torch.equal(t[:rows, ncols:ldp].float(), torch.zeros(rows, ldp - ncols, device="cuda")), tag
    Pk = P[:rows, :ncols].double()
    S64 = Sv.double()
    Pref = torch.softmax(S64, -1)
    if dtype == torch.bfloat16:
        _within(f"{tag} P", Pk, Pref, torch.zeros_like(Pref), 0.0, rel=REL, form="softmax_fwd bf16", out="P")
    else:
        # 4e-7 relative, plus the worst-case rounding of the fp32 row sum: ceil(ncols / 64) additions in each lane, six shuffle levels
        rel = 4e-7 + ((ncols + 63) // 64 + 6) * 2.0 ** -24
        _within(f"{tag} P", Pk, Pref, torch.full_like(Pref, 1e-9), 1.0, rel=rel, form="softmax_fwd fp32", out="P")
    d64 = dPv.double()
    ref = scale * Pk * (d64 - (Pk * d64).sum(-1, keepdim=True))
    A = scale * Pk * (d64.abs() + (Pk * d64.abs()).sum(-1, keepdim=True))
    _within(f"{tag} dS", dS[:rows, :ncols].double(), ref, A, C_SM, rel=REL if dtype == torch.bfloat16 else 4e-7,
            form=f"softmax_bwd {str(dtype)[6:]}", out="dS")


C_F32 = 2.0 ** -14       # fp32 engine: GEMM accumulation over <= 1764 terms plus the softmax


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("nb,H,nq,hd", [(2, 8, 48, 160), (1, 2, 1764, 64)], ids=["vith-neck-self", "global-1764"])
def test_engine_sdpa_against_float64(ops, dt, nb, H, nq, hd):
    """Engine.sdpa (GEMM -> softmax_fwd -> GEMM, and its backward closure) on a small-config engine: the ViT-H neck
    self-attention (head dim 160: above the fused kernels' 128) and a 1764-key global, in both engine modes."""
    import vpu_oracle as vo
    from pvpuformer_amd.engine import Engine, Var
    eng = Engine(vo.make_cfg(embed_dim=128, depth=8, num_heads=4, out_dims=(16, 32, 64, 128), head_channels=32), dt)
    eng.training = True
    td = torch.bfloat16 if dt == "bf16" else torch.float32
    D = H * hd
    nk = nq
    g = torch.Generator().manual_seed(77 + nq)
    mk = lambda n, s: ((torch.rand(nb * n, D, generator=g) * 2 - 1) * s).to(td).cuda()
    Qv, Kv, Vv = Var(mk(nq, 1.5)), Var(mk(nk, 1.5)), Var(mk(nk, 1.5))
    Ov = Var(torch.full((nb * nq, D), float("nan"), device="cuda", dtype=td))
    scale = 1.0 / math.sqrt(hd)
    eng.sdpa((Qv, 0, D, nq), (Kv, 0, D, nk), (Vv, 0, D, nk), (Ov, 0, D, nq), nb, H, nq, nk, hd, scale)
    dO = mk(nq, 1.0)
    Ov.g = dO
    for fn in reversed(eng.tape.fns):
        fn()
    torch.cuda.synchronize()
    hv = lambda t, n: t.double().view(nb, n, H, hd).permute(0, 2, 1, 3).reshape(nb * H, n, hd)
    got = dict(O=hv(Ov.t, nq), dQ=hv(Qv.g, nq), dK=hv(Kv.g, nk), dV=hv(Vv.g, nk))
    ref = _ref(hv(Qv.t, nq), hv(Kv.t, nk), hv(Vv.t, nk), hv(dO, nq), got["O"], scale)
    tag = f"sdpa {dt} nb={nb} H={H} {nq}x{nk} hd={hd}"
    coef, rel = (C_ATTN, REL) if dt == "bf16" else (C_F32, 2.0 ** -22)
    for out, A in (("O", "A_O"), ("dQ", "A_dQ"), ("dK", "A_dK"), ("dV", "A_dV")):
        assert torch.isfinite(got[out]).all(), (tag, out)
        _within(f"{tag} {out}", got[out], ref[out], ref[A], coef, rel, form=f"Engine.sdpa {dt}", out=out)
