"""Dispatch table of the fused-attention tests (tests/test_attention_f64.py): one row per launch pair, with the kernel
instantiation(s) ``vpu_attn_last_kernel()`` must name after the forward and after the backward launch.  Plain data, importable
without a GPU: tests/test_attention_cases_cpu.py checks that the rows reach every launcher branch of xattn_fwd_impl /
xattn_bwd_impl (csrc/attention.hip) and every attention shape the models run.

Row fields:
  entry    "attn" (vpu_attn_fwd / _bwd on a packed qkv matrix), "xattn" (vpu_xattn_fwd / _bwd), "split_k" (long keys:
           vpu_xattn_fwd_split with qdiv = S + vpu_attn_combine, vpu_xattn_bwd_split + vpu_sum_groups of dQ), "split_q" (long
           queries: kdiv = S, vpu_sum_groups of dK / dV)
  nb, H, nq, nk, hd   the whole (unsplit) problem
  lean, onepass       vpu_attn_set_option values for the launch (-1: the library default, lean 1 / onepass 3)
  fwd, bwd            expected vpu_attn_last_kernel() after the forward and after the backward launch
  regime   "ord" (inputs of scale 1.5), "x4" / "x8" (q and k four / eight times larger: the lean forward raises its reference
           maximum several times), "ramp" (keys grow along the sequence: the maximum rises by less than 2^8 -- the lean forward's
           deferred rescale), "flat" (some query rows zero: uniform rows; some dO rows zero)
  S        ranges of a split launch (1 otherwise)
  sens     the test also checks that the bounds reject deliberately wrong float64 answers on this row"""
from collections import namedtuple

Case = namedtuple("Case", "entry nb H nq nk hd lean onepass fwd bwd regime S sens")

CU_COUNT = 256      # MI355X: the persistent window backward's grid is min(nb * H, CUs)


def FL(img, qt, hc):
    return f"attn_fwd_lean_kernel<{img}, {qt}, {hc}>"


def FS(img, qt):
    return f"attn_fwd_kernel<{img}, 1, {qt}>"


def BL(img, q2, k2, hc):
    return f"attn_bwd_dq_lean_kernel<{img}, {q2}, {hc}> attn_bwd_dkdv_lean_kernel<{img}, {k2}, {hc}>"


def BS(img):
    return f"attn_bwd_dq_kernel<{img}, 1> attn_bwd_dkdv_kernel<{img}, 1>"


WINP = "attn_bwd_winp_kernel<1>"
WINX = "attn_bwd_winx_kernel"
WIN = "attn_bwd_win_kernel"


def C(entry, nb, H, nq, nk, hd, fwd, bwd, lean=-1, onepass=-1, regime="ord", S=1, sens=False):
    return Case(entry, nb, H, nq, nk, hd, lean, onepass, fwd, bwd, regime, S, sens)


CASES = [
    # ---- backbone windows (self-attention, window_geometry at 400-672 px): ViT-B / L (patch 16, head dim 64), ViT-H (patch 14, 80)
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), WINX, sens=True),                    # 448 / 672 px, patch 16
    C("attn", 2, 2, 225, 225, 64, FL(64, 2, 64), WIN),                                # 480 px: 8 key blocks
    C("attn", 2, 2, 256, 256, 64, FL(64, 2, 64), WIN),                                # 512 px
    C("attn", 2, 2, 256, 256, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),                # 448 / 672 px, patch 14
    C("attn", 2, 2, 289, 289, 80, FL(128, 2, 96), BS(128)),                          # 480 px, patch 14: 289 % 4 == 1
    C("attn", 2, 2, 324, 324, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),                # 512 px, patch 14
    # ---- globals (one window also covers the grid at 400 px)
    C("attn", 1, 2, 625, 625, 64, FL(64, 2, 64), BS(64)),                             # 400 px, patch 16: 625 % 4 == 1
    C("attn", 1, 2, 784, 784, 64, FL(64, 2, 64), BL(64, 2, 2, 64)),
    C("attn", 1, 2, 900, 900, 64, FL(64, 2, 64), BL(64, 2, 2, 64)),
    C("attn", 1, 2, 1024, 1024, 64, FL(64, 2, 64), BL(64, 2, 2, 64), sens=True),
    C("attn", 1, 2, 1764, 1764, 64, FL(64, 2, 64), BL(64, 2, 2, 64)),                # 672 px, patch 16
    C("attn", 1, 2, 784, 784, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("attn", 1, 2, 1024, 1024, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("attn", 1, 2, 1156, 1156, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("attn", 1, 2, 1296, 1296, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("attn", 1, 2, 2304, 2304, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),              # 672 px, patch 14
    # ---- neck self-attention (2 * num_max_points tokens, head dim D / 8: ViT-B 96, ViT-L 128; ViT-H's 160 takes sdpa)
    C("xattn", 2, 8, 48, 48, 96, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 2, 8, 48, 48, 128, FL(128, 1, 128), BL(128, 1, 1, 128)),
    # ---- neck cross-attention, head dim D / 16: tokens -> image (48 x g^2) and image -> tokens (g^2 x 48)
    C("xattn", 1, 8, 48, 625, 48, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 625, 48, 48, FL(64, 2, 64), BS(64)),
    C("xattn", 1, 8, 48, 784, 48, FL(64, 1, 64), BL(64, 1, 2, 64), sens=True),
    C("xattn", 1, 8, 784, 48, 48, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 900, 48, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 900, 48, 48, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 1024, 48, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 1024, 48, 48, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 1764, 48, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 1764, 48, 48, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 625, 64, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 625, 48, 64, FL(64, 2, 64), BS(64)),
    C("xattn", 1, 8, 48, 784, 64, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 784, 48, 64, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 900, 64, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 900, 48, 64, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 1024, 64, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 1024, 48, 64, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 1764, 64, FL(64, 1, 64), BL(64, 1, 2, 64)),
    C("xattn", 1, 8, 1764, 48, 64, FL(64, 2, 64), BL(64, 2, 1, 64)),
    C("xattn", 1, 8, 48, 784, 80, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 1, 8, 784, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("xattn", 1, 8, 48, 1024, 80, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 1, 8, 1024, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("xattn", 1, 8, 48, 1156, 80, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 1, 8, 1156, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("xattn", 1, 8, 48, 1296, 80, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 1, 8, 1296, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    C("xattn", 1, 8, 48, 2304, 80, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 1, 8, 2304, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96)),
    # ---- head dims the models do not use, and the remaining lean tile pairs
    C("xattn", 3, 2, 20, 33, 16, FL(32, 1, 32), BL(32, 1, 1, 32)),
    C("attn", 2, 3, 196, 196, 32, FL(32, 2, 32), BL(32, 2, 2, 32)),
    C("xattn", 2, 2, 48, 100, 32, FL(32, 1, 32), BL(32, 1, 2, 32)),
    C("xattn", 2, 2, 100, 48, 32, FL(32, 2, 32), BL(32, 2, 1, 32)),
    C("xattn", 2, 3, 48, 48, 48, FL(64, 1, 64), BL(64, 1, 1, 64)),
    C("xattn", 2, 2, 60, 40, 64, FL(64, 1, 64), BL(64, 1, 1, 64)),
    C("xattn", 2, 2, 100, 70, 112, FL(128, 2, 128), BL(128, 2, 1, 128)),
    C("xattn", 1, 2, 48, 300, 112, FL(128, 1, 128), BL(128, 1, 1, 128)),
    # ---- ragged: nq, nk = 1 / 31 (mod 32), nk < 16 (nq % 4 != 0 takes the step backward in the lean family)
    C("xattn", 2, 2, 33, 97, 64, FL(64, 1, 64), BS(64), sens=True),
    C("xattn", 2, 2, 95, 63, 48, FL(64, 2, 64), BS(64)),
    C("xattn", 2, 2, 97, 31, 16, FL(32, 2, 32), BS(32)),
    C("xattn", 2, 2, 63, 1, 80, FL(128, 1, 96), BS(128)),
    C("xattn", 2, 2, 64, 2, 32, FL(32, 1, 32), BL(32, 1, 1, 32)),
    C("xattn", 2, 2, 48, 5, 96, FL(128, 1, 96), BL(128, 1, 1, 96)),
    C("xattn", 2, 2, 129, 65, 112, FL(128, 2, 128), BS(128)),
    # ---- the step kernels (lean = 0): forward with one and with two query tiles per wave
    C("xattn", 2, 2, 48, 100, 32, FS(32, 1), BS(32), lean=0),
    C("xattn", 2, 2, 100, 100, 16, FS(32, 2), BS(32), lean=0),
    C("attn", 1, 2, 784, 784, 64, FS(64, 1), BS(64), lean=0),                       # nk > 256: one tile
    C("attn", 2, 2, 196, 196, 64, FS(64, 2), BS(64), lean=0),
    C("xattn", 1, 4, 48, 784, 80, FS(128, 1), BS(128), lean=0),
    C("xattn", 2, 2, 100, 100, 128, FS(128, 1), BS(128), lean=0),
    C("attn", 1, 2, 97, 97, 48, FS(64, 2), BS(64), lean=0, regime="x8"),
    # ---- the one-pass window backward (head dim 64, nq = nk <= 256)
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), WINP, onepass=2),
    C("attn", 2, 3, 65, 65, 64, FL(64, 2, 64), WINX),                                # 3 key blocks
    C("attn", 2, 2, 97, 97, 64, FL(64, 2, 64), WINX),                                # 4
    C("attn", 2, 2, 159, 159, 64, FL(64, 2, 64), WINX),                              # 5
    C("attn", 2, 2, 175, 175, 64, FL(64, 2, 64), WINX),                              # 6
    C("attn", 75, 4, 100, 100, 64, FL(64, 2, 64), WINX),                             # 300 problems > CUs: the persistent walk
    C("attn", 3, 2, 16, 16, 64, FL(64, 1, 64), WIN),                                 # 1 key block
    C("attn", 2, 2, 50, 50, 64, FL(64, 1, 64), WIN),                                 # 2
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), WIN, onepass=1),                    # 7, per-problem form
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), BL(64, 2, 2, 64), onepass=0),
    # ---- input regimes
    C("attn", 1, 2, 784, 784, 64, FL(64, 2, 64), BL(64, 2, 2, 64), regime="x4"),
    C("attn", 1, 2, 784, 784, 64, FL(64, 2, 64), BL(64, 2, 2, 64), regime="x8"),
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), WINX, regime="x8"),
    C("xattn", 1, 8, 48, 1024, 80, FL(128, 1, 96), BL(128, 1, 1, 96), regime="x4"),
    C("xattn", 1, 8, 48, 1024, 80, FL(128, 1, 96), BL(128, 1, 1, 96), regime="x8"),
    C("xattn", 1, 8, 1024, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96), regime="x8"),
    C("attn", 1, 2, 1024, 1024, 64, FL(64, 2, 64), BL(64, 2, 2, 64), regime="ramp"),
    C("xattn", 1, 8, 48, 1296, 80, FL(128, 1, 96), BL(128, 1, 1, 96), regime="ramp"),
    C("attn", 1, 2, 784, 784, 64, FL(64, 2, 64), BL(64, 2, 2, 64), regime="flat"),
    C("xattn", 1, 8, 48, 784, 48, FL(64, 1, 64), BL(64, 1, 2, 64), regime="flat"),
    C("attn", 2, 2, 196, 196, 64, FL(64, 2, 64), WINX, regime="flat"),
    # ---- split launches (the entry's nq / nk are the whole problem's; the kernels run nk / S or nq / S per entry)
    C("split_k", 1, 8, 48, 784, 48, FL(64, 1, 64), BL(64, 1, 2, 64), S=2),
    C("split_k", 1, 8, 48, 1024, 80, FL(128, 1, 96), BL(128, 1, 1, 96), S=4),
    C("split_k", 1, 8, 48, 2304, 80, FL(128, 1, 96), BL(128, 1, 1, 96), S=8),
    C("split_q", 1, 8, 784, 48, 48, FL(64, 2, 64), BL(64, 2, 1, 64), S=2),
    C("split_q", 1, 8, 1024, 48, 80, FL(128, 2, 96), BL(128, 2, 1, 96), S=4),
    C("split_q", 1, 8, 1792, 48, 64, FL(64, 2, 64), BL(64, 2, 1, 64), S=8),
]
