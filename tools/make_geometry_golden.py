"""Writes tests/golden/geometry*.npz by RUNNING THE REFERENCE at input sizes other than 448 / 672 / 896: the square sizes its
ViT windowing (models_vit.py:225-255 patchify) accepts, see pvpuformer_amd/engine.py window_geometry.  Only the reference runs
here (oracle/vpu_oracle.py's restatement assumes 14-token windows); weights are not stored -- they are regenerated from
``vpu_oracle.synth_state_dict`` (seed 0) exactly as for the other model fixtures, inputs from ``vpu_oracle.synth_batch``.

    python tools/make_geometry_golden.py                 # every case below
    python tools/make_geometry_golden.py eval train table   # (a) + (b), (c), (d)

Cases (key conventions of oracle/make_golden.py run_model_fixture: ``*_sub``, ``*_abs_mean``, ``_loss``, ``_grad_names`` /
``_grad_norms``, ``_grad_slice::``):
  geometry_tiny.npz   (a) tiny (D 128, depth 8, P 16) built at 448, evaluated at 300 / 400 / 480 / 512 after
                          interpolate_pos_embed_inference, click and box prompts.  Keys ``s<S>_<mode>_*``.
  geometry_tinyh.npz  (b) tinyh (P 14, head dim 80) built at 448, evaluated at 400 / 480; the same keys.
  geometry_train.npz  (c) tiny built at 400 (img_size=(400, 400)), train-mode forward (head dropout off), NFL + Dice + P2CL
                          through the reference's own loss objects, backward.  Keys ``train400_click_*``.
  geometry_table.npz  (d) which S in 224..1024 (step 4) the reference runs, P = 16 and P = 14, tiny width, one click forward
                          each: ``sizes``, ``accepted_p16``, ``accepted_p14``.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402
import make_golden as mg  # noqa: E402
import vpu_oracle as vo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY = dict(embed_dim=128, depth=8, num_heads=4, out_dims=(16, 32, 64, 128), head_channels=32)
TINYH = dict(embed_dim=640, depth=8, num_heads=8, patch=14, out_dims=(16, 32, 64, 128), head_channels=32)
B = 2
SEED = 5          # vo.synth_batch seed of every case


def inputs(S, seed=SEED, batch=B):
    bt = vo.synth_batch(batch, S, seed=seed)
    img4 = torch.cat([bt["images"], torch.zeros(batch, 1, S, S)], 1)
    img4[0, 3] = torch.sigmoid(4 * (bt["instances"][0, 0] - 0.5))     # a previous mask, as in a later click iteration
    return bt, img4


def at_size(model, S):
    """scripts/evaluate_vpumodel.py:125: the position embedding re-gridded to the evaluation size."""
    from isegm.model.modeling.pos_embed import interpolate_pos_embed_inference
    interpolate_pos_embed_inference(model.backbone, (S, S), "cpu")


def forward_with_taps(model, img4, pts, boxes, ptype):
    feats = {}
    orig_fb, orig_neck, orig_head = model.backbone.forward_backbone, model.neck.forward, model.head.forward_feat

    def fb(*a, **k):
        feats["bb"] = orig_fb(*a, **k)
        return feats["bb"]

    def nk(*a, **k):
        feats["neck"] = orig_neck(*a, **k)
        return feats["neck"]

    def hd(*a, **k):
        feats["head"] = orig_head(*a, **k)
        return feats["head"]
    model.backbone.forward_backbone, model.neck.forward, model.head.forward_feat = fb, nk, hd
    try:
        prompts = [pts, boxes, [None, None]] if ptype else None
        out = model(img4.clone(), pts.clone(), prompts, ptype, True, False)
    finally:
        model.backbone.forward_backbone, model.neck.forward, model.head.forward_feat = orig_fb, orig_neck, orig_head
    return out, feats


# sub-sampling steps of the stored maps (coarser than run_model_fixture's, so that a file of several sizes stays small); the
# test slices the engine's tensors with the same steps
STEPS = dict(q_out=4, seg_lowres=2, sim_slot=12, sim_pix=4, inst_pix=14, aux_slot=12, aux_pix=21)


def store_outputs(fx, pre, out, feats):
    """run_model_fixture's forward keys under the prefix ``pre`` (steps: STEPS)."""
    st = STEPS
    fx[f"{pre}_backbone_sub"] = feats["bb"].detach()[:, ::37, ::5].contiguous().numpy()
    fx[f"{pre}_backbone_abs_mean"] = np.asarray(feats["bb"].detach().abs().mean().item())
    fx[f"{pre}_q_out_sub"] = feats["neck"][1].detach()[:, :, ::st["q_out"]].contiguous().numpy()
    for i, f in enumerate(feats["neck"][0]):
        fx[f"{pre}_fpn{i}_abs_mean"] = np.asarray(f.detach().abs().mean().item())
        fx[f"{pre}_fpn{i}_sub"] = f.detach()[:, ::9, ::3, ::3].contiguous().numpy()
    fx[f"{pre}_seg_lowres_sub"] = feats["head"][0].detach()[..., ::st["seg_lowres"], ::st["seg_lowres"]].contiguous().numpy()
    fx[f"{pre}_sim_lowres_sub"] = feats["head"][1].detach()[:, ::st["sim_slot"], ::st["sim_pix"], ::st["sim_pix"]].contiguous().numpy()
    fx[f"{pre}_instances_sub"] = mg.sub(out["instances"].detach(), st["inst_pix"])
    fx[f"{pre}_instances_aux_sub"] = mg.sub(out["instances_aux"].detach()[:, ::st["aux_slot"]], st["aux_pix"])
    fx[f"{pre}_instances_mean"] = np.asarray(out["instances"].detach().mean().item())
    fx[f"{pre}_instances_aux_mean"] = np.asarray(out["instances_aux"].detach().mean().item())


def eval_fixture(ref_vpu):
    """(a) + (b): one file per configuration."""
    for name, kw, sizes in (("tiny", TINY, (300, 400, 480, 512)), ("tinyh", TINYH, (400, 480))):
        fx = {"B": np.asarray(B), "images_seed": np.asarray(SEED)}
        fx.update({f"step_{k}": np.asarray(v) for k, v in STEPS.items()})
        cfg = vo.make_cfg(**kw)
        fx.update({f"cfg_{k}": np.asarray(v) for k, v in cfg.items()})
        fx["sizes"] = np.asarray(sizes)
        for S in sizes:
            t0 = time.time()
            model, _ = mg.build_reference(cfg, ref_vpu)
            mg.patch_box_rasteriser(model)
            at_size(model, S)
            bt, img4 = inputs(S)
            fx[f"s{S}_points"] = bt["points"].numpy()
            fx[f"s{S}_boxes"] = bt["boxes"].numpy()
            for mode, ptype in (("click", 0), ("box", 1)):
                with torch.no_grad():
                    out, feats = forward_with_taps(model, img4, bt["points"], bt["boxes"], ptype)
                assert tuple(out["instances"].shape) == (B, 1, S, S)
                store_outputs(fx, f"s{S}_{mode}", out, feats)
            print(f"[geometry_eval] {name} at {S}: {time.time() - t0:.1f}s")
        np.savez_compressed(os.path.join(OUT, f"geometry_{name}.npz"), **fx)


def train_fixture(ref_vpu, ref_losses):
    """(c): a model constructed at 400 x 400 (25 x 25 tokens: one window of 625 tokens, an odd grid for down_32)."""
    S = 400
    cfg = vo.make_cfg(img=S, **TINY)
    model, _ = mg.build_reference(cfg, ref_vpu)
    model.train()
    model.head.dropout = None            # (the engine-side test runs with dropout_ratio 0: no random mask to match)
    bt, img4 = inputs(S)
    gt = bt["instances"]
    fx = {"cfg_" + k: np.asarray(v) for k, v in cfg.items()}
    fx.update({f"step_{k}": np.asarray(v) for k, v in STEPS.items()})
    fx.update(B=np.asarray(B), images_seed=np.asarray(SEED), points=bt["points"].numpy(), boxes=bt["boxes"].numpy())
    for p in model.parameters():
        p.grad = None
    out, feats = forward_with_taps(model, img4, bt["points"], None, 0)
    pre = "train400_click"
    store_outputs(fx, pre, out, feats)
    ed = vo.ed_mask_label(gt, cfg["num_max_points"])
    nfl = ref_losses.NormalizedFocalLossSigmoid(alpha=0.5, gamma=2, penalty_loss=False)
    dice = ref_losses.DiceLoss(use_sigmoid=True, activate=True, naive_dice=True, loss_weight=1.0)
    bce = ref_losses.SigmoidBinaryCrossEntropyLoss(from_sigmoid=True)
    l_nfl = torch.mean(nfl(out["instances"], gt))
    l_dice = torch.mean(dice(out["instances"], gt))
    l_pcl = torch.mean(bce(out["instances_aux"], ed))
    loss = 1.0 * l_nfl + 1.0 * l_dice + 2.0 * l_pcl
    loss.backward()
    fx[f"{pre}_loss"] = np.asarray([loss.item(), l_nfl.item(), l_dice.item(), l_pcl.item()])
    named = dict(model.named_parameters())
    names = list(named)
    fx[f"{pre}_grad_names"] = np.asarray(names)
    fx[f"{pre}_grad_norms"] = np.asarray([float(named[n].grad.norm()) if named[n].grad is not None else -1.0 for n in names])
    fx[f"{pre}_grad_slice::backbone.blocks.0.attn.qkv.weight"] = named["backbone.blocks.0.attn.qkv.weight"].grad[::17, ::13].numpy().copy()
    fx[f"{pre}_grad_slice::neck.ffn_layer.lin1.weight"] = named["neck.ffn_layer.lin1.weight"].grad[::64, ::29].numpy().copy()
    fx[f"{pre}_grad::backbone.pos_embed"] = named["backbone.pos_embed"].grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "geometry_train.npz"), **fx)
    print(f"[geometry_train] loss {loss.item():.6f}")


def table_fixture(ref_vpu):
    """(d): the sizes the reference runs.  A RuntimeError (patchify's view(), the neck's square key PE) is a refusal;
    anything else is a failure of this script."""
    sizes = np.arange(224, 1025, 4)
    fx = {"sizes": sizes}
    for P in (16, 14):
        cfg = vo.make_cfg(patch=P, **TINY)
        model, _ = mg.build_reference(cfg, ref_vpu)
        acc = []
        for S in sizes:
            S = int(S)
            m_pe, m_grid = model.backbone.pos_embed, model.backbone.patch_embed.grid_size
            at_size(model, S)
            bt, img4 = inputs(S, batch=1)
            try:
                with torch.no_grad():
                    model(img4, bt["points"], None, 0, True, False)
                ok = True
            except RuntimeError:
                ok = False
            model.backbone.pos_embed, model.backbone.patch_embed.grid_size = m_pe, m_grid
            acc.append(ok)
            print(f"[geometry_table] P {P} S {S}: {'runs' if ok else 'refused'}", flush=True)
        fx[f"accepted_p{P}"] = np.asarray(acc)
    np.savez_compressed(os.path.join(OUT, "geometry_table.npz"), **fx)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_vpu, ref_losses = ref_import.import_reference()
    which = sys.argv[1:] or ["eval", "train", "table"]
    if "eval" in which:
        eval_fixture(ref_vpu)
    if "train" in which:
        train_fixture(ref_vpu, ref_losses)
    if "table" in which:
        table_fixture(ref_vpu)


if __name__ == "__main__":
    main()
