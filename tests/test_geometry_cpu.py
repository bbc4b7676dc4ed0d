"""CPU: the input-size rule (pvpuformer_amd.engine.window_geometry) against the sizes the reference itself runs
(tests/golden/geometry_table.npz, written by tools/make_geometry_golden.py), and the public constructor at those sizes."""
import os

import numpy as np
import pytest

import vpu_oracle as vo
from test_api_cpu import TINY, make_model


def _legal(S, P):
    from pvpuformer_amd.engine import window_geometry
    try:
        window_geometry(S, P)
        return True
    except ValueError:
        return False


@pytest.mark.parametrize("P", [16, 14])
def test_rule_matches_the_sizes_the_reference_runs(golden_dir, P):
    fx = np.load(os.path.join(golden_dir, "geometry_table.npz"))
    sizes, acc = fx["sizes"], fx[f"accepted_p{P}"]
    assert len(sizes) == 201 and sizes[0] == 224 and sizes[-1] == 1024
    mine = np.array([_legal(int(S), P) for S in sizes])
    assert np.array_equal(mine, acc), [int(S) for S, a, b in zip(sizes, mine, acc) if a != b]
    assert acc.sum() > 40 and (~acc).sum() > 40            # both sets are large: the table is not trivially all-or-nothing


@pytest.mark.parametrize("S,P,expect", [
    (224, 16, (14, 1, 14)), (300, 16, (18, 1, 18)), (336, 16, (21, 1, 21)), (400, 16, (25, 1, 25)), (448, 16, (28, 2, 14)),
    (480, 16, (30, 2, 15)), (512, 16, (32, 2, 16)), (576, 16, (36, 2, 18)), (640, 16, (40, 2, 20)), (672, 16, (42, 3, 14)),
    (720, 16, (45, 3, 15)), (896, 16, (56, 4, 14)), (448, 14, (32, 2, 16)), (400, 14, (28, 1, 28)), (480, 14, (34, 2, 17)),
    (300, 14, (21, 1, 21))])
def test_window_geometry_values(S, P, expect):
    from pvpuformer_amd.engine import window_geometry
    assert window_geometry(S, P) == expect


@pytest.mark.parametrize("S,P", [(500, 16), (560, 16), (600, 16), (208, 16), (196, 14), (0, 16)])
def test_window_geometry_refuses_with_the_rule(S, P):
    from pvpuformer_amd.engine import window_geometry
    with pytest.raises(ValueError, match="window"):
        window_geometry(S, P)


@pytest.mark.parametrize("S,P", [(300, 16), (400, 16), (480, 16), (512, 16), (720, 16), (400, 14), (480, 14)])
def test_constructor_builds_the_parameter_tree_at_legal_sizes(S, P):
    cfg = vo.make_cfg(img=S, patch=P, **TINY)
    m = make_model(cfg)
    g = S // P
    sd = m.state_dict()
    shapes = vo.param_shapes(cfg)
    assert list(sd.keys()) == list(shapes.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), k
    assert tuple(sd["backbone.pos_embed"].shape) == (1, g * g + 1, cfg["embed_dim"])
    assert tuple(sd["neck.ffn_layer.lin1.weight"].shape) == (2048, 2 * S + 3)     # PuE vectors keep the constructor's size
    assert m.backbone.patch_embed.grid_size == (g, g)


@pytest.mark.parametrize("S,P", [(500, 16), (560, 16), (600, 16), (208, 16), (490, 14)])
def test_constructor_refuses_sizes_the_reference_cannot_window(S, P):
    with pytest.raises(ValueError, match="window"):
        make_model(vo.make_cfg(img=S, patch=P, **TINY))


def test_rectangular_inputs_are_refused():
    from pvpuformer_amd.engine import check_square
    from pvpuformer_amd.isegm.model.is_vpu_model import VitMultiGaussianVector_ed_Model
    with pytest.raises(ValueError, match="square"):
        check_square(448, 672)
    cfg = vo.make_cfg(**TINY)
    bp = dict(img_size=(448, 672), patch_size=(16, 16), in_chans=3, embed_dim=cfg["embed_dim"], depth=cfg["depth"],
              num_heads=cfg["num_heads"], mlp_ratio=cfg["mlp_ratio"], qkv_bias=True)
    with pytest.raises(ValueError, match="square"):
        VitMultiGaussianVector_ed_Model(use_disks=True, norm_radius=5, with_prev_mask=True, backbone_params=bp,
                                        neck_params=dict(in_dim=cfg["embed_dim"], out_dims=list(cfg["out_dims"]), img_size=(448, 672)),
                                        head_params=dict(in_channels=list(cfg["out_dims"]), in_index=[0, 1, 2, 3], dropout_ratio=0.1,
                                                         num_classes=1, loss_decode=None, align_corners=False, upsample='x1',
                                                         ed_loss=True, channels=cfg["head_channels"]),
                                        random_split=False, residual=True, with_aux_output=True)


def test_mae_position_embedding_regrids_to_the_model_grid():
    """init_weights_from_pretrained's interpolate_pos_embed: the MAE 14 x 14 grid onto g x g (here 25 x 25 at 400 px)."""
    import torch
    from pvpuformer_amd.isegm.model.modeling.pos_embed import interpolate_pos_embed
    m = make_model(vo.make_cfg(img=400, **TINY))
    ck = {"pos_embed": torch.randn(1, 1 + 14 * 14, 128)}
    interpolate_pos_embed(m.backbone, ck)
    assert tuple(ck["pos_embed"].shape) == (1, 1 + 25 * 25, 128)
