"""CPU: the ``Crops`` transform (isegm/inference/transforms/crops.py) with the torch stand-ins of its two kernels against
the reference's recorded results (tests/golden/crops.npz, tools/make_crops_golden.py), and its plumbing through
``BasePredictor`` / ``get_predictor`` with a stub network that records its calls."""
import os

import numpy as np
import pytest
import torch

from pvpuformer_amd.isegm.inference import batched
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import BasePredictor, crops_params_from_env, get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool
from pvpuformer_amd.isegm.inference.transforms import (AddHorizontalFlip, Crops, LimitLongestSide, SigmoidForPred, ZoomIn,
                                                       get_offsets)

from crops_cases import FIXTURE_CASES, RecordingNet, StandInCrops, fixture, host_blend, host_gather
from sessions_cases import blob_image


@pytest.fixture(autouse=True)
def host_transforms(monkeypatch):
    monkeypatch.setattr(T._device, "crops_gather", host_gather)
    monkeypatch.setattr(T._device, "crops_blend", host_blend)
    monkeypatch.delenv("VPU_EVAL_CROPS", raising=False)


@pytest.fixture(scope="module")
def fx():
    return fixture()


def _clicks(rows):
    return [Click(bool(p), (int(r), int(c)), indx=i) for i, (p, r, c) in enumerate(rows)]


# ---------------------------------------------------------------------------------------------------------- get_offsets
@pytest.mark.parametrize("c", [32, 224, 448])
@pytest.mark.parametrize("r", [0.0, 0.2, 0.5])
def test_get_offsets_equals_the_reference(fx, c, r):
    table = fx[f"off_c{c}_r{int(round(100 * r))}"]
    assert table.shape[0] == 3 * c + 1
    for L in range(c, 4 * c + 1):
        want = [int(v) for v in table[L - c] if v >= 0]
        got = get_offsets(L, c, r)
        assert got == want, (L, c, r)
        assert got[0] == 0 and got[-1] == L - c and got == sorted(got)
        assert all(b - a <= c for a, b in zip(got, got[1:])), (L, c, r)        # no gap: every pixel is covered
    assert get_offsets(c, c, r) == [0]


# -------------------------------------------------------------------------------------------- transform / inv_transform
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_transform_and_inverse_equal_the_reference(fx, name):
    image = torch.from_numpy(fx[f"{name}_image"])
    crop = tuple(int(v) for v in fx[f"{name}_crop_size"])
    t = Crops(crop_size=crop, min_overlap=0.2)
    assert t.image_changed is False and (t.crop_height, t.crop_width) == crop
    tiles, lists = t.transform(image, [_clicks(fx[f"{name}_clicks"])])
    assert t.x_offsets == fx[f"{name}_x_offsets"].tolist() and t.y_offsets == fx[f"{name}_y_offsets"].tolist()
    assert t._counts.dtype == torch.float32 and np.array_equal(t._counts.numpy(), fx[f"{name}_counts"])
    n = len(t.x_offsets) * len(t.y_offsets)
    assert tuple(tiles.shape) == (n, 4, *crop) and t.num_tiles == n
    if f"{name}_tiles" in fx.files:
        assert np.array_equal(tiles.numpy(), fx[f"{name}_tiles"])
    else:
        step = int(fx[f"{name}_tiles_step"])
        assert np.array_equal(tiles[..., ::step, ::step].numpy(), fx[f"{name}_tiles_sub"])
    # the click lists: every click in every tile's list, moved by the tile's offset, inside the tile or not
    assert len(lists) == n
    assert np.array_equal(np.asarray([[c.coords for c in cl] for cl in lists]), fx[f"{name}_tile_clicks"])
    for cl in lists:
        assert [(c.is_positive, c.indx) for c in cl] == [(bool(p), i) for i, (p, _, _) in enumerate(fx[f"{name}_clicks"])]
    blended = t.inv_transform(torch.from_numpy(fx[f"{name}_probs"]))
    assert blended.dtype == torch.float32 and np.array_equal(blended.numpy(), fx[f"{name}_blended"])
    assert t.image_changed is False
    # the second call at the same size reuses the device copies and the coverage map
    held = t._counts
    t.transform(image, [[]])
    assert t._counts is held


def test_pass_through_and_single_tile():
    t = Crops(crop_size=(32, 48))
    clicks = [_clicks([(1, 3, 4)])]
    for shape in ((1, 4, 31, 60), (1, 4, 40, 47)):
        image = torch.rand(*shape)
        out, lists = t.transform(image, clicks)
        assert out is image and lists is clicks and t._counts is None and t.num_tiles == 1
        probs = torch.rand(1, 1, *shape[2:])
        assert t.inv_transform(probs) is probs
    image = torch.rand(1, 4, 32, 48)                        # exactly the crop: one tile at (0, 0)
    out, lists = t.transform(image, clicks)
    assert (t.x_offsets, t.y_offsets) == ([0], [0]) and torch.equal(out, image) and t.num_tiles == 1
    assert [c.coords for c in lists[0]] == [(3, 4)] and torch.equal(t._counts, torch.ones(32, 48))
    probs = torch.rand(1, 1, 32, 48)
    assert torch.equal(t.inv_transform(probs), probs)
    out, _ = t.transform(torch.rand(1, 4, 32, 100), clicks)  # one axis exact, the other tiled
    assert t.y_offsets == [0] and len(t.x_offsets) == out.shape[0] > 1


def test_state_round_trip():
    t = Crops(crop_size=(32, 32))
    assert t.get_state() == (None, None, None)
    big, small = torch.rand(1, 4, 47, 70), torch.rand(1, 4, 40, 33)
    t.transform(big, [[]])
    state = t.get_state()
    assert state[0] == [0, 19, 38] and state[1] == [0, 15] and tuple(state[2].shape) == (47, 70)
    probs = torch.rand(6, 1, 32, 32)
    want = t.inv_transform(probs)
    t.transform(small, [[]])                                 # another size: other offsets are in force now
    assert t.x_offsets == [0, 1] and t.inv_transform(probs[:4]).shape == (1, 1, 40, 33)
    t.set_state(state)
    assert t.get_state() == state and torch.equal(t.inv_transform(probs), want)
    t.reset()
    assert t.get_state() == (None, None, None) and t.inv_transform(probs) is probs
    t.set_state(state)                                       # after a reset as well
    assert torch.equal(t.inv_transform(probs), want)


# -------------------------------------------------------------------------------------------------------------- predictor
def test_pipeline_order():
    crops = Crops(crop_size=(32, 32))
    kinds = lambda p: [type(t) for t in p.transforms]
    zoom = ZoomIn(target_size=(64, 64))
    assert kinds(BasePredictor(None, "cpu", zoom_in=zoom, max_size=800, crops=crops, with_flip=True)) == \
        [ZoomIn, LimitLongestSide, Crops, SigmoidForPred, AddHorizontalFlip]
    assert kinds(BasePredictor(None, "cpu", crops=crops)) == [Crops, SigmoidForPred]
    assert kinds(BasePredictor(None, "cpu", crops=crops, with_flip=True)) == [Crops, SigmoidForPred, AddHorizontalFlip]
    assert kinds(BasePredictor(None, "cpu", zoom_in=zoom, crops=crops)) == [ZoomIn, Crops, SigmoidForPred]
    p = BasePredictor(None, "cpu", with_flip=True)
    assert kinds(p) == [SigmoidForPred, AddHorizontalFlip] and p.crops is None and p.net_rows_limit is None
    with pytest.raises(TypeError):
        BasePredictor(None, "cpu", crops=dict(crop_size=(32, 32)))
    with pytest.raises(ValueError):
        BasePredictor(None, "cpu", net_rows_limit=0)


def test_get_predictor_builds_crops():
    p = get_predictor(RecordingNet(), "NoBRS", "cpu", zoom_in_params=None, crops_params=dict(crop_size=(32, 48), min_overlap=0.5))
    (crops,) = [t for t in p.transforms if isinstance(t, Crops)]
    assert crops is p.crops and (crops.crop_height, crops.crop_width, crops.min_overlap) == (32, 48, 0.5)
    assert [type(t) for t in p.transforms] == [Crops, SigmoidForPred, AddHorizontalFlip]
    assert get_predictor(RecordingNet(), "NoBRS", "cpu").crops is None


def test_eval_crops_environment(monkeypatch):
    for text, want in (("448", dict(crop_size=(448, 448))), (" 320,480 ", dict(crop_size=(320, 480))),
                       ("224, 224, 0.5", dict(crop_size=(224, 224), min_overlap=0.5)), ("", None)):
        monkeypatch.setenv("VPU_EVAL_CROPS", text)
        assert crops_params_from_env() == want, text
    monkeypatch.setenv("VPU_EVAL_CROPS", "32,48,0.25")
    p = get_predictor(RecordingNet(), "NoBRS", "cpu")
    assert (p.crops.crop_height, p.crops.crop_width, p.crops.min_overlap) == (32, 48, 0.25)
    explicit = get_predictor(RecordingNet(), "NoBRS", "cpu", crops_params=dict(crop_size=(16, 16)))   # the argument wins
    assert (explicit.crops.crop_height, explicit.crops.min_overlap) == (16, 0.2)
    for bad in ("big", "448x448", "448,", "1,2,3,4", "0", "-32,32", "448,448,1.0", "448.5"):
        monkeypatch.setenv("VPU_EVAL_CROPS", bad)
        with pytest.raises(ValueError, match="VPU_EVAL_CROPS"):
            get_predictor(RecordingNet(), "NoBRS", "cpu")
    monkeypatch.delenv("VPU_EVAL_CROPS")
    assert get_predictor(RecordingNet(), "NoBRS", "cpu").crops is None


def test_tiled_predictor_stays_off_the_batched_paths():
    tiled = get_predictor(RecordingNet(), "NoBRS", "cpu", zoom_in_params=dict(target_size=(32, 32)),
                          crops_params=dict(crop_size=(16, 16)))
    plain = get_predictor(RecordingNet(), "NoBRS", "cpu", zoom_in_params=dict(target_size=(32, 32)))
    assert batched.batchable(plain) and not batched.batchable(tiled)
    with pytest.raises(ValueError, match="batchable"):
        SessionPool(tiled)


H, W, CROP = 47, 70, (32, 32)            # 2 x 3 tiles at (0, 15) x (0, 19, 38)


def _tiled(net, **kw):
    return BasePredictor(net, "cpu", with_flip=True, crops=Crops(crop_size=CROP), **kw)


def _session(pred):
    image, centre = blob_image(H, W, seed=3)
    pred.set_input_image(image)
    return Clicker(device=None), centre


def test_network_rows_and_mirrored_clicks():
    net = RecordingNet()
    pred = _tiled(net)
    clicker, centre = _session(pred)
    clicks = [(True, centre), (False, (2, 66)), (True, (40, 10))]
    for k, (positive, coords) in enumerate(clicks, 1):
        clicker.add_click(Click(positive, coords))
        out = pred.get_prediction(clicker)
        assert out.shape == (H, W) and np.isfinite(out).all()
        shape, points = net.calls[-1]
        assert len(net.calls) == k and shape == (12, 4, *CROP)          # 2 * tiles rows in ONE call
        n = points.shape[1] // 2
        t = 0
        for dy in (0, 15):
            for dx in (0, 19, 38):
                rows = [p for p in points[t].tolist() if p[2] >= 0]
                mirrored = [p for p in points[6 + t].tolist() if p[2] >= 0]
                held = sorted(clicker.get_clicks()[:k], key=lambda c: not c.is_positive)
                assert rows == [[c.coords[0] - dy, c.coords[1] - dx, c.indx] for c in held]
                assert mirrored == [[r, CROP[1] - c - 1, i] for r, c, i in rows]       # the tile's own width
                t += 1
        assert n == max(sum(p for p, _ in clicks[:k]), sum(not p for p, _ in clicks[:k]))
    assert torch.equal(pred.prev_prediction, torch.from_numpy(out)[None, None])


def test_tiles_equal_the_stub_on_the_whole_image():
    """The stub's logit of a pixel depends on that pixel and on its distance to the clicks only, so every tile holds the values
    of the whole image: the blend of equal probabilities is that probability up to the rounding of sum / count."""
    whole_net, tiled_net = RecordingNet(), RecordingNet()
    whole, tiled = BasePredictor(whole_net, "cpu", with_flip=True), _tiled(tiled_net)
    ca, centre = _session(whole)
    cb, _ = _session(tiled)
    for c in (ca, cb):
        c.add_click(Click(True, centre))
    a, b = whole.get_prediction(ca), tiled.get_prediction(cb)
    assert np.abs(a - b).max() < 1e-6


@pytest.mark.parametrize("limit", [1, 5, 6, 12, 100])
def test_net_rows_limit_chunks_equal_one_forward(limit):
    one_net, chunk_net = RecordingNet(), RecordingNet()
    one, chunked = _tiled(one_net), _tiled(chunk_net, net_rows_limit=limit)
    ca, centre = _session(one)
    cb, _ = _session(chunked)
    for positive, coords in ((True, centre), (False, (5, 60))):
        for c in (ca, cb):
            c.add_click(Click(positive, coords))
        want = one.get_prediction(ca)
        before = len(chunk_net.calls)
        got, _ = chunked.get_vqu_prediction(cb, gt_mask=np.zeros((H, W), np.float32))
        assert np.array_equal(got, want)
        sizes = [shape[0] for shape, _ in chunk_net.calls[before:]]
        assert sum(sizes) == 12 and max(sizes) <= limit and len(sizes) == -(-12 // min(limit, 12))
        assert torch.equal(torch.cat([p for _, p in chunk_net.calls[before:]]), one_net.calls[-1][1])


def test_only_click_prompts_with_several_tiles():
    pred = _tiled(RecordingNet())
    clicker, centre = _session(pred)
    clicker.add_click(Click(True, centre))
    gt = np.zeros((H, W), np.float32)
    for kind in (1, 2):
        with pytest.raises(ValueError, match="tiles"):
            pred.get_vqu_prediction(clicker, gt_mask=gt, as_prompt_type=kind)
    out, prompts = pred.get_vqu_prediction(clicker, gt_mask=gt, as_prompt_type=0)
    assert out.shape == (H, W) and prompts[1] is None and prompts[2] is None and tuple(prompts[0].shape) == (12, 2, 3)
    # state round trip through the predictor: back to the state after click 1, click 2 gives its map again
    saved, held = pred.get_states(), clicker.get_state()
    clicker.add_click(Click(False, (3, 3)))
    second = pred.get_prediction(clicker)
    clicker.add_click(Click(True, (30, 50)))
    assert not np.array_equal(pred.get_prediction(clicker), second)
    pred.set_states(saved)
    clicker.set_state(held)
    clicker.add_click(Click(False, (3, 3)))
    assert np.array_equal(pred.get_prediction(clicker), second)


def test_wrappers_refuse_more_tiles_than_the_kernels_accept():
    from pvpuformer_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vpu_hip.h")).read()
    assert f"#define VPU_CROPS_MAX_TILES_AXIS {ops.CROPS_MAX_TILES_AXIS}\n" in header
    many, one = torch.zeros(ops.CROPS_MAX_TILES_AXIS + 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match=str(ops.CROPS_MAX_TILES_AXIS)):
        ops.crops_gather(torch.zeros(4, 8, 8), many, one, 8, 8)
    with pytest.raises(ValueError, match=str(ops.CROPS_MAX_TILES_AXIS)):
        ops.crops_blend(torch.zeros(many.numel(), 8, 8), one, many, 8, 8)


def test_stand_in_class_ignores_the_module_attributes(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device operation was called")
    monkeypatch.setattr(T._device, "crops_gather", refuse)
    monkeypatch.setattr(T._device, "crops_blend", refuse)
    t = StandInCrops(crop_size=CROP)
    tiles, _ = t.transform(torch.rand(1, 4, H, W), [[]])
    assert t.inv_transform(torch.rand(tiles.shape[0], 1, *CROP)).shape == (1, 1, H, W)
    assert T._device.crops_gather is refuse
