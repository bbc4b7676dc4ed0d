"""GPU: ``vpu_crops_gather`` / ``vpu_crops_blend`` (csrc/evalbatch.hip) against the torch stand-ins on the same device and
against the reference's recorded results, the engine's prompt encoding of clicks that lie outside their tile, and a tiled
``BasePredictor`` against a twin whose ``Crops`` uses the stand-ins: bit for bit in the fp32 engine mode."""
import numpy as np
import pytest
import torch

import vpu_oracle as vo

from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import BasePredictor, get_predictor
from pvpuformer_amd.isegm.inference.transforms import Crops, ZoomIn, get_offsets

from crops_cases import FIXTURE_CASES, KERNEL_CASES, StandInCrops, fixture, host_blend, host_gather
from sessions_cases import blob_image
from test_api_cpu import TINY, make_model

pytestmark = pytest.mark.gpu

IMG = 224
SENTINEL = -7.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _offsets(H, W, ch, cw, overlap):
    ys, xs = get_offsets(H, ch, overlap), get_offsets(W, cw, overlap)
    dev = lambda o: torch.tensor(o, dtype=torch.int32).cuda()
    return ys, xs, dev(ys), dev(xs)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_kernels_equal_the_stand_ins(case):
    _need_gpu()
    from pvpuformer_amd import ops
    H, W, ch, cw, overlap = case
    ys, xs, y_dev, x_dev = _offsets(H, W, ch, cw, overlap)
    tiles = len(ys) * len(xs)
    g = torch.Generator().manual_seed(H * 1000 + W)
    image = torch.rand(1, 4, H, W, generator=g).cuda()
    got = T._device.crops_gather(image, y_dev, x_dev, ch, cw)
    want = host_gather(image, y_dev, x_dev, ch, cw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (tiles, 4, ch, cw) and torch.equal(got, want), (ys, xs)
    # the same planes 4 bytes off a 16-byte boundary: no 16-byte load is legal, the tiles are the same
    shifted = torch.empty(4 * H * W + 1, device="cuda")[1:].view(4, H, W).copy_(image[0])
    assert shifted.data_ptr() % 16 == 4 and torch.equal(ops.crops_gather(shifted, y_dev, x_dev, ch, cw), want)

    probs = torch.rand(tiles, 1, ch, cw, generator=g).cuda()
    out = torch.full((H, W), SENTINEL, device="cuda")
    ops.crops_blend(probs[:, 0].contiguous(), y_dev, x_dev, H, W, out=out)
    want = host_blend(probs, y_dev, x_dev, H, W)
    assert not (out == SENTINEL).any() and torch.isfinite(out).all()           # every pixel is written
    assert torch.equal(out[None, None], want), (ys, xs)
    assert torch.equal(out.cpu()[None, None], host_blend(probs.cpu(), y_dev.cpu(), x_dev.cpu(), H, W))   # and the host's division
    assert torch.equal(T._device.crops_blend(probs, y_dev, x_dev, H, W), want)
    shifted = torch.full((H * W + 1,), SENTINEL, device="cuda")[1:].view(H, W)                # no 16-byte store is legal
    assert torch.equal(ops.crops_blend(probs[:, 0].contiguous(), y_dev, x_dev, H, W, out=shifted)[None, None], want)


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_kernels_equal_the_reference(name):
    _need_gpu()
    fx = fixture()
    crop = tuple(int(v) for v in fx[f"{name}_crop_size"])
    t = Crops(crop_size=crop, min_overlap=0.2)
    tiles, _ = t.transform(torch.from_numpy(fx[f"{name}_image"]).cuda(), [[]])
    assert t.x_offsets == fx[f"{name}_x_offsets"].tolist() and t.y_offsets == fx[f"{name}_y_offsets"].tolist()
    assert t._counts.is_cuda and np.array_equal(t._counts.cpu().numpy(), fx[f"{name}_counts"])
    if f"{name}_tiles" in fx.files:
        assert np.array_equal(tiles.cpu().numpy(), fx[f"{name}_tiles"])
    else:
        step = int(fx[f"{name}_tiles_step"])
        assert np.array_equal(tiles[..., ::step, ::step].cpu().numpy(), fx[f"{name}_tiles_sub"])
    blended = t.inv_transform(torch.from_numpy(fx[f"{name}_probs"]).cuda())
    assert np.array_equal(blended.cpu().numpy(), fx[f"{name}_blended"])


def test_tile_limit_is_refused():
    _need_gpu()
    from pvpuformer_amd import _lib, ops
    many = torch.zeros(ops.CROPS_MAX_TILES_AXIS + 1, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.crops_gather(torch.zeros(1, 4, 4, device="cuda"), many, one, 4, 4)
    buf = torch.zeros(64, device="cuda")
    for name, args in (("vpu_crops_gather", (many.numel(), 1, 1, 4, 4, 4, 4)), ("vpu_crops_blend", (1, many.numel(), 4, 4, 4, 4)),
                       ("vpu_crops_blend", (1, 1, 4, 4, 5, 4))):                     # and a crop larger than the image
        with pytest.raises(_lib.VpuError, match="crops"):
            _lib.call(name, buf.data_ptr(), buf.data_ptr(), many.data_ptr(), many.data_ptr(), *args, None)


# ----------------------------------------------------------------------------------------------------- out-of-tile clicks
def test_prompt_encoding_of_clicks_outside_their_tile():
    """A tile's click list holds every click of the image, so most rows lie outside [0, 224): the PuE rows and the disk maps
    of those rows are the reference's bit for bit."""
    _need_gpu()
    from pvpuformer_amd import ops
    fx = fixture()
    P = fx["oot_points"]
    B, n = P.shape[0], P.shape[1] // 2
    assert ((P[..., 2] >= 0) & ((P[..., :2] < 0) | (P[..., :2] >= IMG)).any(-1)).sum() >= 8
    points = torch.from_numpy(P).cuda()
    lut = torch.from_numpy(vo.click_lut()).cuda()
    E = 2 * IMG + 3
    ld = (E + 7) // 8 * 8
    out = torch.zeros(B, 48, ld, device="cuda")
    out64 = torch.zeros(B, 48, E, device="cuda", dtype=torch.float64)
    ops.pue_encode(points, None, lut, out, out64, B, n, 24, IMG, ld)
    rows = out64.cpu().numpy()
    want = np.zeros_like(rows)
    want[:, :, E - 1] = 1.0                                  # the not-a-point row
    for (b, slot), row in zip(fx["oot_pue_index"], fx["oot_pue_rows"]):
        want[b, slot] = row
    assert np.array_equal(rows, want)
    assert np.array_equal(out[:, :, :E].cpu().numpy().astype(np.float64), want)
    shape = tuple(fx["oot_disks_shape"])
    disks = np.unpackbits(fx["oot_disks_packed"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
    got = torch.zeros(B, 2, IMG, IMG, device="cuda")
    ops.disk_maps(points, None, got, B, n, IMG, IMG, 5.0)
    assert np.array_equal(got.cpu().numpy(), disks)


# -------------------------------------------------------------------------------------------------------------- end to end
_MODELS = {}


def _tiny(dtype):
    if dtype not in _MODELS:
        cfg = vo.make_cfg(img=IMG, **TINY)
        model = make_model(cfg).cuda()
        model.load_state_dict(vo.synth_state_dict(vo.param_shapes(cfg), seed=0), strict=True)
        model.set_compute_dtype(dtype)
        model.eval()
        _MODELS[dtype] = model
    return _MODELS[dtype]


class Rows:
    """The network, with the row count of every call kept."""

    def __init__(self, net):
        self.net, self.with_prev_mask, self.rows = net, net.with_prev_mask, []

    def __call__(self, image, points, *rest):
        self.rows.append(image.shape[0])
        return self.net(image, points, *rest)


H, W = 300, 380
CLICKS = [(True, (150, 190)), (False, (20, 350)), (True, (260, 60))]


def _pair(model, zoom):
    mk_zoom = lambda: None if zoom is None else ZoomIn(**zoom)
    dev = get_predictor(Rows(model), "NoBRS", "cuda", with_flip=True, zoom_in_params=zoom, crops_params=dict(crop_size=(IMG, IMG)))
    twin = BasePredictor(Rows(model), "cuda", with_flip=True, zoom_in=mk_zoom(), crops=StandInCrops(crop_size=(IMG, IMG)))
    assert type(dev.crops) is Crops and type(twin.crops) is StandInCrops and len(dev.transforms) == len(twin.transforms)
    return dev, twin


@pytest.mark.parametrize("zoom,rows", [(None, 8), (dict(target_size=(448, 448), skip_clicks=-1), 18)], ids=["whole", "zoom448"])
def test_end_to_end_fp32_equals_the_stand_in_twin(zoom, rows):
    _need_gpu()
    dev, twin = _pair(_tiny("f32"), zoom)
    image, _ = blob_image(H, W, seed=5)
    clickers = []
    for p in (dev, twin):
        p.set_input_image(image)
        clickers.append(Clicker(device=None))

    def click(k, where):
        for c in clickers:
            c.add_click(Click(*CLICKS[k]))
        a, b = dev.get_prediction(clickers[0]), twin.get_prediction(clickers[1])
        assert a.shape == (H, W) and np.isfinite(a).all(), where
        assert np.array_equal(a, b) and torch.equal(dev.prev_prediction, twin.prev_prediction), where
        assert dev.net.rows[-1] == rows and twin.net.rows[-1] == rows, (where, dev.net.rows)
        return a

    click(0, "click 1")
    saved = [(p.get_states(), c.get_state()) for p, c in zip((dev, twin), clickers)]
    second = click(1, "click 2")
    third = click(2, "click 3")
    assert not np.array_equal(second, third)
    for p, c, (states, held) in zip((dev, twin), clickers, saved):
        p.set_states(states)
        c.set_state(held)
    assert np.array_equal(click(1, "click 2 after set_states"), second)


def test_one_tile_equals_no_crops():
    _need_gpu()
    model = _tiny("f32")
    image, centre = blob_image(IMG, IMG, seed=6)
    tiled = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=None, crops_params=dict(crop_size=(IMG, IMG)))
    plain = get_predictor(model, "NoBRS", "cuda", with_flip=True, zoom_in_params=None)
    clickers = []
    for p in (tiled, plain):
        p.set_input_image(image)
        clickers.append(Clicker(device=None))
    for positive, coords in ((True, centre), (False, (10, 200))):
        for c in clickers:
            c.add_click(Click(positive, coords))
        a, b = tiled.get_prediction(clickers[0]), plain.get_prediction(clickers[1])
        assert tiled.crops.num_tiles == 1 and tiled.crops._counts is not None
        assert np.array_equal(a, b) and torch.equal(tiled.prev_prediction, plain.prev_prediction)


def test_end_to_end_bf16_runs():
    """No bound: the bf16 GEMM instantiation is chosen by the row count, so 8 rows need not run the kernels of 2."""
    _need_gpu()
    dev, _ = _pair(_tiny("bf16"), None)
    dev.set_input_image(blob_image(H, W, seed=5)[0])
    clicker = Clicker(device=None)
    for k in range(2):
        clicker.add_click(Click(*CLICKS[k]))
        out = dev.get_prediction(clicker)
        assert out.shape == (H, W) and out.dtype == np.float32 and np.isfinite(out).all() and dev.net.rows[-1] == 8
        assert 0.0 <= out.min() and out.max() <= 1.0
