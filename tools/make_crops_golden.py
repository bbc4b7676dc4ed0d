"""Writes tests/golden/crops.npz by RUNNING THE REFERENCE's Crops transform (isegm/inference/transforms/crops.py), its PuE click
rows and its DistMaps disks; data only.  Read by tests/test_crops_cpu.py and tests/test_crops_gpu.py.

    python tools/make_crops_golden.py

Keys:
  (1) ``off_c<c>_r<r>`` int32 [3c + 1, n_max]: get_offsets(L, c, r) for L = c .. 4c (row L - c), padded with -1; r as a percentage.
  (2) per case ``a`` ([1, 4, 47, 70], crop (32, 32)) and ``b`` ([1, 4, 50, 90], crop (24, 40)): ``<k>_image``, ``<k>_crop_size``,
      ``<k>_x_offsets``, ``<k>_y_offsets``, ``<k>_counts``, ``<k>_clicks`` [3, 3] (is_positive, row, col), ``<k>_tile_clicks``
      [tiles, 3, 2], ``<k>_tiles`` (case b: ``<k>_tiles_sub``, every ``<k>_tiles_step``-th pixel), ``<k>_probs`` [tiles, 1, ch, cw]
      and ``<k>_blended`` [1, 1, H, W] = inv_transform(probs).
  (3) ``oot_*``: a 300 x 380 image in 224 x 224 tiles (offsets [0, 76] x [0, 156]), three clicks, the tiles' shifted click lists
      and their flip copies laid out as BasePredictor.get_points_nd does -> ``oot_points`` [8, 4, 3]; ``oot_pue_index`` [k, 2]
      (sample, row) of the non-padded points and ``oot_pue_rows`` [k, 2 * 224 + 3] float64 = _guassinvector_click's rows there
      (every other row is the not-a-point row: zeros, 1 in the last entry); ``oot_disks_packed`` / ``oot_disks_shape``: DistMaps(norm_radius=5,
      use_disks=True) of the same points at 224 x 224, packed bits.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402
import make_golden as mg  # noqa: E402
import vpu_oracle as vo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY = dict(embed_dim=128, depth=8, num_heads=4, out_dims=(16, 32, 64, 128), head_channels=32)
IMG = 224

CASES = {  # name: (H, W, crop_size, seed, clicks (is_positive, row, col): in an overlap, under one tile, on the border, tile step)
    "a": (47, 70, (32, 32), 11, [(1, 20, 25), (0, 3, 5), (1, 46, 69)], 1),
    "b": (50, 90, (24, 40), 12, [(1, 15, 30), (1, 2, 3), (0, 49, 89)], 3),
}


def offsets_fixture(fx, get_offsets):
    for c in (32, 224, 448):
        for r in (0.0, 0.2, 0.5):
            rows = [get_offsets(L, c, r) for L in range(c, 4 * c + 1)]
            width = max(len(o) for o in rows)
            table = -np.ones((len(rows), width), np.int32)
            for i, o in enumerate(rows):
                table[i, :len(o)] = o
            fx[f"off_c{c}_r{int(round(100 * r))}"] = table


def transform_fixture(fx, Crops, Click):
    for name, (H, W, crop, seed, clicks, step) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        image = torch.rand(1, 4, H, W, generator=g)
        t = Crops(crop_size=crop, min_overlap=0.2)
        tiles, lists = t.transform(image, [[Click(bool(p), (r, c), indx=i) for i, (p, r, c) in enumerate(clicks)]])
        n = len(t.x_offsets) * len(t.y_offsets)
        assert tuple(tiles.shape) == (n, 4, *crop) and len(lists) == n
        probs = torch.rand(n, 1, *crop, generator=g)
        blended = t.inv_transform(probs)
        counts = t._counts.numpy()
        inside = [[0 <= c.coords[0] < crop[0] and 0 <= c.coords[1] < crop[1] for c in cl] for cl in lists]
        cover = np.asarray(inside).sum(0)
        assert cover[0] > 1 and cover[1] == 1, cover       # the first click lies in an overlap, the second under one tile
        fx[f"{name}_image"] = image.numpy()
        fx[f"{name}_crop_size"] = np.asarray(crop, np.int32)
        fx[f"{name}_x_offsets"] = np.asarray(t.x_offsets, np.int32)
        fx[f"{name}_y_offsets"] = np.asarray(t.y_offsets, np.int32)
        fx[f"{name}_counts"] = counts
        fx[f"{name}_clicks"] = np.asarray(clicks, np.int32)
        fx[f"{name}_tile_clicks"] = np.asarray([[c.coords for c in cl] for cl in lists], np.int32)
        if step == 1:
            fx[f"{name}_tiles"] = tiles.numpy()
        else:
            fx[f"{name}_tiles_step"] = np.asarray(step)
            fx[f"{name}_tiles_sub"] = mg.sub(tiles, step)
        fx[f"{name}_probs"] = probs.numpy()
        fx[f"{name}_blended"] = blended.numpy()
        print(f"[crops] case {name}: x {t.x_offsets} y {t.y_offsets} counts up to {int(counts.max())} click cover {cover}")


def points_nd(lists):
    """BasePredictor.get_points_nd (base.py:195-213) of the click lists, without a clicks limit."""
    n = max(max(sum(c.is_positive for c in cl), sum(not c.is_positive for c in cl)) for cl in lists)
    rows = []
    for cl in lists:
        pos = [c.coords_and_indx for c in cl if c.is_positive]
        neg = [c.coords_and_indx for c in cl if not c.is_positive]
        rows.append(pos + (n - len(pos)) * [(-1, -1, -1)] + neg + (n - len(neg)) * [(-1, -1, -1)])
    return np.asarray(rows, np.float32)


def out_of_tile_fixture(fx, ref_vpu, Crops, Click):
    from isegm.inference.transforms import AddHorizontalFlip
    from isegm.model.ops import DistMaps
    clicks = [Click(True, (100, 200), indx=0), Click(False, (250, 100), indx=1), Click(True, (299, 379), indx=2)]
    t = Crops(crop_size=(IMG, IMG), min_overlap=0.2)
    tiles, lists = t.transform(torch.zeros(1, 4, 300, 380), [clicks])
    assert t.y_offsets == [0, 76] and t.x_offsets == [0, 156]
    tiles, lists = AddHorizontalFlip().transform(tiles, lists)
    P = points_nd(lists)
    assert P.shape == (8, 4, 3)
    model, _ = mg.build_reference(vo.make_cfg(img=IMG, **TINY), ref_vpu)
    with torch.no_grad():
        rows = model._guassinvector_click(torch.from_numpy(P)).numpy()
    assert rows.dtype == np.float64 and rows.shape[0] == 8 and rows.shape[2] == 2 * IMG + 3, rows.shape
    n, slots = P.shape[1] // 2, rows.shape[1] // 2
    index = [(b, (j if j < n else slots + j - n)) for b in range(8) for j in range(2 * n) if P[b, j, 2] >= 0]
    keep = np.zeros(rows.shape[:2], bool)
    for b, s in index:
        keep[b, s] = True
    fx["oot_points"] = P
    fx["oot_pue_index"] = np.asarray(index, np.int32)
    fx["oot_pue_rows"] = rows[keep].reshape(len(index), -1)
    nap = np.zeros(rows.shape[2])
    nap[-1] = 1.0
    assert (rows[~keep] == nap).all()               # every other row is the not-a-point row: zeros, then 1 in the last entry
    dm = DistMaps(norm_radius=5, spatial_scale=1.0, cpu_mode=False, use_disks=True)
    with torch.no_grad():
        disks = dm(torch.zeros(8, 3, IMG, IMG), torch.from_numpy(P)).numpy()
    assert set(np.unique(disks)) <= {0.0, 1.0}
    fx["oot_disks_packed"] = np.packbits(disks.astype(np.uint8))
    fx["oot_disks_shape"] = np.asarray(disks.shape)
    outside = int(((P[..., 2] >= 0) & ((P[..., 0] < 0) | (P[..., 0] >= IMG) | (P[..., 1] < 0) | (P[..., 1] >= IMG))).sum())
    print(f"[crops] out-of-tile: {len(index)} click rows, {outside} outside their tile; "
          f"disk pixels {int(disks.sum())}")
    print("[crops] oracle restatement equal: pue", np.array_equal(vo.pue_click(P, img=IMG), rows),
          " disks", np.array_equal(vo.disk_maps(P, IMG, IMG), disks))


def main():
    torch.manual_seed(0)
    ref_vpu, _ = ref_import.import_reference()
    from isegm.inference.clicker import Click
    from isegm.inference.transforms.crops import Crops, get_offsets
    fx = {}
    offsets_fixture(fx, get_offsets)
    transform_fixture(fx, Crops, Click)
    out_of_tile_fixture(fx, ref_vpu, Crops, Click)
    path = os.path.join(OUT, "crops.npz")
    np.savez_compressed(path, **fx)
    print(f"[crops] wrote {path}: {os.path.getsize(path)} bytes, {len(fx)} keys")


if __name__ == "__main__":
    main()
