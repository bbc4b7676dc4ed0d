"""CPU: run-length maps (isegm/inference/runs.py).  The numpy stand-in and ``RunMap`` against the stream rule written out per
pixel at every shape and pattern of runs_cases.py, the constants against the header, and the three run-length calls of the
pools on the stub network with the host ops after every step of a short script.  Everything is integer: equality is exact."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvpuformer_amd import ops
from pvpuformer_amd.isegm.inference import HostRunOps, RunMap, host_runs_encode
from pvpuformer_amd.isegm.inference import transforms as T
from pvpuformer_amd.isegm.inference.annotation import AnnotationPool
from pvpuformer_amd.isegm.inference.clicker import Click, Clicker
from pvpuformer_amd.isegm.inference.predictors import get_predictor
from pvpuformer_amd.isegm.inference.sessions import SessionPool

from runs_cases import (PATTERNS, SHAPES, THR, case, decode_counts, run_pool_script, shape_id, stream_counts, stream_runs,
                        values_of)
from sessions_cases import PRED_THR, StubNet, blob_image


@pytest.fixture(autouse=True)
def host_transforms(monkeypatch):
    """ZoomIn's two device calls on the host, as in test_annotation_cpu.py."""
    def mask_box(prob, thr, positive_clicks=()):
        m = (prob[0, 0] > thr).numpy().copy()
        count = int(m.sum())
        for r, c in positive_clicks:
            m[int(r), int(c)] = True
        rows, cols = np.nonzero(m)
        if len(rows) == 0:
            return 0, m.shape[0], -1, m.shape[1], -1
        return count, int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())

    monkeypatch.setattr(T._device, "resize_align_corners",
                        lambda x, size: F.interpolate(x.float(), size=tuple(int(s) for s in size), mode="bilinear",
                                                      align_corners=True))
    monkeypatch.setattr(T._device, "mask_box", mask_box)


# ------------------------------------------------------------------------------------------------------------- the type
@pytest.mark.parametrize("kind", [0, 1], ids=["prob", "labels"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_stand_in_follows_the_stream_rule(shape, kind):
    H, W = shape
    for name in PATTERNS:
        src = case(kind, name, H, W)
        v = values_of(src, kind)
        rm = host_runs_encode(src, kind, THR)
        where = (shape, kind, name)
        starts, values = stream_runs(v)
        assert isinstance(rm, RunMap) and rm.size == (H, W), where
        assert rm.starts.dtype == np.int32 and rm.values.dtype == np.int32, where
        assert rm.starts.tolist() == starts and rm.values.tolist() == values, where
        assert rm.lengths().tolist() == np.diff(np.array(starts + [H * W])).tolist(), where
        got = rm.decode()
        assert got.dtype == np.uint16 and got.shape == (H, W) and np.array_equal(got, v), where
        for label in (1, 0, 65535, 7):                                      # 7 never occurs
            counts = rm.counts(label)
            assert all(type(n) is int for n in counts) and counts == stream_counts(v, label), (where, label)
            assert sum(counts) == H * W and rm.area(label) == int((v == label).sum()), (where, label)
            assert rm.to_coco(label) == dict(size=[H, W], counts=counts), (where, label)
            assert np.array_equal(decode_counts(rm.to_coco(label)), v == label), (where, label)
        assert rm.counts(7) == [H * W], where
        if name == "zero":
            assert len(rm) == 1 and rm.values.tolist() == [0], where
        if name == "set":
            assert len(rm) == 1 and rm.counts(1) == [0, H * W], where        # the first stream pixel is set
        if name == "checkerboard":
            assert len(rm) == H * W, where


def test_no_run_starts_where_a_value_continues_into_the_next_column():
    for kind in (0, 1):
        src = case(kind, "boundary", 5, 6)
        v = values_of(src, kind)
        rm = host_runs_encode(src, kind, THR)
        for c in range(5):
            assert (v[4, c] == v[0, c + 1]) == (c % 2 == 0)
            assert ((c + 1) * 5 in rm.starts.tolist()) == (c % 2 == 1), (kind, c)


def test_threshold_is_strict_and_in_fp32():
    above = np.nextafter(np.float32(THR), np.float32(1))
    src = np.array([[THR, above], [above, THR]], dtype=np.float32)
    rm = host_runs_encode(src, 0, THR)
    assert rm.values.tolist() == [0, 1, 0] and rm.starts.tolist() == [0, 1, 3]
    assert case(0, "random", 47, 70).dtype == np.float32 and (case(0, "random", 47, 70) == np.float32(THR)).any()


def test_header_defines_equal_the_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vpu_hip.h")).read()
    assert f"#define VPU_RUNS_BAND_ROWS {ops.RUNS_BAND_ROWS}\n" in header
    assert f"#define VPU_RUNS_COLS {ops.RUNS_COLS}\n" in header
    assert ops.runs_scratch_len([(ops.RUNS_BAND_ROWS + 1, 5), (3, 7)]) == 2 * 10


def test_host_ops_encode_tensors():
    labels = case(1, "random", 33, 130)
    prob = case(0, "ellipse", 47, 70)
    got = HostRunOps().encode([(torch.from_numpy(labels.view(np.int16)), 1, 0.0), (torch.from_numpy(prob), 0, THR)])
    assert np.array_equal(got[0].decode(), labels) and np.array_equal(got[1].decode(), prob > np.float32(THR))
    assert HostRunOps().encode([]) == []


# ------------------------------------------------------------------------------------------------------------- the pools
def _make(zoom):
    zoom_params = dict(skip_clicks=-1, target_size=(32, 32), min_crop_size=12) if zoom else None
    return lambda: get_predictor(StubNet(), "NoBRS", "cpu", with_flip=True, zoom_in_params=zoom_params)


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_session_pool_mask_runs(zoom):
    pool = SessionPool(_make(zoom)(), max_sessions=3, pred_thr=PRED_THR)
    assert isinstance(pool.ops_runs, HostRunOps)
    images = [blob_image(H, W, seed=j) for j, (H, W) in enumerate([(60, 80), (48, 48), (50, 70)])]
    sids = [pool.open(image) for image, _ in images]
    before = pool.readbacks
    fresh = pool.mask_runs()
    assert pool.readbacks == before + 2 and sorted(fresh) == sids
    for sid, (image, _) in zip(sids, images):
        assert fresh[sid].size == image.shape[:2] and fresh[sid].starts.tolist() == [0] and fresh[sid].values.tolist() == [0]
    clicks = {sid: Clicker(device=None) for sid in sids}
    for sid, (_, centre) in zip(sids, images):
        clicks[sid].add_click(Click(True, centre))
    for step in range(3):
        masks = pool.predict({sid: clicks[sid] for sid in sids[:2]} if step == 1 else clicks)
        before = pool.readbacks
        runs = pool.mask_runs(list(masks))
        assert pool.readbacks == before + 2 and sorted(runs) == sorted(masks)
        for sid, mask in masks.items():
            assert np.array_equal(runs[sid].decode(), mask), (step, sid)
            assert np.array_equal(decode_counts(runs[sid].to_coco()), mask) and runs[sid].area() == int(mask.sum()), (step, sid)
            assert mask.any() and not mask.all()
        for sid, (_, (r, c)) in zip(sids, images):
            clicks[sid].add_click(Click(step == 0, (r // 2 + 3 * step, c // 2 + 5)))
    one = pool.mask_runs([sids[2]])
    assert list(one) == [sids[2]]
    before = pool.readbacks
    assert pool.mask_runs([]) == {} and pool.readbacks == before
    pool.close(sids[1])
    assert sorted(pool.mask_runs()) == [sids[0], sids[2]]
    for bad in (sids[1], 7, "0"):
        with pytest.raises(KeyError):
            pool.mask_runs([bad])


@pytest.mark.parametrize("zoom", [False, True], ids=["whole", "zoom32"])
def test_annotation_pool_label_runs_and_export(zoom):
    ann = AnnotationPool(_make(zoom)(), max_images=3)
    assert isinstance(ann.ops_runs, HostRunOps)
    images = [blob_image(H, W, seed=j) for j, (H, W) in enumerate([(60, 80), (48, 48), (50, 70)])]
    seen = []

    def check(where, aids, masks):
        seen.append(where)
        for aid in aids:
            for preview in (True, False):
                want = ann.label_map(aid, preview)
                before = ann.readbacks
                rm = ann.label_runs(aid, preview)
                assert ann.readbacks == before + 2, (where, aid)
                assert rm.size == want.shape and np.array_equal(rm.decode(), want), (where, aid, preview)
            committed, records = ann.label_map(aid, False), ann.objects(aid)
            before = ann.readbacks
            out = ann.export(aid)
            assert ann.readbacks == before + (2 if records else 0), (where, aid)
            assert [{k: v for k, v in e.items() if k != "segmentation"} for e in out] == records, (where, aid)
            for e in out:
                seg = e["segmentation"]
                assert seg["size"] == list(committed.shape) and all(type(n) is int for n in seg["counts"]), (where, aid)
                assert np.array_equal(decode_counts(seg), committed == e["label"]), (where, aid, e["label"])
            if masks is not None and ann.object_count(aid) == 0 and where == "click 1":
                assert np.array_equal(ann.label_runs(aid).decode() == 1, masks[aid]), (where, aid)

    aids = run_pool_script(ann, images, check)
    assert "reopen" in seen and len(seen) == 13
    for aid in aids:
        out = ann.export(aid)
        assert [e["label"] for e in out] == [r["label"] for r in ann.objects(aid)] and len(out) == 2
        newest = out[-1]                                                     # nothing was drawn over the newest object
        assert newest["area"] == sum(newest["segmentation"]["counts"][1::2]) > 0


def test_export_areas_equal_the_records_while_nothing_overlaps():
    ann = AnnotationPool(_make(False)(), max_images=1)
    image, (r, c) = blob_image(60, 80, seed=0)
    aid = ann.open(image)
    before = ann.readbacks
    assert ann.export(aid) == [] and ann.readbacks == before                 # a fresh annotation: the device is not touched
    ann.click({aid: (True, (r, c))})
    assert ann.export(aid) == []                                             # an object in progress is not exported
    first = ann.finish(aid)
    ann.set_mask(aid, np.pad(np.ones((3, 4), dtype=bool), ((0, 57), (0, 76))))
    second = ann.finish(aid)
    out = ann.export(aid)
    assert [e["label"] for e in out] == [1, 2] and second["overwritten"] == 0
    for e, record in zip(out, (first, second)):
        assert e["area"] == record["area"] == sum(e["segmentation"]["counts"][1::2])
    first_pixel_set = out[1]["segmentation"]["counts"]
    assert first_pixel_set[0] == 0 and first_pixel_set[1] == 3               # the mask's first stream pixel is (0, 0)


def test_unknown_ids_raise_key_error():
    ann = AnnotationPool(_make(False)(), max_images=2)
    aid = ann.open(blob_image(48, 48, seed=0)[0])
    for bad in (aid + 1, -1, "0", None):
        with pytest.raises(KeyError):
            ann.label_runs(bad)
        with pytest.raises(KeyError):
            ann.export(bad)
    ann.close(aid)
    with pytest.raises(KeyError):
        ann.export(aid)
