import os

from .base import BasePredictor
from ..transforms import Crops, ZoomIn


def crops_params_from_env(name="VPU_EVAL_CROPS"):
    """``Crops`` keywords from the environment, for an evaluation script that cannot pass ``crops_params`` (in the style of
    ``VPU_EVAL_BATCH``): ``448`` (a square tile), ``448,448`` (height, width) or ``448,448,0.2`` (and the minimal overlap).
    Unset or empty: None."""
    text = os.environ.get(name, "").strip()
    if not text:
        return None
    fields = [f.strip() for f in text.split(",")]
    try:
        if len(fields) not in (1, 2, 3):
            raise ValueError
        sizes = [int(f) for f in fields[:2]]
        overlap = float(fields[2]) if len(fields) == 3 else None
        if min(sizes) < 1 or (overlap is not None and not 0.0 <= overlap < 1.0):
            raise ValueError
    except ValueError:
        raise ValueError(f"{name}={text!r}: expected SIDE, HEIGHT,WIDTH or HEIGHT,WIDTH,OVERLAP (positive integers, 0 <= overlap "
                         "< 1), e.g. 448 or 448,448,0.2") from None
    params = dict(crop_size=(sizes[0], sizes[-1]))
    if overlap is not None:
        params["min_overlap"] = overlap
    return params


def get_predictor(net, brs_mode, device, prob_thresh=0.49, with_flip=True, zoom_in_params=dict(), predictor_params=None,
                  crops_params=None, **kwargs):
    """isegm/inference/predictors/__init__.py:9-99 restricted to the north star's NoBRS mode.  ``crops_params``: keywords of
    ``Crops`` (tiled prediction); None: those of the environment variable VPU_EVAL_CROPS, no tiling when it is unset."""
    if brs_mode != 'NoBRS':
        raise NotImplementedError("only the NoBRS predictor is on the VPUFormer hot path (BRS variants are RITM legacy)")
    zoom_in = ZoomIn(**zoom_in_params) if zoom_in_params is not None else None
    params = dict(predictor_params or {})
    params.pop('optimize_after_n_clicks', None)
    if crops_params is None:
        crops_params = crops_params_from_env()
    crops = Crops(**crops_params) if crops_params is not None else None
    return BasePredictor(net, device, zoom_in=zoom_in, with_flip=with_flip, crops=crops, **params)
