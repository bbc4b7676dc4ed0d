"""Shared by test_sessions_cpu.py and test_sessions_gpu.py: a ``SessionPool`` driven beside one private predictor per
session with the same click lists, and the comparison of the two after every call."""
import numpy as np
import torch

from pvpuformer_amd.isegm.inference.clicker import Click, Clicker

PRED_THR = 0.49


def blob_image(H, W, seed, radius=0.25, centre=(0.5, 0.5)):
    """uint8 [H, W, 3]: a dim noisy background with one bright ellipse of half-axes ``radius`` * (H, W) -> (image, (row, col))."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = int(centre[0] * H), int(centre[1] * W)
    img = rs.rand(H, W, 3) * 0.35
    img[((yy - cy) / (radius * H)) ** 2 + ((xx - cx) / (radius * W)) ** 2 <= 1.0] += 0.55
    return (np.clip(img, 0, 1) * 255).astype(np.uint8), (cy, cx)


class StubNet:
    """Logits from the image brightness, the previous mask and Gaussian bumps at the clicks (weighted by the click's order).
    Each sample is computed alone and not-a-point rows are skipped, so a sample's output depends neither on the batch it is
    in nor on the click padding."""
    with_prev_mask = True

    def __call__(self, image, points, prompts=None, as_prompt_type=0):
        assert as_prompt_type == 0
        B, _, H, W = image.shape
        n = points.shape[1] // 2
        yy = torch.arange(H, dtype=torch.float32, device=image.device)[:, None]
        xx = torch.arange(W, dtype=torch.float32, device=image.device)[None, :]
        out, rows = [], points.tolist()
        for b in range(B):
            x = image[b]
            logit = 8.0 * (x[:3].mean(0) - 0.5) + 2.0 * (x[3] - 0.5)
            for j in range(points.shape[1]):
                r, c, k = (float(v) for v in rows[b][j])
                if r < 0:
                    continue
                bump = torch.exp(-((yy - r) ** 2 + (xx - c) ** 2) / 18.0)
                logit = logit + (6.0 + 0.25 * k) * (1.0 if j < n else -1.0) * bump
            out.append(logit[None, None])
        return {"instances": torch.cat(out, 0)}


class Twin:
    """Session ``sid`` of ``pool`` and the private predictor that must agree with it."""

    def __init__(self, pool, make_predictor, image):
        self.pool, self.sid = pool, pool.open(image)
        self.pred = make_predictor()
        self.pred.set_input_image(image)
        self.clicker = Clicker(device=None)
        self.last = None                # the private predictor's last map (what get_prediction returned)

    def add(self, positive, coords):
        self.clicker.add_click(Click(bool(positive), (int(coords[0]), int(coords[1]))))

    def save(self):
        return self.pool.get_states(self.sid), self.pred.get_states(), self.clicker.get_state()

    def restore(self, saved):
        self.pool.set_states(self.sid, saved[0])
        self.pred.set_states(saved[1])
        self.clicker.set_state(saved[2])


def step(twins, prev_masks=None):
    """One ``predict`` call for ``twins`` (their clickers hold the pending click lists) and one ``get_prediction`` each;
    -> {sid: (pool mask, private map)}.  ``prev_masks``: {twin: tensor [1, 1, H, W]}."""
    prev_masks = prev_masks or {}
    pool = twins[0].pool
    got = pool.predict({t.sid: t.clicker for t in twins}, prev_masks={t.sid: m for t, m in prev_masks.items()} or None)
    assert sorted(got) == sorted(t.sid for t in twins)
    out = {}
    for t in twins:
        t.last = t.pred.get_prediction(t.clicker, prev_masks.get(t))
        out[t.sid] = (got[t.sid], t.last)
    return out


def assert_equal(twins, results, where):
    """Bit for bit: probabilities, and the mask = the private map > pred_thr."""
    for t in twins:
        mask, want = results[t.sid]
        probs = t.pool.probs(t.sid)
        assert tuple(probs.shape) == tuple(t.pred.prev_prediction.shape), (where, t.sid)
        assert torch.equal(probs, t.pred.prev_prediction), (where, t.sid)
        assert mask.dtype == np.bool_ and mask.shape == want.shape, (where, t.sid)
        assert np.array_equal(mask, want > PRED_THR), (where, t.sid)
