"""What the batched inference paths (``batched``, ``sessions``, ``annotation``, ``runs``) share.

``ZoomHost``: ``ZoomIn`` restated on the host from the box read back with the last prediction, and the forward of one size
group.  The bit codec and ``PackedLayout``: the read-back "one 8-int32 record per row, then every row's packed mask".
``host_*``: the torch / numpy pieces the host stand-ins of the kernels are made of.  ``upload_structs``: ctypes descriptor
arrays to the device in one pinned copy.

The three records (csrc/evalbatch.hip, ``MaskRec``), each int32 [8] = counters, box (rmin, rmax, cmin, cmax), zeros:
paste statistics {intersection, union, count | box}, session {area, count | box}, annotation {area, overwritten | box}.
A box without a pixel is (H, -1, W, -1)."""
import numpy as np
import torch

from .transforms import AddHorizontalFlip, Roi, ZoomIn, resize_align_corners

_REC = 4             # int64 per record (int32 [8])


# ------------------------------------------------------------------------------------------------------ ZoomIn on the host
class ZoomHost:
    """Base of ``BatchedEvaluator`` and ``SessionPool``.  A slot ``o`` (an object or a session) carries ``H, W``, its
    ``clicks``, ``roi`` (ZoomIn._object_roi) and ``box``: (count, r0, r1, c0, c1) of ZoomIn._probs > prob_thresh without the
    clicks, None while there is no _probs."""

    def __init__(self, predictor):
        self.pred = predictor
        self.zoom = predictor.zoom_in
        self.flip = any(type(t) is AddHorizontalFlip for t in predictor.transforms)
        self.inv = [t for t in reversed(predictor.transforms) if type(t) is not ZoomIn]   # flip average, then sigmoid
        self.prev_channel = bool(getattr(predictor.net, "with_prev_mask", True))
        self.device = torch.device(predictor.device)

    def _predicted_box(self, o, clicks=()):
        """ZoomIn._predicted_box from the read-back box of the last prediction, joined here with the positive clicks."""
        if o.box is None:
            return None
        count, r0, r1, c0, c1 = o.box
        for c in clicks:
            if c.is_positive:
                r, k = int(c.coords[0]), int(c.coords[1])
                r0, r1, c0, c1 = min(r0, r), max(r1, r), min(c0, k), max(c1, k)
        if count == 0:
            return None
        return Roi(r0, r1, c0, c1).grown(self.zoom.expansion_ratio, self.zoom.min_crop_size).clipped(o.H, o.W)

    def _plan(self, o):
        """ZoomIn.transform of this click: (input roi, network input size, clicks in network coordinates, paste roi)."""
        whole, clicks, zi = Roi.whole(o.H, o.W), o.clicks, self.zoom
        crop = False
        if zi is not None and len(clicks) > zi.skip_clicks:
            box = self._predicted_box(o, clicks)
            if box is None and zi.skip_clicks < 0:
                box = whole                             # zoom from the very first click on
            if box is not None:
                held = o.roi
                if held is None or not Roi(*held).encloses(clicks) or box.overlap(held) < zi.recompute_thresh_iou:
                    o.roi = box
                crop = True
        if crop:
            roi = Roi(*o.roi)
            size = tuple(int(s) for s in roi.output_size(zi.target_size))
            net_clicks = [c.copy(coords=roi.to_crop(c.coords, size)) for c in clicks]
            return roi, size, net_clicks, roi
        return whole, (o.H, o.W), list(clicks), (Roi(*o.roi) if o.roi is not None else whole)

    def _own_rows(self, clicks):
        """Rows per polarity of ``get_points_nd([clicks])``: the click layout the sequential call sees for this slot."""
        pos = sum(c.is_positive for c in clicks)
        n = max(pos, len(clicks) - pos)
        if self.pred.net_clicks_limit is not None:
            n = min(self.pred.net_clicks_limit, n)
        return max(1, n)

    def _wants_recalc(self, o):
        """ZoomIn.check_possible_recalculation after this step's prediction (o.box is its box)."""
        zi = self.zoom
        if zi is None or o.roi is not None or zi.skip_clicks > 0:
            return False
        box = self._predicted_box(o)
        return box is not None and box.overlap(Roi.whole(o.H, o.W)) < 0.50

    def flipped_click_lists(self, lists, width):
        """The click lists of a forward: ``lists`` and, when the predictor flips, their mirror images in a network input
        ``width`` wide behind them (AddHorizontalFlip on a batch: [straight..., mirrored...])."""
        if not self.flip:
            return lists
        return lists + [[c.copy(coords=(c.coords[0], width - c.coords[1] - 1)) for c in cl] for cl in lists]

    def _forward(self, image_nd, points_nd, prompts=None, ptype=0):
        """The network on one size group -> the probabilities at the input's size, after the predictor's own flip average and
        sigmoid on the whole batch.  No prompts and type 0 is the plain two-argument call."""
        if ptype == 0 and prompts is None:
            logits = self.pred.net(image_nd, points_nd)['instances']
        else:
            logits = self.pred.net(image_nd, points_nd, prompts, ptype)['instances']
        if tuple(logits.shape[2:]) != tuple(image_nd.shape[2:]):
            logits = resize_align_corners(logits, image_nd.shape[2:])
        probs = logits
        for t in self.inv:
            probs = t.inv_transform(probs)
        return probs


# ------------------------------------------------------------------------------------------------------ the bit codec
def n_words(hw):
    return (int(hw) + 63) // 64


def pack_mask(mask):
    """bool [H, W] -> uint64 [ceil(H * W / 64)]: pixel i = r * W + c is bit i & 63 of little-endian word i >> 6; the bits at or
    beyond H * W are zero."""
    flat = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
    padded = np.zeros(n_words(flat.size) * 64, dtype=bool)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def unpack_mask(words, H, W):
    """The inverse of ``pack_mask``: 64-bit words (uint64 or the int64 of a read-back) -> bool [H, W]."""
    raw = np.ascontiguousarray(words).view(np.uint64).astype("<u8").view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[:H * W].astype(bool).reshape(H, W)


class PackedLayout:
    """An int64 read-back buffer for rows of ``sizes`` [(H, W)]: ``_REC`` int64 (one record) per row, then every row's packed
    words.  ``size``: its length; ``rec_at(i)`` / ``bits_at(i)``: the int64 offset of row i's record / words."""

    def __init__(self, sizes):
        self.sizes = [(int(H), int(W)) for H, W in sizes]
        self._bits, at = [], _REC * len(self.sizes)
        for H, W in self.sizes:
            self._bits.append(at)
            at += n_words(H * W)
        self.size = at

    def rec_at(self, i):
        return _REC * i

    def bits_at(self, i):
        return self._bits[i]

    def put(self, out, i, rec, words):
        """Writes row i's record (int32 [8]) and packed words (uint64) into ``out`` (int64), as a kernel would."""
        out[_REC * i:_REC * (i + 1)] = rec.view(np.int64)
        out[self._bits[i]:self._bits[i] + len(words)] = words.view(np.int64)

    def decode(self, out, i, masks=True):
        """(record int32 [8], mask bool [H, W] or None without ``masks``) of row i from the read-back ``out`` (int64)."""
        H, W = self.sizes[i]
        rec = out[_REC * i:_REC * (i + 1)].view(np.int32)
        return rec, unpack_mask(out[self._bits[i]:self._bits[i] + n_words(H * W)], H, W) if masks else None


# ------------------------------------------------------------------------------------------------------ host stand-ins
def host_resize(x, size):
    """[N, C, h, w] -> [N, C, *size] as crop_resize resizes: bilinear with align_corners, a copy when the size is the same."""
    if tuple(x.shape[2:]) == tuple(size):
        return x.clone()
    return torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


def host_roi_resize(image, prev, roi, size):
    """Stand-in of vpu_roi_resize_batched for one row: crop_resize(cat(image [3, H, W], prev [H, W]), roi, size) ->
    [1, 4, *size]; ``prev`` None: the image alone, three channels."""
    r0, r1, c0, c1 = roi
    x = image[None] if prev is None else torch.cat((image[None], prev[None, None]), 1)
    return host_resize(x[:, :, r0:r1 + 1, c0:c1 + 1], size)


def host_roi_paste(prob_map, H, W, roi):
    """ZoomIn.inv_transform on the host: ``prob_map`` fp32 [S_h, S_w] resized to the roi and pasted into zeros -> fp32 [H, W]."""
    r0, r1, c0, c1 = roi
    canvas = torch.zeros(H, W, dtype=torch.float32)
    canvas[r0:r1 + 1, c0:c1 + 1] = host_resize(prob_map.float()[None, None], (r1 - r0 + 1, c1 - c0 + 1))[0, 0]
    return canvas


def host_count_box(on, H, W):
    """[count, rmin, rmax, cmin, cmax] of the set pixels of ``on`` (bool [H, W]); [0, H, -1, W, -1] when there is none."""
    at = np.argwhere(on)
    if len(at) == 0:
        return [0, H, -1, W, -1]
    return [len(at), int(at[:, 0].min()), int(at[:, 0].max()), int(at[:, 1].min()), int(at[:, 1].max())]


# ------------------------------------------------------------------------------------------------------ descriptors
def upload_structs(device, *arrays):
    """ctypes arrays of descriptors, one behind the other, to ``device`` in one non-blocking copy from pinned memory ->
    (pinned host tensor, device tensor, byte offset of each array).  The host tensor has to stay alive until the stream has
    synchronised past the copy; an empty array takes no bytes."""
    raw, offsets = bytearray(), []
    for a in arrays:
        offsets.append(len(raw))
        raw += bytes(a)
    host = torch.frombuffer(raw, dtype=torch.uint8).pin_memory()
    return host, host.to(device, non_blocking=True), offsets
