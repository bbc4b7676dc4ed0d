"""The region clean-up rules T1-T8 written per pixel in plain Python: a stack flood fill over explicit 8-
and 4-neighbour lists.  Shares nothing with the stand-in (numpy + scipy) or the kernels."""
import numpy as np

N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
N4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]
INT32_MAX = 2 ** 31 - 1


def components(on, H, W, neighbours):
    """``on``: H lists of W bools -> (label per pixel, 0 off the set, [pixel list per component]); the components are in
    the raster order of their first pixel, which is the first entry of their list."""
    label = [[0] * W for _ in range(H)]
    comps = []
    for r in range(H):
        for c in range(W):
            if not on[r][c] or label[r][c]:
                continue
            k = len(comps) + 1
            label[r][c] = k
            stack, pixels = [(r, c)], []
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                for dy, dx in neighbours:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and on[yy][xx] and not label[yy][xx]:
                        label[yy][xx] = k
                        stack.append((yy, xx))
            comps.append(pixels)
    return label, comps


def tidy_mask(M, H, W, seeds, min_area, max_hole, keep):
    """T1-T6 on ``M`` (H lists of W bools) -> (M2 as H lists of W bools, the number of 8-connected components of M2, M1)."""
    assert keep in ("all", "seeded", "largest")
    max_hole = INT32_MAX if max_hole is None else max_hole
    seeds = [(r, c, bool(p)) for r, c, p in seeds if 0 <= r < H and 0 <= c < W]
    label, comps = components(M, H, W, N8)                                          # T1
    kept = set(label[r][c] for r, c, p in seeds if p and label[r][c])               # T2
    if keep == "all":                                                               # T3
        kept |= set(k + 1 for k, px in enumerate(comps) if len(px) >= min_area)
    elif keep == "largest" and comps:
        best = 0
        for k, px in enumerate(comps):      # (raster order of the first pixel: a later one must be strictly larger)
            if len(px) > len(comps[best]):
                best = k
        kept.add(best + 1)
    M1 = [[label[r][c] in kept for c in range(W)] for r in range(H)]                # T4
    back, holes = components([[not v for v in row] for row in M1], H, W, N4)        # T5
    blocked = set(back[r][c] for r, c, p in seeds if not p and back[r][c])
    M2 = [row[:] for row in M1]
    for k, px in enumerate(holes):
        if k + 1 in blocked or len(px) > max_hole:
            continue
        if any(r == 0 or r == H - 1 or c == 0 or c == W - 1 for r, c in px):
            continue
        for r, c in px:
            M2[r][c] = True                                                         # T6
    return M2, len(components(M2, H, W, N8)[1]), M1                                 # T8: the kept components as they stand in M2


def tidy_ref(add, total, H, W, seeds, min_area, max_hole, keep, thr):
    """-> dict(mask bool [H, W] (M2), kept bool [H, W] (M1), add_out, total_out (fp32 [H, W] or None), rec int32 [8], words uint64)."""
    thr = float(np.float32(thr))
    M = [[False] * W for _ in range(H)]
    for r in range(H):
        for c in range(W):
            t = 0.0 if total is None else float(total[r, c])
            a = 0.0 if add is None else float(add[r, c])
            M[r][c] = (t if t >= a else a) > thr
    M2, n_kept, M1 = tidy_mask(M, H, W, seeds, min_area, max_hole, keep)
    outs = [None if src is None else np.array(src, dtype=np.float32, copy=True) for src in (add, total)]
    words = [0] * ((H * W + 63) // 64)
    area = removed = added = 0
    box = [H, -1, W, -1]
    for r in range(H):
        for c in range(W):
            if M[r][c] and not M2[r][c]:                                            # T7
                removed += 1
                for out in outs:
                    if out is not None:
                        out[r, c] = np.float32(0.0)
            if M2[r][c] and not M[r][c]:
                added += 1
                for out in outs:
                    if out is not None:
                        out[r, c] = np.float32(1.0)
            if M2[r][c]:                                                            # T8
                i = r * W + c
                words[i >> 6] |= 1 << (i & 63)
                area += 1
                box = [min(box[0], r), max(box[1], r), min(box[2], c), max(box[3], c)]
    return dict(mask=np.array(M2, dtype=bool).reshape(H, W), kept=np.array(M1, dtype=bool).reshape(H, W), add_out=outs[0], total_out=outs[1],
                rec=np.array([area, removed, added] + box + [n_kept], dtype=np.int32), words=np.array(words, dtype=np.uint64))


def count_components(mask):
    """The number of 8-connected components of a bool [H, W] array."""
    H, W = mask.shape
    return len(components(mask.tolist(), H, W, N8)[1])
