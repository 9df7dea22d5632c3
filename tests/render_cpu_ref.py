"""numpy restatement of fdet_render_boxes (include/fdet.h), rule by rule, for byte-for-byte comparison.

    render(images, rows, counts, outline, pixelate, blocks, color) -> list of new (H,W,3) uint8 arrays

The outline is written as the pixel predicate of rule 4, not as the four bands the kernel paints, and the pixelation
walks cells by array slices in one sequential pass with an ownership mask: two formulations of each rule."""
import numpy as np

LIM = np.float32(16777216.0)


def box_rect(row):
    """Rule 2.  row: [score,x,y,w,h].  -> (x0, y0, x1, y1, w, h) with fp32 w, h, or None when the box is skipped."""
    x, y, w, h = (np.float32(v) for v in row[1:5])
    with np.errstate(all="ignore"):
        xe, ye = np.float32(x + w), np.float32(y + h)
    if not all(np.isfinite(v) for v in (x, y, w, h)):
        return None
    if w < 1 or h < 1:
        return None
    if any(abs(v) > LIM for v in (x, y, xe, ye)):
        return None
    x0, y0, x1, y1 = int(np.trunc(x)), int(np.trunc(y)), int(np.trunc(xe)), int(np.trunc(ye))
    if x1 == x0 or y1 == y0:            # zero width or height in pixels: a start in (-1, 0) and an end in [0, 1)
        return None
    return x0, y0, x1, y1, w, h


def thickness(w, h):
    return 1 if (w <= 15 or h <= 15) else 3


def _grid(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return xx, yy


def pixelate(src, rects, blocks):
    """Rule 3 on one image.  rects: the valid boxes in row order.  Works on the part of each box inside the image."""
    H, W = src.shape[:2]
    out = src.copy()
    owned = np.zeros((H, W), bool)
    for (x0, y0, x1, y1, _, _) in rects:
        vx0, vy0, vx1, vy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if vx0 > vx1 or vy0 > vy1:
            continue
        cell = max(1, -(-max(x1 - x0 + 1, y1 - y0 + 1) // int(blocks)))
        for j in range((vy0 - y0) // cell, (vy1 - y0) // cell + 1):
            ya, yb = max(y0 + j * cell, vy0), min(y0 + (j + 1) * cell - 1, vy1)
            for i in range((vx0 - x0) // cell, (vx1 - x0) // cell + 1):
                xa, xb = max(x0 + i * cell, vx0), min(x0 + (i + 1) * cell - 1, vx1)
                block = src[ya:yb + 1, xa:xb + 1].reshape(-1, 3).astype(np.int64)
                cnt = block.shape[0]
                mean = ((block.sum(0) + cnt // 2) // cnt).astype(np.uint8)
                free = ~owned[ya:yb + 1, xa:xb + 1]
                out[ya:yb + 1, xa:xb + 1][free] = mean
        owned[vy0:vy1 + 1, vx0:vx1 + 1] = True
    return out


def outline_mask(H, W, rects):
    """Rule 4: the pixels that take the colour."""
    xx, yy = _grid(H, W)
    mask = np.zeros((H, W), bool)
    for (x0, y0, x1, y1, w, h) in rects:
        t = thickness(w, h)
        outer = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
        inner = (xx >= x0 + t) & (xx <= x1 - t) & (yy >= y0 + t) & (yy <= y1 - t)
        mask |= outer & ~inner
    return mask


def render_one(src, rows, count, outline=True, pixelate_=False, blocks=8, color=(0, 0, 255)):
    src = np.asarray(src)
    rects = [r for r in (box_rect(rows[k]) for k in range(int(count))) if r is not None]
    out = pixelate(src, rects, blocks) if pixelate_ else src.copy()
    if outline:
        out[outline_mask(src.shape[0], src.shape[1], rects)] = np.asarray(color, np.uint8)
    return out


def render(images, rows, counts, outline=True, pixelate_=False, blocks=8, color=(0, 0, 255)):
    rows = np.asarray(rows, np.float32)
    return [render_one(im, rows[i], counts[i], outline, pixelate_, blocks, color) for i, im in enumerate(images)]
