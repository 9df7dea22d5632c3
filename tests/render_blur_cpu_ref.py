"""numpy restatement of fdet_render_boxes_blur's step 3b (include/fdet.h) and of the host arithmetic of
`render.blur_table`, for byte-for-byte comparison.

    box_radius(radius), box_params(fr)            PIL's BoxBlur.c arithmetic, scalar by scalar (the table is vectorised)
    table(blocks, radius, n)                      the (n,3) int32 table entry by entry
    validate(tab)                                 the bound the entry point checks on the host
    one_pass(a, r, ww, fw)                        rule 3b.3 along the last axis, written as padded slices
    gaussian(region, r, ww, fw)                   rule 3b.4: three passes along rows, three along columns
    render(images, rows, counts, tab, outline)    the whole entry with blur = 1

The kernel computes a pass from prefix sums with counted edge replication; here the line is padded by replication and
the taps are summed as shifted slices: two formulations of one rule.  A box whose S reaches past the table takes the
table's LAST entry (index min(S, n-1)): beyond n the radius stops growing."""
import math

import numpy as np

import render_cpu_ref as R

f32 = np.float32


def box_radius(radius):
    """BoxBlur.c _gaussian_blur_radius with passes = 3, in float32 as C evaluates it."""
    radius = f32(radius)
    s2 = f32(radius * radius / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))                 # double sqrt, stored as float
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(2 * l + 1) * f32(f32(l * f32(l + 1)) - f32(3 * s2)))
    a = f32(a / f32(6 * f32(s2 - f32((l + 1) * (l + 1)))))
    return f32(l + a)


def box_params(fr):
    """ImagingHorizontalBoxBlur: the integer radius and the two fixed-point weights."""
    fr = f32(fr)
    r = int(fr)
    ww = int(f32(1 << 24) / f32(f32(fr * 2) + 1))              # a FLOAT32 division, then truncation
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def table(blocks=8, radius=None, n=64):
    out = np.zeros((n, 3), np.int32)
    for S in range(n):
        rad = f32(S) / f32(blocks) if radius is None else f32(radius)
        out[S] = box_params(box_radius(rad))
    return out


def validate(tab):
    tab = np.asarray(tab).astype(np.int64).reshape(-1, 3)
    return bool(len(tab) >= 1 and (tab >= 0).all() and ((2 * tab[:, 0] + 1) * tab[:, 1] + 2 * tab[:, 2] <= 1 << 24).all())


def one_pass(a, r, ww, fw):
    """a (..., n) uint8 -> the same shape, rule 3b.3 along the last axis."""
    n = a.shape[-1]
    r, ww, fw = int(r), int(ww), int(fw)
    reach = min(r, n) + 1                                       # every tap further out is the edge value as well
    pad = np.pad(a.astype(np.int64), [(0, 0)] * (a.ndim - 1) + [(reach, reach)], mode="edge")
    acc = np.zeros(a.shape, np.int64)
    inner = min(r, n)
    for d in range(-inner, inner + 1):
        acc += pad[..., reach + d:reach + d + n]
    # the taps between `inner` and r on either side all clamp: (r - inner) times the edge value each
    acc += (r - inner) * (pad[..., :1] + pad[..., -1:])
    far = pad[..., reach - inner - 1:reach - inner - 1 + n] + pad[..., reach + inner + 1:reach + inner + 1 + n]
    out = (ww * acc + fw * far + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def gaussian(region, r, ww, fw):
    """region (h,w,3) uint8 -> rule 3b.4."""
    a = np.ascontiguousarray(np.moveaxis(region, 1, -1))         # (h,3,w): lines along x
    for _ in range(3):
        a = one_pass(a, r, ww, fw)
    a = np.ascontiguousarray(np.moveaxis(a, 0, -1))              # (3,w,h): lines along y
    for _ in range(3):
        a = one_pass(a, r, ww, fw)
    return np.ascontiguousarray(a.transpose(2, 1, 0))            # (h,w,3)


def entry(tab, S):
    return tab[min(int(S), len(tab) - 1)]


def blur(src, rects, tab):
    """Rule 3b on one image.  rects: the valid boxes in row order."""
    H, W = src.shape[:2]
    out = src.copy()
    owned = np.zeros((H, W), bool)
    for (x0, y0, x1, y1, _, _) in rects:
        vx0, vy0, vx1, vy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if vx0 > vx1 or vy0 > vy1:
            continue
        r, ww, fw = entry(tab, max(x1 - x0 + 1, y1 - y0 + 1))
        B = gaussian(src[vy0:vy1 + 1, vx0:vx1 + 1], r, ww, fw)
        free = ~owned[vy0:vy1 + 1, vx0:vx1 + 1]
        out[vy0:vy1 + 1, vx0:vx1 + 1][free] = B[free]
        owned[vy0:vy1 + 1, vx0:vx1 + 1] = True
    return out


def render_one(src, rows, count, tab, outline=False, color=(0, 0, 255)):
    src = np.asarray(src)
    rects = [r for r in (R.box_rect(rows[k]) for k in range(int(count))) if r is not None]
    out = blur(src, rects, np.asarray(tab))
    if outline:
        out[R.outline_mask(src.shape[0], src.shape[1], rects)] = np.asarray(color, np.uint8)
    return out


def render(images, rows, counts, tab, outline=False, color=(0, 0, 255)):
    rows = np.asarray(rows, np.float32)
    return [render_one(im, rows[i], counts[i], tab, outline, color) for i, im in enumerate(images)]
