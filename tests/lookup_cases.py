"""The inputs of the correlation-lookup edge tests (a helper of test_lookup_edges_cpu / _gpu, not a conftest): the maps, the
coordinate lists and the exactly representable data.  A list is a sequence of (x, y) float32 pairs dealt to the P source pixels
of a map in order (`launches` cuts a longer list into several launches); `outlier`, `interior` and `nonfinite` are whole fields
of exactly P pairs.  test_lookup_edges_cpu.py proves on the lists themselves every property the GPU test relies on: the coverage
of the edges and tile phases, the representability of the exact data, and -- through a host restatement of the kernels' index
arithmetic -- that no list makes either kernel address anything outside its level."""
import functools

import numpy as np

MAPS = [(8, 8), (9, 11), (17, 25)]      # one block with a 1x1 level 3; partial blocks, widths no multiple of 4; 3 x 4 blocks
RADII = (4, 3)
LEVELS = 4
FILL = (1.25, 1.5)                      # pads the last launch of a list: a plain in-map point


def level_dims(h, w, levels=LEVELS):
    """Per-level sizes h // 2^l with a minimum of 1."""
    return [(max(h >> l, 1), max(w >> l, 1)) for l in range(levels)]


def edge_floors(n, r):
    """The values floor(x / 2^l) must take on an axis of length n: around the first window that touches the map, the map's
    first and last pixels, and the last window that touches it."""
    return [-r - 2, -r - 1, -r, -r + 1, -1, 0, n - 2, n - 1, n, n + r - 1, n + r, n + r + 1]


def _axis_exact(n_full, r, l):
    """Multiples of 1/4 whose floor at level l takes every edge_floors value: with fraction 0, a small and a large one."""
    n, s = max(n_full >> l, 1), 2.0 ** l
    out = []
    for f in edge_floors(n, r):
        out += [s * f, s * f + 0.25, s * (f + 1) - 0.25]
    return out


@functools.lru_cache(maxsize=None)
def exact(h, w, r):
    """Every coordinate a multiple of 1/4 (fractions at level 3: multiples of 1/32).  Per axis and level every edge_floors value
    with a zero and a non-zero fraction, x and y paired edge with edge (corners) and edge with another edge; and per level the
    16 phases (wx0 mod 4, wy0 mod 4) of the window origin, with negative and with non-negative origins."""
    pts = []
    for l in range(LEVELS):
        xs, ys = _axis_exact(w, r, l), _axis_exact(h, r, l)
        n = len(xs)
        for k in range(n):
            pts.append((xs[k], ys[k]))
            pts.append((xs[k], ys[(7 * k + 5) % n]))
        s = 2.0 ** l
        for a in range(4):
            for b in range(4):
                pts.append((s * (a - 4) + 0.25, s * (b - 4) + 0.5))        # origins a - 4 - r, b - 4 - r: negative
                pts.append((s * (r + a), s * (r + b) + 0.75))              # origins a, b
    return np.array(pts, np.float32)


def _around(v):
    v = np.float32(v)
    with np.errstate(under="ignore"):                  # (the neighbours of 0 are subnormal: wanted)
        return [np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]


@functools.lru_cache(maxsize=None)
def band(h, w, r):
    """The integer edges of levels 0 and 3 moved by one float32 toward -inf and toward +inf (weights 2^-24-ish and 1 - 2^-24-ish,
    and the subnormals around 0), paired with the same edge on the other axis and with an in-map value, then 300 seeded uniform
    points over [-r - 3, w + r + 3) x [-r - 3, h + r + 3)."""
    rs = np.random.RandomState([h, w, r, 1])
    pts = []
    for l in (0, 3):
        s = 2.0 ** l
        ex = [v for f in edge_floors(max(w >> l, 1), r) for v in _around(s * f)]
        ey = [v for f in edge_floors(max(h >> l, 1), r) for v in _around(s * f)]
        for k in range(len(ex)):
            pts.append((ex[k], ey[k]))
            pts.append((ex[k], np.float32(rs.uniform(0, h - 1))))
            pts.append((np.float32(rs.uniform(0, w - 1)), ey[k]))
    rnd = np.stack([rs.uniform(-r - 3, w + r + 3, 300), rs.uniform(-r - 3, h + r + 3, 300)], 1)
    return np.concatenate([np.array(pts, np.float32), rnd.astype(np.float32)])


def far_values(r):
    """+-(1e6 +- 0.5), +-1.5e6, +-3e9, +-1e30 (the clamp of the window origin at +-1e6) and 2^l (+-16384 + r + d), d = -1, 0, 1
    (the clamp of the packed 16-bit drop-test operand: the window origin floor - r lands on +-16384 + d)."""
    v = []
    for sgn in (1.0, -1.0):
        v += [sgn * (1e6 - 0.5), sgn * (1e6 + 0.5), sgn * 1.5e6, sgn * 3e9, sgn * 1e30]
        for l in range(LEVELS):
            v += [2.0 ** l * (sgn * 16384 + r + d) for d in (-1, 0, 1)]
    return np.array(v, np.float32)


@functools.lru_cache(maxsize=None)
def far(h, w, r):
    """Every far value on x with an in-map y, on y with an in-map x, and on both axes: each row is all zeros."""
    v = far_values(r)
    rs = np.random.RandomState([h, w, r, 2])
    pts = []
    for k, a in enumerate(v):
        pts += [(a, np.float32(rs.uniform(0, h - 1))), (np.float32(rs.uniform(0, w - 1)), a), (a, v[(5 * k + 3) % len(v)])]
    return np.array(pts, np.float32)


def smooth(h, w):
    """The identity plus 0.25 on both axes (multiples of 1/4: exact), as (P, 2)."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.reshape(-1) + 0.25, ys.reshape(-1) + 0.25], 1).astype(np.float32)


def block_pixel(h, w, by, bx, last):
    """The first (last) pixel of the 8x8 block (by, bx) that lies in the map, as a pixel index."""
    y0, x0 = 8 * by, 8 * bx
    y, x = (min(y0 + 7, h - 1), min(x0 + 7, w - 1)) if last else (y0, x0)
    return y * w + x


def blocks(h, w):
    return [(by, bx) for by in range((h + 7) // 8) for bx in range((w + 7) // 8)]


def _one_per_block(h, w, values, variant):
    """smooth(h, w) with one pixel per 8x8 block replaced: variant 0 puts the block's k-th value on x of its first pixel,
    variant 1 the NEGATED value on y of its last pixel.  -> (coords (P, 2), indices of the replaced pixels)."""
    c, idx = smooth(h, w), []
    for k, (by, bx) in enumerate(blocks(h, w)):
        i = block_pixel(h, w, by, bx, last=variant == 1)
        v = values[k % len(values)]
        c[i, variant] = -v if variant == 1 else v
        idx.append(i)
    return c, np.array(idx)


def outlier(h, w, r, variant):
    """A smooth field in which exactly one pixel per block carries a far value: every level's bounding box of the block is
    clipped on the side of the far value and whole on the other (for the blocks inside the map)."""
    return _one_per_block(h, w, far_values(r)[2::3], variant)


NONFINITE = np.array([np.nan, np.inf, -np.inf], np.float32)
NONFINITE_STANDIN = np.float32(3e9)


def nonfinite(h, w, variant, standin=False):
    """One pixel per block holds NaN, +Inf or -Inf (variant 0: on x of the block's first pixel, variant 1: negated on y of its
    last); standin=True puts 3e9 in the same places (with the same signs rule)."""
    vals = np.full(3, NONFINITE_STANDIN, np.float32) if standin else NONFINITE
    return _one_per_block(h, w, vals, variant)


INTERIOR_MAP = (17, 25)
INTERIOR_BLOCK = (1, 1)


def interior(r):
    """(17, 25) only: the pixels of the middle block (1, 1) look where every window of theirs lies inside level 0 (floor(x) in
    [r, W - r - 2], floor(y) in [r, H - r - 2]): that block's level-0 box is not clipped, so its windows are not cleared and
    every cell of them must be written.  All other pixels: smooth."""
    h, w = INTERIOR_MAP
    c = smooth(h, w)
    for y in range(8, 16):
        for x in range(8, 16):
            c[y * w + x] = (r + (x - 8) * 1.5 + 0.3125, r + (y - 8) * 0.5 + 0.4375)
    assert c[:, 0].max() < w and r + 7 * 1.5 + 0.3125 < w - r - 1 and r + 7 * 0.5 + 0.4375 < h - r - 1
    return c


def half(h, w, r):
    """Coordinates whose fractions are 0 or 1/2 at EVERY level: multiples of 4, from beyond the first window of level 3 to beyond
    its last."""
    xs = np.arange(-8 * (r + 2), 8 * (max(w >> 3, 1) + r + 2) + 1, 4.0)
    ys = np.arange(-8 * (r + 2), 8 * (max(h >> 3, 1) + r + 2) + 1, 4.0)
    pts = [(xs[k % len(xs)], ys[(5 * k + j) % len(ys)]) for j in range(3) for k in range(max(len(xs), len(ys)))]
    return np.array(pts, np.float32)


def launches(pts, P):
    """A list cut into launches of exactly P pairs, the last one padded with FILL: [(coords (P, 2) float32, n_used)]."""
    pts = np.asarray(pts, np.float32)
    out = []
    for s in range(0, len(pts), P):
        c = np.tile(np.array(FILL, np.float32), (P, 1))
        n = min(P, len(pts) - s)
        c[:n] = pts[s:s + n]
        out.append((c, n))
    return out


# ---- exactly representable data -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume_planes(h, w, seed=0):
    """Per level an independent (P, H_l, W_l) plane set of seeded integers in [-256, 256]: exact in fp32 AND in bf16 (an
    integer below 256 has at most 8 significant bits and 256 is a power of two), so the same planes serve the bf16-storage
    volume.  Returned as float32 arrays, read-only."""
    rs = np.random.RandomState([seed, h, w, 3])
    out = [rs.randint(-256, 257, (h * w, a, b)).astype(np.float32) for a, b in level_dims(h, w)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact_features(h, w, k=256, seed=0):
    """(f1 (P, k), [f2_l (H_l W_l, k)]) of integers in [-2, 2], every level's f2 independent: with alpha = 1 / sqrt(256) = 1/16
    the correlations are multiples of 1/16 of magnitude <= 64."""
    rs = np.random.RandomState([seed, h, w, k, 4])
    f1 = rs.randint(-2, 3, (h * w, k)).astype(np.float32)
    f2 = [rs.randint(-2, 3, (a * b, k)).astype(np.float32) for a, b in level_dims(h, w)]
    return f1, f2


@functools.lru_cache(maxsize=None)
def cross_features(h, w, variant, k=256, seed=0):
    """The operands that exercise the cross terms of the split-bf16 product (terms = 3: a_lo b_hi + a_hi b_lo + a_hi b_hi).
    Variant 0: f2 in multiples of 2^-8 within [-2, 2) (a non-zero low plane) and f1 integer (a zero low plane); variant 1: the
    roles swapped.  Never both: the product of the two low planes is the term the arithmetic drops."""
    rs = np.random.RandomState([seed, h, w, k, 5 + variant])
    fine = lambda n: (rs.randint(-512, 512, (n, k)) / 256.0).astype(np.float32)         # noqa: E731
    coarse = lambda n: rs.randint(-2, 3, (n, k)).astype(np.float32)                     # noqa: E731
    a, b = (coarse, fine) if variant == 0 else (fine, coarse)
    return a(h * w), [b(x * y) for x, y in level_dims(h, w)]


def corr_planes64(f1, f2, h, w, k=256):
    """alpha f1 f2_l^T in float64 as planes (P, H_l, W_l)."""
    a = np.asarray(f1, np.float64)
    return [(a @ np.asarray(b, np.float64).T / np.sqrt(float(k))).reshape(len(a), x, y) for b, (x, y) in zip(f2, level_dims(h, w))]


# ---- convex upsampling ----------------------------------------------------------------------------------------------------------
def convex_case(hf, wf, ld_mask=576, seed=0):
    """(coords (P, 2), wlow (P,), mask (P, ld_mask)) float32: seeded flow of +-4 pixels, logits of +-2 -- and, in the cell in
    the middle, logits of +-80 (the softmax collapses onto one tap; nothing may overflow)."""
    rs = np.random.RandomState([seed, hf, wf])
    P = hf * wf
    ys, xs = np.mgrid[0:hf, 0:wf]
    coords = (np.stack([xs.reshape(-1), ys.reshape(-1)], 1) + rs.uniform(-4, 4, (P, 2))).astype(np.float32)
    wlow = rs.uniform(-3, 3, P).astype(np.float32)
    mask = rs.uniform(-2, 2, (P, ld_mask)).astype(np.float32)
    mask[P // 2, :576] = rs.choice([-80.0, 80.0], 576).astype(np.float32)
    mask[P // 2, :64] = 80.0                                                # (every fine position has one tap at +80 at least)
    return coords, wlow, mask


CONVEX_SHAPES = [(1, 5), (4, 1), (3, 4)]


def convex_values(coords, wlow, hf, wf):
    """The three channels the kernel interpolates, as it forms them in fp32: flow x, flow y (coords minus the grid) and wlow;
    (unscaled float32 (3, P), 8 v float32 (3, P))."""
    ys, xs = np.mgrid[0:hf, 0:wf]
    v = np.stack([coords[:, 0] - xs.reshape(-1).astype(np.float32), coords[:, 1] - ys.reshape(-1).astype(np.float32), wlow])
    assert v.dtype == np.float32
    return v, np.float32(8) * v
