"""The visibility weight map of the photometric refinement (woft_photo_weights) restated in plain numpy, step
by step as include/woft_hip.h states it, with a dtype switch for the soft weight: float32 is the arithmetic the kernel is asked to
do, float64 the reference its values are compared with, and the distance between the two is the yardstick.  Also the seeded cases
of tests/test_photo_weights_cpu.py and tests/test_photo_weights_gpu.py: planted fold planes, overlapping target masks and the
occluded refinement cases."""
import numpy as np

MAX_RADIUS = 4
MODES = ("gate", "soft")
NAN, INF = float("nan"), float("inf")


def raw_map(cost, vis, template_hw, rect, vis_thr, mode, dtype=np.float32):
    """raw(x, y) on the template: 0 outside rect = (ry, rx, rows, cols); inside it 0 unless the cost is finite and vis >= vis_thr
    (in fp32, as the planes are: a NaN vis fails, equality passes); where that holds 1 ('gate') or exp(-cost) * vis computed in
    `dtype` ('soft'), a product that is not finite or not > 0 becoming 0."""
    assert mode in MODES
    h, w = template_hw
    ry, rx, rows, cols = rect
    c = np.asarray(cost, np.float32).reshape(rows, cols)
    v = np.asarray(vis, np.float32).reshape(rows, cols)
    with np.errstate(all="ignore"):
        passed = np.isfinite(c) & (v >= np.float32(vis_thr))
        if mode == "gate":
            val = np.ones((rows, cols), dtype)
        else:
            val = np.exp(-c.astype(dtype)) * v.astype(dtype)
            val = np.where(np.isfinite(val) & (val > 0), val, dtype(0))
    raw = np.zeros((h, w), dtype)
    raw[ry:ry + rows, rx:rx + cols] = np.where(passed, val, dtype(0))
    return raw


def erode(raw, radius):
    """The minimum over |dx|, |dy| <= radius, neighbours outside the array ignored."""
    assert 0 <= radius <= MAX_RADIUS
    h, w = raw.shape
    pad = np.pad(raw, radius, constant_values=np.inf) if radius else raw
    out = np.full((h, w), np.inf, raw.dtype)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out = np.minimum(out, pad[dy:dy + h, dx:dx + w])
    return out


def support_counts(wmap, bits, n_targets):
    """support[t] = the template pixels with bit t of the uint32 plane set and map > 0."""
    bits = np.asarray(bits).view(np.uint32)
    return np.array([np.count_nonzero(((bits >> np.uint32(t)) & np.uint32(1)).astype(bool) & (wmap > 0)) for t in range(n_targets)],
                    np.int32)


def weight_map(cost, vis, template_hw, rect=None, bits=None, n_targets=0, vis_thr=0.5, mode="gate", radius=1, dtype=np.float32):
    """-> (map (h, w) in `dtype`, support (n_targets,) int32 | None): woft_photo_weights as stated."""
    if rect is None:
        rect = (0, 0) + tuple(np.asarray(cost).shape[-2:])
    wmap = erode(raw_map(cost, vis, template_hw, rect, vis_thr, mode, dtype), radius)
    return wmap, (support_counts(wmap, bits, n_targets) if n_targets else None)


def brute_force(cost, vis, template_hw, rect, bits, n_targets, vis_thr, mode, radius):
    """The same map and counts pixel by pixel, neighbour by neighbour, in float32 (slow: small sizes only)."""
    h, w = template_hw
    ry, rx, rows, cols = rect
    c = np.asarray(cost, np.float32).reshape(rows, cols)
    v = np.asarray(vis, np.float32).reshape(rows, cols)

    def raw(x, y):
        yy, xx = y - ry, x - rx
        if not (0 <= yy < rows and 0 <= xx < cols):
            return np.float32(0)
        if not (np.isfinite(c[yy, xx]) and v[yy, xx] >= np.float32(vis_thr)):
            return np.float32(0)
        if mode == "gate":
            return np.float32(1)
        with np.errstate(all="ignore"):
            r = np.float32(np.exp(np.float32(-c[yy, xx])) * v[yy, xx])
        return r if np.isfinite(r) and r > 0 else np.float32(0)
    wmap = np.zeros((h, w), np.float32)
    counts = np.zeros(n_targets, np.int32)
    for y in range(h):
        for x in range(w):
            m = min(raw(x + dx, y + dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
                    if 0 <= x + dx < w and 0 <= y + dy < h)
            wmap[y, x] = m
            for t in range(n_targets):
                if m > 0 and (int(bits[y, x]) >> t) & 1:
                    counts[t] += 1
    return wmap, counts


# ---- the kernel's cases -------------------------------------------------------------------------------------------------------------
TEMPLATE_HW = (40, 72)
RECTS = {"whole": (0, 0, 40, 72), "inner": (5, 9, 24, 40)}
VIS_THR = 0.5
TILE_W, TILE_H = 64, 16          # the kernel's tile (csrc/photo_weights.hip): pixel (64, *) and (*, 16) are the first past a boundary


def planted_planes(rect, seed=0):
    """(cost, vis) fp32 of the rectangle's size: costs in [0, 3), vis in [0.5, 1) -- most pixels pass -- with planted +inf and NaN
    costs, NaN vis, a vis exactly at the threshold, one just below it, and failing pixels (vis 0) at the positions the erosion's
    rules are about: a template corner and edge (where the rectangle reaches them), the first pixel past a tile boundary in x and
    in y, and the rectangle's own border."""
    ry, rx, rows, cols = rect
    rng = np.random.default_rng(100 + seed)
    cost = rng.uniform(0.0, 3.0, (rows, cols)).astype(np.float32)
    vis = rng.uniform(0.5, 1.0, (rows, cols)).astype(np.float32)
    at = rng.choice(rows * cols, 12, replace=False)
    cost.reshape(-1)[at[0]], cost.reshape(-1)[at[1]] = INF, NAN
    cost.reshape(-1)[at[2]] = -INF
    vis.reshape(-1)[at[3]] = NAN
    vis.reshape(-1)[at[4]] = np.float32(VIS_THR)
    vis.reshape(-1)[at[5]] = np.nextafter(np.float32(VIS_THR), np.float32(0))
    vis.reshape(-1)[at[6:]] = 0.2
    zeros = [(0, 0), (rows - 1, cols - 1), (0, cols // 2), (rows // 2, 0), (rows - 1, 7), (3, cols - 1)]       # corners, borders
    for ty, tx in ((TILE_H, 20), (20, TILE_W), (TILE_H, TILE_W), (2 * TILE_H, 30), (TILE_H - 1, TILE_W - 1)):   # (template coordinates)
        if ry <= ty < ry + rows and rx <= tx < rx + cols:
            zeros.append((ty - ry, tx - rx))
    for y, x in zeros:
        vis[y, x] = 0.0
    return cost, vis


def target_masks(K, seed=0):
    """K overlapping boolean masks on the template; with K = 32 target 31 (the top bit) covers most of the template."""
    h, w = TEMPLATE_HW
    rng = np.random.default_rng(200 + seed)
    masks = []
    for t in range(K):
        m = np.zeros((h, w), bool)
        y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
        m[y0:y0 + int(rng.integers(4, h // 2 + 1)), x0:x0 + int(rng.integers(4, w // 2 + 1))] = True
        masks.append(m)
    masks[0][8:30, 10:70] = True                                 # (overlaps most of the others, crosses the tile boundaries)
    if K == 32:
        masks[31][:] = False
        masks[31][1:, 2:] = True
    return masks


def pack_bits(masks):
    """pack_target_bits' layout without the package: bit t of a pixel set where masks[t] is."""
    bits = np.zeros(masks[0].shape, np.uint32)
    for t, m in enumerate(masks):
        bits |= (np.asarray(m) != 0).astype(np.uint32) << np.uint32(t)
    return bits


# ---- the occluded refinement --------------------------------------------------------------------------------------------------------
OCCLUDER_HW, OCCLUDER_OFFSET, OCCLUDER_CELL = (30, 22), (5, 4), 3


def occlusion_case(seed):
    """photo_host.base_case(seed) with an occluder over part of the target -> (template, mask, frame, H_gt, W0, vis): a block 22
    pixels wide and 30 high of random texture in 3 x 3-pixel cells pasted into the frame with its top-left corner at (smallest corner x
    + 5, smallest corner y + 4) of the box projected by H_gt, and vis (h, w) float32 = the truth on the template: 0 where any of the
    four bilinear taps of the pixel under H_gt is a pasted pixel, 1 elsewhere."""
    import photo_host as ph
    template, mask, frame, H_gt, W0 = ph.base_case(seed)
    frame = frame.copy()
    c = ph.project(H_gt, ph.box_corners(ph.BOX))
    x0, y0 = int(np.floor(c[:, 0].min())) + OCCLUDER_OFFSET[0], int(np.floor(c[:, 1].min())) + OCCLUDER_OFFSET[1]
    oh, ow = OCCLUDER_HW
    rs = np.random.RandomState(1000 + seed)
    cells = rs.randint(0, 256, (-(-oh // OCCLUDER_CELL), -(-ow // OCCLUDER_CELL), 3)).astype(np.uint8)
    block = np.repeat(np.repeat(cells, OCCLUDER_CELL, 0), OCCLUDER_CELL, 1)[:oh, :ow]
    frame[y0:y0 + oh, x0:x0 + ow] = block
    pasted = np.zeros(frame.shape[:2], bool)
    pasted[y0:y0 + oh, x0:x0 + ow] = True
    h, w = mask.shape
    ys, xs = np.mgrid[:h, :w]
    q = ph.project(H_gt, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64))
    u, v = q[:, 0].reshape(h, w), q[:, 1].reshape(h, w)
    fu, fv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    hf, wf = pasted.shape
    hit = np.zeros((h, w), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = fv + dy, fu + dx
            inside = (yy >= 0) & (yy < hf) & (xx >= 0) & (xx < wf)
            hit |= inside & pasted[np.clip(yy, 0, hf - 1), np.clip(xx, 0, wf - 1)]
    return template, mask, frame, H_gt, W0, (~hit).astype(np.float32)


def corner_error(H, H_gt):
    import photo_host as ph
    return ph.corner_distance(ph.BOX, H, H_gt)
