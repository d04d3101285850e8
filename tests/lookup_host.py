"""Host restatements of the lookup kernels (a helper of test_lookup_edges_cpu, not a conftest): the fp32 arithmetic of the
bilinear sample, of the flow-head gather and of the convex upsampling in numpy float32, operation by operation in the kernels'
order (the library is built without contraction to FMA, so numpy's float32 rounds where the kernels round), and the integer
arithmetic by which woft_corr_lookup and woft_corr_lookup_otf turn a coordinate into tile indices, bounding boxes, stream rows
and window cells.  The index restatement ASSERTS, for the coordinates it is given, that everything the kernels would dereference
lies inside its level -- the condition under which wild and non-finite coordinates may be handed to a GPU at all."""
import numpy as np

CLAMP = np.float32(1.0e6)


def window_origin(c, l, r):
    """floorf, the weights, the clamp to +-1e6 (fmaxf / fminf return the other operand for a NaN: np.fmax / np.fmin) and the
    int conversion, for one axis: c float32 (n,) -> (origin int64, weight float32).  The conversion is asserted defined."""
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        xs = np.asarray(c, np.float32) * np.float32(1.0 / (1 << l))
        fl = np.floor(xs)
        fw = xs - fl                                   # (NaN for a non-finite coordinate: that pixel's own row only)
        fl = np.fmin(np.fmax(fl, -CLAMP), CLAMP)
    assert fl.dtype == np.float32 and np.isfinite(fl).all() and (np.abs(fl) <= 1.0e6).all()
    return fl.astype(np.int64) - r, fw


def lookup32(planes, coords, radius):
    """The sample of corr_lookup_kernel / corr_lookup_otf_kernel in float32: top = q00 (1 - fx) + q01 fx, bot likewise, v = top
    (1 - fy) + bot fy, taps outside the map 0.  planes[l] (P, H_l, W_l), coords (P, 2) -> (P, L (2r+1)^2) float32."""
    c = np.asarray(coords, np.float32)
    P, n, one = len(c), 2 * radius + 1, np.float32(1.0)
    out = []
    for l, pl in enumerate(planes):
        pl = np.asarray(pl, np.float32)
        H, W = pl.shape[1:]
        wx0, fx = window_origin(c[:, 0], l, radius)
        wy0, fy = window_origin(c[:, 1], l, radius)
        xs, ys = wx0[:, None] + np.arange(n + 1)[None], wy0[:, None] + np.arange(n + 1)[None]
        ok = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]
        patch = np.where(ok, pl[np.arange(P)[:, None, None], np.clip(ys, 0, H - 1)[:, :, None],
                                np.clip(xs, 0, W - 1)[:, None, :]], np.float32(0))
        fx, fy = fx[:, None, None], fy[:, None, None]
        with np.errstate(invalid="ignore", under="ignore"):
            top = patch[:, :n, :n] * (one - fx) + patch[:, :n, 1:] * fx
            bot = patch[:, 1:, :n] * (one - fx) + patch[:, 1:, 1:] * fx
            v = top * (one - fy) + bot * fy
        assert v.dtype == np.float32
        out.append(v.transpose(0, 2, 1).reshape(P, n * n))
    return np.concatenate(out, 1)


def gather32(part, n_planes, hf, wf, bias=None):
    """flow_head_gather_kernel / the folded gather of corr_lookup_otf_kernel in float32 and in their order: per tap the planes
    are summed first (plane 0 + plane 1 + ...), then the taps are added to the bias, ky outer, kx inner; a tap outside the grid
    adds 0.  -> (P, 2) float32."""
    P = hf * wf
    pt = np.asarray(part, np.float32)[:n_planes * P, :18].reshape(n_planes, hf, wf, 9, 2)
    pad = np.zeros((n_planes, hf + 2, wf + 2, 9, 2), np.float32)
    pad[:, 1:-1, 1:-1] = pt
    d = np.zeros((hf, wf, 2), np.float32) + (np.zeros(2, np.float32) if bias is None else np.asarray(bias, np.float32)[:2])
    for ky in range(3):
        for kx in range(3):
            t = pad[:, ky:ky + hf, kx:kx + wf, 3 * ky + kx]
            v = t[0].copy()
            for p in range(1, n_planes):
                v = v + t[p]
            d = d + v
    assert d.dtype == np.float32
    return d.reshape(P, 2)


def convex32(values8, mask, hf, wf):
    """convex_upsample_kernel's softmax and weighted sum in float32 and in its order, for channels whose neighbour values 8 v
    are given (already rounded as the kernel rounds them): values8 (C, hf wf) float32, mask (hf wf, >= 576) -> (C, 8 hf, 8 wf)."""
    v8 = np.asarray(values8, np.float32)
    C = v8.shape[0]
    m = np.asarray(mask, np.float32)[:, :576].reshape(hf, wf, 9, 8, 8)
    mx = m.max(2, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(m - mx)
        assert e.dtype == np.float32
        den = np.zeros((hf, wf, 8, 8), np.float32)
        for k in range(9):
            den = den + e[:, :, k]
        pad = np.zeros((C, hf + 2, wf + 2), np.float32)
        pad[:, 1:-1, 1:-1] = v8.reshape(C, hf, wf)
        acc = np.zeros((C, hf, wf, 8, 8), np.float32)
        for k in range(9):
            s = e[:, :, k] / den
            acc = acc + s[None] * pad[:, k // 3:k // 3 + hf, k % 3:k % 3 + wf][..., None, None]
    assert acc.dtype == np.float32
    return acc.transpose(0, 1, 3, 2, 4).reshape(C, 8 * hf, 8 * wf)


# ---- index arithmetic -----------------------------------------------------------------------------------------------------------
def check_volume_indices(coords, dims, r):
    """corr_lookup_kernel (4 x 4 tiles, a 16 x 16 patch per level): for every pixel and level the tiles it loads lie inside the
    tiled plane, every window cell inside the map lies in a loaded tile, and every LDS read of a sample stays inside the patch.
    Returns the number of tile loads checked."""
    c = np.asarray(coords, np.float32)
    PW, n_loads = 16, 0
    for l, (H, W) in enumerate(dims):
        ht, wt = (H + 3) // 4, (W + 3) // 4
        wx0, _ = window_origin(c[:, 0], l, r)
        wy0, _ = window_origin(c[:, 1], l, r)
        px, py = wx0 & 3, wy0 & 3                                           # the origin inside the patch
        assert (py * PW + px + (2 * r + 1) * PW + 2 * r + 1 < 16 * PW).all()               # the farthest LDS read of a sample
        assert (px + 2 * r + 1 < PW).all() and (py + 2 * r + 1 < 16).all()
        a = np.arange(4)
        tx, ty = (wx0 >> 2)[:, None] + a[None], (wy0 >> 2)[:, None] + a[None]             # arithmetic shifts: floor divisions
        assert np.array_equal(wx0 >> 2, np.floor_divide(wx0, 4)) and np.array_equal(wx0 & 3, np.mod(wx0, 4))
        lx = (tx >= 0) & (tx < wt) & (4 * a[None] < px[:, None] + 2 * r + 2)
        ly = (ty >= 0) & (ty < ht) & (4 * a[None] < py[:, None] + 2 * r + 2)
        load = ly[:, :, None] & lx[:, None, :]
        tile = ty[:, :, None] * wt + tx[:, None, :]
        assert ((tile[load] >= 0) & (tile[load] < ht * wt)).all()                          # ... times 16 elements: inside the plane
        n_loads += int(load.sum())
        k = np.arange(2 * r + 2)
        for w0, p0, lim, ok, t in ((wx0, px, W, lx, tx), (wy0, py, H, ly, ty)):            # window cells inside the map are loaded
            cell, b = w0[:, None] + k[None], (p0[:, None] + k[None]) >> 2                  # ... b: where the patch holds the cell
            inmap = (cell >= 0) & (cell < lim)
            assert np.take_along_axis(ok, b, 1)[inmap].all()
            assert np.array_equal(np.take_along_axis(t, b, 1)[inmap], np.floor_divide(cell, 4)[inmap])   # ... from the cell's own tile
    return n_loads


def check_otf_indices(coords, hf, wf, dims, r):
    """corr_lookup_otf_kernel: per 8x8 block and level the bounding box of the window origins, its clip at the map, the stream
    rows of its positions, the packed 16-bit drop test and the window cell a dropped value lands in.  Asserts that every stream
    row lies inside the level, that the 16-bit test admits exactly the positions inside a pixel's window, that an admitted
    value lands inside that pixel's window array, and that the windows of an UNCLIPPED box are written in every cell (they
    are not cleared) while a clipped box leaves exactly the cells outside the map unwritten (they are cleared).
    Returns {(block y, block x, level): clipped}."""
    c = np.asarray(coords, np.float32).reshape(hf, wf, 2)
    NW, WS = 2 * r + 1, 2 * r + 2
    clipped_of = {}
    for by_ in range((hf + 7) // 8):
        for bx_ in range((wf + 7) // 8):
            blk = c[8 * by_:8 * by_ + 8, 8 * bx_:8 * bx_ + 8].reshape(-1, 2)               # the block's pixels inside the grid
            for l, (H, W) in enumerate(dims):
                assert 0 < H <= 16384 and 0 < W <= 16384
                wx0, _ = window_origin(blk[:, 0], l, r)
                wy0, _ = window_origin(blk[:, 1], l, r)
                ox, oy = np.clip(wx0, -16384, 16384), np.clip(wy0, -16384, 16384)
                b0, b1, b2, b3 = wx0.min(), wx0.max(), wy0.min(), wy0.max()
                clipped = bool(b0 < 0 or b2 < 0 or b1 + NW > W - 1 or b3 + NW > H - 1)
                clipped_of[(by_, bx_, l)] = clipped
                bx0, by0 = max(b0, 0), max(b2, 0)
                bx1, by1 = min(b1 + NW, W - 1), min(b3 + NW, H - 1)
                bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
                N = bw * bh if bw > 0 and bh > 0 else 0
                bw = max(bw, 1)
                pos = np.arange(N)
                ty, tx = by0 + pos // bw, bx0 + pos % bw
                assert ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)).all()                 # the rows the stream reads
                # the drop test: both 16-bit halves of (tx | ty << 16) - (ox | oy << 16), no borrow between the halves
                dx, dy = (tx[None] - ox[:, None]) & 0xffff, (ty[None] - oy[:, None]) & 0xffff
                inside16 = (dx < WS) & (dy < WS)
                rx, ry = tx[None] - wx0[:, None], ty[None] - wy0[:, None]
                inside = (rx >= 0) & (rx < WS) & (ry >= 0) & (ry < WS)
                assert np.array_equal(inside16, inside)
                assert (((32767 - ox) & 0xffff) >= WS).all() and (((32767 - oy) & 0xffff) >= WS).all()     # columns past the box
                cell = (tx[None] - ox[:, None]) * WS + (ty[None] - oy[:, None])            # s_pm + d_q4, in floats, minus tid * WLD
                assert ((cell[inside] >= 0) & (cell[inside] < WS * WS)).all()
                written = np.zeros((len(blk), WS * WS), bool)
                pi, _ = np.nonzero(inside)
                written[pi, cell[inside]] = True
                k = np.arange(WS)
                inmap = (((wx0[:, None] + k[None]) >= 0) & ((wx0[:, None] + k[None]) < W))[:, :, None] & \
                        (((wy0[:, None] + k[None]) >= 0) & ((wy0[:, None] + k[None]) < H))[:, None, :]
                assert np.array_equal(written.reshape(-1, WS, WS), inmap)                  # cell (cx, cy) at cx * WS + cy
                assert clipped or written.all()
    return clipped_of
