"""float64 numpy restatement of woft_hsynth_render / woft_hsynth_labels, written from the semantics in include/woft_hip.h
(DESIGN.md section 23), plus the fixed cases the CPU and the GPU tests share.  Occluders here are (tex (ho, wo, 4) uint8 numpy,
H_occ 3x3 texture -> destination), as the public interface takes them."""
import numpy as np


def _source(Hinv, xs, ys):
    d = Hinv[2, 0] * xs + Hinv[2, 1] * ys + Hinv[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = (Hinv[0, 0] * xs + Hinv[0, 1] * ys + Hinv[0, 2]) / d
        sy = (Hinv[1, 0] * xs + Hinv[1, 1] * ys + Hinv[1, 2]) / d
    return sx, sy, d


def _bilinear(planes, sx, sy):
    """Zero-border bilinear sample of planes (h, w, C) float64 at (sx, sy) -> (..., C).  Non-finite coordinates give NaN."""
    h, w = planes.shape[:2]
    bad = ~(np.isfinite(sx) & np.isfinite(sy))
    sx0, sy0 = np.where(bad, 0.0, sx), np.where(bad, 0.0, sy)
    fx0, fy0 = np.floor(sx0), np.floor(sy0)
    fx, fy = (sx0 - fx0)[..., None], (sy0 - fy0)[..., None]
    x0 = np.clip(fx0, -4, w + 4).astype(np.int64)
    y0 = np.clip(fy0, -4, h + 4).astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return planes[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]
    top = tap(y0, x0) * (1 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1 - fx) + tap(y0 + 1, x0 + 1) * fx
    out = top * (1 - fy) + bot * fy
    out[bad] = np.nan
    return out


def _premultiplied(tex):
    t = tex.astype(np.float64)
    a = t[..., 3:4] / 255.0
    return np.concatenate([a * t[..., :3], a], 2)          # (ho, wo, 4): O_b, O_g, O_r, A


def render(base, H_gt, occluders=(), gain=None, bias=None, out_hw=None):
    """-> (out_f64 (h, w, 3) un-rounded, cover (h, w))."""
    h, w = base.shape[:2] if out_hw is None else out_hw
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy, _ = _source(np.linalg.inv(np.asarray(H_gt, np.float64)), xs, ys)
    v = _bilinear(base.astype(np.float64), sx, sy)
    g = np.ones(3) if gain is None else np.broadcast_to(np.asarray(gain, np.float64).ravel(), (3,))
    b = np.zeros(3) if bias is None else np.broadcast_to(np.asarray(bias, np.float64).ravel(), (3,))
    v = g * v + b
    keep = np.ones((h, w))
    for tex, H_occ in occluders:
        ox, oy, _ = _source(np.linalg.inv(np.asarray(H_occ, np.float64)), xs, ys)
        s = _bilinear(_premultiplied(tex), ox, oy)
        A = s[..., 3]
        v = (1 - A)[..., None] * v + s[..., :3]
        keep = keep * (1 - A)
    return v, 1 - keep


def labels(src_hw, H_gt, occluders=(), out_hw=None, lo=0.25, hi=0.75, detail=False):
    """-> (flow (2, hs, ws) float64, visible (hs, ws) float64, valid (hs, ws) bool); detail: also (px, py, d, T, inside)."""
    hs, ws = src_hw
    h, w = src_hw if out_hw is None else out_hw
    ys, xs = np.mgrid[0:hs, 0:ws].astype(np.float64)
    px, py, d = _source(np.asarray(H_gt, np.float64), xs, ys)
    flow = np.stack([px - xs, py - ys])
    with np.errstate(invalid="ignore"):
        inside = (d > 0) & (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    keep = np.ones((hs, ws))
    for tex, H_occ in occluders:
        ox, oy, _ = _source(np.linalg.inv(np.asarray(H_occ, np.float64)), px, py)
        keep = keep * (1 - _bilinear(_premultiplied(tex), ox, oy)[..., 3])
    T = 1 - keep
    with np.errstate(invalid="ignore"):
        seen = inside & (T <= lo)
        hidden = ~inside | (T >= hi)
    out = (flow, seen.astype(np.float64), seen | hidden)
    return out + ((px, py, d, T, inside),) if detail else out


def sample_bilinear(img, x, y):
    """img (h, w, C) float64 at the points (x, y) (arrays of equal shape), zero border."""
    return _bilinear(img, np.asarray(x, np.float64), np.asarray(y, np.float64))


# ---- the fixed cases of tests/test_hsynth_gpu.py; tests/test_hsynth_cpu.py asserts the margins its label test relies on -------
BASE_HW = (24, 40)
DST_HWS = ((1, 1), (3, 5), (17, 33))
CASE_SEED = 56          # (chosen so that test_hsynth_cpu.test_label_margins holds; change the seed, never the margins)


def base_image():
    return np.random.RandomState(CASE_SEED).randint(0, 256, BASE_HW + (3,)).astype(np.uint8)


def textures():
    """A 1x1 and a 9x13 BGRA texture with every alpha value in play, and two more 9x13 ones with a hard alpha."""
    rs = np.random.RandomState(CASE_SEED + 1)
    t1 = np.array([[[200, 40, 90, 255]]], np.uint8)
    t2 = rs.randint(0, 256, (9, 13, 4)).astype(np.uint8)
    t3 = rs.randint(0, 256, (9, 13, 4)).astype(np.uint8)
    t3[..., 3] = np.where(t3[..., 3] > 100, 255, 0)
    t4 = rs.randint(0, 256, (9, 13, 4)).astype(np.uint8)
    t4[..., 3] = 255
    return [t1, t2, t3, t4]


def _place(scale, angle, cx, cy, tex):
    ho, wo = tex.shape[:2]
    ca, sa = scale * np.cos(angle), scale * np.sin(angle)
    tx, ty = (wo - 1) / 2.0, (ho - 1) / 2.0
    return np.array([[ca, -sa, cx - ca * tx + sa * ty], [sa, ca, cy - sa * tx - ca * ty], [0.0, 0.0, 1.0]])


def occluder_sets(out_hw):
    """{n_occ: occluders} for a destination of out_hw: 0, 1, 2 (overlapping: both cover the frame's centre) and 4."""
    from woft_amd.hsynth import random_homography
    h, w = out_hw
    t1, t2, t3, t4 = textures()
    rs = np.random.RandomState(CASE_SEED + 2)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    o1 = (t1, _place(max(1.0, 0.45 * min(h, w)), 0.3, cx + 0.21, cy - 0.17, t1))       # the 1x1 texture, magnified
    o2 = (t2, _place(max(0.11, 0.05 * min(h, w)), -0.7, cx - 0.4, cy + 0.3, t2) @ random_homography(rs, 9, 13, 0.1))
    o3 = (t3, _place(max(0.13, 0.04 * min(h, w)), 1.9, cx + 0.3 * w, cy - 0.1 * h, t3))
    o4 = (t4, _place(max(0.09, 0.03 * min(h, w)), 0.1, cx - 0.25 * w, cy + 0.2 * h, t4) @ random_homography(rs, 9, 13, 0.2))
    return {0: [], 1: [o2], 2: [o2, o1], 4: [o1, o2, o3, o4]}


def homographies(out_hw):
    """name -> H_gt (base -> destination): identity, a non-integer translation, two random_homography draws (composed with the
    scaling of the base frame onto the destination frame, so that the destination sees the image)."""
    from woft_amd.hsynth import random_homography
    hs, ws = BASE_HW
    h, w = out_hw
    fit = np.diag([max(w - 1, 1) / (ws - 1.0), max(h - 1, 1) / (hs - 1.0), 1.0])
    rs = np.random.RandomState(CASE_SEED + 3)
    return {"identity": np.eye(3),
            "translation": np.array([[1.0, 0.0, 2.37], [0.0, 1.0, -1.61], [0.0, 0.0, 1.0]]),
            "random0": fit @ random_homography(rs, hs, ws, 0.2),
            "random1": fit @ random_homography(rs, hs, ws, 0.3)}


def horizon_homography():
    """A homography whose horizon (d = 0) crosses the base image: d > 0 on its left part, d <= 0 on the right."""
    hs, ws = BASE_HW
    return np.array([[1.0, 0.02, 1.3], [0.01, 1.0, 0.7], [-1.0 / (0.62 * ws), 0.0002, 1.0]])


def label_cases():
    """(name, H_gt, occluders, out_hw) of the GPU label test: every destination size x homography x occluder set, and the
    horizon-in-frame homography with every occluder set."""
    for out_hw in DST_HWS:
        for hname, H in homographies(out_hw).items():
            for n, occ in occluder_sets(out_hw).items():
                yield f"{out_hw}-{hname}-{n}", H, occ, out_hw
    for n, occ in occluder_sets(DST_HWS[-1]).items():
        yield f"horizon-{n}", horizon_homography(), occ, DST_HWS[-1]
