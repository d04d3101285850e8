"""Helpers of the multi-target photometric refinement's tests: the mask sets on photo_host's base scene, the
per-target starting poses and the byte comparison of a batched result with a single-target one.  Nothing here computes an expected
value: the tests compare the multi-target path with the single-target entry points."""
import numpy as np

import photo_host as ph

H, W = ph.TEMPLATE_HW


def _rect(y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def mask_set(K):
    """K masks on the 64 x 96 template.  K = 1: the base mask (a box of 57 x 40 = 2280 candidates: two partials).  K >= 3: also a
    mask that overlaps it and touches the template's border row and column (30 x 40: one partial), and a 1 x 3 mask (fewer pixels
    than unknowns: never launched).  K = 32: 28 small rectangles, many overlapping, and on bit 31 a 30 x 40 rectangle."""
    masks = [ph.base_mask()]
    if K >= 3:
        masks += [_rect(0, 30, 0, 40), _rect(40, 41, 80, 83)]
    rs = np.random.RandomState(77)
    while len(masks) < K - 1:
        y0, x0 = int(rs.randint(1, H - 22)), int(rs.randint(1, W - 26))
        masks.append(_rect(y0, y0 + int(rs.randint(14, 21)), x0, x0 + int(rs.randint(16, 25))))
    if len(masks) < K:
        masks.append(_rect(30, 60, 50, 90))
    assert len(masks) == K
    return masks


def poses(W0, K):
    """K starting poses: W0 moved by a fifth of a pixel per step, different for neighbouring targets."""
    out = np.repeat(np.asarray(W0, np.float64)[None], K, 0)
    for t in range(K):
        out[t, 0, 2] += 0.2 * (t % 5 - 2)
        out[t, 1, 2] -= 0.15 * (t % 3 - 1)
    return out


INFO_ARRAYS = ("H_iter", "gain", "bias", "cost", "n_valid", "step")


def assert_same_refinement(got, want, tag):
    """(H, info) of target t of a batched refinement against PhotoTemplate.refine's: every byte but host_wait_s."""
    (Hm, im), (Hs, isg) = got, want
    assert np.array_equal(Hm, Hs), (tag, "H", Hm, Hs)
    assert (im.status, im.best, im.n_set) == (isg.status, isg.best, isg.n_set), (tag, im.status, isg.status, im.best, isg.best)
    for name in INFO_ARRAYS:
        a, b = getattr(im, name), getattr(isg, name)
        # (bytes, not values: a NaN -- the step no iterate took, the cost of an iterate without a valid pixel -- has to be the same NaN)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, name, a, b)
    for name in ("rms_before", "rms_after"):
        a, b = getattr(im, name), getattr(isg, name)
        assert a == b or (a != a and b != b), (tag, name, a, b)
