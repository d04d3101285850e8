"""The inputs of the image-geometry tests (a helper of test_image_geometry_cpu / _gpu and test_window_kernels_gpu, not a conftest):
frame sizes, seeded images, the generic homographies that run under the classification rule of fp64_refs.classify_bytes, and the
exact homographies (source coordinates on integers and half-integers only) whose bytes are known in integer arithmetic.  The CPU
test proves on the references alone every condition the GPU test puts on these inputs."""
import functools

import numpy as np

SIZES = [(61, 83), (64, 64), (1, 1), (1, 97), (53, 1)]
THIN = [(1, 1), (1, 97), (53, 1)]            # nothing may be excused here: a handful of bytes each
CHANNELS = [1, 3, 4]
CAP = 0.005                                  # share of bytes a generic case may excuse: above it the case proves too little

GENERIC = {
    "mild": np.array([[1.01, 0.02, 3.4], [-0.015, 0.99, -2.2], [1e-5, -2e-5, 1.0]]),
    "strong": np.array([[0.8, 0.35, 20.0], [-0.3, 1.2, -15.0], [1.5e-3, -1e-3, 1.0]]),
    "horizon": np.array([[1.0, 0.1, 2.0], [0.05, 1.0, -3.0], [-2e-2, 3e-3, 1.0]]),
}
# `horizon` has ITS OWN third row vanish inside the frame (at x = 50), but the warp divides by the third row of the INVERSE, which
# stays within [0.66, 2.53] on these frames.  Handed over inverted, the kernel's denominator d = -0.02 x + 0.003 y + 1 does cross
# the frame: pixels with d < 0, and huge finite coordinates beside the line.
GENERIC["horizon-inv"] = np.linalg.inv(GENERIC["horizon"])
CROSSED = [(61, 83), (64, 64), (1, 97)]      # the frames wide enough for the line d = 0 of `horizon-inv` (x ~ 50)
FAR = np.array([[1.0, 0.0, 10000.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])               # the frame carried wholly outside
INT_SHIFTS = [(3, 5), (-7, 2), (0, -4), (-1, -1), (1, 0), (200, 0), (0, -300), (-97, 53)]
HALF_SHIFTS = [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (-2.5, 3.5)]

RESIZE_SIZES = [(37, 45), (39, 47), (1, 1), (1, 97), (53, 1), (64, 64), (8, 8)]
RESIZE_FACTORS = [2, 3, 4, 1.5]


def image(h, w, c, seed=0):
    """Seeded noise (the steepest gradients a frame can have): (h, w) for c == 1, else (h, w, c)."""
    rs = np.random.RandomState([seed, h, w, c])
    return rs.randint(0, 256, (h, w) if c == 1 else (h, w, c)).astype(np.uint8)


DZERO_SEED = 26      # `dzero` has rational source coordinates with small denominators, which makes bytes within band of a tie
#                      several times as common as under the generic homographies (0.1 - 0.2 %): this seed is one for which the
#                      thin frames have none (the CPU test asserts it)


def case_image(name, h, w, c):
    """The image a non-exact case runs on."""
    return image(h, w, c, seed=DZERO_SEED if name == "dzero" else 0)


def mask_image(h, w, seed=0):
    """A seeded binary mask (0 / 255) with both values everywhere: one wrong source pixel shows."""
    rs = np.random.RandomState([seed, h, w, 255])
    return ((rs.uniform(size=(h, w)) > 0.5) * 255).astype(np.uint8)


def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def dzero(h, w):
    """(Hm, Hinv, k): Hinv = [[1, 0, 1/4], [0, 1, 3/4], [1, 1, -k]] has d = x + y - k, EXACTLY 0.0 on the anti-diagonal x + y = k
    (which crosses every frame here: k = 31, or 0 for a frame too small for that) and negative before it.  The quarter offsets
    keep every other pixel off the places where the rule excuses: 4 x + 1 and 4 y + 3 are odd, so sx, sy are never -1, w or h
    and never a half-integer.  Hm is the analytic inverse; det = -(k + 1) is a power of two, so every entry is a dyadic
    number and np.linalg.inv(Hm) can give Hinv back bit for bit (asserted wherever the case is used)."""
    k = 31 if h + w - 2 >= 31 else 0
    q = 1.0 / (k + 1)
    Hinv = np.array([[1.0, 0.0, 0.25], [0.0, 1.0, 0.75], [1.0, 1.0, -float(k)]])
    Hm = q * np.array([[k + 0.75, -0.25, 0.25], [-0.75, k + 0.25, 0.75], [1.0, 1.0, -1.0]])
    return Hm, Hinv, k


def homography(name, h, w):
    """The non-exact homographies by name: the generic three, `dzero` and `far`."""
    if name == "dzero":
        return dzero(h, w)[0]
    return FAR if name == "far" else GENERIC[name]


def shift_zero_fill(img, tx, ty):
    """dst(x, y) = src(x - tx, y - ty) by numpy slices, zero where the source is outside."""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    if abs(tx) < w and abs(ty) < h:
        out[max(ty, 0):h + min(ty, 0), max(tx, 0):w + min(tx, 0)] = img[max(-ty, 0):h + min(-ty, 0), max(-tx, 0):w + min(-tx, 0)]
    return out


def exact_cases(h, w):
    """[(name, Hm, Hinv, sx2, sy2, by_numpy)]: Hinv the analytic inverse, (sx2, sy2) the source coordinates DOUBLED as integer
    grids, by_numpy (or None) the same warp as plain numpy indexing of an (h, w[, c]) array with zero fill.  Every fp32
    operation of the kernel is exact for these (the fractions are 0 or 1/2), so the bytes are known with no band."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    cases = []
    for tx, ty in INT_SHIFTS:
        cases.append((f"shift({tx},{ty})", translation(tx, ty), translation(-tx, -ty), 2 * (xs - tx), 2 * (ys - ty),
                      functools.partial(shift_zero_fill, tx=tx, ty=ty)))
    for tx, ty in HALF_SHIFTS:
        cases.append((f"half({tx},{ty})", translation(tx, ty), translation(-tx, -ty), 2 * xs - int(2 * tx), 2 * ys - int(2 * ty),
                      None))
    fx = np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    fy = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]])
    fxy = np.array([[-1.0, 0.0, w - 1.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]])
    cases.append(("flip-x", fx, fx, 2 * (w - 1 - xs), 2 * ys, lambda a: a[:, ::-1]))
    cases.append(("flip-y", fy, fy, 2 * xs, 2 * (h - 1 - ys), lambda a: a[::-1]))
    cases.append(("turn-180", fxy, fxy, 2 * (w - 1 - xs), 2 * (h - 1 - ys), lambda a: a[::-1, ::-1]))
    if h == w:                                                             # dst(x, y) = src(y, n - 1 - x)
        r90 = np.array([[0.0, -1.0, h - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        r90i = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, h - 1.0], [0.0, 0.0, 1.0]])
        cases.append(("turn-90", r90, r90i, 2 * ys, 2 * (h - 1 - xs), lambda a: np.rot90(a, -1)))
    cases.append(("up-2", np.diag([2.0, 2.0, 1.0]), np.diag([0.5, 0.5, 1.0]), xs, ys, None))
    return cases


def share(flags):
    return float(np.mean(flags)) if flags.size else 0.0
