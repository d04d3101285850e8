"""Synthetic-homography training pairs with occlusion labels, made on the device.

What the losses of `weights_at`, `visibility_at` and `visibility_map` consume: an image, the same image seen through a known
homography with a photometric change and pasted occluders, the exact homography, the flow it induces and a per-pixel visibility
label with its valid mask.  The reference's training configs name such a data set (`COCOHSynth`), its code is not part of the
reference: the semantics here are this project's own (include/woft_hip.h, `woft_hsynth_render` / `woft_hsynth_labels`).  Two HIP
launches per sample; everything random comes from `numpy.random.RandomState`, so a sample is a function of its seed.
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops, synth

HSynthSample = namedtuple("HSynthSample", "src dst H_gt flow_gt visible valid")
MAX_OCCLUDERS = 4          # WOFT_HSYNTH_MAX_OCC


def _device_u8(img, what, channels, multiple=1):
    """(H, W, channels) uint8, numpy or device tensor -> contiguous device tensor (checked before anything is uploaded)."""
    if isinstance(img, np.ndarray):
        dtype, ok_dtype = img.dtype, img.dtype == np.uint8
    elif isinstance(img, torch.Tensor):
        dtype, ok_dtype = img.dtype, img.dtype == torch.uint8
    else:
        raise TypeError(f"{what}: a uint8 numpy image or device tensor is expected, got {type(img).__name__}")
    if not ok_dtype:
        raise TypeError(f"{what}: a uint8 image is expected, got {dtype}")
    shape = tuple(img.shape)
    if len(shape) != 3 or shape[2] != channels or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what}: shape (H, W, {channels}) is expected, got {shape}")
    if shape[0] % multiple or shape[1] % multiple:
        raise ValueError(f"{what}: height and width must be multiples of {multiple}, got {shape[:2]}")
    if isinstance(img, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(img)).cuda()
    if not img.is_cuda:
        raise ValueError(f"{what}: a device tensor (or a numpy image) is expected, got a tensor on {img.device}")
    return img.contiguous()


def _h33(Hmat, what):
    Hmat = np.asarray(Hmat, dtype=np.float64)
    if Hmat.shape != (3, 3) or not np.all(np.isfinite(Hmat)):
        raise ValueError(f"{what}: a finite 3x3 matrix is expected, got shape {Hmat.shape}")
    return Hmat


def _hw(v, what):
    try:
        h, w = (int(x) for x in v)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: a (height, width) pair is expected, got {v!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"{what}: positive sizes are expected, got {(h, w)}")
    return h, w


def _occluders(occluders):
    occluders = list(occluders)
    if len(occluders) > MAX_OCCLUDERS:
        raise ValueError(f"occluders: at most {MAX_OCCLUDERS} are composited, got {len(occluders)}")
    out = []
    for k, oc in enumerate(occluders):
        if not isinstance(oc, (tuple, list)) or len(oc) != 2:
            raise TypeError(f"occluders[{k}]: a (tex_bgra, H_occ) pair is expected")
        out.append((_device_u8(oc[0], f"occluders[{k}] texture", 4), _h33(oc[1], f"occluders[{k}] H_occ")))
    return out


def render_pair(base, H_gt, occluders=(), gain=None, bias=None, out_hw=None, want_f32=False, want_cover=False):
    """The second frame of a pair: `base` ((hs, ws, 3) uint8, device tensor or numpy image) seen through H_gt (3x3, base ->
    destination), times gain plus bias (a number or three, per channel), under the occluders [(tex_bgra (ho, wo, 4) uint8, H_occ
    3x3 texture -> destination)] composited in order; black outside the base image.  -> dst (h, w, 3) uint8 on the device
    (out_hw, default the base's size); with want_f32 or want_cover: (dst, the un-rounded float32 (h, w, 3) image or None, the
    occluders' joint coverage (h, w) float32 or None)."""
    base = _device_u8(base, "base", 3)
    H_gt = _h33(H_gt, "H_gt")
    occ = _occluders(occluders)
    h, w = base.shape[:2] if out_hw is None else _hw(out_hw, "out_hw")

    def three(v, what):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64).ravel()
        if a.size not in (1, 3) or not np.all(np.isfinite(a)):
            raise ValueError(f"{what}: one finite number or three (per channel) are expected, got {v!r}")
        return np.broadcast_to(a, (3,)).tolist()
    gain, bias = three(gain, "gain"), three(bias, "bias")
    dev = base.device
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    f32 = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if want_f32 else None
    cover = torch.empty((h, w), dtype=torch.float32, device=dev) if want_cover else None
    ops.hsynth_render(base, H_gt, occ, gain, bias, dst, f32, cover)
    return (dst, f32, cover) if (want_f32 or want_cover) else dst


def pair_labels(src_hw, H_gt, occluders=(), out_hw=None, lo=0.25, hi=0.75):
    """The labels of the pair `render_pair` makes with the same arguments, per template pixel of the (hs, ws) base image:
    -> (flow_gt (2, hs, ws) float32, visible (hs, ws) float32 in {0, 1}, valid (hs, ws) bool), on the device.  A pixel is visible
    when it lands inside the (h, w) destination frame with at most `lo` of it covered by occluders, not visible when it leaves the
    frame or at least `hi` is covered, and not valid (an occluder's soft edge) in between."""
    hs, ws = _hw(src_hw, "src_hw")
    h, w = (hs, ws) if out_hw is None else _hw(out_hw, "out_hw")
    H_gt = _h33(H_gt, "H_gt")
    occ = _occluders(occluders)
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo < hi <= 1.0):
        raise ValueError(f"lo, hi: 0 <= lo < hi <= 1 is expected, got {lo!r}, {hi!r}")
    dev = occ[0][0].device if occ else torch.device("cuda", torch.cuda.current_device())
    flow = torch.empty((2, hs, ws), dtype=torch.float32, device=dev)
    visible = torch.empty((hs, ws), dtype=torch.float32, device=dev)
    valid = torch.empty((hs, ws), dtype=torch.bool, device=dev)
    ops.hsynth_labels((hs, ws), H_gt, occ, (h, w), lo, hi, flow, visible, valid)
    return flow, visible, valid


def _solve(A, b):
    """Gaussian elimination with partial pivoting in element-wise fp64 operations (no LAPACK: the same bits on every machine)."""
    M = np.concatenate([np.asarray(A, np.float64), np.asarray(b, np.float64)[:, None]], 1)
    n = M.shape[0]
    for i in range(n):
        p = i + int(np.argmax(np.abs(M[i:, i])))
        if M[p, i] == 0.0:
            raise np.linalg.LinAlgError("singular system")
        if p != i:
            M[[i, p]] = M[[p, i]]
        for j in range(i + 1, n):
            M[j] = M[j] - (M[j, i] / M[i, i]) * M[i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = M[i, n]
        for j in range(i + 1, n):
            s = s - M[i, j] * x[j]
        x[i] = s / M[i, i]
    return x


def homography_from_4pts(src, dst):
    """The homography that maps four points src (4, 2) onto dst (4, 2), h33 = 1, solved in fp64 on the host."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        (x, y), (u, v) = src[k], dst[k]
        A[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
        b[2 * k], b[2 * k + 1] = u, v
    return np.append(_solve(A, b), 1.0).reshape(3, 3)


def _strictly_convex(q):
    """Quadrilateral q (4, 2) in the order top-left, top-right, bottom-right, bottom-left (y down) keeps that orientation and is
    strictly convex: every turn has a positive cross product."""
    for k in range(4):
        a, b, c = q[k], q[(k + 1) % 4], q[(k + 2) % 4]
        if (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) <= 0.0:
            return False
    return True


def random_homography(rs, h, w, max_shift=0.2):
    """A homography of an (h, w) image: its four corners are moved by up to max_shift of the shorter side each way (uniform, from
    the numpy RandomState rs) and the 4-point homography is solved in fp64; drawn again while the moved quadrilateral is not
    strictly convex with the corners' original orientation.  -> 3x3 float64, image -> moved image."""
    if not isinstance(rs, np.random.RandomState):
        raise TypeError(f"rs: a numpy.random.RandomState is expected, got {type(rs).__name__}")
    h, w = _hw((h, w), "h, w")
    max_shift = float(max_shift)
    if not (0.0 <= max_shift < float("inf")):
        raise ValueError(f"max_shift: a finite number >= 0 is expected, got {max_shift!r}")
    corners = np.array([[0.0, 0.0], [w - 1.0, 0.0], [w - 1.0, h - 1.0], [0.0, h - 1.0]])
    if h < 2 or w < 2:
        raise ValueError(f"h, w: an image of at least 2 x 2 pixels is expected, got {(h, w)}")
    r = max_shift * min(h, w)
    while True:
        moved = corners + rs.uniform(-r, r, (4, 2))
        if _strictly_convex(moved):
            return homography_from_4pts(corners, moved)


def make_occluder(rs, ho, wo):
    """A BGRA occluder texture (ho, wo, 4) uint8: the colour of synth.make_template, a hard 0 / 255 alpha that is a random
    ellipse or a random convex polygon (the corners of one drawn on an ellipse), both inside the texture."""
    if not isinstance(rs, np.random.RandomState):
        raise TypeError(f"rs: a numpy.random.RandomState is expected, got {type(rs).__name__}")
    ho, wo = _hw((ho, wo), "ho, wo")
    th, tw = max(8, -(-ho // 8) * 8), max(8, -(-wo // 8) * 8)
    colour = synth.make_template(th, tw, seq_id=int(rs.randint(0, 1 << 16)))[:ho, :wo]
    ys, xs = np.mgrid[0:ho, 0:wo].astype(np.float64)
    cy, cx = (ho - 1) / 2.0, (wo - 1) / 2.0
    ry, rx = max(cy, 0.5) * rs.uniform(0.6, 1.0), max(cx, 0.5) * rs.uniform(0.6, 1.0)
    if rs.randint(0, 2) == 0:
        inside = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
    else:
        ang = np.sort(rs.uniform(0.0, 2.0 * np.pi, int(rs.randint(3, 8))))
        px, py = cx + rx * np.cos(ang), cy + ry * np.sin(ang)
        inside = np.ones((ho, wo), bool)
        for k in range(len(ang)):                       # (ascending angles: the interior has a cross product >= 0 with every edge)
            ex, ey = px[(k + 1) % len(ang)] - px[k], py[(k + 1) % len(ang)] - py[k]
            inside &= ex * (ys - py[k]) - ey * (xs - px[k]) >= 0.0
    alpha = np.where(inside, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([colour, alpha[..., None]], 2))


class HSynth:
    """A map-style data set of synthetic-homography pairs over `images` (uint8 (H, W, 3), numpy or device tensors, H and W
    multiples of 8: the 'nopad' contract of the shipped training configs).  ds[i] -> HSynthSample(src, dst, H_gt, flow_gt,
    visible, valid): src = images[i], dst = render_pair(...) and the labels of pair_labels(...) on the device, H_gt a numpy
    float64 array (src -> dst).  A sample is a function of (seed, i) -- ds.sample(i, epoch) folds an epoch number in -- drawn from
    numpy.random.RandomState([seed, i, epoch]): the homography (random_homography, max_shift), between n_occluders[0] and
    n_occluders[1] occluders (a texture of occluder_textures -- default: eight make_occluder textures drawn from the seed --
    through a random similarity times a random_homography of the texture, the longer side between 0.2 and 0.5 of the frame's
    shorter one, centred anywhere in the frame), one gain and one bias for all channels from gain_range and bias_range."""

    def __init__(self, images, occluder_textures=None, seed=0, max_shift=0.2, n_occluders=(0, 2), gain_range=(0.8, 1.2),
                 bias_range=(-20, 20), lo=0.25, hi=0.75):
        self.images = [_device_u8(im, f"images[{k}]", 3, multiple=8) for k, im in enumerate(images)]
        self.seed = int(seed)
        if not (0 <= self.seed < 1 << 32):
            raise ValueError(f"seed: 0 <= seed < 2^32 is expected, got {seed!r}")
        n0, n1 = (int(v) for v in n_occluders)
        if not (0 <= n0 <= n1 <= MAX_OCCLUDERS):
            raise ValueError(f"n_occluders: 0 <= min <= max <= {MAX_OCCLUDERS} is expected, got {n_occluders!r}")
        self.n_occluders = (n0, n1)
        self.max_shift = float(max_shift)
        self.gain_range = tuple(float(v) for v in gain_range)
        self.bias_range = tuple(float(v) for v in bias_range)
        if len(self.gain_range) != 2 or self.gain_range[0] > self.gain_range[1]:
            raise ValueError(f"gain_range: (low, high) is expected, got {gain_range!r}")
        if len(self.bias_range) != 2 or self.bias_range[0] > self.bias_range[1]:
            raise ValueError(f"bias_range: (low, high) is expected, got {bias_range!r}")
        self.lo, self.hi = float(lo), float(hi)
        if not (0.0 <= self.lo < self.hi <= 1.0):
            raise ValueError(f"lo, hi: 0 <= lo < hi <= 1 is expected, got {lo!r}, {hi!r}")
        if occluder_textures is None:
            rs = np.random.RandomState([self.seed, 0x0CC1])
            occluder_textures = [] if n1 == 0 else [make_occluder(rs, int(rs.randint(32, 97)), int(rs.randint(32, 97)))
                                                    for _ in range(8)]
        self.textures = [_device_u8(t, f"occluder_textures[{k}]", 4) for k, t in enumerate(occluder_textures)]
        if n1 > 0 and not self.textures:
            raise ValueError("occluder_textures: at least one texture is expected when n_occluders allows an occluder")

    def __len__(self):
        return len(self.images)

    def draw(self, i, epoch=0):
        """The random part of sample (i, epoch), on the host: (H_gt, [(texture index, H_occ)], gain, bias)."""
        i, epoch = int(i), int(epoch)
        if not (0 <= i < len(self.images)):
            raise IndexError(f"HSynth index {i} out of range for {len(self.images)} images")
        if not (0 <= epoch < 1 << 32):
            raise ValueError(f"epoch: 0 <= epoch < 2^32 is expected, got {epoch!r}")
        rs = np.random.RandomState([self.seed, i, epoch])
        h, w = self.images[i].shape[:2]
        H_gt = random_homography(rs, h, w, self.max_shift)
        occ = []
        for _ in range(int(rs.randint(self.n_occluders[0], self.n_occluders[1] + 1))):
            t = int(rs.randint(0, len(self.textures)))
            ho, wo = self.textures[t].shape[:2]
            s = rs.uniform(0.2, 0.5) * min(h, w) / max(ho, wo)
            a = rs.uniform(0.0, 2.0 * np.pi)
            cx, cy = rs.uniform(0.0, w - 1.0), rs.uniform(0.0, h - 1.0)
            ca, sa = s * np.cos(a), s * np.sin(a)
            tx, ty = (wo - 1) / 2.0, (ho - 1) / 2.0
            place = np.array([[ca, -sa, cx - ca * tx + sa * ty], [sa, ca, cy - sa * tx - ca * ty], [0.0, 0.0, 1.0]])
            bend = random_homography(rs, ho, wo, self.max_shift) if min(ho, wo) >= 2 else np.eye(3)
            occ.append((t, place @ bend))
        gain = float(rs.uniform(*self.gain_range))
        bias = float(rs.uniform(*self.bias_range))
        return H_gt, occ, gain, bias

    def sample(self, i, epoch=0):
        H_gt, occ, gain, bias = self.draw(i, epoch)
        src = self.images[int(i)]
        occluders = [(self.textures[t], H_occ) for t, H_occ in occ]
        dst = render_pair(src, H_gt, occluders, gain=gain, bias=bias)
        flow, visible, valid = pair_labels(src.shape[:2], H_gt, occluders, lo=self.lo, hi=self.hi)
        return HSynthSample(src, dst, H_gt, flow, visible, valid)

    def __getitem__(self, i):
        return self.sample(i, 0)
