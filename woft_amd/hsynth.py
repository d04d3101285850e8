"""Synthetic-homography training pairs with occlusion labels, made on the device.

What the losses of `weights_at`, `visibility_at` and `visibility_map` consume: an image, the same image seen through a known
homography with a photometric change and pasted occluders, the exact homography, the flow it induces and a per-pixel visibility
label with its valid mask.  The reference's training configs name such a data set (`COCOHSynth`), its code is not part of the
reference: the semantics here are this project's own (include/woft_hip.h, `woft_hsynth_render` / `woft_hsynth_labels`).  Two HIP
launches per sample; everything random comes from `numpy.random.RandomState`, so a sample is a function of its seed.

Opt-in (`woft_hsynth_render_bg`, `woft_hsynth_augment`): a background image behind the warped plane, and
`augment` -- blur, colour map, noise -- over the rendered frame, one more launch each for the frames it is asked for.
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops, synth

HSynthSample = namedtuple("HSynthSample", "src dst H_gt flow_gt visible valid")
HSynthAugment = namedtuple("HSynthAugment", "background background_H blur_sigma saturation hue contrast noise_sigma seed_dst seed_src")
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


def render_pair(base, H_gt, occluders=(), gain=None, bias=None, out_hw=None, want_f32=False, want_cover=False, background=None,
                background_H=None, want_plane=False):
    """The second frame of a pair: `base` ((hs, ws, 3) uint8, device tensor or numpy image) seen through H_gt (3x3, base ->
    destination), times gain plus bias (a number or three, per channel), under the occluders [(tex_bgra (ho, wo, 4) uint8, H_occ
    3x3 texture -> destination)] composited in order; black outside the base image, or `background` ((hb, wb, 3) uint8, numpy or
    device) seen through background_H (3x3, background -> destination; default the identity) with a replicate border, behind the
    plane and under the gain, the bias and the occluders.  -> dst (h, w, 3) uint8 on the device (out_hw, default the base's
    size); with want_f32 or want_cover: (dst, the un-rounded float32 (h, w, 3) image or None, the occluders' joint coverage (h, w)
    float32 or None); with want_plane (a background is needed): those three and the plane's coverage (h, w) float32."""
    base = _device_u8(base, "base", 3)
    H_gt = _h33(H_gt, "H_gt")
    occ = _occluders(occluders)
    h, w = base.shape[:2] if out_hw is None else _hw(out_hw, "out_hw")
    if background is None:
        if background_H is not None or want_plane:
            raise ValueError("background: background_H and want_plane need a background image")
    else:
        background = _device_u8(background, "background", 3)
        background_H = np.eye(3) if background_H is None else _h33(background_H, "background_H")

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
    if background is None:
        ops.hsynth_render(base, H_gt, occ, gain, bias, dst, f32, cover)
        return (dst, f32, cover) if (want_f32 or want_cover) else dst
    plane = torch.empty((h, w), dtype=torch.float32, device=dev) if want_plane else None
    ops.hsynth_render_bg(base, H_gt, occ, gain, bias, background, background_H, dst, f32, cover, plane)
    if want_plane:
        return dst, f32, cover, plane
    return (dst, f32, cover) if (want_f32 or want_cover) else dst


MAX_BLUR = 7               # WOFT_HSYNTH_MAX_BLUR
GREY_BGR = (0.114, 0.587, 0.299)


def blur_taps(sigma):
    """The taps of augment's blur: exp(-i^2 / (2 sigma^2)) for i = -r .. r with r = min(7, ceil(3 sigma)), normalised to sum 1 in
    float64 and then rounded to float32.  sigma = 0: the single tap 1 (no blur)."""
    sigma = float(sigma)
    if not (0.0 <= sigma < float("inf")):
        raise ValueError(f"blur_sigma: a finite number >= 0 is expected, got {sigma!r}")
    r = min(MAX_BLUR, int(np.ceil(3.0 * sigma)))
    if r == 0:
        return np.ones(1, np.float32)
    i = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def colour_matrix(saturation=1.0, hue=0.0, contrast=1.0):
    """augment's affine colour map u = M t + o on (B, G, R), composed in float64: a saturation about the grey 0.114 B + 0.587 G +
    0.299 R, then a rotation by `hue` (radians) about the grey axis B = G = R, then a contrast about 127.5.  -> (M (3, 3), o (3,))
    float64; (1, 0, 1) gives the identity and a zero offset exactly."""
    s, th, k = float(saturation), float(hue), float(contrast)
    if not all(np.isfinite(v) for v in (s, th, k)):
        raise ValueError(f"saturation, hue, contrast: finite numbers are expected, got {(saturation, hue, contrast)!r}")
    eye, ones = np.eye(3), np.ones((3, 3))
    S = s * eye + (1.0 - s) * ones * np.asarray(GREY_BGR)[None, :]
    c, sn = np.cos(th), np.sin(th)
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    R = c * eye + ((1.0 - c) / 3.0) * ones + (sn / np.sqrt(3.0)) * K
    RS = R[:, 0:1] * S[0:1, :] + R[:, 1:2] * S[1:2, :] + R[:, 2:3] * S[2:3, :]       # (element-wise: no BLAS, the same bits everywhere)
    return k * RS, np.full(3, 127.5 * (1.0 - k))


def augment(frame, blur_sigma=0.0, saturation=1.0, hue=0.0, contrast=1.0, noise_sigma=0.0, seed=0, want_f32=False):
    """Photometric augmentation of a device frame ((H, W, 3) uint8 or float32, B, G, R), in one launch: a Gaussian blur
    (blur_taps(blur_sigma), replicate border), the colour map colour_matrix(saturation, hue, contrast) (left out when it is the
    identity), noise of standard deviation noise_sigma that is a function of (seed, pixel, channel), rounding.  -> the uint8
    frame; with want_f32: (uint8 frame, the un-rounded float32 one).  A uint8 frame is converted to float32 first (one torch
    op); a float32 one, such as render_pair's un-rounded output, is read as it is and left unchanged."""
    if not isinstance(frame, torch.Tensor) or frame.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"frame: a uint8 or float32 device tensor is expected, got {getattr(frame, 'dtype', type(frame).__name__)}")
    if not frame.is_cuda:
        raise ValueError(f"frame: a device tensor is expected, got a tensor on {frame.device}")
    if frame.dim() != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError(f"frame: shape (H, W, 3) is expected, got {tuple(frame.shape)}")
    taps = blur_taps(blur_sigma)
    M, o = colour_matrix(saturation, hue, contrast)
    noise_sigma, seed = float(noise_sigma), int(seed)
    if not (0.0 <= noise_sigma < float("inf")):
        raise ValueError(f"noise_sigma: a finite number >= 0 is expected, got {noise_sigma!r}")
    if not (0 <= seed < 1 << 32):
        raise ValueError(f"seed: 0 <= seed < 2^32 is expected, got {seed!r}")
    identity = np.array_equal(M, np.eye(3)) and not o.any()
    colour = None if identity else np.concatenate([M.ravel(), o]).astype(np.float32)
    src = frame.contiguous() if frame.dtype == torch.float32 else frame.float().contiguous()
    out_u8 = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    out_f32 = torch.empty_like(src) if want_f32 else None
    ops.hsynth_augment(src, taps, colour, noise_sigma, seed, out_u8, out_f32)
    return (out_u8, out_f32) if want_f32 else out_u8


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
    shorter one, centred anywhere in the frame), one gain and one bias for all channels from gain_range and bias_range.

    Opt-in, all off by default (then a sample is the launches and the bytes it was without them): `backgrounds`, a list of uint8
    (hb, wb, 3) images of at least 2 x 2 pixels, one of which is put behind the plane through a random similarity times a
    random_homography of it that keeps the frame covered; `blur_sigma`, `noise_sigma`, `saturation`, `hue`, `contrast`, (low,
    high) ranges drawn uniformly for `augment` of dst (render_pair's un-rounded frame is augmented: the render's own uint8 is not
    the sample's dst); `augment_src`: src goes through `augment` too, with the same blur, its own noise seed and no colour
    change.  These draws come from a RandomState of their own, numpy.random.RandomState([seed, i, epoch, 0xA06]): H_gt, the
    occluders, gain and bias -- and with them flow_gt, visible and valid -- are what they are without the new keywords."""

    def __init__(self, images, occluder_textures=None, seed=0, max_shift=0.2, n_occluders=(0, 2), gain_range=(0.8, 1.2),
                 bias_range=(-20, 20), lo=0.25, hi=0.75, backgrounds=None, blur_sigma=(0, 0), noise_sigma=(0, 0),
                 saturation=(1, 1), hue=(0, 0), contrast=(1, 1), augment_src=False):
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
        self.backgrounds = [_device_u8(b, f"backgrounds[{k}]", 3) for k, b in enumerate(backgrounds or [])]
        for k, b in enumerate(self.backgrounds):
            if min(b.shape[:2]) < 2:
                raise ValueError(f"backgrounds[{k}]: an image of at least 2 x 2 pixels is expected, got {tuple(b.shape[:2])}")

        def span(v, what, least):
            v = tuple(float(x) for x in v)
            if len(v) != 2 or not (least <= v[0] <= v[1] < float("inf")):
                raise ValueError(f"{what}: a finite (low, high) with {least} <= low <= high is expected, got {v!r}")
            return v
        self.blur_sigma = span(blur_sigma, "blur_sigma", 0.0)
        self.noise_sigma = span(noise_sigma, "noise_sigma", 0.0)
        self.saturation = span(saturation, "saturation", -float("inf"))
        self.hue = span(hue, "hue", -float("inf"))
        self.contrast = span(contrast, "contrast", -float("inf"))
        self.augment_src = bool(augment_src)
        self.augmented = bool(self.backgrounds) or self.augment_src or self.blur_sigma != (0.0, 0.0) \
            or self.noise_sigma != (0.0, 0.0) or self.saturation != (1.0, 1.0) or self.hue != (0.0, 0.0) \
            or self.contrast != (1.0, 1.0)

    def __len__(self):
        return len(self.images)

    def draw(self, i, epoch=0):
        """The random part of sample (i, epoch), on the host: (H_gt, [(texture index, H_occ)], gain, bias), and with any of the
        background / augmentation keywords on a fifth field, an HSynthAugment (background index or None, background_H or None,
        blur_sigma, saturation, hue, contrast, noise_sigma, seed_dst, seed_src)."""
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
        if not self.augmented:
            return H_gt, occ, gain, bias
        return H_gt, occ, gain, bias, self._draw_augment(np.random.RandomState([self.seed, i, epoch, 0xA06]), h, w)

    def _draw_augment(self, rs, h, w):
        b, H_bg = None, None
        if self.backgrounds:
            b = int(rs.randint(0, len(self.backgrounds)))
            hb, wb = self.backgrounds[b].shape[:2]
            # the bent background holds its rectangle inset by the corners' largest move, and that the disc of radius `inner`
            # about its centre; scaled to at least the frame's half diagonal and moved by no more than the excess, the disc covers
            # the frame under any rotation
            shift = min(self.max_shift, 0.2)
            bend = random_homography(rs, hb, wb, shift)
            inner = 0.5 * (min(hb, wb) - 1.0) - shift * min(hb, wb)
            outer = 0.5 * float(np.hypot(h - 1.0, w - 1.0))
            s = max(outer, 0.5) / inner * rs.uniform(1.0, 1.5)
            a = rs.uniform(0.0, 2.0 * np.pi)
            slack = (s * inner - outer) / np.sqrt(2.0)
            cx, cy = (w - 1) / 2.0 + rs.uniform(-slack, slack), (h - 1) / 2.0 + rs.uniform(-slack, slack)
            ca, sa = s * np.cos(a), s * np.sin(a)
            tx, ty = (wb - 1) / 2.0, (hb - 1) / 2.0
            place = np.array([[ca, -sa, cx - ca * tx + sa * ty], [sa, ca, cy - sa * tx - ca * ty], [0.0, 0.0, 1.0]])
            H_bg = place @ bend
        scalars = [float(rs.uniform(*r)) for r in (self.blur_sigma, self.saturation, self.hue, self.contrast, self.noise_sigma)]
        seed_dst, seed_src = (int(v) for v in rs.randint(0, 1 << 32, 2, dtype=np.uint64))
        return HSynthAugment(b, H_bg, *scalars, seed_dst, seed_src)

    def sample(self, i, epoch=0):
        H_gt, occ, gain, bias, *aug = self.draw(i, epoch)
        src = self.images[int(i)]
        occluders = [(self.textures[t], H_occ) for t, H_occ in occ]
        flow, visible, valid = pair_labels(src.shape[:2], H_gt, occluders, lo=self.lo, hi=self.hi)
        if not aug:
            dst = render_pair(src, H_gt, occluders, gain=gain, bias=bias)
            return HSynthSample(src, dst, H_gt, flow, visible, valid)
        a = aug[0]
        bg = None if a.background is None else self.backgrounds[a.background]
        f32 = render_pair(src, H_gt, occluders, gain=gain, bias=bias, want_f32=True, background=bg, background_H=a.background_H)[1]
        dst = augment(f32, a.blur_sigma, a.saturation, a.hue, a.contrast, a.noise_sigma, a.seed_dst)
        if self.augment_src:
            src = augment(src, blur_sigma=a.blur_sigma, noise_sigma=a.noise_sigma, seed=a.seed_src)
        return HSynthSample(src, dst, H_gt, flow, visible, valid)

    def __getitem__(self, i):
        return self.sample(i, 0)
