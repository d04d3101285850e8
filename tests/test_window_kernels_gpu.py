"""The search-window kernels (csrc/window.hip) against what they replace, EXACTLY: the windowed warp against the full-frame kernel's
output sliced, the rectangle copy against a torch slice, the mask bounding box against numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import ops  # noqa: E402
from woft_amd.window import Box  # noqa: E402
import geometry_cases as G  # noqa: E402

H, W = 123, 157                      # odd on purpose
HOMOGRAPHIES = {
    "identity": np.eye(3),
    "mild": np.array([[1.01, 0.02, 3.4], [-0.015, 0.99, -2.2], [1e-5, -2e-5, 1.0]]),
    "strong": np.array([[0.8, 0.35, 20.0], [-0.3, 1.2, -15.0], [1.5e-3, -1e-3, 1.0]]),
}
WINDOWS = {"whole": (0, 0, H, W), "top-left": (0, 0, 40, 33), "top-right": (0, W - 51, 47, 51), "bottom-left": (H - 30, 0, 30, 64),
           "bottom-right": (H - 61, W - 17, 61, 17), "inner": (31, 42, 57, 71), "one-pixel": (H - 1, W - 1, 1, 1),
           "one-row": (60, 0, 1, W), "exclusive-crop": (0, 0, H - 1, W - 1)}


def _image(c, seed=0):
    rs = np.random.RandomState(seed)
    shape = (H, W) if c == 1 else (H, W, c)
    return torch.from_numpy(rs.randint(0, 256, shape).astype(np.uint8)).cuda()


def _check_windows_against_full_frame(img, Hm, nearest, what):
    """Every window of WINDOWS == the full-frame kernel's output sliced; and either output alone.  -> the full-frame validity."""
    full, full_valid = torch.empty_like(img), torch.empty((H, W), dtype=torch.uint8, device="cuda")
    ops.warp_perspective_u8(img, Hm, full, full_valid, nearest=nearest)
    for name, (y0, x0, rows, cols) in WINDOWS.items():
        out = torch.full((rows, cols) + tuple(img.shape[2:]), 77, dtype=torch.uint8, device="cuda")
        valid = torch.full((rows, cols), 77, dtype=torch.uint8, device="cuda")
        ops.warp_perspective_window_u8(img, Hm, (y0, x0, rows, cols), out, valid, nearest=nearest)
        assert torch.equal(out, full[y0:y0 + rows, x0:x0 + cols]), (what, nearest, name)
        assert torch.equal(valid, full_valid[y0:y0 + rows, x0:x0 + cols]), (what, nearest, name)
    # either output alone (bilinear: validity only / image only)
    y0, x0, rows, cols = WINDOWS["inner"]
    out = torch.empty((rows, cols) + tuple(img.shape[2:]), dtype=torch.uint8, device="cuda")
    ops.warp_perspective_window_u8(img, Hm, WINDOWS["inner"], out, None, nearest=nearest)
    assert torch.equal(out, full[y0:y0 + rows, x0:x0 + cols])
    if not nearest:
        valid = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        ops.warp_perspective_window_u8(img, Hm, WINDOWS["inner"], None, valid)
        assert torch.equal(valid, full_valid[y0:y0 + rows, x0:x0 + cols])
    return full_valid


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hname", list(HOMOGRAPHIES))
def test_windowed_warp_is_the_full_warp_sliced(hname, c, nearest):
    full_valid = _check_windows_against_full_frame(_image(c, seed=c), HOMOGRAPHIES[hname], nearest, (hname, c))
    assert int(full_valid.sum()) > 0


# Where the shared per-pixel arithmetic has its edges (test_image_geometry_gpu pins the full-frame kernel there independently): a
# horizon inside the frame, a denominator of exactly 0.0, a frame carried wholly outside, source coordinates on integers and on
# half-integers.
EDGE_HOMOGRAPHIES = {
    "horizon": G.GENERIC["horizon"],
    "horizon-inv": G.GENERIC["horizon-inv"],
    "dzero": G.dzero(H, W)[0],
    "far": G.FAR,
    "shift(-7,2)": G.translation(-7, 2),
    "half(-2.5,3.5)": G.translation(-2.5, 3.5),
}


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hname", list(EDGE_HOMOGRAPHIES))
def test_windowed_warp_is_the_full_warp_sliced_at_the_edges(hname, c, nearest):
    full_valid = _check_windows_against_full_frame(_image(c, seed=c), EDGE_HOMOGRAPHIES[hname], nearest, (hname, c))
    assert (int(full_valid.sum()) == 0) == (hname == "far")
    if hname == "dzero":
        assert np.array_equal(np.linalg.inv(EDGE_HOMOGRAPHIES[hname]), G.dzero(H, W)[1])
        ys, xs = np.mgrid[0:H, 0:W]
        assert not full_valid.cpu().numpy()[xs + ys == G.dzero(H, W)[2]].any()


@pytest.mark.parametrize("c", [1, 3, 4])
def test_rectangle_copy_is_a_torch_slice(c):
    img = _image(c, seed=10 + c)
    for name, (y0, x0, rows, cols) in WINDOWS.items():
        got = ops.crop_u8(img, (y0, x0, rows, cols))
        want = img[y0:y0 + rows, x0:x0 + cols].contiguous()
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want), (c, name)
    big = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)).cuda()
    assert torch.equal(ops.crop_u8(big, (135, 241, 809, 1437)), big[135:135 + 809, 241:241 + 1437].contiguous())


def _np_bbox(m):
    b = Box.from_mask(m)
    return [int(b.tl_y), int(b.br_y), int(b.tl_x), int(b.br_x), int(bool(np.any(m)))]


def test_mask_bounding_box_is_numpys():
    rs = np.random.RandomState(5)
    masks = []
    for (h, w) in [(123, 157), (64, 64), (1, 1), (7, 333), (333, 7), (1080, 1920), (257, 1023)]:
        z = np.zeros((h, w), np.uint8)
        masks.append(z.copy())                                             # empty
        masks.append(np.full((h, w), 255, np.uint8))                       # full
        for _ in range(3):                                                 # single pixels, corners included
            m = z.copy()
            m[rs.randint(h), rs.randint(w)] = rs.randint(1, 256)
            masks.append(m)
        for y, x in ((0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)):
            m = z.copy()
            m[y, x] = 1
            masks.append(m)
        for _ in range(4):                                                 # random blobs (a few rectangles and specks)
            m = z.copy()
            for _ in range(rs.randint(1, 4)):
                y0, x0 = rs.randint(h), rs.randint(w)
                m[y0:y0 + rs.randint(1, max(2, h // 3)), x0:x0 + rs.randint(1, max(2, w // 3))] = 255
            masks.append(m)
    ws = ops.mask_bbox_ws()
    for i, m in enumerate(masks):
        t = torch.from_numpy(m).cuda()
        got = ops.mask_bbox(t, ws=ws).cpu().tolist()
        assert got == _np_bbox(m), (i, m.shape, got, _np_bbox(m))
        assert int(ws.view(torch.int32).abs().sum()) == 0                 # the scratch is left zeroed
    # an unaligned mask (a view one byte into a buffer): the byte path
    buf = torch.zeros(50 * 61 + 1, dtype=torch.uint8, device="cuda")
    m = np.zeros((50, 61), np.uint8)
    m[11:30, 5:44] = 9
    buf[1:].copy_(torch.from_numpy(m).reshape(-1))
    assert ops.mask_bbox(buf[1:].view(50, 61), ws=ws).cpu().tolist() == _np_bbox(m)


@pytest.mark.parametrize("hname", list(HOMOGRAPHIES))
def test_fused_mask_warp_and_bounding_box(hname):
    """The carried template mask and its box in one launch == the nearest-neighbour warp kernel followed by numpy."""
    Hm = HOMOGRAPHIES[hname]
    m = np.zeros((H, W), np.uint8)
    m[30:90, 40:120] = 255
    t = torch.from_numpy(m).cuda()
    want = torch.empty_like(t)
    ops.warp_perspective_u8(t, Hm, want, None, nearest=True)
    warped = torch.full_like(t, 77)
    got = ops.mask_bbox(t, Hmat=Hm, warped=warped).cpu().tolist()
    assert torch.equal(warped, want)
    assert got == _np_bbox(want.cpu().numpy())
    assert ops.mask_bbox(t, Hmat=Hm).cpu().tolist() == got                 # without materialising the warped mask
    far = np.array([[1, 0, 10000.0], [0, 1, 0], [0, 0, 1.0]])              # carried out of the frame: the all-zero case
    assert ops.mask_bbox(t, Hmat=far).cpu().tolist() == [0, 0, 0, 0, 0]
