"""Host restatement of the backward of the weighted least-squares homography fit (woft_amd/csrc/hfit.hip `hfit_bwd_one`; a
helper of the backward tests, not a conftest): float64 numpy, written as plainly as possible, stage by stage as DESIGN.md
section 15 states them.  `forward` is the fit itself (Hartley normalisation, the rows of build_rows, normal equations, H = T2^-1
Hn T1, H / (H33 + 1e-8)); `backward` returns the gradients of sum(gout * H_out) with respect to both point sets and the
weights.  One element at a time: a, b (N, 2), w (N,) or None, gout (3, 3)."""
import numpy as np

EPS = 1e-8


def _normalise(p):
    m = p.mean(axis=0)
    c = p - m
    d = np.sqrt((c * c).sum(axis=1))
    dbar = d.mean()
    s = np.sqrt(2.0) / (dbar + EPS)
    T = np.array([[s, 0.0, -s * m[0]], [0.0, s, -s * m[1]], [0.0, 0.0, 1.0]])
    return s * c, T, (m, c, d, dbar, s)


def _rows(p1, p2):
    """Unweighted rows: A (N, 2, 8), b (N, 2); row 0 is the x-row, row 1 the y-row of build_rows."""
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    n = len(x1)
    A = np.zeros((n, 2, 8))
    bb = np.zeros((n, 2))
    A[:, 0, 3], A[:, 0, 4], A[:, 0, 5], A[:, 0, 6], A[:, 0, 7] = -x1, -y1, -1.0, y2 * x1, y2 * y1
    bb[:, 0] = -y2
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2], A[:, 1, 6], A[:, 1, 7] = x1, y1, 1.0, -x2 * x1, -x2 * y1
    bb[:, 1] = x2
    return A, bb


def _solve(a, b, w):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = a.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, np.float64).reshape(n)
    p1, T1, st1 = _normalise(a)
    p2, T2, st2 = _normalise(b)
    A, bb = _rows(p1, p2)
    At = (wv[:, None, None] * A).reshape(2 * n, 8)
    bt = (wv[:, None] * bb).reshape(2 * n)
    G = At.T @ At
    x = np.linalg.solve(G, At.T @ bt)
    Hn = np.append(x, 1.0).reshape(3, 3)
    T2i = np.linalg.inv(T2)
    H = T2i @ Hn @ T1
    return dict(n=n, wv=wv, p1=p1, p2=p2, T1=T1, T2=T2, st1=st1, st2=st2, A=A, bb=bb, At=At, bt=bt, G=G, x=x, Hn=Hn, T2i=T2i, H=H)


def forward(a, b, w=None):
    """-> H_out (3, 3) float64."""
    f = _solve(a, b, w)
    return f["H"] / (f["H"][2, 2] + EPS)


def _through_normalisation(gpn, gT, st):
    """Stage (e): gradient of the points from the gradient of the normalised points gpn (N, 2) and of T (3, 3)."""
    m, c, d, dbar, s = st
    n = c.shape[0]
    gs = (gpn * c).sum() + gT[0, 0] + gT[1, 1] - gT[0, 2] * m[0] - gT[1, 2] * m[1]
    g_dbar = -gs * s / (dbar + EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(d[:, None] > 0.0, c / d[:, None], 0.0)          # torch's sub-gradient of norm at 0
    gd = s * gpn + (g_dbar / n) * unit
    return gd - gd.mean(axis=0) + np.array([-s * gT[0, 2], -s * gT[1, 2]]) / n


def backward(a, b, w, gout):
    """-> (gpa (N, 2), gpb (N, 2), gw (N,) or None when w is None)."""
    f = _solve(a, b, w)
    n, wv, x, H, Hn, T1, T2i = f["n"], f["wv"], f["x"], f["H"], f["Hn"], f["T1"], f["T2i"]
    gout = np.asarray(gout, np.float64).reshape(3, 3)
    # (a) out = H / (H33 + eps)
    den = H[2, 2] + EPS
    gH = gout / den
    gH[2, 2] -= (gout * H).sum() / den ** 2
    # (b) H = T2^-1 Hn T1
    gHn = T2i.T @ gH @ T1.T
    gT1 = (T2i @ Hn).T @ gH
    gT2 = -T2i.T @ (gH @ (Hn @ T1).T) @ T2i.T
    gx = gHn.reshape(9)[:8]
    # (c) adjoint solve
    u = np.linalg.solve(f["G"], gx)
    # (d) per correspondence, on the weighted rows
    At, bt = f["At"].reshape(n, 2, 8), f["bt"].reshape(n, 2)
    r = At @ x - bt                                             # (N, 2)
    v = At @ u
    gAt = -(r[:, :, None] * u[None, None, :] + v[:, :, None] * x[None, None, :])      # (N, 2, 8)
    gbt = v
    gw = (gAt * f["A"]).sum(axis=(1, 2)) + (gbt * f["bb"]).sum(axis=1)
    gA, gb = wv[:, None, None] * gAt, wv[:, None] * gbt
    x1, y1, x2, y2 = f["p1"][:, 0], f["p1"][:, 1], f["p2"][:, 0], f["p2"][:, 1]
    gp1 = np.stack([-gA[:, 0, 3] + y2 * gA[:, 0, 6] + gA[:, 1, 0] - x2 * gA[:, 1, 6],
                    -gA[:, 0, 4] + y2 * gA[:, 0, 7] + gA[:, 1, 1] - x2 * gA[:, 1, 7]], axis=1)
    gp2 = np.stack([-x1 * gA[:, 1, 6] - y1 * gA[:, 1, 7] + gb[:, 1],
                    x1 * gA[:, 0, 6] + y1 * gA[:, 0, 7] - gb[:, 0]], axis=1)
    # (e) p_n = s (p - m), T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]
    gpa = _through_normalisation(gp1, gT1, f["st1"])
    gpb = _through_normalisation(gp2, gT2, f["st2"])
    return gpa, gpb, (None if w is None else gw)


def case(n, seed, batch=1):
    """Seeded test case in the conditions the backward tests are stated for: points in [100, 1800] x [80, 1000] (N < 7: near
    the corners and the centre of that box, in general position), a homography within 5 % of the identity per element, 0.5 px
    noise, 10 % outliers of 30 px (rounded up: N = 7 has one, without it the weight gradient is all cancellation and the float32
    oracle is 1e-4 .. 1e-3 from float64), weights in [0.05, 0.95], a full random gout.  -> float32 a, b (B, N, 2), w (B, N),
    gout (B, 3, 3)."""
    rs = np.random.RandomState(seed)
    a = np.stack([rs.uniform(100, 1800, (batch, n)), rs.uniform(80, 1000, (batch, n))], -1)
    if n < 7:
        cx = np.array([200.0, 1700.0, 1600.0, 150.0, 900.0, 500.0, 1300.0])[:n]
        cy = np.array([100.0, 180.0, 950.0, 900.0, 500.0, 300.0, 700.0])[:n]
        a = np.stack([cx, cy], -1)[None] + rs.uniform(-40, 40, (batch, n, 2))
    H = np.eye(3)[None] + rs.uniform(-1, 1, (batch, 3, 3)) * np.array([[0.05, 0.05, 20.0], [0.05, 0.05, 20.0], [2e-5, 2e-5, 0.0]])
    ah = np.concatenate([a, np.ones((batch, n, 1))], -1) @ H.transpose(0, 2, 1)
    b = ah[..., :2] / ah[..., 2:] + rs.normal(0, 0.5, (batch, n, 2))
    no = -(-n // 10)
    ang = rs.uniform(0, 2 * np.pi, (batch, no))
    b[:, :no] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], -1)
    w = rs.uniform(0.05, 0.95, (batch, n))
    gout = rs.normal(0, 1, (batch, 3, 3))
    return a.astype(np.float32), b.astype(np.float32), w.astype(np.float32), gout.astype(np.float32)
