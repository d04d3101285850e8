"""Numpy restatement of the two warm-start operations (csrc/warm.hip), the rule the kernels are tested against:
brute force, fp64, lowest point index on a tie.  No device, no scipy."""
import numpy as np


def coords_init_flow(flow_init):
    """(2, hf, wf) fp32 -> (coords (P, 2) fp32 = grid + flow_init in ONE fp32 add each, flow (P, 2) = flow_init itself)."""
    f = np.asarray(flow_init, np.float32)
    _, hf, wf = f.shape
    ys, xs = np.mgrid[:hf, :wf]
    coords = np.stack([xs.astype(np.float32) + f[0], ys.astype(np.float32) + f[1]], -1).reshape(-1, 2)
    return coords.astype(np.float32), np.stack([f[0], f[1]], -1).reshape(-1, 2)


def forward_interpolate(flow):
    """(2, hf, wf) fp32 -> (2, hf, wf) fp32.  Point i (row-major) lands at (x0 + dx, y0 + dy) in fp64 and is valid iff
    0 < x1 < wf and 0 < y1 < hf (strictly); every cell takes (dx, dy) of the valid point with the smallest squared distance
    ddx*ddx + ddy*ddy (fp64), the lowest index among equals (np.argmin returns the first); no valid point: zeros."""
    f = np.asarray(flow, np.float32)
    _, hf, wf = f.shape
    ys, xs = np.mgrid[:hf, :wf]
    dx, dy = f[0].reshape(-1), f[1].reshape(-1)
    x1 = xs.reshape(-1).astype(np.float64) + dx.astype(np.float64)
    y1 = ys.reshape(-1).astype(np.float64) + dy.astype(np.float64)
    valid = (x1 > 0) & (x1 < wf) & (y1 > 0) & (y1 < hf)
    out = np.zeros_like(f)
    if not valid.any():
        return out
    cx, cy = xs.reshape(-1, 1).astype(np.float64), ys.reshape(-1, 1).astype(np.float64)
    ddx, ddy = cx - x1[None], cy - y1[None]
    d = ddx * ddx + ddy * ddy
    d[:, ~valid] = np.inf
    best = np.argmin(d, axis=1)
    out[0], out[1] = dx[best].reshape(hf, wf), dy[best].reshape(hf, wf)
    return out
