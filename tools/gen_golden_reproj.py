"""Generate the projection-error fixture tests/golden/reproj_errors.npz by running the REFERENCE itself.

Run only where the reference checkout is present (the tests read the fixture, never the reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_reproj.py

Uses oracle.gen_golden's stubs unchanged (kornia's two homogeneous conversions are the restatements of oracle/hfit_ref.py
there: their parity stays unpinned, everything around them is the reference's own code).  The fixture holds one seeded case --
4 homographies (ground truth and a perturbed estimate each), 16 points -- and what the reference's torch_reproj_errors,
torch_proj_diff_errors, torch_H_proj, torch_e2p, torch_p2e (float32, batched) and reproj_errors (float64 numpy, per
homography pair, mean and per point) return for it.  Arrays only.
"""
import sys
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle.gen_golden import GOLD, install_stubs  # noqa: E402

B, N, BOX, SEED = 4, 16, 16.0, 20


def make_case(seed=SEED, batch=B, n=N, box=BOX):
    """-> GT_H, est_H (batch, 3, 3) float64 and pts (batch, 2, n) float64: points in [0, box]^2, homographies a few per cent
    from the identity with a translation of up to half a pixel, the estimate a perturbation of the ground truth of half that
    size.  Small and well conditioned on purpose: the tests hold a float32 evaluation to an absolute 1e-4 px, and float32
    rounds relative to the coordinates and to the condition number of the inverted homography."""
    rs = np.random.RandomState(seed)
    eye = np.eye(3)[None]
    scale = np.array([[0.05, 0.05, 0.5], [0.05, 0.05, 0.5], [2e-4, 2e-4, 0.0]])[None]
    gt = eye + scale * rs.uniform(-1, 1, (batch, 3, 3))
    est = gt + 0.5 * scale * rs.uniform(-1, 1, (batch, 3, 3))
    pts = rs.uniform(0.0, box, (batch, 2, n))
    return gt, est, pts


def main():
    install_stubs()
    import pytracking.utils.least_squares_H as L
    gt, est, pts = make_case()
    f = lambda x: torch.from_numpy(x.astype(np.float32))
    G, E, P = f(gt), f(est), f(pts)
    out = dict(seed=SEED, GT_H=G.numpy(), est_H=E.numpy(), pts=P.numpy())
    out["torch_reproj_errors"] = L.torch_reproj_errors(G, E, P).numpy()
    out["torch_proj_diff_errors"] = L.torch_proj_diff_errors(G, E, P).numpy()
    out["torch_H_proj"] = L.torch_H_proj(G, P).numpy()
    out["torch_e2p"] = L.torch_e2p(P).numpy()
    out["torch_p2e"] = L.torch_p2e(torch.matmul(G, L.torch_e2p(P))).numpy()
    # the numpy helper takes one homography pair and (2, N) points, in float64 (the float32 inputs above, widened)
    g64, e64, p64 = (out[k].astype(np.float64) for k in ("GT_H", "est_H", "pts"))
    out["reproj_errors_mean"] = np.array([L.reproj_errors(g64[b].copy(), e64[b].copy(), p64[b].copy()) for b in range(B)])
    out["reproj_errors_all"] = np.stack([L.reproj_errors(g64[b].copy(), e64[b].copy(), p64[b].copy(), mean=False)
                                         for b in range(B)])
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
    p = GOLD / "reproj_errors.npz"
    np.savez_compressed(p, **out)
    print(f"{p.name:40s} {p.stat().st_size / 1024:9.1f} KB")


if __name__ == "__main__":
    main()
