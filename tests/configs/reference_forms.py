"""The reference's own tracker config files, restated in their form, selected by get_config(kind): the callables shape their
inputs with einops, log at DEBUG level, define the IRLS re-weighting as a nested function and import the library through
the reference's paths only (no woft_amd import, no tags, flow config without a `precision` key).
  "wlsq"             configs/WOFT.py (= ..._noreliableinl_wLSq.py): weighted LSq, 20 % inliers within 5 px
  "wlsq_downscale2"  configs/WOFT_downscale_2x.py: the same on inputs downscaled 2x, padding mode 'RAFT'
  "wirls"            configs/..._noreliableinl_wIRLSq.py (ablation_08.py is the same file): IRLS, Huber k = 2
  "plain"            configs/..._noreliableinl_plainLSq.py: the estimator hands the library weights=None
  "always_wlsq"      configs/..._alwayswarp_wLSq.py: weighted LSq, the re-detection test is `return True`
  "never_plain"      configs/..._neverwarp_plainLSq.py: weights=None, the re-detection test is `return False`"""
import logging
from pathlib import Path

import einops
import numpy as np
import torch

from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
from pytracking.utils.config import Config, load_config
from pytracking.utils.least_squares_H import (IRLSq_Huber, find_homography_IRLSq_QR, find_homography_nonhomogeneous_QR,
                                              torch_proj_errors)

logger = logging.getLogger(__name__)

KINDS = ("wlsq", "wlsq_downscale2", "wirls", "plain", "always_wlsq", "never_plain")


def inlier_test(H_prewarped2init, template_coords, cur_pw_coords, weights):
    errs = torch_proj_errors(H_prewarped2init,
                             einops.rearrange(cur_pw_coords, 'xy N -> 1 xy N', xy=2),
                             einops.rearrange(template_coords, 'xy N -> 1 xy N', xy=2))
    frac = torch.mean((errs <= 5).float())
    logger.debug(f"inlier fraction {frac}")
    return frac > 0.2


def always(H_prewarped2init, template_coords, cur_pw_coords, weights):
    return True


def never(H_prewarped2init, template_coords, cur_pw_coords, weights):
    return False


def weighted_lsq(pts_A, pts_B, weights=None):
    logger.debug(f"{pts_A.shape[1]} correspondences")
    return find_homography_nonhomogeneous_QR(pts_A, pts_B, weights=weights)


def plain_lsq(pts_A, pts_B, weights=None):
    logger.debug(f"{pts_A.shape[1]} correspondences")
    return find_homography_nonhomogeneous_QR(pts_A, pts_B, weights=None)


def weighted_irls(pts_A, pts_B, weights=None):
    logger.debug(f"{pts_A.shape[1]} correspondences")

    def huber(residuals):
        return IRLSq_Huber(residuals, k=2)
    return find_homography_IRLSq_QR(pts_A, pts_B, weights=weights, reweighting_fn=huber)


def sobol_500(coords_a, coords_b, weights):
    assert coords_a.shape == coords_b.shape
    n = coords_a.shape[1]
    assert weights.shape == (1, n)
    if n <= 500:
        return coords_a, coords_b, weights
    keep = np.zeros(n) > 0
    u = torch.quasirandom.SobolEngine(dimension=1).draw(500).cpu().numpy().flatten()
    keep[np.round(n * u).astype(np.int32)] = True
    return coords_a[:, keep], coords_b[:, keep], weights[:, keep]


def get_config(kind="wlsq"):
    estimator, redetection = {"wlsq": (weighted_lsq, inlier_test), "wlsq_downscale2": (weighted_lsq, inlier_test),
                              "wirls": (weighted_irls, inlier_test), "plain": (plain_lsq, inlier_test),
                              "always_wlsq": (weighted_lsq, always), "never_plain": (plain_lsq, never)}[kind]
    root = Path(__file__).resolve().parents[2]
    conf = Config()
    conf.tracker_class = YAOFTrackerSingleControl
    conf.flow_config = load_config(root / 'pytracking' / 'optical_flow' / 'configs' / 'v2_SNOB_large_g05_RAFT.py')
    del conf.flow_config.precision             # a reference flow config has no such key
    conf.flow_config.weights_postprocessing_fn = None
    if kind == "wlsq_downscale2":
        conf.flow_config.padding_mode = 'RAFT'
    conf.flow_numpy_out = False
    conf.H_estimator = estimator
    conf.redet_success_fn = redetection
    conf.pw_mask = True
    conf.no_prewarp_after_N = 10
    conf.subsampler_fn = sobol_500
    if kind == "wlsq_downscale2":
        conf.downscale_inputs = 2
    return conf
