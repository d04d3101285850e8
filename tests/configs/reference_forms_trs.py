"""A tracker config that fits the RANSAC similarity (least_squares_H.py:349-363, find_homography_TRS), written in the form of
the reference's configs: the callables are defined inline, shape their inputs with einops and log at DEBUG level, the estimator
hands the library its weights (the library takes no other parameter in the reference), the library is imported through the
reference's paths only (no woft_amd import, no tags, flow config without a `precision` key)."""
import logging
from pathlib import Path

import einops
import numpy as np
import torch

from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
from pytracking.utils.config import Config, load_config
from pytracking.utils.least_squares_H import find_homography_TRS, torch_proj_errors

logger = logging.getLogger(__name__)


def inlier_test(H_prewarped2init, template_coords, cur_pw_coords, weights):
    errs = torch_proj_errors(H_prewarped2init,
                             einops.rearrange(cur_pw_coords, 'xy N -> 1 xy N', xy=2),
                             einops.rearrange(template_coords, 'xy N -> 1 xy N', xy=2))
    frac = torch.mean((errs <= 5).float())
    logger.debug(f"inlier fraction {frac}")
    return frac > 0.2


def find_homography(pts_A, pts_B, weights=None):
    logger.debug(f"{pts_A.shape[1]} correspondences")
    return find_homography_TRS(pts_A, pts_B, weights=weights)


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


def get_config():
    root = Path(__file__).resolve().parents[2]
    conf = Config()
    conf.tracker_class = YAOFTrackerSingleControl
    conf.flow_config = load_config(root / 'pytracking' / 'optical_flow' / 'configs' / 'v2_SNOB_large_g05_RAFT.py')
    del conf.flow_config.precision             # a reference flow config has no such key
    conf.flow_config.weights_postprocessing_fn = None
    conf.flow_numpy_out = False
    conf.H_estimator = find_homography
    conf.redet_success_fn = inlier_test
    conf.pw_mask = True
    conf.no_prewarp_after_N = 10
    conf.subsampler_fn = sobol_500
    return conf
