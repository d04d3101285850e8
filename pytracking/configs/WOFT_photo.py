"""WOFT with a photometric refinement of every re-detected frame's pose (`photo_refine` = the Gauss-Newton iteration count): the
homography fitted to the flow correspondences is aligned to the frame's pixels before it becomes the tracker's pose.  Further keys,
all optional: `photo_gain_bias` (True), `photo_huber_k` (None; grey levels), `photo_stride` (1), `photo_min_valid` (0.5),
`photo_eps` (1e-3 px), `photo_blur_sigma` (0: no pre-blur).  The reference's tracker has no such stage: the keys are this project's."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.photo_refine = 10
    return conf
