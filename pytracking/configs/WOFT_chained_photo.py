"""WOFT on multi-delta chained flow with a photometric refinement of every fitted frame's pose (`chain_photo_refine` = the
Gauss-Newton iteration count): WOFT_chained.py plus the key.  The homography fitted to the chains' correspondences at 1/8
resolution is aligned to the frame's pixels before it becomes the tracker's pose.  Further keys, all optional, the meaning and
defaults of WOFT_photo.py's: `chain_photo_gain_bias`, `chain_photo_huber_k`, `chain_photo_stride`, `chain_photo_min_valid`,
`chain_photo_eps`, `chain_photo_blur_sigma`."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained.py')
    conf.chain_photo_refine = 10
    return conf
