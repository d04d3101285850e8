"""WOFT on multi-delta chained flow whose photometric refinement is weighted by the chains' visibility (`chain_photo_weights`):
WOFT_chained_photo.py plus the key.  Per frame one launch (woft_photo_weights) turns the fold's cost and visibility into a weight
map on the template -- 'gate': 1 where the chain is valid and visible (vis >= `chain_vis_thr`), 0 elsewhere; 'soft': exp(-cost) * vis
there -- eroded by `chain_photo_erode` pixels (1), so that the refinement does not align occluded pixels to the occluder.  A target
with less than `chain_photo_min_support` (0.25: a configurable default, not a tuned value) of its mask left keeps the fit's pose
(meta.photo.status 'LOW_SUPPORT')."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained_photo.py')
    conf.chain_photo_weights = 'gate'
    return conf
