"""WOFT on multi-delta chained flow (this project's own tracker, no counterpart in the reference): per frame the flows of
`chain_deltas` -- None = template -> frame, d = frame t-d -> frame t chained onto the stored result of frame t-d -- are folded
into the per-pixel most reliable chain, and the homography is fitted to the chains that are valid, visible and inside the template
mask.  The chain keys below are the defaults, written out.  A frame costs one flow per delta."""
from pathlib import Path

from pytracking.tracker.WOFT_chained import WOFTChained
from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.tracker_class = WOFTChained
    conf.chain_deltas = (None, 1, 2, 4, 8, 16, 32)
    conf.chain_vis_thr = 0.5
    conf.chain_unit_cost = 1.0
    conf.chain_iters = None
    conf.chain_weights = True
    return conf
