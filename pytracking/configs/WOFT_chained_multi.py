"""WOFT on multi-delta chained flow for several planar targets of one template frame (this project's own tracker, no counterpart
in the reference): WOFT_chained.py with the multi-target tracker class.  `init(frame, masks)` takes 1 to 32 masks, `track(frame)`
returns a (K, 3, 3) stack of homographies and K metas; the flows and their fold are computed once per frame, whatever K is."""
from pathlib import Path

from pytracking.tracker.WOFT_chained import WOFTChainedMulti
from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained.py')
    conf.tracker_class = WOFTChainedMulti
    return conf
