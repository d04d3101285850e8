"""WOFT with the search-window tracker: the flows run on the tracked plane's box plus a margin instead of the whole frame.
The reference's WOFTWindow reads `search_window_margin` but none of its shipped configs sets it: 0.25 (a quarter of the box's
size on every side) is this project's choice, not a reference value.  A window's sides are no multiples of 8, which the default
padding_mode 'nopad' refuses (in the reference as here): RAFT's replicate padding, as in WOFT_downscale_2x.py."""
from pathlib import Path

from pytracking.tracker.WOFT_window import WOFTWindow
from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.tracker_class = WOFTWindow
    conf.search_window_margin = 0.25
    conf.flow_config.padding_mode = 'RAFT'
    return conf
