"""WOFT on multi-delta chained flow for several planar targets, on ONE search window (this project's own tracker, no counterpart in
the reference): WOFT_chained_multi.py whose flows run on the union of the targets' boxes plus `search_window_margin` instead of on
whole frames; the window follows the targets.  One window-sized flow per delta and frame, whatever the number of targets.  Windows
are seldom multiples of 8, which padding_mode 'nopad' refuses: RAFT's replicate padding, as in WOFT_chained_window.py.  The direct
candidate is not pre-warped: K targets have K poses."""
from pathlib import Path

from pytracking.tracker.WOFT_chained_multi_window import WOFTChainedMultiWindow
from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained_multi.py')
    conf.tracker_class = WOFTChainedMultiWindow
    conf.flow_config.padding_mode = 'RAFT'
    conf.search_window_margin = 0.25
    conf.chain_prewarp = False
    return conf
