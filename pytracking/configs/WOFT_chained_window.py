"""WOFT on multi-delta chained flow, on search windows (this project's own tracker, no counterpart in the reference):
WOFT_chained.py whose flows run on the tracked plane's box plus `search_window_margin` instead of on whole frames; the window
follows the object.  Window sides are multiples of `chain_window_quantum` (or the whole side), so the sizes the flow provider meets
repeat.  Windows are seldom multiples of 8, which padding_mode 'nopad' refuses: RAFT's replicate padding, as in WOFT_window.py.
The chain and window keys below are the defaults, written out.  A frame costs one window-sized flow per delta."""
from pathlib import Path

from pytracking.tracker.WOFT_chained_window import WOFTChainedWindow
from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained.py')
    conf.tracker_class = WOFTChainedWindow
    conf.flow_config.padding_mode = 'RAFT'
    conf.search_window_margin = 0.25
    conf.chain_window_quantum = 64
    conf.chain_window_min = 8 * 20
    conf.chain_prewarp = True
    return conf
