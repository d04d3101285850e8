"""WOFT with the forward-backward check: both stages also run the reverse flow, and a correspondence survives only where the two
flows agree -- |f + b|^2 <= fb_alpha * (|f|^2 + |b|^2) + fb_beta, b the reverse flow sampled where f lands -- and f lands inside
the frame.  About two flows per stage.  The reference's tracker has no such check: key, rule and constants are this project's
choices (the constants are the customary ones of the optical-flow literature), not reference values."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.fb_check = 'gate'
    conf.fb_alpha = 0.01
    conf.fb_beta = 0.5
    return conf
