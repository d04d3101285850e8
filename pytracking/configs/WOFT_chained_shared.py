"""WOFT_chained with the encoder passes shared between the flows of a frame: every frame is encoded once and serves, as a
frame-features record, as the target of its own K flows and as the source of later chained flows.  The
results are those of WOFT_chained, bit for bit; each stored frame keeps 66.4 MB more at 1080p."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained.py')
    conf.chain_share_features = True
    return conf
