"""Several planar targets on one chained flow, each fitted pose refined photometrically under the chains' visibility
(`chain_photo_weights`): WOFT_chained_multi_photo.py plus the key.  One woft_photo_weights launch per frame makes the weight map
every target shares and counts each target's visible support, whatever the number of targets; a target under
`chain_photo_min_support` of its mask is left out of the batched refinement.  Further keys as in WOFT_chained_photo_occl.py."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained_multi_photo.py')
    conf.chain_photo_weights = 'gate'
    return conf
