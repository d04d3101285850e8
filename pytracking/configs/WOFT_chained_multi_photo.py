"""Several planar targets on one chained flow, each fitted pose refined photometrically (`chain_photo_refine` = the Gauss-Newton
iteration count): WOFT_chained_multi.py plus the key.  The targets that are not lost go through one batched refinement per frame
(woft_photo_refine_multi): one call and one read more, whatever the number of targets.  Further keys as in WOFT_chained_photo.py."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT_chained_multi.py')
    conf.chain_photo_refine = 10
    return conf
