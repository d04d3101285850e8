"""WOFT with the MaskHead's visibility mask consumed by the tracker: the flow network is the 'weighted_masked' one (a checkpoint
with mask_head.net.* tensors of the structure below), and a correspondence survives only where the head's visibility probability
exceeds `visibility_thr` (visibility_mode 'gate'; 'weight' scales the flow weights by the probability instead).  The reference's
tracker consumes no mask: mode, threshold and structure are this project's choices, not reference values."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.flow_config.raft_type = 'weighted_masked'
    conf.flow_config.class_params.mask_estimation = True
    conf.flow_config.class_params.mask_head_structure = [(128, 3), (128, 3)]
    conf.visibility_mode = 'gate'
    conf.visibility_thr = 0.5
    return conf
