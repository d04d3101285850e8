"""WOFT with RAFT's video warm start in the lost-frame branch: from the second frame of a run of lost frames on, the frame
t-1 -> t flow starts from the forward-interpolated flow of the previous one instead of from zero (`warm_start_local`).  The
optional key `warm_start_iters` gives those flows their own iteration count (default: the flow config's `iters`).  The
reference's tracker has no such option: the key is this project's."""
from pathlib import Path

from pytracking.utils.config import load_config


def get_config():
    conf = load_config(Path(__file__).resolve().parent / 'WOFT.py')
    conf.warm_start_local = True
    return conf
