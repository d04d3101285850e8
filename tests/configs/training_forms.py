"""A flow-training config written the way the reference's optical_flow/training_configs modules are: the estimator and the
loss come from the library through the reference's import paths (no woft_amd import) and are stored on conf.train as the
batched weighted least-squares fit and the re-projection error.  Only the fields the library serves are set; datasets,
weight files and the optimiser settings of a real training config are outside this project."""
from pytracking.utils.config import Config
from pytracking.utils.least_squares_H import torch_reproj_errors, find_homography_nonhomogeneous_QR


def get_config():
    conf = Config()
    conf.train = Config()
    conf.train.H_estimator = find_homography_nonhomogeneous_QR
    conf.train.loss_fn = torch_reproj_errors
    return conf
