from woft_amd.chained import WOFTChained, chain_correspondences  # noqa: F401
