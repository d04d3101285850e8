from woft_amd.chained import WOFTChained, WOFTChainedMulti, chain_correspondences  # noqa: F401
