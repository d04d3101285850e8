from woft_amd.chained_window import WindowedMultiFlowTracker, WOFTChainedWindow, chain_fold_window  # noqa: F401
