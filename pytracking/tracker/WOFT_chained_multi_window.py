from woft_amd.chained_multi_window import WOFTChainedMultiWindow  # noqa: F401
