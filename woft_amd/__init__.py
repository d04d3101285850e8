def __getattr__(name):
    # (resolved on first use: importing the package itself stays free of torch and of the HIP library)
    if name == "forward_interpolate":
        from .warm import forward_interpolate
        return forward_interpolate
    if name in ("chain_flow", "fb_consistency"):
        from .interpolation import chain_flow, fb_consistency
        return chain_flow if name == "chain_flow" else fb_consistency
    if name in ("chain_fold", "MultiFlowTracker"):
        from .multiflow import MultiFlowTracker, chain_fold
        return chain_fold if name == "chain_fold" else MultiFlowTracker
    if name in ("chain_correspondences", "WOFTChained"):
        from .chained import WOFTChained, chain_correspondences
        return chain_correspondences if name == "chain_correspondences" else WOFTChained
    if name in ("WOFTChainedMulti", "pack_target_bits"):
        from . import chained
        return getattr(chained, name)
    if name in ("chain_fold_window", "WindowedMultiFlowTracker", "WOFTChainedWindow"):
        from . import chained_window
        return getattr(chained_window, name)
    if name == "WOFTChainedMultiWindow":
        from .chained_multi_window import WOFTChainedMultiWindow
        return WOFTChainedMultiWindow
    if name in ("HSynth", "HSynthSample", "HSynthAugment", "render_pair", "pair_labels", "random_homography", "make_occluder",
                "augment", "blur_taps", "colour_matrix"):
        from . import hsynth
        return getattr(hsynth, name)
    if name in ("PhotoTemplate", "PhotoTemplateMulti", "refine_homography", "photo_weight_map"):
        from . import photo
        return getattr(photo, name)
    if name == "FrameFeatures":
        from .flow_provider import FrameFeatures
        return FrameFeatures
    raise AttributeError(f"module 'woft_amd' has no attribute {name!r}")
