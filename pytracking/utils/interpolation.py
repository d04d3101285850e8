from woft_amd.interpolation import bilinear_interpolate_torch, chain_flow, fb_consistency, flow_warp_coords  # noqa: F401
