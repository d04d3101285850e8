def __getattr__(name):
    # (resolved on first use: importing the package itself stays free of torch and of the HIP library)
    if name == "forward_interpolate":
        from .warm import forward_interpolate
        return forward_interpolate
    raise AttributeError(f"module 'woft_amd' has no attribute {name!r}")
