"""photoverse_amd: MI355X-native (gfx950) implementation of PhotoVerse's denoising hot path.

Python host layer over ``libphotoverse_hip.so`` (hand-written HIP kernels, C-ABI in ``include/photoverse_hip.h``).
There is no CPU or eager fallback: ops raise if the library or a HIP device is missing.
"""
__version__ = "0.1.0"


def __getattr__(name):           # lazy: importing the package stays free of torch
    if name == "AutoencoderTiny":
        from .vae_tiny import AutoencoderTiny
        return AutoencoderTiny
    if name == "RRDBNet":
        from .upscaler import RRDBNet
        return RRDBNet
    if name in ("WindowedDenoiseLoop", "window_origins", "window_profile"):
        from . import multidiffusion
        return getattr(multidiffusion, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
