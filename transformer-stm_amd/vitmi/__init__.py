"""vitmi — MI355X-native (gfx950) ViT forward/backward training path.

See DESIGN.md.  ``vitmi.modules`` holds the nn.Module API, ``vitmi.ops`` the
tensor wrappers over the C ABI in ``include/vitmi.h`` (``libvitmi.so``).
"""
from .config import ViTConfig, preset, config_c1, config_c2, config_c3, config_c5  # noqa: F401

__version__ = "0.1.0"


def _lazy():
    from . import modules, ops  # noqa: F401
    return modules, ops


def __getattr__(name):
    # vitmi.losses / vitmi.augment (the classification recipe), imported on first use like the rest:
    # importing the package alone stays free of torch
    if name in ("losses", "augment"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "DropPath":   # the stochastic-depth module (vitmi.modules), same lazy import
        from .modules import DropPath
        return DropPath
    if name == "LayerScale":   # the per-channel branch scale (vitmi.modules), likewise
        from .modules import LayerScale
        return LayerScale
    if name in ("patch_keep", "PATCH_SITE"):   # patch dropout's subset selection (vitmi.ops) and its hash site
        from . import ops
        return getattr(ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
