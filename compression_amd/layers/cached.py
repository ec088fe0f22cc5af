"""What the layers that keep device values between calls share: the hooks that drop those values when the weights may
have changed, copies and pickles that leave them behind, and the numbers that name a weight value to the library."""
from __future__ import annotations

import copy
import itertools
import os

__all__ = ["CachedValues", "KEYED_WEIGHTS", "FLIPPED", "new_weights_key", "drop_weights_key", "version_of"]

def version_of(t):
    """The tensor's version counter, or None where it has none (tensors created under
    torch.inference_mode raise on `_version`)."""
    try:
        return t._version
    except RuntimeError:
        return None

# One number per distinct value of a layer's weights (include/tfc_hip.h, tfc_conv2d_weights_key): the library keeps
# the kernels' packed fragments of a keyed value between calls instead of packing them in front of every launch.
# On unless TFC_CONV_KEYED_WEIGHTS=0.
KEYED_WEIGHTS = os.environ.get("TFC_CONV_KEYED_WEIGHTS", "1") not in ("", "0")
FLIPPED = 1 << 62                   # (the key of the flipped kernel of the same value)
_WEIGHT_KEYS = itertools.count(1)

def new_weights_key():
    return next(_WEIGHT_KEYS)

def drop_weights_key(key):
    """Releases the library's packed fragments of a key (in stream order)."""
    try:
        from .. import _lib
        lib = _lib.lib()
        lib.tfc_conv2d_drop_weights(key)
        lib.tfc_conv2d_drop_weights(key | FLIPPED)
    except Exception:                                        # interpreter shutdown, library never loaded
        pass

class CachedValues:
    """Mixin in front of torch.nn.Module for a layer that keeps values derived from its weights in the instance
    attributes named in `_cache_attrs`.  The layer's own `invalidate_kernel_cache()` drops them; loading a state dict,
    `.to()` / `.cuda()` / `.half()` and `train()` / `eval()` call it.  The caches are keyed on storage and version
    counter, which a write through `.data` advances neither of: call it after such a write.  They may hold native
    handles, so they are not copied or pickled with the module: a copy rebuilds its own on first use (copy.deepcopy for
    an EMA model, torch.save of the module object)."""

    _cache_attrs = ()

    def invalidate_kernel_cache(self):
        raise NotImplementedError

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_kernel_cache()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_kernel_cache()
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode=True):
        self.invalidate_kernel_cache()
        return super().train(mode)

    def __del__(self):
        try:
            self.invalidate_kernel_cache()       # (what a cache holds of the library's is released with the layer)
        except Exception:                        # interpreter shutdown, a layer whose constructor raised
            pass

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._cache_attrs}

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update((k, copy.deepcopy(v, memo)) for k, v in self.__dict__.items() if k not in self._cache_attrs)
        return new
