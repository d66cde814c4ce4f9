"""Invalidation of the packed / folded weight copies the native path keeps.

A module that caches derived tensors (bf16-packed weights, BN folds, scratch
grids) in ``self.__dict__`` lists the keys in ``_native_cache``; they are dropped
whenever the parameters may have changed or moved: ``train()`` / ``eval()``,
``load_state_dict`` and ``_apply`` (``.to()``, ``.cuda()``, ``.half()`` ...).

``_native_cache`` is a tuple of keys that are REMOVED from ``__dict__`` (the code
that reads them tests ``key in self.__dict__``), or a mapping of key to what a
dropped key is rebound to: ``None``, or a factory of the fresh value (``dict``).
"""


class NativeCacheMixin:
    _native_cache = ()

    def invalidate_hip_cache(self):
        """Drop every cached copy; call it after changing weights by hand."""
        rule = self._native_cache
        if isinstance(rule, dict):
            for key, fresh in rule.items():
                self.__dict__[key] = None if fresh is None else fresh()
        else:
            for key in rule:
                self.__dict__.pop(key, None)

    def train(self, mode=True):
        self.invalidate_hip_cache()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_hip_cache()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_hip_cache()
        return super()._apply(fn, *args, **kwargs)


def invalidate_all(module):
    """``invalidate_hip_cache`` of ``module`` and of every sub-module that has one: for a
    change no nn.Module event announces (``VeonOccupancyPath.set_vocabulary``)."""
    for m in module.modules():
        drop = getattr(m, 'invalidate_hip_cache', None)
        if drop is not None:
            drop()
