"""The life cycle shared by the objects that run on a registration context: IterativeClosestPoint, SCManager,
ISCGeneration and PoseGraph."""
from __future__ import annotations

import ctypes as C

from ._lib import check
from .ndt import NormalDistributionsTransform


class _CtxObject:
    """Runs on a registration context: its own, or the one of an existing NormalDistributionsTransform
    (`registration=`).  A subclass with a library handle keeps it in `_handle` and names the C-ABI function that
    destroys it in `_DESTROY`; `_WHAT` names the detector in the error for an unknown parameter keyword."""

    _DESTROY: str | None = None
    _WHAT = ""
    _handle = None
    _reg = None
    _own = False

    def __init__(self, device: int, registration: NormalDistributionsTransform | None):
        self._own = registration is None
        self._reg = NormalDistributionsTransform(device) if registration is None else registration
        self._lib = self._reg._lib

    def _with_overrides(self, params, overrides: dict, convert=None):
        """`params` (a parameter struct) with the keyword overrides set; `convert(name, value)` adapts a value."""
        names = tuple(k for k, _ in type(params)._fields_)
        for k, v in overrides.items():
            if k not in names:
                raise TypeError(f"unknown {self._WHAT} parameter {k!r}")
            setattr(params, k, convert(k, v) if convert else v)
        return params

    def _default_params(self, struct, default_fn: str, overrides: dict, convert=None):
        """The library's defaults (`default_fn` fills a `struct`) with the keyword overrides set."""
        p = struct()
        check(getattr(self._lib, default_fn)(C.byref(p)))
        return self._with_overrides(p, overrides, convert)

    def close(self):
        if self._handle:
            getattr(self._lib, self._DESTROY)(self._handle)  # before its context
            self._handle = None
        if self._own and self._reg is not None:
            self._reg.close()
        self._reg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def registration(self) -> NormalDistributionsTransform:
        return self._reg

    @property
    def ctx(self):
        return self._reg.ctx
