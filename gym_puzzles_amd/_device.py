"""What the classes over ``libmrp.so``'s handles share (``Batch``, ``DeviceVecNormalize``,
``DevicePolicy``, ``DevicePPO``): the one checker of the tensors that reach a kernel, the pointer and
stream helpers, and ``Handle``, the owner of one C handle.  Pure Python at import; torch is imported
when a tensor is checked."""
from __future__ import annotations

import ctypes

_Tensor = None      # torch.Tensor, looked up at the first check: these helpers sit on every launch's host path


def check_tensor(who, name, t, dev, dtype, shape):
    """``ValueError`` unless ``t`` is a contiguous tensor of ``dtype`` and ``shape`` on ``dev`` (a CUDA
    ``torch.device`` with its index).  Nothing is launched on a tensor that has not passed this."""
    global _Tensor
    if _Tensor is None:
        import torch
        _Tensor = torch.Tensor
    if not isinstance(t, _Tensor):
        raise ValueError(f"{who}: {name} is not a tensor")
    if not t.is_cuda or t.device != dev:
        raise ValueError(f"{who}: {name} is on {t.device}, expected {dev}")
    if t.dtype != dtype:
        raise ValueError(f"{who}: {name} is {t.dtype}, expected {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} is {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} is not contiguous")


def check_tensors(who, dev, specs):
    """``check_tensor`` on every ``(name, tensor, dtype, shape, optional)`` of ``specs``, in order; None
    passes only where ``optional``."""
    for name, t, dtype, shape, optional in specs:
        if t is not None or not optional:
            check_tensor(who, name, t, dev, dtype, shape)


def ptr(t):
    """The device address of a checked tensor as a pointer argument of the ABI (a plain int: the ABI's
    ``argtypes`` convert it); None (NULL) for None."""
    return None if t is None else t.data_ptr()


def stream_of(dev):
    """The current torch stream of ``dev`` as a pointer argument of the ABI (0 is the null stream)."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def index_of(dev) -> int:
    if dev.index is not None:
        return dev.index
    import torch
    return torch.cuda.current_device()


class Handle:
    """Owner of one handle of the C ABI.  A subclass names its functions (``_DESTROY``,
    ``_LAST_ERROR``) and the codes that mean the caller's mistake (``_VALUE_ERRORS``, raised as
    ``ValueError``; every other code raises ``MrpError``).  ``self._h`` is the handle, and reading it
    raises ``ValueError("<Class> is closed")`` after ``close()``: a method cannot reach the library
    with a freed handle."""

    _DESTROY = _LAST_ERROR = None
    _VALUE_ERRORS = ()          # MRP_E_ARG = -1, MRP_E_STATE = -3
    _handle = None

    def _error(self, rc, msg):
        from ._native import MrpError
        return (ValueError if rc in self._VALUE_ERRORS else MrpError)(msg)

    def _open(self, create, *args):
        """``create(*args, &handle)``; raises with the library's message, keeps the handle."""
        from ._native import load
        self._L = load()
        h = ctypes.c_void_p()
        rc = getattr(self._L, create)(*args, ctypes.byref(h))
        if rc != 0:
            raise self._error(rc, f"{create} failed ({rc}): {getattr(self._L, self._LAST_ERROR)(None).decode()}")
        self._handle = h

    @property
    def _h(self):
        if self._handle is None:
            raise ValueError(f"{type(self).__name__} is closed")
        return self._handle

    def _check_rc(self, rc):
        if rc != 0:
            raise self._error(rc, getattr(self._L, self._LAST_ERROR)(self._handle).decode())

    def close(self):
        if self._handle is not None:
            getattr(self._L, self._DESTROY)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
