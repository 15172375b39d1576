"""Device buffers for the GPU tests, without torch: ctypes on libamdhip64 (hipMalloc / hipFree / synchronous hipMemcpy). The library is found by name or,
failing that, through libcleanrl_hip.so, which links it."""
import ctypes as C
import os

import numpy as np

_R = None


def _rt():
    global _R
    if _R is None:
        try:
            R = C.CDLL("libamdhip64.so")
        except OSError:
            import cleanrl_jl_amd as crl
            R = C.CDLL(crl._lib.LIB_PATH)
        R.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        R.hipFree.argtypes = [C.c_void_p]
        R.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        R.hipDeviceSynchronize.argtypes = []
        _R = R
    return _R


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")


class Buf:
    """nbytes of device memory; data_ptr() makes it a pointer argument of the device-pointer calls."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._p = C.c_void_p()
        _ok(_rt().hipMalloc(C.byref(self._p), max(self.nbytes, 1)), "hipMalloc")

    def data_ptr(self):
        return self._p.value or 0

    def at(self, byte_offset):
        return self.data_ptr() + int(byte_offset)

    def put(self, arr, byte_offset=0):
        a = arr if arr.flags.f_contiguous or arr.flags.c_contiguous else np.ascontiguousarray(arr)
        assert byte_offset + a.nbytes <= self.nbytes
        _ok(_rt().hipMemcpy(C.c_void_p(self.at(byte_offset)), a.ctypes.data_as(C.c_void_p), a.nbytes, 1), "hipMemcpy H2D")
        return self

    def get(self, dtype, shape=None, order="F", byte_offset=0):
        out = np.zeros((self.nbytes - byte_offset) // np.dtype(dtype).itemsize if shape is None else shape, dtype, order=order)
        assert byte_offset + out.nbytes <= self.nbytes
        _ok(_rt().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.at(byte_offset)), out.nbytes, 2), "hipMemcpy D2H")
        return out

    def free(self):
        if self._p.value:
            _rt().hipFree(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def upload(arr):
    return Buf(arr.nbytes).put(arr)


def device_sync():
    _ok(_rt().hipDeviceSynchronize(), "hipDeviceSynchronize")
