"""Which kernels a block launched, from the library's own per-kernel statistics (vitmi_stats_*)."""
import ctypes

from vitmi import _lib


class kernel_stats:
    """vitmi_stats_enable(1) around a block; afterwards .calls(substring) of the mangled kernel
    names, and .work[name] = (calls, flops, bytes) as recorded."""

    def __enter__(self):
        _lib.lib().vitmi_stats_enable(1)
        self.k = {}
        self.work = {}
        return self

    def __exit__(self, *exc):
        lib = _lib.lib()
        try:
            for i in range(lib.vitmi_stats_count()):
                name = ctypes.create_string_buffer(1024)
                calls, fl, by = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
                lib.vitmi_stats_get(i, name, 1024, ctypes.byref(calls), ctypes.byref(fl), ctypes.byref(by))
                self.k[name.value.decode()] = calls.value
                self.work[name.value.decode()] = (calls.value, fl.value, by.value)
        finally:
            lib.vitmi_stats_enable(0)
        return False

    def calls(self, sub):
        return sum(c for n, c in self.k.items() if sub in n)

    def summary(self, subs=("gemm_kernel", "gemm256_kernel", "gemm_tail_fixup_kernel", "splitk_reduce")):
        return {s: self.calls(s) for s in subs if self.calls(s)}
