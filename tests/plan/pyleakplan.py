"""Builds tests/plan/leak_host.cpp (the leak planner of polycap_amd/csrc/hip/pc_leak_plan.h, host only) and calls it."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIPD = os.path.join(os.path.dirname(os.path.dirname(HERE)), "polycap_amd", "csrc", "hip")


class LeakPlanner:
    def __init__(self, directory, flags=()):
        so = os.path.join(str(directory), "leak_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD, *flags,
                               os.path.join(HERE, "leak_host.cpp"), "-o", so])
        self.L = L = C.CDLL(so)
        L.leak_grid.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(C.c_int64)]
        L.leak_grid.restype = None
        L.leak_capacity.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_int64]
        L.leak_grown.argtypes = [C.c_int64]
        L.leak_capacity.restype = L.leak_grown.restype = C.c_int64
        L.leak_order_considered.argtypes = [C.c_int, C.c_int64, C.c_int64]
        L.leak_order.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_uint64)]
        self.block = L.leak_block()
        self.frame_header = L.leak_frame_header()

    def grid(self, n_items, ne, max_depth, stack_bytes, n_cu):
        """-> (blocks, lanes)"""
        out = (C.c_int64 * 2)()
        self.L.leak_grid(n_items, ne, max_depth, stack_bytes, n_cu, out)
        return out[0], out[1]

    def capacity(self, option, ne, n, floor):
        return self.L.leak_capacity(option, ne, n, floor)

    def grown(self, needed):
        return self.L.leak_grown(needed)

    def considered(self, enabled, n, lanes):
        return bool(self.L.leak_order_considered(int(enabled), n, lanes))

    def order(self, est, lanes, n_cu):
        """-> dict(ordered, top, total, n_heavy, order): order is None when the slot order is kept"""
        est = np.ascontiguousarray(est, dtype=np.uint32)
        order = np.full(est.size, 0xffffffff, dtype=np.uint32)
        out = (C.c_uint64 * 3)()
        ordered = bool(self.L.leak_order(est.ctypes.data, est.size, lanes, n_cu, order.ctypes.data, out))
        if not ordered:
            assert np.all(order == 0xffffffff)
        return dict(ordered=ordered, top=out[0], total=out[1], n_heavy=out[2], order=order if ordered else None)
