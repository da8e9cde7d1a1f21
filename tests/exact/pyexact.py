"""What tests/test_exact_cpu.py and scripts/record_exact_functions.py share: the host build of tests/exact/exact_host.cpp (pc_exact.h
alone) and the calls of the library's public host functions on integer inputs (tests/golden/exact_functions.json)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIPD = os.path.join(os.path.dirname(os.path.dirname(HERE)), "polycap_amd", "csrc", "hip")
M64 = 2 ** 64 - 1


def pairs(values):
    """128-bit integers -> flat uint64 (lo, hi) pairs"""
    return np.array([x for v in values for x in (v & M64, v >> 64)], dtype=np.uint64)


def _both(a, b):
    return [float(x) for x in np.ravel(a)] + ([] if b is None else [float(x) for x in np.ravel(b)])


def call(fn, i):
    """the public function `fn` on the integers of one case -> its outputs as a flat list of floats"""
    from polycap_amd import hip
    if fn == "pc_hip_fixed_to_double":
        return [hip.fixed_to_double(i["lo"], i["hi"])]
    if fn == "pc_hip_efficiencies":         # sum_weights = num / 2^20, exactly
        return _both(hip.efficiencies([n / 2.0 ** 20 for n in i["num"]], i["counters"]), None)
    if fn == "pc_hip_efficiency_stderr":
        return _both(hip.efficiency_stderr(pairs(i["A"]), pairs(i["B"]), i["counters"]), None)
    if fn == "pc_hip_relay_efficiencies":
        return _both(*hip.relay_efficiencies(pairs(i["A"]), None if i["B"] is None else pairs(i["B"]), i["counters"]))
    if fn == "pc_hip_scan_efficiencies":    # counters [P][6]; A, B [P][ne]
        P = len(i["counters"])
        return _both(*hip.scan_efficiencies(i["counters"], pairs(sum(i["A"], [])).reshape(P, -1, 2),
                                            None if i["B"] is None else pairs(sum(i["B"], [])).reshape(P, -1, 2)))
    if fn == "pc_hip_tally_stderr":
        return _both(hip.tally_stderr(np.array(i["sums"], dtype=np.uint64), pairs(i["squares"]).reshape(-1, 2), i["n_started"]), None)
    if fn == "pc_hip_select_transmission":
        return _both(*hip.select_transmission(np.array(i["pw"], dtype=np.uint64), np.array(i["rw"], dtype=np.uint64), pairs(i["p2"]), pairs(i["r2"])))
    raise KeyError(fn)


class ExactHost:
    """tests/exact/exact_host.cpp as a shared library"""

    def __init__(self, directory):
        so = os.path.join(str(directory), "exact_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD,
                               os.path.join(HERE, "exact_host.cpp"), "-o", so])
        self.L = L = C.CDLL(so)
        u64, u64p, i64p = C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        L.exact_value_hex.argtypes = [u64, u64, C.c_char_p, C.c_int]
        L.exact_scales_hex.argtypes = [C.c_char_p, C.c_int]
        L.exact_add.argtypes = [u64, u64, u64, u64, u64p]
        L.exact_add_pairs.argtypes = [u64p, u64p, C.c_size_t]
        L.exact_split.argtypes = [u64, u64, i64p]
        L.exact_join.argtypes = [i64p, u64p]
        L.exact_stderr.argtypes = [u64, u64, u64, u64, C.c_int64]
        L.exact_stderr.restype = C.c_double

    def value(self, v):
        """pc_exact_value as an exact integer: the long double is printed in hex (%La)"""
        buf = C.create_string_buffer(64)
        self.L.exact_value_hex(v & M64, v >> 64, buf, 64)
        return int(float_from_hex_ld(buf.value.decode()))

    def scales(self):
        buf = C.create_string_buffer(192)
        self.L.exact_scales_hex(buf, 192)
        return [int(float_from_hex_ld(s)) for s in buf.value.decode().split()]

    def add(self, a, b):
        out = (C.c_uint64 * 2)()
        self.L.exact_add(a & M64, a >> 64, b & M64, b >> 64, out)
        return out[0] | (out[1] << 64)

    def add_pairs(self, acc, part):
        a, b = pairs(acc), pairs(part)
        p = C.POINTER(C.c_uint64)
        self.L.exact_add_pairs(a.ctypes.data_as(p), b.ctypes.data_as(p), len(acc))
        return [int(a[2 * k]) | (int(a[2 * k + 1]) << 64) for k in range(len(acc))]

    def split(self, v):
        limb = (C.c_int64 * 4)()
        self.L.exact_split(v & M64, v >> 64, limb)
        return list(limb)

    def join(self, limbs):
        out = (C.c_uint64 * 2)()
        self.L.exact_join((C.c_int64 * 4)(*limbs), out)
        return out[0] | (out[1] << 64)

    def stderr(self, A, B, N):
        """pc_exact_stderr(A / (N 2^62), B / (N 2^62), N): the efficiency's standard error from its exact sums"""
        return self.L.exact_stderr(A & M64, A >> 64, B & M64, B >> 64, N)


def float_from_hex_ld(s):
    """a %La string (64-bit mantissa) -> Fraction, exactly"""
    from fractions import Fraction
    mant, exp = s.lower().split("p")
    assert mant.startswith("0x")
    whole, _, frac = mant[2:].partition(".")
    return Fraction(int(whole + frac, 16), 16 ** len(frac)) * Fraction(2) ** int(exp)
