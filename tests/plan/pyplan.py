"""Builds tests/plan/plan_host.cpp (the launch planner of polycap_amd/csrc/hip/pc_plan.h, host only) and calls it with dicts."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HIPD = os.path.join(os.path.dirname(os.path.dirname(HERE)), "polycap_amd", "csrc", "hip")


class Planner:
    def __init__(self, directory, flags=()):
        so = os.path.join(str(directory), "plan_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD, *flags,
                               os.path.join(HERE, "plan_host.cpp"), "-o", so])
        self.L = L = C.CDLL(so)
        for fn in (L.plan_opt_names, L.plan_input_names, L.plan_field_names):
            fn.restype = C.c_char_p
        self.opt_names = L.plan_opt_names().decode().split()
        self.input_names = L.plan_input_names().decode().split()
        self.field_names = L.plan_field_names().decode().split()
        d = (C.c_int32 * len(self.opt_names))()
        L.plan_default_opts(d)
        self.default_opts = dict(zip(self.opt_names, d))

    def plan(self, inputs, opts=None):
        """inputs: every name of input_names; opts: option values that differ from the defaults -> dict of the plan's fields"""
        o = dict(self.default_opts, **(opts or {}))
        assert set(o) == set(self.opt_names) and set(inputs) == set(self.input_names), (sorted(o), sorted(inputs))
        co = (C.c_int32 * len(self.opt_names))(*[int(o[k]) for k in self.opt_names])
        ci = (C.c_double * len(self.input_names))(*[float(inputs[k]) for k in self.input_names])
        out = (C.c_int64 * len(self.field_names))()
        self.L.plan_launch(co, ci, out)
        return dict(zip(self.field_names, out))
