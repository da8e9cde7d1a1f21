"""Builds tests/plan/images_host.cpp (the pure half of polycap_amd/csrc/hip/pc_images.h, host only) and calls it."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
INC = os.path.join(ROOT, "include")

NONE, RECORDS, PLANES, COMPACT = range(4)


class HipImages(C.Structure):
    """struct pc_hip_images of include/polycap-hip.h"""
    _fields_ = [("src_start_coords", C.c_void_p * 2), ("pc_start_coords", C.c_void_p * 2), ("pc_start_dir", C.c_void_p * 2),
                ("pc_start_elecv", C.c_void_p * 2), ("pc_exit_coords", C.c_void_p * 3), ("pc_exit_dir", C.c_void_p * 2),
                ("pc_exit_elecv", C.c_void_p * 2), ("pc_exit_nrefl", C.c_void_p), ("pc_exit_dtravel", C.c_void_p),
                ("exit_coord_weights", C.c_void_p)]


class Images:
    def __init__(self, directory):
        so = os.path.join(str(directory), "images_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD, "-I", INC,
                               os.path.join(HERE, "images_host.cpp"), "-o", so])
        self.L = L = C.CDLL(so)
        for fn in (L.images_opt_names, L.images_plan_field_names):
            fn.restype = C.c_char_p
        self.opt_names = L.images_opt_names().decode().split()
        self.plan_fields = L.images_plan_field_names().decode().split()
        self.n_fields = L.images_n_fields()
        self.max_parts = L.images_max_parts()
        d = (C.c_int32 * len(self.opt_names))()
        L.images_default_opts(d)
        self.default_opts = dict(zip(self.opt_names, d))

    def plan(self, n_slots, ne, keep_images, **opts):
        """-> dict of the plan's fields, with "begin": the parts + 1 bounds"""
        o = dict(self.default_opts, **opts)
        assert set(o) == set(self.opt_names), sorted(o)
        co = (C.c_int32 * len(self.opt_names))(*[int(o[k]) for k in self.opt_names])
        fields = (C.c_int64 * len(self.plan_fields))()
        begin = (C.c_int64 * (self.max_parts + 1))()
        self.L.images_plan(C.c_int64(n_slots), int(ne), int(keep_images), co, fields, begin)
        p = dict(zip(self.plan_fields, fields))
        p["begin"] = list(begin)[:p["parts"] + 1]
        return p

    def layout(self, layout, n_total, ne, lo):
        out = (C.c_int64 * 5)()
        self.L.images_layout(int(layout), C.c_int64(n_total), C.c_int64(ne), C.c_int64(lo), out)
        return dict(zip(("ss", "fs", "ws", "base", "w_base"), out))

    def block_span(self, first, count, n_total, blk_shift, b, e):
        out = (C.c_int64 * 2)()
        self.L.images_block_span(C.c_int64(first), C.c_int64(count), C.c_int64(n_total), int(blk_shift), C.c_int64(b), C.c_int64(e), out)
        return out[0], out[1]

    def planes(self, images):
        out = (C.c_void_p * (self.n_fields + 1))()
        self.L.images_planes(C.byref(images), out)
        return [p or 0 for p in out]
