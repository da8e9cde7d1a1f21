"""TEST-ONLY: the arithmetic of pc_device.h element by element, on the device (probe.hip) or in the host compile of the same header
(tests/emul/pc_emul.cpp, IEEE sqrt, division and exp).  Both take the per-energy constants from the product's own setup
(pc_build_tables) of the Problem passed in.  Op MARCH (run_march) walks photons through the certified march of the Problem's whole
profile; op FLIGHTS (run_flights) carries that march on through the reflections; ops WALL, OUTER and HEX (run_wall, run_outer,
run_hex) call the wall search of pc_leak.h on the profile."""
import ctypes as C
import os
import subprocess

import numpy as np

from polycap_amd._cabi import ProblemS, c_double_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
SO = os.path.join(_HERE, "libpc_probe.so")
_LIB = None

OPS = dict(sqrt=0, div=1, exp=2, f3=3, f3s=4, f3x1=5, f3x2=6, ff0=7, ff1=8, re_fast=9, re3=10, re0=11, re1=12)
GROUP = dict(f3x2=2)              # elements one device thread evaluates (one energy per group)
# geometry ops (probe_ops.h): rows of their own widths, one entry point of their own
GEOM_OPS = dict(segment=13, geom=14, bounce=15)
GEOM_IN = dict(segment=14, geom=9, bounce=9)
GEOM_OUT = 8
SETUP_REJECT = -100               # the product's setup rejects the element's two-node profile: pc_segment is never reached
SEG_COLS = ("z0", "z1", "cap0", "cap1", "zh0", "zh1", "kx", "ky", "Px", "Py", "Pz", "dx", "dy", "dz")
SEG_OUT = ("hx", "hy", "hz", "nx", "ny", "nz", "p0x", "p0y")
GEOM_OUT_COLS = ("alfa", "st2", "es2", "ep2", "sd2", "c2", "fs", "fp")
# columns of the input rows (probe_ops.h)
COLS = ("c", "st2", "es2", "ep2", "sd2", "fs", "fp", "w")
EC_FIELDS = ("n_re", "n_im", "ninv2_re", "ninv2_im", "rough_c", "valid", "d2", "n2_re", "n2_im", "zi2", "rough_k2")


def _sources():
    hip = os.path.join(_ROOT, "polycap_amd", "csrc", "hip")
    return [os.path.join(_HERE, "probe.hip"), os.path.join(_HERE, "probe_ops.h"),
            os.path.join(hip, "pc_device.h"), os.path.join(hip, "pc_problem.h"), os.path.join(hip, "pc_leak.h"),
            os.path.join(_ROOT, "include", "polycap-hip.h")]


def compile_cmd(out=SO):
    """hipcc with the library's own code generation (polycap_amd._build.HIPFLAGS: -O3 -ffp-contract=off, gfx950)."""
    from polycap_amd import _build
    return ["hipcc"] + _build.HIPFLAGS + ["-I" + _HERE, "-shared", "-o", out, _sources()[0]]


def build(force=False):
    """Builds libpc_probe.so when it is missing or older than its sources; returns its path."""
    srcs = _sources()
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        tmp = SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(compile_cmd(tmp))
        os.replace(tmp, SO)
    return SO


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        L.probe_run.argtypes = [C.POINTER(ProblemS), C.c_int, C.c_int64, C.POINTER(C.c_int32), c_double_p, c_double_p,
                                C.POINTER(C.c_int32), C.c_char_p]
        L.probe_run.restype = C.c_int
        L.probe_run_geom.argtypes = [C.POINTER(ProblemS), C.c_int, C.c_int64, C.POINTER(C.c_int32), c_double_p, C.c_int, c_double_p,
                                     C.c_int, C.POINTER(C.c_int32), C.c_char_p]
        L.probe_run_geom.restype = C.c_int
        L.probe_run_march.argtypes = [C.POINTER(ProblemS), C.c_int64, c_double_p, C.c_int, c_double_p, C.c_int,
                                      C.POINTER(C.c_int32), C.c_char_p]
        L.probe_run_march.restype = C.c_int
        for f in (L.probe_run_wall, L.probe_run_outer, L.probe_run_hex, L.probe_run_flights,
                  L.probe_run_sincos, L.probe_run_uniform, L.probe_run_enter, L.probe_run_exit):
            f.argtypes = L.probe_run_march.argtypes
            f.restype = C.c_int
        _LIB = L
    return _LIB


def rows(n, **cols):
    """Input rows [n, 8]: named columns (COLS) broadcast to n, the rest 0 (w defaults to 1)."""
    x = np.zeros((n, len(COLS)))
    x[:, COLS.index("w")] = 1.0
    for k, v in cols.items():
        x[:, COLS.index(k)] = v
    return x


def run(problem, op, e, x, device=True):
    """Evaluates op on the rows x [n, 8] at energy indices e [n] of `problem`: (out [n, 2], code [n]).  device=False: the
    host compile of the same call."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, len(COLS))
    n = x.shape[0]
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, dtype=np.int32), (n,)))
    out = np.zeros((n, 2))
    code = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    if device:
        err = C.create_string_buffer(256)
        r = lib().probe_run(C.byref(problem.s), OPS[op], n, e.ctypes.data_as(ip), x.ctypes.data_as(c_double_p),
                            out.ctypes.data_as(c_double_p), code.ctypes.data_as(ip), err)
        if r:
            raise RuntimeError("probe_run(%s) failed: %d %s" % (op, r, err.value.decode(errors="replace")))
    else:
        from tests.emul import pyemul
        r = pyemul.lib().emul_probe_run(C.byref(problem.s), OPS[op], n, e.ctypes.data_as(ip), x.ctypes.data_as(c_double_p),
                                        out.ctypes.data_as(c_double_p), code.ctypes.data_as(ip))
        if r:
            raise RuntimeError("emul_probe_run(%s) failed: %d" % (op, r))
    return out, code


def run_geom(problem, op, x, e=0, device=True):
    """Evaluates the geometry op ('segment', 'geom', 'bounce') on the rows x [n, GEOM_IN[op]]: (out [n, 8], code [n])."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, GEOM_IN[op])
    n = x.shape[0]
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, dtype=np.int32), (n,)))
    out = np.zeros((n, GEOM_OUT))
    code = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    args = (C.byref(problem.s), GEOM_OPS[op], n, e.ctypes.data_as(ip), x.ctypes.data_as(c_double_p), GEOM_IN[op],
            out.ctypes.data_as(c_double_p), GEOM_OUT, code.ctypes.data_as(ip))
    if device:
        err = C.create_string_buffer(256)
        r = lib().probe_run_geom(*args, err)
        if r:
            raise RuntimeError("probe_run_geom(%s) failed: %d %s" % (op, r, err.value.decode(errors="replace")))
    else:
        from tests.emul import pyemul
        r = pyemul.lib().emul_probe_run_geom(*args)
        if r:
            raise RuntimeError("emul_probe_run_geom(%s) failed: %d" % (op, r))
    return out, code


# op MARCH (probe_ops.h): one photon per row through the certified march of the problem's whole profile
MARCH_OP = 16
MARCH_IN = 11
MARCH_K = 64
MARCH_HEAD = 22
MARCH_OUT = MARCH_HEAD + 4 * MARCH_K
MARCH_COLS = ("x", "y", "z", "dx", "dy", "dz", "ex", "ey", "ez", "literal", "K")
MARCH_HEAD_COLS = ("state", "rc0", "qr", "kx", "ky", "bnd", "i0", "dx", "dy", "dz",
                   "how", "i", "rc", "C0", "Px", "Py", "Pz", "nx", "ny", "nz", "cosalfa", "n_trail")
END_STEPS, END_REFLECT, END_EXIT, END_EVENT, END_ENTRANCE = range(5)
STEP_FIRST, STEP_SINGLE, STEP_L1, STEP_L2, STEP_LOWER, STEP_MISS, STEP_HIT, STEP_DONE = range(8)
STEP_NAMES = ("first", "single", "L1", "L2", "lowered", "literal miss", "literal hit", "literal end")
ST_MARCH = 2


def run_march(problem, x, device=True):
    """Op MARCH on the rows x [n, MARCH_IN] (MARCH_COLS): (out [n, MARCH_OUT], code [n]); out[:, :MARCH_HEAD] are
    MARCH_HEAD_COLS, then MARCH_K trail entries of (i before, i after, kind, creep)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, MARCH_IN)
    n = x.shape[0]
    out = np.zeros((n, MARCH_OUT))
    code = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    args = (C.byref(problem.s), n, x.ctypes.data_as(c_double_p), MARCH_IN, out.ctypes.data_as(c_double_p), MARCH_OUT,
            code.ctypes.data_as(ip))
    if device:
        err = C.create_string_buffer(256)
        r = lib().probe_run_march(*args, err)
        if r:
            raise RuntimeError("probe_run_march failed: %d %s" % (r, err.value.decode(errors="replace")))
    else:
        from tests.emul import pyemul
        r = pyemul.lib().emul_probe_run_march(*args)
        if r:
            raise RuntimeError("emul_probe_run_march failed: %d" % r)
    return out, code


def march_head(out):
    """the named columns of MARCH output rows"""
    return {k: out[:, j] for j, k in enumerate(MARCH_HEAD_COLS)}


def march_trail(row):
    """trail of one MARCH output row: list of (i before, i after, kind, creep) as ints"""
    nt = int(row[MARCH_HEAD_COLS.index("n_trail")])
    return [tuple(int(v) for v in row[MARCH_HEAD + 4 * t: MARCH_HEAD + 4 * t + 4]) for t in range(nt)]


# op FLIGHTS (probe_ops.h): op MARCH carried on through the reflections, up to FLIGHTS_NB flights per row
FLIGHTS_OP = 20
FLIGHTS_IN, FLIGHTS_K, FLIGHTS_NB, FLIGHTS_HEAD, FLIGHTS_FL, FLIGHTS_ENTRY = 12, 128, 12, 22, 24, 5
FLIGHTS_TRAIL = FLIGHTS_HEAD + FLIGHTS_FL * FLIGHTS_NB
FLIGHTS_OUT = FLIGHTS_TRAIL + FLIGHTS_ENTRY * FLIGHTS_K
FLIGHTS_COLS = MARCH_COLS + ("NB",)
FLIGHTS_HEAD_COLS = MARCH_HEAD_COLS[:10] + ("how", "rc", "irefl", "n_flights", "n_trail", "i", "Px", "Py", "Pz", "ex_dx", "ex_dy", "ex_dz")
FLIGHT_COLS = ("irefl", "i", "lv", "bnd", "first", "Px", "Py", "Pz", "dx", "dy", "dz",
               "end", "i_end", "nx", "ny", "nz", "cosalfa", "ix", "hx", "hy", "hz", "C0", "spare0", "spare1")
CHAIN_EXIT, CHAIN_EVENT, CHAIN_LIMIT, CHAIN_FLIGHTS, CHAIN_PASSES, CHAIN_ENTRANCE = range(6)
CHAIN_NAMES = ("exit", "event", "limit", "flights", "passes", "entrance")
LV_LATER = 2


def run_flights(problem, x, device=True):
    """Op FLIGHTS on the rows x [n, FLIGHTS_IN] (FLIGHTS_COLS): (out [n, FLIGHTS_OUT], code [n]); out[:, :FLIGHTS_HEAD] are
    FLIGHTS_HEAD_COLS, then FLIGHTS_NB flights of FLIGHT_COLS, then FLIGHTS_K trail entries of (flight, i before, i after, kind, creep)."""
    return _run_leak(problem, "flights", x, FLIGHTS_IN, FLIGHTS_OUT, device)


def flights_of(row):
    """the flights of one FLIGHTS output row: list of dicts of FLIGHT_COLS"""
    nf = int(row[FLIGHTS_HEAD_COLS.index("n_flights")])
    return [dict(zip(FLIGHT_COLS, row[FLIGHTS_HEAD + FLIGHTS_FL * f: FLIGHTS_HEAD + FLIGHTS_FL * (f + 1)])) for f in range(nf)]


def flights_trail(row):
    """trail of one FLIGHTS output row: list of (flight, i before, i after, kind, creep) as ints"""
    nt = int(row[FLIGHTS_HEAD_COLS.index("n_trail")])
    return [tuple(int(v) for v in row[FLIGHTS_TRAIL + 5 * t: FLIGHTS_TRAIL + 5 * t + 5]) for t in range(nt)]


# the leak ops (probe_ops.h): the wall search of pc_leak.h on the problem's whole profile
WALL_IN, WALL_K, WALL_HEAD, WALL_ENTRY, WALL_SHARED = 9, 96, 20, 17, 12
WALL_OUT = WALL_HEAD + WALL_ENTRY * WALL_K
WALL_COLS = ("Px", "Py", "Pz", "dx", "dy", "dz", "literal", "hint", "max_units")
WALL_HEAD_COLS = ("begin", "q_i", "r_i", "z_id0",
                  "wt", "d_travel", "q_out", "r_out", "hx", "hy", "hz", "px", "py", "pz", "nst", "dist", "z_id", "iesc", "units", "how")
WALL_END_COLS = WALL_HEAD_COLS[4:18]          # what the certified and the literal search of a row must agree on
WALL_TRAIL_COLS = ("state", "z_id_b", "z_id_a", "pz_b", "pz_a", "nst_b", "nst_a", "q_i", "r_i", "q_new", "r_new", "iesc",
                   "kind", "skip0", "skip1", "skip2", "visit")
WALL_FINISHED, WALL_CAPPED = 0, 1
WALL_UNITS_DEVICE, WALL_UNITS_HOST = 200000, 50000000
LS_WALL_STEP, LS_WALL_PROBE, LS_INWALL_END = 3, 4, 6
KIND_CERTIFIED, KIND_LITERAL, KIND_PROBE = 0, 1, 2
OUTER_IN, OUTER_OUT = 7, 4
OUTER_COLS = ("cx", "cy", "cz", "dx", "dy", "dz", "literal")
HEX_IN, HEX_OUT = 3, 2


def _run_leak(problem, name, x, in_w, out_w, device):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, in_w)
    n = x.shape[0]
    out = np.zeros((n, out_w))
    code = np.zeros(n, dtype=np.int32)
    args = (C.byref(problem.s), n, x.ctypes.data_as(c_double_p), in_w, out.ctypes.data_as(c_double_p), out_w,
            code.ctypes.data_as(C.POINTER(C.c_int32)))
    if device:
        err = C.create_string_buffer(256)
        r = getattr(lib(), "probe_run_" + name)(*args, err)
        if r:
            raise RuntimeError("probe_run_%s failed: %d %s" % (name, r, err.value.decode(errors="replace")))
    else:
        from tests.emul import pyemul
        r = getattr(pyemul.wall_lib() if name == "wall" else pyemul.lib(), "emul_probe_run_" + name)(*args)
        if r:
            raise RuntimeError("emul_probe_run_%s failed: %d" % (name, r))
    return out, code


def run_wall(problem, x, device=True):
    """Op WALL on the rows x [n, WALL_IN] (WALL_COLS): (out [n, WALL_OUT], code [n]); out[:, :WALL_HEAD] are WALL_HEAD_COLS, then
    WALL_K trail entries of WALL_TRAIL_COLS.  The last five trail columns (the kind of the unit) are filled by the host compile only
    (-1 on the device)."""
    return _run_leak(problem, "wall", x, WALL_IN, WALL_OUT, device)


def run_outer(problem, x, device=True):
    """Op OUTER on the rows x [n, OUTER_IN] (OUTER_COLS): (out [n, 4] = return value, ox, oy, oz; code [n])"""
    return _run_leak(problem, "outer", x, OUTER_IN, OUTER_OUT, device)


def run_hex(problem, x, device=True):
    """Op HEX on the rows x [n, 3] = x, y, zz: (out [n, 2] = q, r; code [n])"""
    return _run_leak(problem, "hex", x, HEX_IN, HEX_OUT, device)


# the ops of a photon's two ends (probe_ops.h): sampler primitives, pc_launch_init, pc_in_exit_window
SINCOS_IN, SINCOS_OUT = 1, 2
UNIFORM_IN, UNIFORM_OUT, UNIFORM_D = 6, 1, 4095
UNIFORM_COLS = ("seed_lo", "seed_hi", "slot_lo", "slot_hi", "attempt", "d")
ENTER_IN = 9
ENTER_COLS = MARCH_COLS[:9]
ENTER_OUT_COLS = ("state", "rc", "q", "r", "qr", "kx", "ky", "kn", "bnd", "i", "Px", "Py", "Pz", "dx", "dy", "dz", "ex", "ey", "ez",
                  "first", "lv", "idzd", "sx", "sy", "ox", "oy", "irefl", "dtravel", "C0", "w0", "wset")
ENTER_OUT = len(ENTER_OUT_COLS)
EXIT_IN, EXIT_OUT = 6, 1
EXIT_COLS = ("Px", "Py", "Pz", "dx", "dy", "dz")


def run_sincos(problem, x, device=True):
    """Op SINCOS on x [n]: out [n, 2] = sn, cs of pc_sincos_quadrant"""
    return _run_leak(problem, "sincos", x, SINCOS_IN, SINCOS_OUT, device)[0]


def uniform_rows(seed, slot, attempt, d):
    """rows of op UNIFORM from Python integers (broadcast): the 64-bit seed and slot split into 32-bit halves"""
    seed, slot, attempt, d = np.broadcast_arrays(np.asarray(seed, dtype=object), np.asarray(slot, dtype=object),
                                                 np.asarray(attempt, dtype=object), np.asarray(d, dtype=object))
    M = 0xffffffff
    return np.array([[int(s) & M, int(s) >> 32, int(t) & M, int(t) >> 32, int(a), int(k)]
                     for s, t, a, k in zip(seed.ravel(), slot.ravel(), attempt.ravel(), d.ravel())], dtype=np.float64)


def run_uniform(problem, x, device=True):
    """Op UNIFORM on the rows x [n, 6] (UNIFORM_COLS; uniform_rows): out [n] = uniform #d of the stream"""
    return _run_leak(problem, "uniform", x, UNIFORM_IN, UNIFORM_OUT, device)[0][:, 0]


def run_enter(problem, x, device=True):
    """Op ENTER on the rows x [n, 9] (ENTER_COLS): (out [n, ENTER_OUT] of ENTER_OUT_COLS, code [n] = rc)"""
    return _run_leak(problem, "enter", x, ENTER_IN, ENTER_OUT, device)


def run_exit(problem, x, device=True):
    """Op EXIT on the rows x [n, 6] (EXIT_COLS): out [n] = pc_in_exit_window"""
    return _run_leak(problem, "exit", x, EXIT_IN, EXIT_OUT, device)[0][:, 0]


def wall_trail(row):
    """trail of one WALL output row: array [units recorded, WALL_ENTRY]"""
    nt = min(int(row[WALL_HEAD_COLS.index("units")]), WALL_K)
    return row[WALL_HEAD:WALL_HEAD + WALL_ENTRY * nt].reshape(nt, WALL_ENTRY)


def wall_shared(out):
    """the part of WALL output rows both builds fill: the head and the first WALL_SHARED columns of every trail entry"""
    tr = out[:, WALL_HEAD:].reshape(out.shape[0], WALL_K, WALL_ENTRY)[:, :, :WALL_SHARED]
    return np.concatenate([out[:, :WALL_HEAD], tr.reshape(out.shape[0], -1)], axis=1)


def energy_consts(problem):
    """pc_energy_const of every energy as pc_build_tables makes it: dict of arrays named after the struct's fields."""
    from tests.emul import pyemul
    a = np.zeros((problem.n_energies, len(EC_FIELDS)))
    r = pyemul.lib().emul_energy_consts(C.byref(problem.s), a.ctypes.data_as(c_double_p))
    if r:
        raise RuntimeError("emul_energy_consts failed: %d" % r)
    return {k: a[:, j].copy() for j, k in enumerate(EC_FIELDS)}
