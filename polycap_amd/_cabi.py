"""ctypes declarations of the thin HIP C-ABI (include/polycap-hip.h) and of libpolycap's loader.

The library is built in-tree (polycap_amd/lib/libpolycap.so) by polycap_amd._build / __graft_entry__.build().
There is no Python or CPU fallback for the trace path: if the shared library is missing, import fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POLYCAP_AMD_LIB") or os.path.join(_HERE, "lib", "libpolycap.so")   # override: A/B builds only

c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)

PC_HIP_OK = 0
PC_HIP_ERR_NO_DEVICE = -1
PC_HIP_ERR_INVALID = -2
PC_HIP_ERR_RUNTIME = -3
PC_HIP_ERR_MEMORY = -4
PC_HIP_ERR_ATTEMPTS = -5
PC_HIP_LEAK_HDR = 12   # doubles before the weights of one leak event (include/polycap-hip.h)


class ErrS(C.Structure):
    """polycap_error (include/polycap.h); the one ctypes type every binding module uses for it"""
    _fields_ = [("code", C.c_int), ("message", C.c_char_p)]


class ProblemS(C.Structure):
    """struct pc_hip_problem"""
    _fields_ = [("nmax", C.c_int32), ("z", c_double_p), ("cap", c_double_p), ("ext", c_double_p),
                ("sig_rough", C.c_double), ("n_cap", C.c_int64), ("density", C.c_double),
                ("n_energies", C.c_size_t), ("energies", c_double_p), ("amu", c_double_p), ("scatf", c_double_p),
                ("d_source", C.c_double), ("src_x", C.c_double), ("src_y", C.c_double),
                ("src_sigx", C.c_double), ("src_sigy", C.c_double),
                ("src_shiftx", C.c_double), ("src_shifty", C.c_double), ("hor_pol", C.c_double)]


class ImagesS(C.Structure):
    """struct pc_hip_images"""
    _fields_ = [("src_start_coords", c_double_p * 2), ("pc_start_coords", c_double_p * 2),
                ("pc_start_dir", c_double_p * 2), ("pc_start_elecv", c_double_p * 2),
                ("pc_exit_coords", c_double_p * 3), ("pc_exit_dir", c_double_p * 2),
                ("pc_exit_elecv", c_double_p * 2), ("pc_exit_nrefl", c_int64_p),
                ("pc_exit_dtravel", c_double_p), ("exit_coord_weights", c_double_p)]


class SpotSpecS(C.Structure):
    """struct pc_hip_spot_spec"""
    _fields_ = [("n_planes", C.c_int32), ("distances", c_double_p), ("x0", C.c_double), ("x1", C.c_double),
                ("y0", C.c_double), ("y1", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("n_energies", C.c_int32), ("energies", C.POINTER(C.c_int32)), ("regime", C.c_int32)]


class HistAxisS(C.Structure):
    """struct pc_hip_hist_axis"""
    _fields_ = [("quantity", C.c_int32), ("d", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("lo", C.c_double), ("hi", C.c_double), ("n_bins", C.c_int32)]


class HistSpecS(C.Structure):
    """struct pc_hip_hist_spec"""
    _fields_ = [("n_axes", C.c_int32), ("axes", C.POINTER(HistAxisS)), ("n_energies", C.c_int32),
                ("energies", C.POINTER(C.c_int32)), ("regime", C.c_int32)]


class JointPairS(C.Structure):
    """struct pc_hip_joint_pair"""
    _fields_ = [("u", HistAxisS), ("v", HistAxisS)]


class JointSpecS(C.Structure):
    """struct pc_hip_joint_spec"""
    _fields_ = [("n_pairs", C.c_int32), ("pairs", C.POINTER(JointPairS)), ("n_energies", C.c_int32),
                ("energies", C.POINTER(C.c_int32)), ("regime", C.c_int32)]


class SelectCutS(C.Structure):
    """struct pc_hip_select_cut"""
    _fields_ = [("axis", HistAxisS), ("negate", C.c_int32)]


class SelectSpecS(C.Structure):
    """struct pc_hip_select_spec"""
    _fields_ = [("n_cuts", C.c_int32), ("cuts", C.POINTER(SelectCutS))]


class EmitS(C.Structure):
    """struct pc_hip_emit"""
    _fields_ = [("focus", C.c_double), ("sample_angle", C.c_double), ("depth", C.c_double), ("det_angle", C.c_double),
                ("wd", C.c_double), ("off_u", C.c_double), ("off_v", C.c_double), ("target_half", C.c_double),
                ("seed", C.c_uint64), ("n_map", C.c_int32), ("map", C.POINTER(C.c_int32))]


class SlabS(C.Structure):
    """struct pc_hip_slab"""
    _fields_ = [("emit", EmitS), ("thickness", C.c_double), ("n_mu_in", C.c_int32), ("mu_in", c_double_p),
                ("n_mu_out", C.c_int32), ("mu_out", c_double_p)]


class LayersS(C.Structure):
    """struct pc_hip_layers"""
    _fields_ = [("emit", EmitS), ("n_layers", C.c_int32), ("thickness", c_double_p), ("n_mu_in", C.c_int32), ("mu_in", c_double_p),
                ("n_mu_out", C.c_int32), ("mu_out", c_double_p), ("production", c_double_p)]


def dptr(a):
    return a.ctypes.data_as(c_double_p)


# column order of the [n, 17] image array of TraceContext.images(): planes of struct pc_hip_images, nrefl as column 15
IMAGE_PLANES = [("src_start_coords", 2), ("pc_start_coords", 2), ("pc_start_dir", 2), ("pc_start_elecv", 2),
                ("pc_exit_coords", 3), ("pc_exit_dir", 2), ("pc_exit_elecv", 2)]


def images_struct(planes, nrefl, weights):
    """pc_hip_images over planes [17, n] (row 16 = d_travel; row 15 unused), nrefl [n] int64, weights [n, nE]."""
    s = ImagesS()
    k = 0
    for name, m in IMAGE_PLANES:
        arr = getattr(s, name)
        for j in range(m):
            arr[j] = dptr(planes[k])
            k += 1
    s.pc_exit_nrefl = nrefl.ctypes.data_as(c_int64_p)
    s.pc_exit_dtravel = dptr(planes[16])
    s.exit_coord_weights = dptr(weights)
    return s


class Problem:
    """Owns the numpy arrays behind a pc_hip_problem."""

    def __init__(self, z, cap, ext, sig_rough, n_cap, density, energies, amu, scatf,
                 d_source=2000.0, src_x=0.2065, src_y=0.2065, src_sigx=0.0, src_sigy=0.0,
                 src_shiftx=0.0, src_shifty=0.0, hor_pol=0.0):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.z, self.cap, self.ext = f(z), f(cap), f(ext)
        self.energies, self.amu, self.scatf = f(energies).ravel(), f(amu).ravel(), f(scatf).ravel()
        if not (self.z.shape == self.cap.shape == self.ext.shape and self.z.ndim == 1):
            raise ValueError("z, cap, ext must be 1-D arrays of equal length")
        if not (self.energies.shape == self.amu.shape == self.scatf.shape):
            raise ValueError("energies, amu, scatf must have equal length")
        self.nmax = self.z.shape[0] - 1
        self.n_energies = self.energies.shape[0]
        self.sig_rough, self.n_cap, self.density = float(sig_rough), int(n_cap), float(density)
        self.source = (float(d_source), float(src_x), float(src_y), float(src_sigx), float(src_sigy),
                       float(src_shiftx), float(src_shifty), float(hor_pol))
        self.s = ProblemS(self.nmax, dptr(self.z), dptr(self.cap), dptr(self.ext),
                          self.sig_rough, self.n_cap, self.density,
                          self.n_energies, dptr(self.energies), dptr(self.amu), dptr(self.scatf), *self.source)


_LIB = None


def lib():
    """Loads libpolycap.so (host C + HIP kernels). Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "polycap_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the trace path." % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    P = C.POINTER
    L.pc_hip_device_count.restype = C.c_int
    L.pc_hip_last_error.restype = C.c_char_p
    L.pc_hip_ctx_create.argtypes = [P(ProblemS), C.c_int, P(C.c_void_p)]
    L.pc_hip_ctx_create.restype = C.c_int
    L.pc_hip_ctx_destroy.argtypes = [C.c_void_p]
    L.pc_hip_ctx_destroy.restype = None
    L.pc_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.pc_hip_set_option.restype = C.c_int
    L.pc_hip_launch_photons.argtypes = [C.c_void_p, C.c_int64, c_double_p, c_double_p, c_double_p,
                                        P(C.c_int32), c_double_p, c_double_p, c_double_p, c_double_p,
                                        c_int64_p, c_double_p]
    L.pc_hip_launch_photons.restype = C.c_int
    L.pc_hip_launch_photons_leak.argtypes = L.pc_hip_launch_photons.argtypes
    L.pc_hip_launch_photons_leak.restype = C.c_int
    L.pc_hip_transmission_run_leak.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
    L.pc_hip_transmission_run_leak.restype = C.c_int
    L.pc_hip_leak_counts.argtypes = [C.c_void_p, c_int64_p, c_int64_p]
    L.pc_hip_leak_counts.restype = C.c_int
    L.pc_hip_leak_events.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p]
    L.pc_hip_leak_events.restype = C.c_int
    L.pc_hip_leak_events_view.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_double)), c_int64_p]
    L.pc_hip_leak_events_view.restype = C.c_int
    L.pc_hip_sample_photons.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, c_int64_p, P(C.c_uint32), c_double_p]
    L.pc_hip_sample_photons.restype = C.c_int
    L.pc_hip_transmission_run.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
    L.pc_hip_transmission_run.restype = C.c_int
    L.pc_hip_transmission_wait.argtypes = [C.c_void_p, P(C.c_float)]
    L.pc_hip_transmission_wait.restype = C.c_int
    L.pc_hip_transmission_totals.argtypes = [C.c_void_p, c_double_p, c_int64_p, P(C.c_uint64)]
    L.pc_hip_transmission_totals.restype = C.c_int
    L.pc_hip_transmission_images.argtypes = [C.c_void_p, C.c_int64, C.c_int64, P(ImagesS)]
    L.pc_hip_transmission_images.restype = C.c_int
    L.pc_hip_transmission_records.argtypes = [C.c_void_p, C.c_int64, C.c_int64, P(C.c_double)]
    L.pc_hip_transmission_records.restype = C.c_int
    L.pc_hip_transmission_slot_ids.argtypes = [C.c_void_p, C.c_int64, C.c_int64, c_int64_p]
    L.pc_hip_transmission_slot_ids.restype = C.c_int
    L.pc_hip_leak_set_order.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64, C.c_int64]
    L.pc_hip_leak_set_order.restype = C.c_int
    L.pc_hip_leak_slot_units.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]
    L.pc_hip_leak_slot_units.restype = C.c_int
    L.pc_hip_phase_stats.argtypes = [C.c_void_p, c_int64_p]
    L.pc_hip_phase_stats.restype = C.c_int
    L.pc_hip_last_kernel.argtypes = [C.c_void_p]
    L.pc_hip_last_kernel.restype = C.c_int
    L.pc_hip_sweep_stats.argtypes = [C.c_void_p, c_int64_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.pc_hip_sweep_stats.restype = C.c_int
    L.pc_hip_device_synchronize.argtypes = [C.c_void_p]
    L.pc_hip_device_synchronize.restype = C.c_int
    L.pc_hip_group_create.argtypes = [P(ProblemS), C.c_int, P(C.c_int), P(C.c_void_p)]
    L.pc_hip_group_create.restype = C.c_int
    L.pc_hip_group_destroy.argtypes = [C.c_void_p]
    L.pc_hip_group_destroy.restype = None
    L.pc_hip_group_size.argtypes = [C.c_void_p]
    L.pc_hip_group_size.restype = C.c_int
    L.pc_hip_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.pc_hip_group_set_option.restype = C.c_int
    L.pc_hip_group_run.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_int]
    L.pc_hip_group_run.restype = C.c_int
    L.pc_hip_group_run_leak.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_int]
    L.pc_hip_group_run_leak.restype = C.c_int
    L.pc_hip_group_last_kernel.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_group_last_kernel.restype = C.c_int
    L.pc_hip_group_images.argtypes = [C.c_void_p, P(ImagesS)]
    L.pc_hip_group_images.restype = C.c_int
    L.pc_hip_group_totals.argtypes = [C.c_void_p, C.c_int, c_double_p, c_int64_p, P(C.c_uint64), P(C.c_int), P(C.c_float)]
    L.pc_hip_group_totals.restype = C.c_int
    L.pc_hip_transmission_moments.argtypes = [C.c_void_p, P(C.c_uint64)]
    L.pc_hip_transmission_moments.restype = C.c_int
    L.pc_hip_group_moments.argtypes = [C.c_void_p, P(C.c_uint64)]
    L.pc_hip_group_moments.restype = C.c_int
    L.pc_hip_efficiency_stderr.argtypes = [C.c_size_t, P(C.c_uint64), P(C.c_uint64), c_int64_p, c_double_p]
    L.pc_hip_efficiency_stderr.restype = None
    L.pc_hip_efficiencies.argtypes = [C.c_size_t, c_double_p, c_int64_p, c_double_p]
    L.pc_hip_efficiencies.restype = None
    L.pc_hip_fixed_to_double.argtypes = [C.c_uint64, C.c_uint64]
    L.pc_hip_fixed_to_double.restype = C.c_double
    L.pc_hip_spot_validate.argtypes = [P(SpotSpecS), C.c_size_t]
    L.pc_hip_spot_validate.restype = C.c_int
    L.pc_hip_spot_create.argtypes = [C.c_void_p, P(SpotSpecS), P(C.c_void_p)]
    L.pc_hip_spot_create.restype = C.c_int
    L.pc_hip_group_spot_create.argtypes = [C.c_void_p, P(SpotSpecS), P(C.c_void_p)]
    L.pc_hip_group_spot_create.restype = C.c_int
    L.pc_hip_spot_destroy.argtypes = [C.c_void_p]
    L.pc_hip_spot_destroy.restype = None
    L.pc_hip_spot_add.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_spot_add.restype = C.c_int
    L.pc_hip_spot_read.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), c_int64_p]
    L.pc_hip_spot_read.restype = C.c_int
    L.pc_hip_spot_reset.argtypes = [C.c_void_p]
    L.pc_hip_spot_reset.restype = C.c_int
    L.pc_hip_spot_info.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int)]
    L.pc_hip_spot_info.restype = C.c_int
    L.pc_hip_beam_create.argtypes = [C.c_void_p, P(C.c_void_p)]
    L.pc_hip_beam_create.restype = C.c_int
    L.pc_hip_group_beam_create.argtypes = [C.c_void_p, P(C.c_void_p)]
    L.pc_hip_group_beam_create.restype = C.c_int
    L.pc_hip_beam_destroy.argtypes = [C.c_void_p]
    L.pc_hip_beam_destroy.restype = None
    L.pc_hip_beam_add.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_beam_add.restype = C.c_int
    L.pc_hip_beam_read.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), c_int64_p]
    L.pc_hip_beam_read.restype = C.c_int
    L.pc_hip_beam_reset.argtypes = [C.c_void_p]
    L.pc_hip_beam_reset.restype = C.c_int
    L.pc_hip_beam_info.argtypes = [C.c_void_p, P(C.c_int)]
    L.pc_hip_beam_info.restype = C.c_int
    L.pc_hip_beam_params.argtypes = [C.c_size_t, P(C.c_uint64), c_double_p]
    L.pc_hip_beam_params.restype = None
    L.pc_hip_beam_at.argtypes = [C.c_size_t, P(C.c_uint64), C.c_size_t, c_double_p, c_double_p]
    L.pc_hip_beam_at.restype = None
    L.pc_hip_beam_columns.argtypes = []
    L.pc_hip_beam_columns.restype = C.c_char_p
    L.pc_hip_hist_validate.argtypes = [P(HistSpecS), C.c_size_t]
    L.pc_hip_hist_validate.restype = C.c_int
    L.pc_hip_hist_create.argtypes = [C.c_void_p, P(HistSpecS), P(C.c_void_p)]
    L.pc_hip_hist_create.restype = C.c_int
    L.pc_hip_group_hist_create.argtypes = [C.c_void_p, P(HistSpecS), P(C.c_void_p)]
    L.pc_hip_group_hist_create.restype = C.c_int
    L.pc_hip_hist_destroy.argtypes = [C.c_void_p]
    L.pc_hip_hist_destroy.restype = None
    L.pc_hip_hist_add.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_hist_add.restype = C.c_int
    L.pc_hip_hist_read.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), c_int64_p]
    L.pc_hip_hist_read.restype = C.c_int
    L.pc_hip_hist_reset.argtypes = [C.c_void_p]
    L.pc_hip_hist_reset.restype = C.c_int
    L.pc_hip_hist_info.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int32), P(C.c_int)]
    L.pc_hip_hist_info.restype = C.c_int
    L.pc_hip_hist_quantile.argtypes = [C.c_int32, C.c_double, C.c_double, P(C.c_uint64), C.c_uint64, C.c_double]
    L.pc_hip_hist_quantile.restype = C.c_double
    L.pc_hip_hist_fwhm.argtypes = [C.c_int32, C.c_double, C.c_double, P(C.c_uint64), c_double_p, c_double_p]
    L.pc_hip_hist_fwhm.restype = C.c_double
    L.pc_hip_joint_validate.argtypes = [P(JointSpecS), C.c_size_t]
    L.pc_hip_joint_validate.restype = C.c_int
    L.pc_hip_joint_create.argtypes = [C.c_void_p, P(JointSpecS), P(C.c_void_p)]
    L.pc_hip_joint_create.restype = C.c_int
    L.pc_hip_group_joint_create.argtypes = [C.c_void_p, P(JointSpecS), P(C.c_void_p)]
    L.pc_hip_group_joint_create.restype = C.c_int
    L.pc_hip_joint_destroy.argtypes = [C.c_void_p]
    L.pc_hip_joint_destroy.restype = None
    L.pc_hip_joint_add.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_joint_add.restype = C.c_int
    L.pc_hip_joint_read.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), c_int64_p]
    L.pc_hip_joint_read.restype = C.c_int
    L.pc_hip_joint_reset.argtypes = [C.c_void_p]
    L.pc_hip_joint_reset.restype = C.c_int
    L.pc_hip_joint_info.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int32), P(C.c_int)]
    L.pc_hip_joint_info.restype = C.c_int
    L.pc_hip_joint_marginal.argtypes = [C.c_int32, C.c_int32, P(C.c_uint64), C.c_int, P(C.c_uint64)]
    L.pc_hip_joint_marginal.restype = C.c_int
    L.pc_hip_joint_parse.argtypes = [C.c_char_p, C.c_size_t, P(JointPairS), P(C.c_int32), P(C.c_int32), P(C.c_int32), C.c_char_p, C.c_size_t]
    L.pc_hip_joint_parse.restype = C.c_int
    L.pc_hip_select_validate.argtypes = [P(SelectSpecS)]
    L.pc_hip_select_validate.restype = C.c_int
    L.pc_hip_select_create.argtypes = [C.c_void_p, P(SelectSpecS), P(C.c_void_p)]
    L.pc_hip_select_create.restype = C.c_int
    L.pc_hip_group_select_create.argtypes = [C.c_void_p, P(SelectSpecS), P(C.c_void_p)]
    L.pc_hip_group_select_create.restype = C.c_int
    L.pc_hip_select_destroy.argtypes = [C.c_void_p]
    L.pc_hip_select_destroy.restype = None
    L.pc_hip_select_apply.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_select_apply.restype = C.c_int
    L.pc_hip_select_read.argtypes = [C.c_void_p, c_int64_p, c_int64_p, P(C.c_uint64), P(C.c_uint64)]
    L.pc_hip_select_read.restype = C.c_int
    L.pc_hip_select_info.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int32), P(SelectCutS)]
    L.pc_hip_select_info.restype = C.c_int
    L.pc_hip_select_gather.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, c_int64_p]
    L.pc_hip_select_gather.restype = C.c_int
    L.pc_hip_select_draw.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_int64, C.c_int64, c_double_p, c_int64_p, P(C.c_uint64)]
    L.pc_hip_select_draw.restype = C.c_int
    for stem in ("spot", "beam", "hist", "joint"):
        fn = getattr(L, "pc_hip_%s_add_selected" % stem)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        fn.restype = C.c_int
    L.pc_hip_select_parse.argtypes = [C.c_char_p, P(SelectCutS), P(C.c_int32), C.c_char_p, C.c_size_t]
    L.pc_hip_select_parse.restype = C.c_int
    for stem in ("spot", "hist", "joint", "select"):
        fn = getattr(L, "pc_hip_%s_track_squares" % stem)
        fn.argtypes = [C.c_void_p]
        fn.restype = C.c_int
        fn = getattr(L, "pc_hip_%s_read_squares" % stem)
        fn.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64)]
        fn.restype = C.c_int
    L.pc_hip_tally_stderr.argtypes = [C.c_size_t, P(C.c_uint64), P(C.c_uint64), C.c_int64, c_double_p]
    L.pc_hip_tally_stderr.restype = None
    L.pc_hip_select_transmission.argtypes = [C.c_size_t, P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), c_double_p, c_double_p]
    L.pc_hip_select_transmission.restype = None
    L.pc_hip_device_memory.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64)]
    L.pc_hip_device_memory.restype = C.c_int
    u64p = P(C.c_uint64)
    L.pc_hip_scan_validate.argtypes = [c_double_p, C.c_int64, C.c_int64]     # points: [P, 3] doubles = pc_hip_scan_point[P]
    L.pc_hip_scan_validate.restype = C.c_int
    L.pc_hip_scan_run.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, c_double_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32]
    L.pc_hip_scan_run.restype = C.c_int
    L.pc_hip_scan_wait.argtypes = [C.c_void_p, P(C.c_float)]
    L.pc_hip_scan_wait.restype = C.c_int
    L.pc_hip_scan_last_kernel.argtypes = [C.c_void_p]
    L.pc_hip_scan_last_kernel.restype = C.c_int
    L.pc_hip_group_scan_last_kernel.argtypes = [C.c_void_p, C.c_int]
    L.pc_hip_group_scan_last_kernel.restype = C.c_int
    L.pc_hip_scan_totals.argtypes = [C.c_void_p, c_int64_p, u64p, u64p]
    L.pc_hip_scan_totals.restype = C.c_int
    L.pc_hip_scan_efficiencies.argtypes = [C.c_size_t, C.c_int64, c_int64_p, u64p, u64p, c_double_p, c_double_p]
    L.pc_hip_scan_efficiencies.restype = None
    L.pc_hip_group_scan_run.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, c_double_p, C.c_int64, C.c_int64, C.c_uint32]
    L.pc_hip_group_scan_run.restype = C.c_int
    L.pc_hip_group_scan_wait.argtypes = [C.c_void_p, P(C.c_float)]
    L.pc_hip_group_scan_wait.restype = C.c_int
    L.pc_hip_group_scan_totals.argtypes = [C.c_void_p, c_int64_p, u64p, u64p]
    L.pc_hip_group_scan_totals.restype = C.c_int
    L.pc_hip_relay_validate.argtypes = [c_double_p]                          # placement: 3 doubles = pc_hip_relay_placement
    L.pc_hip_relay_validate.restype = C.c_int
    L.pc_hip_relay_run.argtypes = [C.c_void_p, C.c_void_p, c_double_p]
    L.pc_hip_relay_run.restype = C.c_int
    L.pc_hip_relay_totals.argtypes = [C.c_void_p, c_int64_p, u64p, u64p]
    L.pc_hip_relay_totals.restype = C.c_int
    L.pc_hip_relay_efficiencies.argtypes = [C.c_size_t, u64p, u64p, c_int64_p, c_double_p, c_double_p]
    L.pc_hip_relay_efficiencies.restype = None
    L.pc_hip_pose_validate.argtypes = [c_double_p]                           # pose: 5 doubles = pc_hip_pose
    L.pc_hip_pose_validate.restype = C.c_int
    L.pc_hip_pose_basis.argtypes = [c_double_p, c_double_p]
    L.pc_hip_pose_basis.restype = C.c_int
    L.pc_hip_pose_run.argtypes = [C.c_void_p, C.c_void_p, c_double_p, C.c_void_p]
    L.pc_hip_pose_run.restype = C.c_int
    L.pc_hip_pose_counts.argtypes = [C.c_void_p, c_int64_p]
    L.pc_hip_pose_counts.restype = C.c_int
    L.pc_hip_emit_validate.argtypes = [P(EmitS)]
    L.pc_hip_emit_validate.restype = C.c_int
    L.pc_hip_emit_frame.argtypes = [P(EmitS), c_double_p]
    L.pc_hip_emit_frame.restype = C.c_int
    L.pc_hip_emit_run.argtypes = [C.c_void_p, C.c_void_p, P(EmitS), C.c_void_p]
    L.pc_hip_emit_run.restype = C.c_int
    L.pc_hip_emit_counts.argtypes = [C.c_void_p, c_int64_p]
    L.pc_hip_emit_counts.restype = C.c_int
    L.pc_hip_slab_validate.argtypes = [P(SlabS)]
    L.pc_hip_slab_validate.restype = C.c_int
    L.pc_hip_slab_frame.argtypes = [P(SlabS), c_double_p]
    L.pc_hip_slab_frame.restype = C.c_int
    L.pc_hip_slab_run.argtypes = [C.c_void_p, C.c_void_p, P(SlabS), C.c_void_p]
    L.pc_hip_slab_run.restype = C.c_int
    L.pc_hip_layers_validate.argtypes = [P(LayersS)]
    L.pc_hip_layers_validate.restype = C.c_int
    L.pc_hip_layers_frame.argtypes = [P(LayersS), c_double_p]
    L.pc_hip_layers_frame.restype = C.c_int
    L.pc_hip_layers_run.argtypes = [C.c_void_p, C.c_void_p, P(LayersS), C.c_void_p]
    L.pc_hip_layers_run.restype = C.c_int
    L.pc_transmission_efficiencies_from_totals.argtypes = [C.c_void_p, C.c_int64, c_double_p, c_int64_p, P(ImagesS), C.c_void_p]
    L.pc_transmission_efficiencies_from_totals.restype = C.c_void_p
    _LIB = L
    return L
