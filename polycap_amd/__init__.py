"""polycap_amd -- MI355X-native implementation of polycap's per-photon Monte-Carlo trace path.

The package is a thin Python layer over libpolycap.so (host C + hand-written HIP kernels for gfx950):
  * polycap_amd.hip.TraceContext  -- the thin HIP C-ABI (include/polycap-hip.h): explicit photon batches,
    device-side source sampling and the slot-range transmission driver;
  * polycap_amd.hip.SpotMap       -- spot maps: 2-D histograms of the photons of a run on planes behind the optic, on the GPU;
  * polycap_amd.hip.Histograms    -- exact 1-D histograms of per-photon quantities per energy (FWHM, encircled energy), on the GPU;
  * polycap_amd.hip.Selection -- cuts on per-photon quantities evaluated on the GPU, through which any of the tallies is filled;
    Selection.gather fetches the per-photon data of the selected photons alone, compacted in order on the GPU;
    Selection.draw an unweighted sample of them, n photons of equal weight, resampled in exact integers on the GPU;
  * polycap_amd.hip.JointHistograms -- exact joint 2-D histograms of two per-photon quantities per energy (phase space), on the GPU;
  * polycap_amd.hip.BeamMoments   -- exact exit-beam moments per energy (focal distance, waist, divergence), on the GPU;
  * TraceContext.scan / scan_points -- transmission per source position (alignment curves, focal spot, depth response) in one
    launch, exact totals per point;
  * TraceContext.relay            -- the exit beam of one optic through a second one (confocal set-ups), on the GPU;
    the second optic may be tilted and a Selection may stand between the two as an aperture (relay_rocking_curve);
  * TraceContext.emit             -- a thin sample between the two optics: the first one's exit photons re-emit isotropically
    in the sheet and the second optic, at 90 degrees as a rule, collects (emit_frame, emit_valid, emit_depth_scan); with
    thickness, mu_in and mu_out the sample is a slab that attenuates both ways (emit_slab_frame, emit_slab_valid); with layers
    it is a stack of layers, each with its attenuation and its production coefficient (emit_layers_frame, emit_layers_valid);
  * polycap_amd.capi              -- ctypes mirror of the reference's C API (polycap_profile/_description/
    _source/_photon/...), i.e. what the reference's Cython module binds;
  * polycap_amd.distributed       -- one-process-per-GPU sharding of the slot range + RCCL reduce of the
    per-energy histogram.
There is no CPU implementation of the trace path in this package.
"""
from ._cabi import Problem, lib  # noqa: F401
from .hip import TraceContext, TraceGroup, SpotMap, BeamMoments, Histograms, JointHistograms, Selection, select_cuts, select_parse, select_all, joint_marginal, joint_parse, hist_fwhm, hist_quantile, beam_params, HipError, device_count, efficiencies, efficiency_stderr, fixed_to_double, IMG_FIELDS  # noqa: F401
from .hip import scan_points, scan_efficiencies  # noqa: F401
from .hip import tally_stderr, select_transmission, pairs_sum  # noqa: F401
from .hip import relay_efficiencies, relay_placement_valid, relay_basis, relay_rocking_curve, RELAY_COUNTERS  # noqa: F401
from .hip import emit_valid, emit_frame, emit_depth_scan, emit_slab_valid, emit_slab_frame, emit_layers_valid, emit_layers_frame  # noqa: F401
from .decks import problem_from_inp, optical_constants, optical_constants_provider  # noqa: F401

__version__ = "1.2"
