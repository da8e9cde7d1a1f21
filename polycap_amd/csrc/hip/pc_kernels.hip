/*
 * pc_kernels.hip -- gfx950 kernels of the photon trace path + the thin C-ABI of include/polycap-hip.h.
 * The library's one translation unit: nothing but its headers, in the order in which they depend on each other.
 *
 * Kernel shape (CDNA4, wave64):
 *   - persistent waves: grid = CUs x resident blocks; every wave pulls chunks of exit-photon slots from one
 *     global counter, every lane owns one slot at a time and retries it until a photon is transmitted
 *     (reference driver loop src/polycap-source.c:744-884);
 *   - profile tables (z, cap, zh, cap^2, hexd: 5 x (nmax+1) fp64 = 40 KB for nmax=999) are staged once per
 *     workgroup into LDS; per-energy constants are wave-uniform scalar loads;
 *   - the photon life cycle is scheduled wave-wide by phase (MARCH / EVENT / NEW) with ballots so that the
 *     expensive, rare code (segment quadratic + Fresnel, source sampling) runs with many active lanes;
 *   - totals are accumulated in exact 128-bit fixed point, so they do not depend on scheduling or on how
 *     slots are split over devices.
 * No MFMA: there is no dense contraction in this path.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "polycap-hip.h"
#include "pc_device.h"
#include "pc_leak.h"
#include "pc_problem.h"
#include "pc_moments.h"
#include "pc_plan.h"
#include "pc_exact.h"
#include "pc_totals.h"          /* struct pc_totals: the block the kernels add to */
#include "pc_host.h"            /* the error text and the owners of GPU resources */
#include "pc_kargs.h"           /* what every trace kernel is launched with */
#include "pc_images.h"          /* the record fields the kernels write; the store and the fetch need the owners and pc_kargs */
#include "pc_trace_kernel.h"
#include "pc_pool_kernel.h"
#include "pc_producer_kernel.h"
#include "pc_wave_kernel.h"     /* empty without -DPC_EXPERIMENTS */
#include "pc_sweep_kernel.h"
#include "pc_leak_run.h"        /* struct pc_leak_run, ahead of the context that holds it */
#include "pc_sweep_cert.h"
#include "pc_ctx.h"
#include "pc_launch.h"
#include "pc_leak_kernels.h"
#include "pc_leak_run.h"        /* the one header included twice: its functions need the context, the launch code and the leak kernels */
#include "pc_options.h"
#include "pc_batch.h"
#include "pc_run.h"
#include "pc_group.h"
#include "pc_tally.h"
#include "pc_spot.h"
#include "pc_beam.h"
#include "pc_hist.h"            /* with pc_cells.h, which it includes between its host part and its C functions */
#include "pc_joint.h"
#include "pc_select.h"
#include "pc_gather.h"
#include "pc_draw.h"
#include "pc_scan.h"
#include "pc_relay.h"
#include "pc_emit.h"
#include "pc_emit_layers.h"
