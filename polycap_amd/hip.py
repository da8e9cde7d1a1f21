"""Python front-end of the thin HIP C-ABI (include/polycap-hip.h): numpy in, numpy out.

TraceContext wraps one pc_hip_ctx (problem resident on one GPU).  Everything here calls into
libpolycap.so; nothing is computed in Python and nothing falls back to the CPU.
"""
import ctypes as C

import numpy as np

from . import _cabi
from ._cabi import Problem, dptr, c_int64_p


class HipError(RuntimeError):
    def __init__(self, where, status):
        msg = _cabi.lib().pc_hip_last_error()
        super().__init__("%s failed (%d): %s" % (where, status, msg.decode() if msg else ""))
        self.status = status


def device_count():
    return int(_cabi.lib().pc_hip_device_count())


IMG_FIELDS = ("src_start_x", "src_start_y", "pc_start_x", "pc_start_y", "pc_start_dir_x", "pc_start_dir_y",
              "pc_start_elecv_x", "pc_start_elecv_y", "pc_exit_x", "pc_exit_y", "pc_exit_z",
              "pc_exit_dir_x", "pc_exit_dir_y", "pc_exit_elecv_x", "pc_exit_elecv_y", "nrefl", "dtravel")


class TraceContext:
    """One problem (optic + glass + energies + source) uploaded to one MI355X."""

    def __init__(self, problem, device=0):
        if not isinstance(problem, Problem):
            raise TypeError("problem must be a polycap_amd.Problem")
        self.problem = problem
        self._L = _cabi.lib()
        h = C.c_void_p()
        st = self._L.pc_hip_ctx_create(C.byref(problem.s), int(device), C.byref(h))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_ctx_create", st)
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pc_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, name, value):
        st = self._L.pc_hip_set_option(self._h, name.encode(), int(value))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_set_option", st)
        if name == "weight_squares":
            self._weight_squares = bool(value)

    def scan(self, seed, points, n_per_point, max_attempts=1, slot0=0, first=0, count=None):
        """Transmission per source position in one launch (pc_hip_scan_run; the contract is in include/polycap-hip.h): points
        [P, 3] of (d_source, src_shiftx, src_shifty), e.g. from scan_points() (NaN d_source = the problem's own); n_per_point
        slots per point, slot j of every point on the stream of slot slot0 + j; the flat indices [first, first + count) are traced
        (default: all).  Returns counters [P, 6], sumw_fixed [P, ne, 2], sumw2_fixed (option "weight_squares") or None,
        efficiencies [P, ne], stderr [P, ne] or None, kernel_ms, kernel (the name of the kernel that traced the scan, from
        KERNELS: with more than 8 energies the logging kernel if option "scan_log" is 1 and the scan can log)."""
        pts = _scan_array(points, self.problem)
        n_pts = pts.shape[0]
        count = n_pts * int(n_per_point) - int(first) if count is None else int(count)
        st = self._L.pc_hip_scan_run(self._h, int(seed), int(slot0), dptr(pts), n_pts, int(n_per_point), int(first), count,
                                     int(max_attempts))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_scan_run", st)
        ms = C.c_float(0)
        st = self._L.pc_hip_scan_wait(self._h, C.byref(ms))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_scan_wait", st)
        r = _scan_fetch(self._L.pc_hip_scan_totals, self._h, n_pts, self.problem.n_energies, getattr(self, "_weight_squares", False))
        r["kernel_ms"] = float(ms.value)
        r["kernel"] = self.KERNELS.get(int(self._L.pc_hip_scan_last_kernel(self._h)))
        return r

    def device_synchronize(self):
        """hipDeviceSynchronize on the context's device (every stream)."""
        st = self._L.pc_hip_device_synchronize(self._h)
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_device_synchronize", st)

    # -- polycap_photon_launch for a batch of explicit photons
    def launch_photons(self, start, direction, elecv, leak_calc=False):
        """leak_calc=True: polycap_photon_launch(..., leak_calc=true); the events are then available from leaks()"""
        st_ = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
        di = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
        ev = np.ascontiguousarray(elecv, dtype=np.float64).reshape(-1, 3)
        n = st_.shape[0]
        ne = self.problem.n_energies
        rc = np.zeros(n, dtype=np.int32)
        w = np.zeros((n, ne))
        ec, ed, ee = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        ir = np.zeros(n, dtype=np.int64)
        dt = np.zeros(n)
        fn = self._L.pc_hip_launch_photons_leak if leak_calc else self._L.pc_hip_launch_photons
        st = fn(self._h, n, dptr(st_), dptr(di), dptr(ev),
                rc.ctypes.data_as(C.POINTER(C.c_int32)), dptr(w), dptr(ec), dptr(ed), dptr(ee),
                ir.ctypes.data_as(c_int64_p), dptr(dt))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_launch_photons_leak" if leak_calc else "pc_hip_launch_photons", st)
        return dict(rc=rc, weights=w, exit_coords=ec, exit_dir=ed, exit_elecv=ee, i_refl=ir, d_travel=dt)

    # -- polycap_source_get_photon on the device
    def sample_photons(self, seed, slots, attempts=None):
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        n = slots.shape[0]
        attempts = np.zeros(n, dtype=np.uint32) if attempts is None else np.ascontiguousarray(attempts, dtype=np.uint32)
        out = np.zeros((n, 12))
        st = self._L.pc_hip_sample_photons(self._h, int(seed), n, slots.ctypes.data_as(c_int64_p),
                                           attempts.ctypes.data_as(C.POINTER(C.c_uint32)), dptr(out))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_sample_photons", st)
        return out

    # -- polycap_source_get_transmission_efficiencies for a slot range
    def run(self, seed, slot0, n_slots, max_attempts=1 << 20, keep_images=False, leak_calc=False):
        fn = self._L.pc_hip_transmission_run_leak if leak_calc else self._L.pc_hip_transmission_run
        st = fn(self._h, int(seed), int(slot0), int(n_slots), int(max_attempts), int(bool(keep_images)))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_run_leak" if leak_calc else "pc_hip_transmission_run", st)
        self._last_n = int(n_slots)

    def leaks(self, copy=True):
        """(ext, int): the leak events of the last leak_calc run, arrays [n, 12 + nE] with columns slot, attempt,
        x, y, z, dir x y z, elecv x y z, n_refl, weights; in the reference's list order (the device puts them into it).
        copy=False: read-only views of the context's own pinned lists, valid until its next leak run."""
        out = []
        stride = _cabi.PC_HIP_LEAK_HDR + self.problem.n_energies
        for kind in (0, 1):
            ptr = C.POINTER(C.c_double)()
            n = C.c_int64(0)
            st = self._L.pc_hip_leak_events_view(self._h, kind, C.byref(ptr), C.byref(n))
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_leak_events_view", st)
            if n.value == 0:
                out.append(np.zeros((0, stride)))
                continue
            a = np.ctypeslib.as_array(ptr, shape=(n.value, stride))
            if copy:
                a = a.copy()
            else:
                a.flags.writeable = False
            out.append(a)
        return out[0], out[1]

    def device_memory(self):
        """(free, total) bytes of the context's device"""
        f, t = C.c_uint64(0), C.c_uint64(0)
        st = self._L.pc_hip_device_memory(self._h, C.byref(f), C.byref(t))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_device_memory", st)
        return int(f.value), int(t.value)

    def wait(self):
        ms = C.c_float(0)
        st = self._L.pc_hip_transmission_wait(self._h, C.byref(ms))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_wait", st)
        return float(ms.value)

    def totals(self, check=True):
        ne = self.problem.n_energies
        sw = np.zeros(ne)
        cnt = np.zeros(6, dtype=np.int64)
        fx = np.zeros(2 * ne, dtype=np.uint64)
        st = self._L.pc_hip_transmission_totals(self._h, dptr(sw), cnt.ctypes.data_as(c_int64_p),
                                                fx.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st != _cabi.PC_HIP_OK and (check or st != _cabi.PC_HIP_ERR_ATTEMPTS):
            raise HipError("pc_hip_transmission_totals", st)
        return dict(sum_weights=sw, counters=cnt, sumw_fixed=fx.reshape(ne, 2),
                    i_exit=int(cnt[0]), not_entered=int(cnt[1]), not_transmitted=int(cnt[2]), sum_irefl=int(cnt[3]),
                    failed_slots=int(cnt[4]), launches=int(cnt[5]), i_start=int(cnt[0] + cnt[1] + cnt[2]))

    def moments(self):
        """Exact sums of the squared exit weights of the last run, made with option "weight_squares" = 1
        (pc_hip_transmission_moments): uint64 array [n_energies, 2] of (lo, hi) pairs in units of 2^-62, laid out like
        totals()["sumw_fixed"].  With those and the counters, efficiency_stderr() gives the standard errors."""
        ne = self.problem.n_energies
        fx = np.zeros(2 * ne, dtype=np.uint64)
        st = self._L.pc_hip_transmission_moments(self._h, fx.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_moments", st)
        return fx.reshape(ne, 2)

    KERNELS = {0: "pc_trace_kernel", 1: "pc_trace_pool_kernel", 2: "pc_trace_producer_kernel", 3: "pc_trace_wave_kernel",
               4: "pc_trace_log_kernel", 5: "pc_leak_kernel"}

    def last_kernel(self):
        """Name of the kernel that traced the last source run (None before the first)."""
        return self.KERNELS.get(int(self._L.pc_hip_last_kernel(self._h)))

    def phase_stats(self):
        """Average active lanes per scheduler phase of the last run (diagnostics)."""
        st = np.zeros(6, dtype=np.int64)
        rc = self._L.pc_hip_phase_stats(self._h, st.ctypes.data_as(c_int64_p))
        if rc != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_phase_stats", rc)
        names = ("march", "event", "new")
        return {n: dict(phases=int(st[2 * i]), lanes=int(st[2 * i + 1]),
                        avg_lanes=float(st[2 * i + 1]) / max(1, int(st[2 * i]))) for i, n in enumerate(names)}

    def sweep_stats(self):
        """Weight sweeps of the last run of the logging many-energy kernel: wave-level passes and (pass, reflection) iterations,
        the host's tameness threshold and the proxy energies."""
        st = np.zeros(4, dtype=np.int64)
        ct = C.c_double(0.)
        pr = (C.c_int * 2)(-1, -1)
        rc = self._L.pc_hip_sweep_stats(self._h, st.ctypes.data_as(c_int64_p), C.byref(ct), pr)
        if rc != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_sweep_stats", rc)
        return dict(passes=int(st[0]), iterations=int(st[1]), ct_tame=float(ct.value), proxies=[int(pr[0]), int(pr[1])],
                    wave_life_sum=int(st[2]), wave_life_max=int(st[3]))

    def images(self, first=0, count=None):
        """Image data of slots [first, first+count) of the last run: images [count, 17] (the planes of pc_hip_images in
        their order, one row per slot, the reflection count as a float in column 15), exit_weights [count, nE], nrefl.
        One row per slot is also how the device keeps them, so the records are fetched as they are."""
        count = self._last_n - first if count is None else count
        ne = self.problem.n_energies
        rec = np.empty((count, 17 + ne))
        st = self._L.pc_hip_transmission_records(self._h, int(first), int(count), dptr(rec))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_records", st)
        nrefl = rec[:, 15].view(np.int64).copy() if count else np.zeros(0, dtype=np.int64)
        rec[:, 15] = nrefl
        return dict(images=rec[:, :17], exit_weights=rec[:, 17:], nrefl=nrefl)

    def image_planes(self, first=0, count=None):
        """The same through pc_hip_transmission_images: SoA planes [17, count] as the reference's struct _polycap_images
        holds them (what the C host layer uses), exit_weights [count, nE], nrefl."""
        count = self._last_n - first if count is None else count
        ne = self.problem.n_energies
        planes = np.zeros((17, count))
        nrefl = np.zeros(count, dtype=np.int64)
        w = np.zeros((count, ne))
        s = _cabi.images_struct(planes, nrefl, w)
        st = self._L.pc_hip_transmission_images(self._h, int(first), int(count), C.byref(s))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_images", st)
        planes[15] = nrefl
        return dict(planes=planes, exit_weights=w, nrefl=nrefl)

    def slot_ids(self, first=0, count=None):
        """Slot of the photon at positions [first, first+count) of the image planes of the last run: the identity, except
        after a compact run (options compact_images + slot_ids), whose planes are in the order of completion."""
        count = self._last_n - first if count is None else count
        ids = np.zeros(count, dtype=np.int64)
        st = self._L.pc_hip_transmission_slot_ids(self._h, int(first), int(count), ids.ctypes.data_as(c_int64_p))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_slot_ids", st)
        return ids

    def leak_set_order(self, order, n_heavy=0):
        """Order in which the next leak_calc source runs of len(order) slots hand out their slots (heaviest first); the first
        n_heavy go to the heavy lanes.  An empty order restores slot order."""
        o = np.ascontiguousarray(order, dtype=np.uint32)
        st = self._L.pc_hip_leak_set_order(self._h, o.ctypes.data_as(C.POINTER(C.c_uint32)), int(o.size), int(n_heavy))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_leak_set_order", st)

    def leak_slot_units(self, first=0, count=None):
        """Units of work per slot of the last leak_calc source run (option leak_slot_units = 1)."""
        count = self._last_n - first if count is None else count
        u = np.zeros(count, dtype=np.uint32)
        st = self._L.pc_hip_leak_slot_units(self._h, int(first), int(count), u.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_leak_slot_units", st)
        return u

    def relay(self, other, gap, offset=(0., 0.), tilt=(0., 0.), select=None):
        """Relays the exit photons of this context's last source run (made with keep_images) through the optic of `other`, a
        context on the same device with the same energy grid whose z = 0 lies `gap` cm behind this optic's exit plane, its axis
        displaced by `offset` = (x, y) cm (pc_hip_relay_run; the contract is in include/polycap-hip.h).  Nothing per-photon
        leaves the device.  With `tilt` = (x, y) rad the second optic's axis is turned towards +x and +y, and `select`, a Selection
        of this context applied to its exit photons, stands between the two optics as an aperture: only the photons it passes
        are relayed (pc_hip_pose_run; with the defaults the call is the one it was).  Returns efficiencies of the train per energy,
        efficiency_stderr (option "weight_squares" on `other`, else None), counters by name (RELAY_COUNTERS, and missed and
        rejected), sum_weights, sumw_fixed [ne, 2], sumw2_fixed or None, n_records and kernel_ms of the second stage's trace.
        Afterwards other.records() / images(), SpotMap(other, ...) and BeamMoments(other) describe the beam behind the second
        optic."""
        if not isinstance(other, TraceContext):
            raise TypeError("relay: other must be a TraceContext")
        if select is not None and not isinstance(select, Selection):
            raise TypeError("relay: select must be a Selection")
        tilt = (float(tilt[0]), float(tilt[1]))
        if select is None and tilt == (0., 0.):
            pl = np.array([float(gap), float(offset[0]), float(offset[1])], dtype=np.float64)
            st = self._L.pc_hip_relay_run(self._h, other._h, dptr(pl))
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_relay_run", st)
        else:
            st = self._L.pc_hip_pose_run(self._h, other._h, dptr(_pose(gap, offset, tilt)), None if select is None else select._h)
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_pose_run", st)
        other._relay_squares = getattr(other, "_weight_squares", False)      # as the relay was made, whatever the option is set to later
        r = other.relay_totals()
        other._last_n = r["n_records"]
        r["kernel_ms"] = other.wait()
        return r

    def emit(self, other, focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=None, seed=0, energy_map=None,
             select=None, thickness=None, mu_in=None, mu_out=None, layers=None):
        """An emit relay: the exit photons of this context's last source run (made with keep_images) hit a thin sample sheet
        through the point `depth` cm along its normal from (0, 0, focus) behind this optic's exit plane, the normal turned by
        `sample_angle` rad from this optic's axis towards +x; every photon that reaches the sheet re-emits one photon towards
        `other`, whose axis is turned by `det_angle` rad (pi/2: the confocal geometry) and whose entrance centre lies `wd` cm from
        the focus, displaced by `offset` = (u, v) cm in its own entrance plane (pc_hip_emit_run; the contract is in
        include/polycap-hip.h).  The emitted direction is drawn towards a square of half-side `target_half` in the entrance plane
        of `other`, with the stream (seed, slot of the photon), and carries the square's solid angle over 4 pi as a weight.
        target_half defaults to ext[0] of `other`, the circumradius of its entrance hexagon (pc_outside_hex tests |y| and the two
        other edge normals against ext * cos(pi/6), so the hexagon's corners lie at |x| = ext): the square covers the entrance
        face.  `energy_map`[e] = the energy of this context whose weight energy e of `other` takes (fluorescence: excited at one
        energy, detected at another); None: both contexts share one grid.  `select`: a Selection of this context, as in relay().
        Returns what relay() returns, with missed_sample, missed_detector (their sum is `missed`) and rejected in counters; the
        efficiencies are per photon started into this optic and per unit interaction probability in the sheet.
        With `thickness` (cm), `mu_in` [this context's energies] and `mu_out` [the energies of `other`] (1/cm) the sample is a slab
        behind the sheet: every photon interacts at a depth drawn uniformly along its path through the slab, attenuated by mu_in
        on the way there and by mu_out on the emitted ray's way out, through the back or, in the reflection geometry, through the
        front (pc_hip_slab_run).  The efficiencies are then per unit fluorescence-production coefficient (1/cm).  The three come
        together or not at all (ValueError).
        With `layers`, a list of mappings with `thickness` (cm), `mu_in` [this context's energies], `mu_out` and optionally
        `production` [the energies of `other`] (1/cm; production defaults to ones), the sample is a stack of up to 16 layers
        behind the sheet, the first one in front (pc_hip_layers_run): the interaction takes its layer's production coefficient and
        both rays are attenuated through every layer they cross.  The efficiencies then hold the production coefficients.
        `layers` excludes thickness, mu_in and mu_out (ValueError)."""
        if not isinstance(other, TraceContext):
            raise TypeError("emit: other must be a TraceContext")
        if select is not None and not isinstance(select, Selection):
            raise TypeError("emit: select must be a Selection")
        if target_half is None:
            target_half = float(other.problem.ext[0])
        sel = None if select is None else select._h
        if _layers_given("emit", layers, thickness, mu_in, mu_out):
            spec, keep = _layers_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map, layers)
            st = self._L.pc_hip_layers_run(self._h, other._h, C.byref(spec), sel)
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_layers_run", st)
        elif _slab_given("emit", thickness, mu_in, mu_out):
            spec, keep = _slab_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map, thickness, mu_in, mu_out)
            st = self._L.pc_hip_slab_run(self._h, other._h, C.byref(spec), sel)
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_slab_run", st)
        else:
            spec, keep = _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map)
            st = self._L.pc_hip_emit_run(self._h, other._h, C.byref(spec), sel)
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_emit_run", st)
        other._relay_squares = getattr(other, "_weight_squares", False)
        r = other.relay_totals()
        other._last_n = r["n_records"]
        r["kernel_ms"] = other.wait()
        return r

    def relay_totals(self):
        """Totals of the last relay into this context (pc_hip_relay_totals, pc_hip_relay_efficiencies): see relay()."""
        ne = self.problem.n_energies
        sq = getattr(self, "_relay_squares", False)
        cnt = np.zeros(8, dtype=np.int64)
        a = np.zeros(2 * ne, dtype=np.uint64)
        b = np.zeros(2 * ne, dtype=np.uint64) if sq else None
        u64p = C.POINTER(C.c_uint64)
        st = self._L.pc_hip_relay_totals(self._h, cnt.ctypes.data_as(c_int64_p), a.ctypes.data_as(u64p), b.ctypes.data_as(u64p) if sq else None)
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_relay_totals", st)
        lost = np.zeros(2, dtype=np.int64)
        st = self._L.pc_hip_pose_counts(self._h, lost.ctypes.data_as(c_int64_p))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_pose_counts", st)
        eff, err = relay_efficiencies(a, b, cnt)
        counters = dict(zip(RELAY_COUNTERS, (int(v) for v in cnt)), missed=int(lost[0]), rejected=int(lost[1]))
        el = np.zeros(3, dtype=np.int64)
        if self._L.pc_hip_emit_counts(self._h, el.ctypes.data_as(c_int64_p)) == _cabi.PC_HIP_OK:      # the relay was an emit relay
            counters.update(missed_sample=int(el[0]), missed_detector=int(el[1]))
        return dict(efficiencies=eff, efficiency_stderr=err, counters=counters,
                    counters_array=cnt, sum_weights=np.array([fixed_to_double(a[2 * e], a[2 * e + 1]) for e in range(ne)]),
                    sumw_fixed=a.reshape(ne, 2), sumw2_fixed=None if b is None else b.reshape(ne, 2), n_records=int(cnt[1]))

    def records(self, first=0, count=None):
        """Image records [count, 17 + nE] of the last run or relay as the device keeps them (pc_hip_transmission_records): the
        planes of IMG_FIELDS in their order, the reflection count as int64 bits in column 15, then the weights."""
        count = self._last_n - first if count is None else count
        rec = np.empty((count, 17 + self.problem.n_energies))
        st = self._L.pc_hip_transmission_records(self._h, int(first), int(count), dptr(rec))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_transmission_records", st)
        return rec

    def transmission(self, seed, slot0, n_slots, max_attempts=1 << 20, keep_images=False, leak_calc=False, leak_views=False):
        """run + wait + totals (+ images, + leak events: copies, or with leak_views views of the context's lists) in one call."""
        self.run(seed, slot0, n_slots, max_attempts, keep_images, leak_calc)
        ms = self.wait()
        r = self.totals()
        r["kernel_ms"] = ms
        r["efficiencies"] = efficiencies(r["sum_weights"], r["counters"])
        if keep_images:
            r.update(self.images(0, n_slots))
        if leak_calc:
            r["ext"], r["int"] = self.leaks(copy=not leak_views)
        return r

    def draw(self, kind="exit", **kw):
        """Selection.draw through a selection that every entry passes (select_all), made, applied and dropped here: an unweighted
        sample of n entries of the last run, e.g. draw(energy=0, n=100000, seed=1)."""
        return _draw_all(self, kind, kw)


class TraceGroup:
    """One problem on several devices driven from this process (pc_hip_group_*): contiguous slot ranges per member, one
    RCCL all-reduce (or the identical host sum) of the totals.  `devices` may repeat an index."""

    def __init__(self, problem, devices):
        self.problem = problem
        self._L = _cabi.lib()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = self._L.pc_hip_group_create(C.byref(problem.s), len(devices), devs, C.byref(h))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_create", st)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.pc_hip_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, name, value):
        st = self._L.pc_hip_group_set_option(self._h, name.encode(), int(value))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_set_option", st)
        if name == "weight_squares":
            self._weight_squares = bool(value)

    def scan(self, seed, points, n_per_point, max_attempts=1, slot0=0):
        """TraceContext.scan over the group: the flat range [0, P * n_per_point) is split into one contiguous piece per member
        (pc_hip_group_scan_run) and the members' totals are added exactly; kernel_ms is the longest member's, kernel the list
        of the members' kernel names."""
        pts = _scan_array(points, self.problem)
        n_pts = pts.shape[0]
        st = self._L.pc_hip_group_scan_run(self._h, int(seed), int(slot0), dptr(pts), n_pts, int(n_per_point), int(max_attempts))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_scan_run", st)
        ms = C.c_float(0)
        st = self._L.pc_hip_group_scan_wait(self._h, C.byref(ms))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_scan_wait", st)
        r = _scan_fetch(self._L.pc_hip_group_scan_totals, self._h, n_pts, self.problem.n_energies, getattr(self, "_weight_squares", False))
        r["kernel_ms"] = float(ms.value)
        n = int(self._L.pc_hip_group_size(self._h))
        r["kernel"] = [TraceContext.KERNELS.get(int(self._L.pc_hip_group_scan_last_kernel(self._h, k))) for k in range(n)]
        return r

    def last_kernels(self):
        """Names of the kernels that traced the members' shares of the last run."""
        n = int(self._L.pc_hip_group_size(self._h))
        return [TraceContext.KERNELS.get(int(self._L.pc_hip_group_last_kernel(self._h, k))) for k in range(n)]

    def transmission(self, seed, n_slots, max_attempts=1 << 20, keep_images=False, reduce=-1):
        """reduce: -1 automatic (RCCL when the devices are distinct and librccl loads), 0 host sum, 1 RCCL or fail"""
        import time
        t0 = time.perf_counter()
        st = self._L.pc_hip_group_run(self._h, int(seed), int(n_slots), int(max_attempts), int(bool(keep_images)))
        self.enqueue_s = time.perf_counter() - t0          # pc_hip_group_run only enqueues: the members trace asynchronously
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_run", st)
        ne = self.problem.n_energies
        r = {}
        if keep_images:
            planes = np.zeros((17, n_slots))
            nrefl = np.zeros(n_slots, dtype=np.int64)
            w = np.zeros((n_slots, ne))
            s = _cabi.images_struct(planes, nrefl, w)
            st = self._L.pc_hip_group_images(self._h, C.byref(s))
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_group_images", st)
            planes[15] = nrefl
            r.update(images=planes.T.copy(), exit_weights=w, nrefl=nrefl)
        sw = np.zeros(ne)
        cnt = np.zeros(6, dtype=np.int64)
        fx = np.zeros(2 * ne, dtype=np.uint64)
        by, ms = C.c_int(0), C.c_float(0)
        st = self._L.pc_hip_group_totals(self._h, int(reduce), dptr(sw), cnt.ctypes.data_as(c_int64_p),
                                         fx.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(by), C.byref(ms))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_totals", st)
        r.update(sum_weights=sw, counters=cnt, sumw_fixed=fx.reshape(ne, 2), reduced_by_rccl=bool(by.value), kernel_ms=float(ms.value),
                 i_exit=int(cnt[0]), i_start=int(cnt[0] + cnt[1] + cnt[2]), efficiencies=efficiencies(sw, cnt))
        return r

    def moments(self):
        """The squared exit weights' exact sums of the group's last run (option "weight_squares" = 1), summed over the members with
        the weights' sums by the run's totals (pc_hip_group_moments): uint64 [n_energies, 2] of (lo, hi) pairs."""
        ne = self.problem.n_energies
        fx = np.zeros(2 * ne, dtype=np.uint64)
        st = self._L.pc_hip_group_moments(self._h, fx.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_group_moments", st)
        return fx.reshape(ne, 2)

    def draw(self, kind="exit", **kw):
        """Selection.draw through a selection that every entry passes (select_all), made, applied and dropped here: an unweighted
        sample of n entries of the last run, e.g. draw(energy=0, n=100000, seed=1)."""
        return _draw_all(self, kind, kw)


RELAY_COUNTERS = ("n_in", "exit", "absorbed", "glass", "outside", "error", "skipped", "n_started_a")


def _pose(gap, offset, tilt):
    return np.array([float(gap), float(offset[0]), float(offset[1]), float(tilt[0]), float(tilt[1])], dtype=np.float64)


def relay_placement_valid(gap, offset=(0., 0.), tilt=(0., 0.)):
    """True when pc_hip_relay_validate accepts the placement, or with a `tilt` pc_hip_pose_validate the pose (host only)."""
    if tuple(tilt) == (0., 0.):
        pl = np.array([float(gap), float(offset[0]), float(offset[1])], dtype=np.float64)
        return _cabi.lib().pc_hip_relay_validate(dptr(pl)) == _cabi.PC_HIP_OK
    return _cabi.lib().pc_hip_pose_validate(dptr(_pose(gap, offset, tilt))) == _cabi.PC_HIP_OK


def relay_basis(gap, offset, tilt):
    """The axes u, v, n of the second optic of a tilted relay in the first one's exit frame, float64 [9] = u0 u1 u2 v0 v1 v2 n0 n1 n2
    (pc_hip_pose_basis, host only): the nine numbers the kernels get."""
    b = np.zeros(9)
    st = _cabi.lib().pc_hip_pose_basis(dptr(_pose(gap, offset, tilt)), dptr(b))
    if st != _cabi.PC_HIP_OK:
        raise HipError("pc_hip_pose_basis", st)
    return b


def relay_rocking_curve(ctx_a, ctx_b, gap, tilts, offset=(0., 0.), select=None):
    """A rocking curve of the second optic: one relay of ctx_a's last run into ctx_b per (tilt_x, tilt_y) of `tilts`, a host loop.
    Returns tilts [n, 2], efficiencies [n, n_energies], efficiency_stderr [n, n_energies] (option "weight_squares" on ctx_b, else
    None) and the relays' counters as a list of dicts."""
    tl = np.asarray(tilts, dtype=np.float64).reshape(-1, 2)
    eff, err, cnt = [], [], []
    for tx, ty in tl:
        r = ctx_a.relay(ctx_b, gap, offset, (tx, ty), select)
        eff.append(r["efficiencies"])
        err.append(r["efficiency_stderr"])
        cnt.append(r["counters"])
    have = len(err) > 0 and all(e is not None for e in err)
    return dict(tilts=tl, efficiencies=np.array(eff).reshape(len(tl), -1), efficiency_stderr=np.array(err).reshape(len(tl), -1) if have else None,
                counters=cnt)


def _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map):
    """(pc_hip_emit, what its map points to)"""
    s = _cabi.EmitS(float(focus), float(sample_angle), float(depth), float(det_angle), float(wd), float(offset[0]), float(offset[1]),
                    float(target_half), int(seed), 0, None)
    m = None
    if energy_map is not None:
        m = np.ascontiguousarray(energy_map, dtype=np.int32).reshape(-1)
        s.n_map = int(m.shape[0])
        s.map = m.ctypes.data_as(C.POINTER(C.c_int32))
    return s, m


def emit_valid(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1., energy_map=None):
    """True when pc_hip_emit_validate accepts the spec (host only; the map against two contexts' grids is checked by emit())."""
    spec, keep = _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, energy_map)
    return _cabi.lib().pc_hip_emit_validate(C.byref(spec)) == _cabi.PC_HIP_OK


def emit_frame(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1.):
    """The frame of an emit relay in the first optic's exit frame (pc_hip_emit_frame, host only): the sixteen numbers the kernels
    get, as a dict of n_s [3] (the sheet's normal), h_s (its offset), u, v, n [3 each] (the second optic's axes), c_b [3] (its
    entrance centre) and frame [16] (all of them in this order)."""
    spec, keep = _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, None)
    f = np.zeros(16)
    st = _cabi.lib().pc_hip_emit_frame(C.byref(spec), dptr(f))
    if st != _cabi.PC_HIP_OK:
        raise HipError("pc_hip_emit_frame", st)
    return dict(n_s=f[0:3], h_s=float(f[3]), u=f[4:7], v=f[7:10], n=f[10:13], c_b=f[13:16], frame=f)


def _slab_given(who, thickness, mu_in, mu_out):
    """False: none of a slab's three arguments is given; True: all of them are"""
    given = [v is not None for v in (thickness, mu_in, mu_out)]
    if any(given) and not all(given):
        raise ValueError(who + ": thickness, mu_in and mu_out describe a slab together: give all three or none")
    return all(given)


def _slab_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map, thickness, mu_in, mu_out):
    """(pc_hip_slab, what its pointers point to)"""
    e, m = _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map)
    mi = np.ascontiguousarray(mu_in, dtype=np.float64).reshape(-1)
    mo = np.ascontiguousarray(mu_out, dtype=np.float64).reshape(-1)
    s = _cabi.SlabS(e, float(thickness), int(mi.shape[0]), dptr(mi), int(mo.shape[0]), dptr(mo))
    return s, (m, mi, mo)


def emit_slab_valid(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1., energy_map=None, thickness=None,
                    mu_in=None, mu_out=None):
    """True when pc_hip_slab_validate accepts the spec of a slab emit (host only; the map and the tables' lengths against two
    contexts' grids are checked by emit())."""
    if not _slab_given("emit_slab_valid", thickness, mu_in, mu_out):
        raise ValueError("emit_slab_valid: thickness, mu_in and mu_out are needed")
    spec, keep = _slab_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, energy_map, thickness, mu_in, mu_out)
    return _cabi.lib().pc_hip_slab_validate(C.byref(spec)) == _cabi.PC_HIP_OK


def emit_slab_frame(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1., thickness=None):
    """The frame of a slab emit (pc_hip_slab_frame, host only): what emit_frame returns, with k [3] (the slab's normal in the second
    optic's axes) and thickness, and frame [20] = the emit's sixteen numbers, k, thickness."""
    if thickness is None:
        raise ValueError("emit_slab_frame: thickness is needed")
    spec, keep = _slab_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, None, thickness, [0.], [0.])
    f = np.zeros(20)
    st = _cabi.lib().pc_hip_slab_frame(C.byref(spec), dptr(f))
    if st != _cabi.PC_HIP_OK:
        raise HipError("pc_hip_slab_frame", st)
    return dict(n_s=f[0:3], h_s=float(f[3]), u=f[4:7], v=f[7:10], n=f[10:13], c_b=f[13:16], k=f[16:19], thickness=float(f[19]), frame=f)


def _layers_given(who, layers, thickness, mu_in, mu_out):
    """False: no stack of layers is given; True: one is, and none of a slab's three arguments beside it"""
    if layers is None:
        return False
    if any(v is not None for v in (thickness, mu_in, mu_out)):
        raise ValueError(who + ": layers describes the whole sample: give it without thickness, mu_in and mu_out")
    return True


def _layers_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map, layers):
    """(pc_hip_layers, what its pointers point to).  layers: mappings with thickness, mu_in, mu_out and optionally production
    (ones); the rows of a table must have one length (ValueError)."""
    e, m = _emit_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, seed, energy_map)
    layers = list(layers)
    for j, lay in enumerate(layers):
        missing = [k for k in ("thickness", "mu_in", "mu_out") if k not in lay]
        unknown = [k for k in lay if k not in ("thickness", "mu_in", "mu_out", "production")]
        if missing or unknown:
            raise ValueError("layers[%d]: a layer has thickness, mu_in, mu_out and optionally production (missing %s, unknown %s)" % (j, missing, unknown))
    th = np.ascontiguousarray([float(lay["thickness"]) for lay in layers], dtype=np.float64).reshape(-1)
    rows_in = [np.asarray(lay["mu_in"], dtype=np.float64).reshape(-1) for lay in layers]
    rows_out = [np.asarray(lay["mu_out"], dtype=np.float64).reshape(-1) for lay in layers]
    rows_q = [np.ones(len(o)) if lay.get("production") is None else np.asarray(lay["production"], dtype=np.float64).reshape(-1)
              for lay, o in zip(layers, rows_out)]
    n_in = len(rows_in[0]) if layers else 0
    n_out = len(rows_out[0]) if layers else 0
    for j in range(len(layers)):
        if len(rows_in[j]) != n_in:
            raise ValueError("layers[%d]: mu_in has %d entries, layers[0]'s has %d" % (j, len(rows_in[j]), n_in))
        if len(rows_out[j]) != n_out or len(rows_q[j]) != n_out:
            raise ValueError("layers[%d]: mu_out has %d and production %d entries, layers[0]'s mu_out has %d" % (j, len(rows_out[j]), len(rows_q[j]), n_out))
    flat = lambda rows: np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), dtype=np.float64)
    mi, mo, q = flat(rows_in), flat(rows_out), flat(rows_q)
    s = _cabi.LayersS(e, len(layers), dptr(th), int(n_in), dptr(mi), int(n_out), dptr(mo), dptr(q))
    return s, (m, th, mi, mo, q)


def emit_layers_valid(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1., energy_map=None, layers=None):
    """True when pc_hip_layers_validate accepts the spec of a layered emit (host only; the map and the tables' row lengths against
    two contexts' grids are checked by emit())."""
    if layers is None:
        raise ValueError("emit_layers_valid: layers is needed")
    spec, keep = _layers_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, energy_map, layers)
    return _cabi.lib().pc_hip_layers_validate(C.byref(spec)) == _cabi.PC_HIP_OK


def emit_layers_frame(focus, sample_angle, depth, det_angle, wd, offset=(0., 0.), target_half=1., layers=None):
    """The frame of a layered emit (pc_hip_layers_frame, host only): what emit_slab_frame returns for the stack's total thickness,
    with qmax (the largest production coefficient), bounds [n_layers + 1] (the layers' boundaries, summed left to right as the
    library sums them) and frame [21] = the slab's twenty numbers, qmax."""
    if layers is None:
        raise ValueError("emit_layers_frame: layers is needed")
    spec, keep = _layers_spec(focus, sample_angle, depth, det_angle, wd, offset, target_half, 0, None, layers)
    f = np.zeros(21)
    st = _cabi.lib().pc_hip_layers_frame(C.byref(spec), dptr(f))
    if st != _cabi.PC_HIP_OK:
        raise HipError("pc_hip_layers_frame", st)
    bounds = np.zeros(len(keep[1]) + 1)
    for j, t in enumerate(keep[1]):
        bounds[j + 1] = bounds[j] + t
    return dict(n_s=f[0:3], h_s=float(f[3]), u=f[4:7], v=f[7:10], n=f[10:13], c_b=f[13:16], k=f[16:19], thickness=float(f[19]), qmax=float(f[20]),
                bounds=bounds, frame=f)


def emit_depth_scan(ctx_a, ctx_b, depths, focus, sample_angle, det_angle, wd, offset=(0., 0.), target_half=None, seed=0,
                    energy_map=None, select=None, thickness=None, mu_in=None, mu_out=None, layers=None):
    """A depth scan of the sample: one emit of ctx_a's last run into ctx_b per depth of `depths`, a host loop with one seed, so
    that every depth re-emits with the same random numbers (common random numbers: smooth curves).  Returns depths [n],
    efficiencies [n, n_energies], efficiency_stderr [n, n_energies] (option "weight_squares" on ctx_b, else None) and the emits'
    counters as a list of dicts.  thickness, mu_in, mu_out: a slab behind the sheet, as in emit(); the curve is then the one an
    instrument records, self-absorption included.  layers: a stack of layers in their place, as in emit(): the depth profile of a
    layered sample."""
    dl = np.asarray(depths, dtype=np.float64).reshape(-1)
    eff, err, cnt = [], [], []
    for d in dl:
        r = ctx_a.emit(ctx_b, focus, sample_angle, float(d), det_angle, wd, offset, target_half, seed, energy_map, select,
                       thickness, mu_in, mu_out, layers)
        eff.append(r["efficiencies"])
        err.append(r["efficiency_stderr"])
        cnt.append(r["counters"])
    have = len(err) > 0 and all(e is not None for e in err)
    return dict(depths=dl, efficiencies=np.array(eff).reshape(len(dl), -1), efficiency_stderr=np.array(err).reshape(len(dl), -1) if have else None,
                counters=cnt)


def relay_efficiencies(sumw_fixed, sumw2_fixed, counters):
    """(efficiencies, standard errors or None) of a train of two optics from a relay's exact totals (pc_hip_relay_efficiencies,
    host only): sumw_fixed / sumw2_fixed [n_energies, 2] or flat (lo, hi) pairs, counters the relay's eight."""
    a = np.ascontiguousarray(sumw_fixed, dtype=np.uint64).reshape(-1)
    b = None if sumw2_fixed is None else np.ascontiguousarray(sumw2_fixed, dtype=np.uint64).reshape(-1)
    cnt = np.ascontiguousarray(counters, dtype=np.int64)
    if cnt.shape[0] != 8 or a.shape[0] % 2 or (b is not None and b.shape != a.shape):
        raise ValueError("relay_efficiencies: eight counters and n_energies (lo, hi) pairs per sum are needed")
    ne = a.shape[0] // 2
    eff = np.zeros(ne)
    err = None if b is None else np.zeros(ne)
    u64p = C.POINTER(C.c_uint64)
    _cabi.lib().pc_hip_relay_efficiencies(ne, a.ctypes.data_as(u64p), None if b is None else b.ctypes.data_as(u64p),
                                          cnt.ctypes.data_as(c_int64_p), dptr(eff), None if err is None else dptr(err))
    return eff, err


SPOT_KINDS = {"exit": 0, "extleak": 1, "intleak": 2}


def _kind(kind):
    return SPOT_KINDS[kind] if isinstance(kind, str) else int(kind)


def tally_stderr(sums, squares, n_started):
    """Standard error of every cell in weight per started photon (pc_hip_tally_stderr, host only): sums uint64 [...] = S, squares
    uint64 [..., 2] = S2 as (lo, hi) pairs, n_started = counters 0 + 1 + 2 of the run or runs that were added.  Doubles shaped like
    sums; NaN when fewer than two photons were started."""
    a = np.ascontiguousarray(sums, dtype=np.uint64)
    b = np.ascontiguousarray(squares, dtype=np.uint64)
    if b.shape != a.shape + (2,):
        raise ValueError("tally_stderr: squares must be shaped like sums with a trailing [2]")
    out = np.zeros(a.shape, dtype=np.float64)
    u64p = C.POINTER(C.c_uint64)
    _cabi.lib().pc_hip_tally_stderr(a.size, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), int(n_started), dptr(out))
    return out


def select_transmission(passed_w, rejected_w, passed_w2, rejected_w2):
    """(T, T_err) per energy of one kind of a selection's totals (pc_hip_select_transmission, host only): T = P / (P + R) and its
    error by the delta method from the exact sums of W and of W*W over the passing and the rejected entries; NaN where P + R == 0."""
    pw = np.ascontiguousarray(passed_w, dtype=np.uint64).ravel()
    rw = np.ascontiguousarray(rejected_w, dtype=np.uint64).ravel()
    p2 = np.ascontiguousarray(passed_w2, dtype=np.uint64).reshape(-1, 2)
    r2 = np.ascontiguousarray(rejected_w2, dtype=np.uint64).reshape(-1, 2)
    ne = pw.shape[0]
    if rw.shape[0] != ne or p2.shape[0] != ne or r2.shape[0] != ne:
        raise ValueError("select_transmission: passed_w, rejected_w [n_energies] and passed_w2, rejected_w2 [n_energies, 2] are needed")
    T, err = np.zeros(ne), np.zeros(ne)
    u64p = C.POINTER(C.c_uint64)
    _cabi.lib().pc_hip_select_transmission(ne, pw.ctypes.data_as(u64p), rw.ctypes.data_as(u64p), p2.ctypes.data_as(u64p), r2.ctypes.data_as(u64p),
                                           dptr(T), dptr(err))
    return T, err


class _Tally:
    """What SpotMap, BeamMoments and Histograms share: the handle of a pc_hip_<_stem>_* object made on a TraceContext or a
    TraceGroup, its lifetime, add and reset."""
    _stem = None
    _cells = "bins"              # the key of read() that holds the cells
    squares = False

    def _track(self, squares):
        """squares=True of the constructors: every add also keeps the exact sum of W*W per cell (pc_hip_<_stem>_track_squares)"""
        if squares:
            self._call("track_squares")
            self.squares = True

    def _read_squares(self, cells_shape, outside_shape):
        sq = np.zeros(tuple(cells_shape) + (2,), dtype=np.uint64)
        out = np.zeros(tuple(outside_shape) + (2,), dtype=np.uint64)
        self._call("read_squares", sq.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(squares=sq, outside_squares=out)

    def stderr(self, n_started):
        """Standard error of every cell read now, in weight per started photon (tally_stderr): doubles shaped like the cells of
        read().  n_started: counters 0 + 1 + 2 of the run or runs that were added.  Needs squares=True."""
        if not self.squares:
            raise ValueError("stderr: the object was made without squares=True")
        r = self.read()
        return tally_stderr(r[self._cells], r["squares"], n_started)

    def _create(self, owner, spec=None):
        self._L = _cabi.lib()
        self.owner = owner                      # keeps the context alive as long as the object
        h = C.c_void_p()
        name = "pc_hip_%s%s_create" % ("group_" if isinstance(owner, TraceGroup) else "", self._stem)
        st = getattr(self._L, name)(owner._h, *(() if spec is None else (C.byref(spec),)), C.byref(h))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_%s_create" % self._stem, st)
        self._h = h

    def _call(self, what, *args):
        name = "pc_hip_%s_%s" % (self._stem, what)
        st = getattr(self._L, name)(self._h, *args)
        if st != _cabi.PC_HIP_OK:
            raise HipError(name, st)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, "pc_hip_%s_destroy" % self._stem)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, kind="exit", select=None):
        """Adds the exit photons ("exit" / 0), extleak ("extleak" / 1) or intleak ("intleak" / 2) events of the last run; with a
        Selection applied for that kind, only the entries that pass it (an entry it rejects does not exist for the tally)."""
        if select is None:
            self._call("add", _kind(kind))
        else:
            self._call("add_selected", _kind(kind), select._h)

    def reset(self):
        self._call("reset")


class SpotMap(_Tally):
    """Spot maps of a TraceContext or a TraceGroup (pc_hip_spot_*): weighted 2-D histograms of where the entries of the last run
    cross planes `distances` cm behind the optic's exit face, inside the window (x0, x1, y0, y1) cm cut into bins = (nx, ny),
    one map per selected energy (energies: indices, None = all).  Exact uint64 sums of round_half_even(w * 2^32); the contract is
    written down in include/polycap-hip.h.  regime: 0 automatic, 1 LDS tiles, 2 energies across lanes."""

    _stem = "spot"

    def __init__(self, owner, distances, window, bins, energies=None, regime=0, squares=False):
        self.distances = np.ascontiguousarray(distances, dtype=np.float64).ravel()
        self.window = tuple(float(v) for v in window)
        self.nx, self.ny = (int(bins[0]), int(bins[1]))
        self.energies = None if energies is None else np.ascontiguousarray(energies, dtype=np.int32).ravel()
        spec = _cabi.SpotSpecS(self.distances.shape[0], dptr(self.distances), *self.window, self.nx, self.ny,
                               0 if self.energies is None else self.energies.shape[0],
                               None if self.energies is None else self.energies.ctypes.data_as(C.POINTER(C.c_int32)), int(regime))
        self._create(owner, spec)
        dims = (C.c_int32 * 4)()
        wide = C.c_int(0)
        self._L.pc_hip_spot_info(self._h, dims, C.byref(wide))
        self.shape = tuple(int(d) for d in dims)       # (planes, selected energies, ny, nx)
        self.wide = bool(wide.value)
        self._track(squares)

    def read(self):
        """bins [planes, energies, ny, nx] and outside [planes, energies] as uint64, the entry count, and the same as weights
        (maps = bins * 2^-32, outside_map).  With squares=True also squares [planes, energies, ny, nx, 2] and outside_squares
        [planes, energies, 2]: the exact sums of W*W as (lo, hi) pairs in units of 2^-64."""
        np_, ns = self.shape[0], self.shape[1]
        bins = np.zeros(self.shape, dtype=np.uint64)
        out = np.zeros((np_, ns), dtype=np.uint64)
        n = C.c_int64(0)
        self._call("read", bins.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n))
        r = dict(bins=bins, outside=out, n_entries=int(n.value), maps=bins.astype(np.float64) * 2.0 ** -32,
                 outside_map=out.astype(np.float64) * 2.0 ** -32)
        if self.squares:
            r.update(self._read_squares(bins.shape, out.shape))
        return r


BEAM_SUMS = ("W", "WX", "WY", "WU", "WV", "WXX", "WXY", "WXU", "WXV", "WYY", "WYU", "WYV", "WUU", "WUV", "WVV")
BEAM_AT = ("x", "y", "size_x", "size_y", "size_r")


def beam_columns():
    """the 26 column names of pc_hip_beam_params, in order"""
    return tuple(_cabi.lib().pc_hip_beam_columns().decode().split(","))


def beam_params(sums, distances=None):
    """Derived parameters of exact beam sums uint64 [n_energies, 15, 2] (pc_hip_beam_params, host only): a dict of the named
    columns (arrays over the energies).  With distances (cm behind the exit face) also the centroid and RMS sizes there
    (pc_hip_beam_at) as at_x, at_y, at_size_x, at_size_y, at_size_r [n_energies, n_distances]."""
    L = _cabi.lib()
    S = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 15, 2)
    ne = S.shape[0]
    rows = np.zeros((ne, 26), dtype=np.float64)
    L.pc_hip_beam_params(ne, S.ctypes.data_as(C.POINTER(C.c_uint64)), dptr(rows))
    out = {name: rows[:, k].copy() for k, name in enumerate(beam_columns())}
    if distances is not None:
        d = np.ascontiguousarray(distances, dtype=np.float64).ravel()
        at = np.zeros((ne, d.shape[0], 5), dtype=np.float64)
        L.pc_hip_beam_at(ne, S.ctypes.data_as(C.POINTER(C.c_uint64)), d.shape[0], dptr(d), dptr(at))
        out["distances"] = d
        for k, name in enumerate(BEAM_AT):
            out["at_" + name] = at[:, :, k].copy()
    return out


class BeamMoments(_Tally):
    """Exit-beam moments of a TraceContext or a TraceGroup (pc_hip_beam_*): the exact second-moment matrix of position and slope
    of the entries of the last run at the optic's exit face, per energy, as signed 128-bit integer sums on the device.  The
    contract is written down in include/polycap-hip.h.  One object keeps the sums of all three kinds (exit, extleak, intleak)."""

    _stem = "beam"

    def __init__(self, owner):
        self._create(owner)
        ne = C.c_int(0)
        self._L.pc_hip_beam_info(self._h, C.byref(ne))
        self.n_energies = int(ne.value)

    def read(self):
        """sums uint64 [3, n_energies, 15, 2] of (lo, hi) pairs (kinds exit, extleak, intleak; sums in the order of BEAM_SUMS),
        outside uint64 [3, n_energies] and n_entries [3]"""
        ne = self.n_energies
        sums = np.zeros((3, ne, 15, 2), dtype=np.uint64)
        out = np.zeros((3, ne), dtype=np.uint64)
        n = (C.c_int64 * 3)()
        self._call("read", sums.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        return dict(sums=sums, outside=out, n_entries=np.array([int(v) for v in n], dtype=np.int64))

    def params(self, distances=None, kind="exit"):
        """beam_params of the sums of `kind` read now"""
        return beam_params(self.read()["sums"][_kind(kind)], distances)


HIST_QUANTITIES = ("x", "y", "r", "slope_x", "slope_y", "tan_theta", "nrefl", "dtravel", "r_start", "z")
JOINT_QUANTITIES = HIST_QUANTITIES + ("start_x", "start_y")      # the axes of a joint histogram: the start coordinates as well


def hist_axes(axes, names=HIST_QUANTITIES):
    """A ctypes array of pc_hip_hist_axis from a list of dicts (keys as in POLYCAP_HIST: axis, d, centre=(cx, cy), range=(lo, hi),
    bins) or tuples (axis, (lo, hi), bins[, d[, (cx, cy)]]); axis is a name of `names` (HIST_QUANTITIES, or JOINT_QUANTITIES for the
    axes of a joint histogram) or its index."""
    arr = (_cabi.HistAxisS * max(len(axes), 1))()
    for k, a in enumerate(axes):
        if not isinstance(a, dict):
            a = dict(zip(("axis", "range", "bins", "d", "centre"), a))
        unknown = set(a) - {"axis", "range", "bins", "d", "centre"}
        if unknown:
            raise ValueError("histogram axis %d: unknown keys %s" % (k, sorted(unknown)))
        q = a["axis"]
        q = names.index(q) if isinstance(q, str) else int(q)
        cx, cy = a.get("centre", (0., 0.))
        lo, hi = a["range"]
        arr[k] = _cabi.HistAxisS(q, float(a.get("d", 0.)), float(cx), float(cy), float(lo), float(hi), int(a["bins"]))
    return arr


def hist_fwhm(bins, lo, hi):
    """(fwhm, left, right) of one histogram, uint64 bins over [lo, hi) (pc_hip_hist_fwhm, host only): NaN when the profile does not
    fall below half its maximum on both sides inside the range."""
    b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
    l, r = C.c_double(0.), C.c_double(0.)
    w = _cabi.lib().pc_hip_hist_fwhm(b.shape[0], float(lo), float(hi), b.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(l), C.byref(r))
    return float(w), float(l.value), float(r.value)


def hist_quantile(bins, lo, hi, q, outside=0):
    """The value below which the fraction q of the inside weight of one histogram lies (pc_hip_hist_quantile, host only)."""
    b = np.ascontiguousarray(bins, dtype=np.uint64).ravel()
    return float(_cabi.lib().pc_hip_hist_quantile(b.shape[0], float(lo), float(hi), b.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  int(outside), float(q)))


class Histograms(_Tally):
    """Histograms of a TraceContext or a TraceGroup (pc_hip_hist_*): weighted 1-D histograms of per-entry quantities of the last
    run, one per axis and selected energy (energies: indices, None = all), all filled in one pass.  Exact uint64 sums of
    round_half_even(w * 2^32), kept per kind (exit, extleak, intleak); the contract is written down in include/polycap-hip.h.
    axes: see hist_axes.  regime: 0 automatic, 1 workgroup-private LDS histograms, 2 energies across lanes."""

    _stem = "hist"

    def __init__(self, owner, axes, energies=None, regime=0, squares=False):
        self._axes = hist_axes(axes)
        self.energies = None if energies is None else np.ascontiguousarray(energies, dtype=np.int32).ravel()
        spec = _cabi.HistSpecS(len(axes), self._axes, 0 if self.energies is None else self.energies.shape[0],
                               None if self.energies is None else self.energies.ctypes.data_as(C.POINTER(C.c_int32)), int(regime))
        self._create(owner, spec)
        dims = (C.c_int32 * 3)()
        off = (C.c_int32 * (len(axes) + 1))()
        reg = C.c_int(0)
        self._L.pc_hip_hist_info(self._h, dims, off, C.byref(reg))
        self.n_axes, self.n_selected, self.total_bins = (int(d) for d in dims)
        self.offsets = [int(v) for v in off]
        self.regime = int(reg.value)
        self.axes = [dict(axis=HIST_QUANTITIES[a.quantity], d=a.d, centre=(a.cx, a.cy), range=(a.lo, a.hi), bins=a.n_bins)
                     for a in self._axes[:self.n_axes]]
        self._track(squares)

    def read(self):
        """bins uint64 [3, energies, total_bins] (kinds exit, extleak, intleak; the axes one after the other), outside uint64
        [3, axes, energies], n_entries [3]; axes: per axis a view [3, energies, n_bins] of the bins; edges: per axis its n_bins + 1
        bin edges.  With squares=True also squares [3, energies, total_bins, 2] and outside_squares [3, axes, energies, 2]: the exact
        sums of W*W as (lo, hi) pairs in units of 2^-64."""
        bins = np.zeros((3, self.n_selected, self.total_bins), dtype=np.uint64)
        out = np.zeros((3, self.n_axes, self.n_selected), dtype=np.uint64)
        n = (C.c_int64 * 3)()
        self._call("read", bins.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        o = self.offsets
        r = dict(bins=bins, outside=out, n_entries=np.array([int(v) for v in n], dtype=np.int64),
                 axes=[bins[:, :, o[a]:o[a + 1]] for a in range(self.n_axes)],
                 edges=[np.linspace(x["range"][0], x["range"][1], x["bins"] + 1) for x in self.axes])
        if self.squares:
            r.update(self._read_squares(bins.shape, out.shape))
        return r

    def _one(self, axis, energy, kind):
        k = _kind(kind)
        r = self.read()
        return r["axes"][axis][k, energy], self.axes[axis]["range"], r["outside"][k, axis, energy]

    def fwhm(self, axis, energy, kind="exit"):
        """(fwhm, left, right) of axis `axis` at the selected energy number `energy`, read now (hist_fwhm)"""
        b, (lo, hi), _ = self._one(axis, energy, kind)
        return hist_fwhm(b, lo, hi)

    def quantile(self, axis, energy, q, kind="exit"):
        """the q-quantile of the inside weight of axis `axis` at the selected energy number `energy`, read now (hist_quantile)"""
        b, (lo, hi), out = self._one(axis, energy, kind)
        return hist_quantile(b, lo, hi, q, out)


def _axis_dict(a):
    return dict(axis=JOINT_QUANTITIES[a.quantity], d=a.d, centre=(a.cx, a.cy), range=(a.lo, a.hi), bins=a.n_bins)


def joint_pairs(pairs):
    """A ctypes array of pc_hip_joint_pair from a list of (u, v), each an axis as hist_axes takes it, by a name of JOINT_QUANTITIES"""
    arr = (_cabi.JointPairS * max(len(pairs), 1))()
    for k, uv in enumerate(pairs):
        if len(uv) != 2:
            raise ValueError("joint pair %d: a pair is two axes (u, v)" % k)
        a = hist_axes(list(uv), JOINT_QUANTITIES)
        arr[k] = _cabi.JointPairS(a[0], a[1])
    return arr


def pairs_sum(pairs, axis):
    """(lo, hi) pairs uint64 [..., 2] summed exactly along `axis` of the leading dimensions (Python integers): the square sums of
    cells add as their weights do, so a marginal, a rebinned profile or a region of interest keeps an exact S2."""
    p = np.asarray(pairs, dtype=np.uint64)
    if p.ndim < 2 or p.shape[-1] != 2:
        raise ValueError("pairs_sum: (lo, hi) pairs [..., 2] are needed")
    axis = axis % (p.ndim - 1)
    v = p[..., 0].astype(object) + p[..., 1].astype(object) * (1 << 64)
    t = np.asarray(v.sum(axis=axis), dtype=object)
    lo, hi = np.frompyfunc(lambda x: x & ((1 << 64) - 1), 1, 1)(t), np.frompyfunc(lambda x: x >> 64, 1, 1)(t)
    return np.stack([np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)], axis=-1)


def joint_marginal(cells, which):
    """The exact uint64 sums of the cells [nv, nu] of one (kind, pair, energy) over v (which "u": [nu], the histogram of u of what
    both ranges hold) or over u (which "v": [nv]) (pc_hip_joint_marginal, host only)."""
    c = np.ascontiguousarray(cells, dtype=np.uint64)
    if c.ndim != 2 or which not in ("u", "v"):
        raise ValueError("joint_marginal: cells [nv, nu] and which \"u\" or \"v\" are needed")
    nv, nu = c.shape
    out = np.zeros(nv if which == "v" else nu, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    st = _cabi.lib().pc_hip_joint_marginal(nu, nv, c.ctypes.data_as(u64p), 1 if which == "v" else 0, out.ctypes.data_as(u64p))
    if st != _cabi.PC_HIP_OK:
        raise HipError("pc_hip_joint_marginal", st)
    return out


def joint_parse(value, n_energies):
    """A value of POLYCAP_JOINT into (pairs, energies): pairs a list of (u, v) axis dicts, energies a list of indices or None for all
    (pc_hip_joint_parse, host only).  ValueError with the reason, which names the item, when it is refused."""
    pairs = (_cabi.JointPairS * 8)()
    sel = (C.c_int32 * max(int(n_energies), 1))()
    n_pairs, n_sel = C.c_int32(0), C.c_int32(0)
    why = C.create_string_buffer(512)
    st = _cabi.lib().pc_hip_joint_parse(value.encode(), int(n_energies), pairs, C.byref(n_pairs), sel, C.byref(n_sel), why, len(why))
    if st != _cabi.PC_HIP_OK:
        raise ValueError("POLYCAP_JOINT=%s: %s" % (value, why.value.decode()))
    return ([(_axis_dict(p.u), _axis_dict(p.v)) for p in pairs[:n_pairs.value]],
            None if n_sel.value == 0 else [int(e) for e in sel[:n_sel.value]])


class JointHistograms(_Tally):
    """Joint histograms of a TraceContext or a TraceGroup (pc_hip_joint_*): weighted 2-D histograms of two per-entry quantities of
    the last run, one per pair of axes (u, v) and selected energy (energies: indices, None = all), all filled in one pass.  Exact
    uint64 sums of round_half_even(w * 2^32), kept per kind (exit, extleak, intleak); the contract is written down in
    include/polycap-hip.h.  pairs: see joint_pairs.  regime: 0 automatic, 1 workgroup-private LDS tiles, 2 energies across lanes."""

    _stem = "joint"
    _cells = "cells"

    def __init__(self, owner, pairs, energies=None, regime=0, squares=False):
        self._pairs = joint_pairs(pairs)
        self.energies = None if energies is None else np.ascontiguousarray(energies, dtype=np.int32).ravel()
        spec = _cabi.JointSpecS(len(pairs), self._pairs, 0 if self.energies is None else self.energies.shape[0],
                                None if self.energies is None else self.energies.ctypes.data_as(C.POINTER(C.c_int32)), int(regime))
        self._create(owner, spec)
        dims = (C.c_int32 * 3)()
        off = (C.c_int32 * (len(pairs) + 1))()
        reg = C.c_int(0)
        self._L.pc_hip_joint_info(self._h, dims, off, C.byref(reg))
        self.n_pairs, self.n_selected, self.total_cells = (int(d) for d in dims)
        self.offsets = [int(v) for v in off]
        self.regime = int(reg.value)
        self.pairs = [(_axis_dict(p.u), _axis_dict(p.v)) for p in self._pairs[:self.n_pairs]]
        self._track(squares)

    def read(self):
        """cells uint64 [3, energies, total_cells] (kinds exit, extleak, intleak; the pairs one after the other, each [iv][iu]),
        outside uint64 [3, pairs, energies], n_entries [3]; pairs: per pair a view [3, energies, nv, nu] of the cells; edges: per
        pair the (u, v) bin edges.  With squares=True also squares [3, energies, total_cells, 2], outside_squares [3, pairs, energies,
        2] and pairs_squares (views [3, energies, nv, nu, 2]): the exact sums of W*W as (lo, hi) pairs in units of 2^-64."""
        cells = np.zeros((3, self.n_selected, self.total_cells), dtype=np.uint64)
        out = np.zeros((3, self.n_pairs, self.n_selected), dtype=np.uint64)
        n = (C.c_int64 * 3)()
        self._call("read", cells.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        o = self.offsets
        r = dict(cells=cells, outside=out, n_entries=np.array([int(v) for v in n], dtype=np.int64),
                 pairs=[cells[:, :, o[p]:o[p + 1]].reshape(3, self.n_selected, v["bins"], u["bins"]) for p, (u, v) in enumerate(self.pairs)],
                 edges=[tuple(np.linspace(x["range"][0], x["range"][1], x["bins"] + 1) for x in uv) for uv in self.pairs])
        if self.squares:
            r.update(self._read_squares(cells.shape, out.shape))
            sq = r["squares"]
            r["pairs_squares"] = [sq[:, :, o[p]:o[p + 1]].reshape(3, self.n_selected, v["bins"], u["bins"], 2) for p, (u, v) in enumerate(self.pairs)]
        return r

    def marginal(self, pair, which, kind="exit", squares=False):
        """uint64 [energies, nu] (which "u") or [energies, nv] ("v"): the exact marginal sums of pair `pair`, read now (joint_marginal).
        squares=True (an object made with squares=True): the exact marginals of S2 instead, (lo, hi) pairs [energies, nu or nv, 2]
        (pairs_sum): the square sums of cells add as their weights do."""
        if which not in ("u", "v"):
            raise ValueError("marginal: which \"u\" or \"v\" is needed")
        if squares:
            if not self.squares:
                raise ValueError("marginal: the object was made without squares=True")
            return pairs_sum(self.read()["pairs_squares"][pair][_kind(kind)], 1 if which == "u" else 2)
        c = self.read()["pairs"][pair][_kind(kind)]
        return np.stack([joint_marginal(c[e], which) for e in range(self.n_selected)])

    def density(self, pair, efficiencies, kind="exit", n_started=None):
        """[energies, nv, nu] in efficiency units as the spot maps of the public call are, read now: cell * efficiencies[e] /
        (inside + outside) with efficiencies [energies] those of the selected energies; 0 where an energy holds no weight.
        With n_started (an object made with squares=True; counters 0 + 1 + 2 of the runs added): (density, error), the error map
        being the cells' standard errors (tally_stderr) in the same units, efficiencies[e] * stderr * n_started / ((inside +
        outside) 2^-32); the normalising total is taken as exact."""
        if n_started is not None and not self.squares:
            raise ValueError("density: the error map needs an object made with squares=True")
        r = self.read()
        k = _kind(kind)
        c, out = r["pairs"][pair][k], r["outside"][k, pair]
        eff = np.asarray(efficiencies, dtype=np.float64).ravel()
        if eff.shape[0] != self.n_selected:
            raise ValueError("density: one efficiency per selected energy is needed")
        dens = np.zeros(c.shape, dtype=np.float64)
        err = np.zeros(c.shape, dtype=np.float64)
        sig = None if n_started is None else tally_stderr(c, r["pairs_squares"][pair][k], n_started)
        for e in range(self.n_selected):
            total = int(c[e].sum(dtype=np.uint64)) + int(out[e])
            if total:
                dens[e] = eff[e] * c[e].astype(np.float64) / float(total)
                if sig is not None:
                    err[e] = eff[e] * sig[e] * float(n_started) / (float(total) * 2.0 ** -32)
        return dens if n_started is None else (dens, err)


def select_cuts(cuts):
    """A ctypes array of pc_hip_select_cut from a list of cuts, each an axis as hist_axes takes it (a name of JOINT_QUANTITIES) without
    bins, as a dict that may carry not=True (pass what the range does not hold), or as a tuple (axis, (lo, hi)[, d[, (cx, cy)[, not]]])."""
    arr = (_cabi.SelectCutS * max(len(cuts), 1))()
    for k, c in enumerate(cuts):
        if not isinstance(c, dict):
            c = dict(zip(("axis", "range", "d", "centre", "not"), c))
        c = dict(c)
        negate = c.pop("not", False)
        if "bins" in c:
            raise ValueError("selection cut %d: a cut has no bins" % k)
        arr[k] = _cabi.SelectCutS(hist_axes([dict(c, bins=1)], JOINT_QUANTITIES)[0], 1 if negate else 0)
    return arr


def _cut_dict(c):
    a = c.axis
    d = dict(axis=JOINT_QUANTITIES[a.quantity], d=a.d, centre=(a.cx, a.cy), range=(a.lo, a.hi))
    d["not"] = bool(c.negate)
    return d


def select_parse(value):
    """A value of POLYCAP_SELECT into a list of cut dicts (pc_hip_select_parse, host only).  ValueError with the reason, which names the
    item or the cut, when it is refused."""
    cuts = (_cabi.SelectCutS * 8)()
    n = C.c_int32(0)
    why = C.create_string_buffer(512)
    st = _cabi.lib().pc_hip_select_parse(value.encode(), cuts, C.byref(n), why, len(why))
    if st != _cabi.PC_HIP_OK:
        raise ValueError("POLYCAP_SELECT=%s: %s" % (value, why.value.decode()))
    return [_cut_dict(c) for c in cuts[:n.value]]


def select_all():
    """The list of one cut that every entry of every kind passes: a reflection count in [0, 2^62).  Selection(owner, select_all())
    is the whole run as a selection, for draw() or gather() without a cut."""
    return [dict(axis="nrefl", range=(0., 2.0 ** 62))]


def _draw_all(owner, kind, kw):
    with Selection(owner, select_all()) as sel:
        sel.apply(kind)
        return sel.draw(kind, **kw)


class Selection:
    """A selection of a TraceContext or a TraceGroup (pc_hip_select_*): 1 to 8 cuts on per-entry quantities of the last run, ANDed
    (cuts: see select_cuts).  apply(kind) evaluates them on the device and returns the exact totals; tally.add(kind, select=sel) then
    fills any tally of the same owner with the passing entries only.  A mask belongs to the entries it was made from: after the next
    run it is stale and has to be applied again.  The contract is written down in include/polycap-hip.h."""

    def __init__(self, owner, cuts, squares=False):
        self._L = _cabi.lib()
        self.owner = owner                      # keeps the context alive as long as the object
        self.squares = False
        self._cuts = select_cuts(cuts)
        spec = _cabi.SelectSpecS(len(cuts), self._cuts)
        h = C.c_void_p()
        name = "pc_hip_%sselect_create" % ("group_" if isinstance(owner, TraceGroup) else "")
        st = getattr(self._L, name)(owner._h, C.byref(spec), C.byref(h))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_select_create", st)
        self._h = h
        nc, ne = C.c_int32(0), C.c_int32(0)
        self._L.pc_hip_select_info(self._h, C.byref(nc), C.byref(ne), None)
        self.n_cuts, self.n_energies = int(nc.value), int(ne.value)
        self.cuts = [_cut_dict(c) for c in self._cuts[:self.n_cuts]]
        if squares:
            st = self._L.pc_hip_select_track_squares(self._h)
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_select_track_squares", st)
            self.squares = True

    def close(self):
        if getattr(self, "_h", None):
            self._L.pc_hip_select_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def read(self):
        """n_pass [3], n_seen [3] (kinds exit, extleak, intleak; zeros for a kind not applied), passed_w and rejected_w uint64
        [3, n_energies]: the exact sums of round_half_even(w * 2^32) over the passing and over the rejected entries.  With
        squares=True also passed_w2 and rejected_w2 uint64 [3, n_energies, 2]: the exact sums of W*W as (lo, hi) pairs."""
        n_pass, n_seen = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        pw = np.zeros((3, self.n_energies), dtype=np.uint64)
        rw = np.zeros((3, self.n_energies), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        st = self._L.pc_hip_select_read(self._h, n_pass, n_seen, pw.ctypes.data_as(u64p), rw.ctypes.data_as(u64p))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_select_read", st)
        r = dict(n_pass=np.array([int(v) for v in n_pass], dtype=np.int64), n_seen=np.array([int(v) for v in n_seen], dtype=np.int64),
                 passed_w=pw, rejected_w=rw)
        if self.squares:
            p2 = np.zeros((3, self.n_energies, 2), dtype=np.uint64)
            r2 = np.zeros((3, self.n_energies, 2), dtype=np.uint64)
            st = self._L.pc_hip_select_read_squares(self._h, p2.ctypes.data_as(u64p), r2.ctypes.data_as(u64p))
            if st != _cabi.PC_HIP_OK:
                raise HipError("pc_hip_select_read_squares", st)
            r.update(passed_w2=p2, rejected_w2=r2)
        return r

    def transmission(self, kind="exit"):
        """(T, T_err) per energy of the kind's totals read now (select_transmission): the transmission of the selection, a pinhole's
        for a cut on r, and its standard error.  Needs squares=True."""
        if not self.squares:
            raise ValueError("transmission: the selection was made without squares=True")
        r, k = self.read(), _kind(kind)
        return select_transmission(r["passed_w"][k], r["rejected_w"][k], r["passed_w2"][k], r["rejected_w2"][k])

    def apply(self, kind="exit"):
        """Evaluates the cuts on the entries of `kind` of the last run; returns read()"""
        st = self._L.pc_hip_select_apply(self._h, _kind(kind))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_select_apply", st)
        return self.read()

    def gather(self, kind="exit", first=0, count=None, positions=False):
        """The per-entry data of the passing entries numbered [first, first + count) of a kind the selection was applied for
        (pc_hip_select_gather; count None = all from first on), in the order of their positions: records [count, 17 + n_energies]
        for the exit photons -- the rows TraceContext.records() has at those positions, the reflection count as int64 bits in
        column 15 -- or [count, 12 + n_energies] for a leak kind, the rows of leaks().  With positions=True also the int64
        positions [count] (global ones for a group), strictly increasing.  Only the selected rows leave the device."""
        k = _kind(kind)
        first = int(first)
        if count is None:
            count = max(int(self.read()["n_pass"][k]) - first, 0)
        count = int(count)
        row = (17 if k == 0 else _cabi.PC_HIP_LEAK_HDR) + self.n_energies
        rec = np.empty((max(count, 0), row))
        pos = np.empty(max(count, 0), dtype=np.int64) if positions else None
        st = self._L.pc_hip_select_gather(self._h, k, first, count, dptr(rec) if count > 0 else None,
                                          pos.ctypes.data_as(c_int64_p) if positions and count > 0 else None)
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_select_gather", st)
        return (rec, pos) if positions else rec


    def draw(self, kind="exit", energy=0, n=None, phase=None, seed=None, first=0, count=None, positions=False):
        """An unweighted sample of the passing entries of a kind the selection was applied for (pc_hip_select_draw): n draws in
        proportion to the quantised weights at energy index `energy`, by systematic resampling in exact integers on the device; the
        draws [first, first + count) are returned (count None = all from first on).  phase: a uint32; None takes one from
        numpy.random.default_rng(seed).  A dict of records [count, row] (the rows gather() has at the drawn positions, an entry as
        often as it was drawn), positions (int64 [count], not decreasing; with positions=True), total (T, the exact sum of the
        quantised weights drawn from), weight (total * 2^-32 / n: what every draw stands for per started photon), phase and n."""
        k = _kind(kind)
        if n is None:
            raise ValueError("draw: n, the size of the sample, is needed")
        n, first = int(n), int(first)
        if phase is None:
            phase = int(np.random.default_rng(seed).integers(0, 1 << 32, dtype=np.uint64))
        phase = int(phase)
        if not 0 <= phase < (1 << 32):
            raise ValueError("draw: phase must be a uint32, got %d" % phase)
        if not -(1 << 63) <= n < (1 << 63):
            raise ValueError("draw: n must be in [1, 2^31 - 1], got %d" % n)
        if count is None:
            count = max(n - first, 0)
        count = int(count)
        row = (17 if k == 0 else _cabi.PC_HIP_LEAK_HDR) + self.n_energies
        if not (1 <= n < (1 << 31) and first >= 0 and 0 <= count <= n - first):
            rows = min(max(count, 0), 1)          # the call refuses these before it writes: no array of a size nobody asked for in earnest
        else:
            rows = count
        rec = np.empty((rows, row))
        pos = np.empty(rows, dtype=np.int64) if positions else None
        total = C.c_uint64(0)
        st = self._L.pc_hip_select_draw(self._h, k, int(energy), n, phase, first, count, dptr(rec) if count > 0 else None,
                                        pos.ctypes.data_as(c_int64_p) if positions and count > 0 else None, C.byref(total))
        if st != _cabi.PC_HIP_OK:
            raise HipError("pc_hip_select_draw", st)
        r = dict(records=rec, total=int(total.value), weight=int(total.value) * 2.0 ** -32 / n, phase=phase, n=n)
        if positions:
            r["positions"] = pos
        return r


def scan_points(x=(0.,), y=(0.,), d_source=None):
    """Points of a scan, [len(d) * len(y) * len(x), 3] rows of (d_source, src_shiftx, src_shifty) in cm: the grid of the axes with
    x varying fastest, then y, then d_source (row = (id * len(y) + iy) * len(x) + ix).  d_source None = the problem's own (NaN
    in the rows, filled in by scan()); a number or a sequence of them otherwise."""
    xs = np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel()
    ys = np.atleast_1d(np.asarray(y, dtype=np.float64)).ravel()
    ds = np.array([np.nan]) if d_source is None else np.atleast_1d(np.asarray(d_source, dtype=np.float64)).ravel()
    d, yy, xx = np.meshgrid(ds, ys, xs, indexing="ij")
    return np.stack([d.ravel(), xx.ravel(), yy.ravel()], axis=1)


def _scan_array(points, problem):
    pts = np.array(points, dtype=np.float64, order="C", copy=True)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("scan points must be an array [P, 3] of (d_source, src_shiftx, src_shifty)")
    pts[np.isnan(pts[:, 0]), 0] = problem.source[0]
    return pts


def _scan_fetch(fn, h, n_pts, ne, squares):
    cnt = np.zeros((n_pts, 6), dtype=np.int64)
    a = np.zeros((n_pts, ne, 2), dtype=np.uint64)
    b = np.zeros((n_pts, ne, 2), dtype=np.uint64) if squares else None
    u64p = C.POINTER(C.c_uint64)
    st = fn(h, cnt.ctypes.data_as(c_int64_p), a.ctypes.data_as(u64p), b.ctypes.data_as(u64p) if squares else None)
    if st != _cabi.PC_HIP_OK:
        raise HipError(fn.__name__, st)
    eff, err = scan_efficiencies(cnt, a, b)
    return dict(counters=cnt, sumw_fixed=a, sumw2_fixed=b, efficiencies=eff, stderr=err)


def scan_efficiencies(counters, sumw_fixed, sumw2_fixed=None):
    """Per-row efficiencies [P, ne] and (with sumw2_fixed) standard errors of a scan's totals (pc_hip_scan_efficiencies):
    counters [P, 6], sumw_fixed / sumw2_fixed [P, ne, 2].  A row where nothing entered a capillary has efficiency 0."""
    cnt = np.ascontiguousarray(counters, dtype=np.int64).reshape(-1, 6)
    n_pts = cnt.shape[0]
    a = np.ascontiguousarray(sumw_fixed, dtype=np.uint64).reshape(n_pts, -1)
    ne = a.shape[1] // 2
    b = None if sumw2_fixed is None else np.ascontiguousarray(sumw2_fixed, dtype=np.uint64).reshape(n_pts, 2 * ne)
    eff = np.zeros((n_pts, ne))
    err = None if b is None else np.zeros((n_pts, ne))
    u64p = C.POINTER(C.c_uint64)
    _cabi.lib().pc_hip_scan_efficiencies(ne, n_pts, cnt.ctypes.data_as(c_int64_p), a.ctypes.data_as(u64p),
                                         None if b is None else b.ctypes.data_as(u64p), dptr(eff), None if err is None else dptr(err))
    return eff, err


def efficiencies(sum_weights, counters):
    sw = np.ascontiguousarray(sum_weights, dtype=np.float64)
    cnt = np.ascontiguousarray(counters, dtype=np.int64)
    if cnt.shape[0] < 6:
        cnt = np.concatenate([cnt, np.zeros(6 - cnt.shape[0], dtype=np.int64)])
    eff = np.zeros_like(sw)
    _cabi.lib().pc_hip_efficiencies(sw.shape[0], dptr(sw), cnt.ctypes.data_as(c_int64_p), dptr(eff))
    return eff


def fixed_to_double(lo, hi):
    return float(_cabi.lib().pc_hip_fixed_to_double(int(lo), int(hi)))


def efficiency_stderr(sumw_fixed, sumw2_fixed, counters):
    """Standard error of every efficiency from a run's exact moments (pc_hip_efficiency_stderr, include/polycap-hip.h):
    sumw_fixed / sumw2_fixed as totals()["sumw_fixed"] and moments() ([n_energies, 2] or flat uint64 (lo, hi) pairs), counters as
    totals()["counters"].  NaN where fewer than two photons were started."""
    a = np.ascontiguousarray(sumw_fixed, dtype=np.uint64).reshape(-1)
    b = np.ascontiguousarray(sumw2_fixed, dtype=np.uint64).reshape(-1)
    if a.shape != b.shape or a.shape[0] % 2:
        raise ValueError("efficiency_stderr: sumw_fixed and sumw2_fixed must both hold n_energies (lo, hi) pairs")
    cnt = np.ascontiguousarray(counters, dtype=np.int64)
    if cnt.shape[0] < 6:
        cnt = np.concatenate([cnt, np.zeros(6 - cnt.shape[0], dtype=np.int64)])
    out = np.zeros(a.shape[0] // 2)
    _cabi.lib().pc_hip_efficiency_stderr(out.shape[0], a.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         cnt.ctypes.data_as(c_int64_p), dptr(out))
    return out
