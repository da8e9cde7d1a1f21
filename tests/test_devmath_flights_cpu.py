"""Soundness of the march certificates on flights AFTER a reflection -- pc_march_first_ok with the start on the wall, pc_march_ok at
strides 1, PC_L1 and PC_L2 and the creep loop of pc_event_pre on the ray pc_event_post and pc_trace_begin re-derive (pc_device.h) --
against rational arithmetic.  Product code is called unchanged through probe op FLIGHTS (tests/devmath/probe_ops.h) in the host
compile: pc_launch_init, pc_march_step, pc_event_pre and, on a hit, pc_event_post(.., 1), flight after flight.  The exact side
(tests/devmath/exact.py: fractions.Fraction, no tolerance anywhere) decides alone: the ray of flight f is the line through the P and
d the probe reports for that flight, so nothing here depends on the reflection arithmetic (tests/test_devmath_geom_cpu.py covers
that).  The grids (tests/devmath/grid.py, flight_grids) aim later flights by time reversal.  The same checks run on the device's
outputs in tests/test_gpu_devmath_flights.py.  No trace kernel is involved.

What is asserted, per profile:
  soundness   in every flight every segment a certified step skipped (first-segment certificate, single, PC_L1, PC_L2, creep) has
              exact max g < 0, strictly; the flight's first segment counts from exact.admissible_from(P.z) on, every later one
              whole.  A flight that is outside its capillary at the admissible start of its first segment (exact g >= 0 there: the
              flight after a crossing the reference's 1e-5 guard dropped) contains no certified step for as long as it stays
              outside: none at all when it never comes back (exact g >= 0 at every later node), else none that starts before the
              first node at which it is exactly back inside.  Two things keep this from being "no certified step at all", and both
              are what the reference does as well (the literal chain agrees bit for bit): cap_kink's wall turns outward again at
              the next node, so every guard row re-enters its capillary two segments on and is certified from there, soundly (the
              first assertion covers those steps); and a first-segment certificate whose admissible range is empty (P.z + 1e-5
              beyond the segment's end) passes wherever the photon is -- it skips nothing a root could lie in.  The flight's own
              start P does not enter the condition: it is the rounded hit point, whose exact g is a rounding residue of either
              sign, and a first flight with g(P) > 0 is refused at the entrance.
  literal     the same rows with Pm.literal = 1 give the same chain bit for bit: per flight the start i, P, d, the end kind, normal,
              cosalfa, ix and hit point; at the end how, rc, irefl and the number of flights
  state       at a flight's start irefl is the flight number, i the previous ix, first is set (the first pass is the first-segment
              certificate, a literal visit or the exit), lv is PC_LV_LATER (0 for boundary capillaries), P is the previous hit bit
              for bit and d the three fused multiply-adds of the previous d, normal and cosine, recomputed with exact rounding
  tightness   a later flight of the centre or the middle capillary flying forwards, whose exact g at the start of the range the
              first-segment certificate tests (the larger of z_i and P.z + 1e-5) and at the segment's end is below -2 adj, passes that
              certificate: the first pass is of kind FIRST.  (The certificate compares its two values with -adj; adj is at least
              m = max(1e-6 capmin^2, 1e-10 capmax extmax), a million times the rounding of g, so a factor 2 covers what the doubles
              lose.)  A certificate that tested the wrong point would stay sound whenever both its points lie inside -- |q| - R is
              convex along a segment -- and show only here.
  limit       a chain ends with rc 1 from pc_event_post exactly when irefl exceeds nmax
  endings     no row runs out of passes; a row runs out of flights exactly when all FLIGHT_NB flights ended in a hit
  not vacuous the counts of the issue's table, by the exact side and the trail, over all profiles (FLOORS)
The measured figures are printed (run with -s) and stand in DESIGN.md §3 and profiles/flights_cert.txt.
"""
import collections
import functools
import math

import numpy as np
import pytest

from tests.devmath import exact, grid, pyprobe
from tests.emul import pyemul

H = {k: j for j, k in enumerate(pyprobe.FLIGHTS_HEAD_COLS)}
FC = {k: j for j, k in enumerate(pyprobe.FLIGHT_COLS)}
CERTIFIED = (pyprobe.STEP_FIRST, pyprobe.STEP_SINGLE, pyprobe.STEP_L1, pyprobe.STEP_L2)
LITERAL = (pyprobe.STEP_MISS, pyprobe.STEP_HIT, pyprobe.STEP_DONE)
PROFILES = tuple(grid.flight_profiles())
NEAR = 1e-6
# what the exact side counts over all profiles, at least (the issue's table)
FLOORS = dict(near_node=200, L1=300, L2=50, creep=100, first_passed=100, first_refused=100, ix_next=10, guard_dropped=16,
              guard_hit=16, six_flights=100)


@functools.lru_cache(maxsize=None)
def flight_case(name):
    g = grid.flight_grids()[name]
    t = pyemul.march_tables(g["problem"])
    return dict(name=name, p=g["problem"], rows=g["rows"], meta=g["meta"], t=t, prof=exact.march_profile(t), nmax=len(t["z"]) - 1)


def run_rows(name, device=False, literal=False):
    S = flight_case(name)
    x = S["rows"].copy()
    x[:, pyprobe.FLIGHTS_COLS.index("literal")] = 1.0 if literal else 0.0
    return pyprobe.run_flights(S["p"], x, device=device)


@functools.lru_cache(maxsize=None)
def host_run(name, literal=False):
    return run_rows(name, device=False, literal=literal)


def entered(out):
    return out[:, H["state"]] == pyprobe.ST_MARCH


def flight_block(row, f):
    return row[pyprobe.FLIGHTS_HEAD + pyprobe.FLIGHTS_FL * f: pyprobe.FLIGHTS_HEAD + pyprobe.FLIGHTS_FL * (f + 1)]


class ExactFlight:
    """the exact side of one flight: its ray through the reported P along the reported d, max g per segment on demand"""

    def __init__(self, S, fl, kxy):
        self.i0 = int(fl[FC["i"]])
        self.Pz = float(fl[FC["Pz"]])
        self.ray = exact.MarchRay(S["prof"], fl[FC["Px"]:FC["Pz"] + 1], fl[FC["dx"]:FC["dz"] + 1], kxy)
        self.adm = exact.admissible_from(self.Pz)
        self._mg = {}
        self._out = None

    def maxg(self, j):
        if j not in self._mg:
            r = self.ray.max_g(j, self.adm if j == self.i0 else None)
            self._mg[j] = None if r is None else r[0]
        return self._mg[j]

    def outside_at_start(self, z_end):
        """exact g >= 0 at the admissible start of the flight's first segment (False when that lies beyond the profile)"""
        if self._out is None:
            self._out = bool(self.adm < z_end and self.ray.g_at(self.adm) >= 0)
        return self._out


_EXACT = {}


def exact_flight(name, row, f):
    fl = flight_block(row, f)
    key = (name, fl[FC["i"]:FC["dz"] + 1].tobytes(), row[H["kx"]:H["ky"] + 1].tobytes())
    if key not in _EXACT:
        _EXACT[key] = ExactFlight(flight_case(name), fl, row[H["kx"]:H["ky"] + 1])
    return _EXACT[key]


def trail_by_flight(row):
    by = collections.defaultdict(list)
    for f, ib, ia, kind, creep in pyprobe.flights_trail(row):
        by[f].append((ib, ia, kind, creep))
    return by


def check_soundness(name, out, who):
    """every certified step of every flight skipped only segments with exact max g < 0; a flight outside its capillary at its
    admissible start holds no certified step; returns the measurements of the profile (steps by kind at irefl >= 1, smallest slack,
    nearest certified miss, the counts of the not-vacuous table)"""
    S = flight_case(name)
    t = S["t"]
    zend = S["prof"]["z"][-1]
    steps = dict.fromkeys(pyprobe.STEP_NAMES + ("creep",), 0)
    cnt = dict.fromkeys(FLOORS, 0)
    cnt.update(flights=0, later=0, outside=0, outside_back=0)
    worst = dict(slack=math.inf, slack_at=None, nearest=math.inf, nearest_at=None)
    bad, bad_out = [], []
    for idx in np.flatnonzero(entered(out)):
        row, m = out[idx], S["meta"][idx]
        nf = int(row[H["n_flights"]])
        by = trail_by_flight(row)
        cnt["flights"] += nf
        cnt["six_flights"] += nf >= 6
        for f in range(nf):
            fl = flight_block(row, f)
            ex = exact_flight(name, row, f)
            later = f >= 1
            cnt["later"] += later
            kinds = set()
            certified_from = []          # start nodes of the certified steps that skipped a non-empty admissible range
            for ib, ia, kind, creep in by.get(f, ()):
                if later:
                    steps[pyprobe.STEP_NAMES[kind]] += 1
                if kind in CERTIFIED:
                    assert ia - ib == {pyprobe.STEP_FIRST: 1, pyprobe.STEP_SINGLE: 1, pyprobe.STEP_L1: t["L1"],
                                       pyprobe.STEP_L2: t["L2"]}[kind], (name, who, idx, f, ib, ia, kind)
                    skipped, k2 = range(ib, ia), kind
                elif kind in LITERAL and creep:
                    if later:
                        steps["creep"] += 1
                    kinds.add("creep")
                    skipped, k2 = range(ib, ib + creep), pyprobe.STEP_SINGLE
                else:
                    continue
                kinds.add(kind)
                top = None
                for j in skipped:
                    g = ex.maxg(j)
                    if g is None:            # the admissible range of the first segment is empty
                        continue
                    if not g < 0:
                        bad.append((int(idx), f, m["fam"], m["cap"], m["delta"], ib, ia, pyprobe.STEP_NAMES[kind], j, float(g)))
                    top = g if top is None or g > top else top
                if top is not None:
                    certified_from.append(ib)
                if top is not None and top < 0:
                    kn = float(np.hypot(row[H["kx"]], row[H["ky"]]))
                    mg = _margin(t, k2, ib, kn)
                    sl = float(-top) / mg if mg > 0 and math.isfinite(mg) else math.inf
                    label = "creep" if kind in LITERAL else pyprobe.STEP_NAMES[kind]
                    if sl < worst["slack"]:
                        worst["slack"], worst["slack_at"] = sl, (int(idx), f, label, ib)
                    if float(-top) < worst["nearest"]:
                        worst["nearest"], worst["nearest_at"] = float(-top), (int(idx), f, label, ib)
            outside = ex.outside_at_start(zend)
            cnt["outside"] += outside
            if outside:
                # the first node beyond the admissible start at which the ray is exactly back inside its capillary
                back = next((j for j in range(ex.i0 + 1, S["nmax"] + 1) if S["prof"]["z"][j] >= ex.adm and ex.ray.g_node(j) < 0), None)
                cnt["outside_back"] += back is not None
                if any(back is None or ib < back for ib in certified_from):
                    bad_out.append((int(idx), f, m["fam"], m["cap"], m["off"], back, by.get(f)))
            # the guard rows, by the exact side: the flight that follows the first crossing (guard: flight 1; guard0: flight 0)
            if m["fam"] in ("guard", "guard0") and f == (1 if m["fam"] == "guard" else 0):
                if outside:
                    cnt["guard_dropped"] += 1
                elif ex.ray.g_at(exact.fr(ex.Pz) + 3 * exact.TEN_MU) > 0:        # crossed between 1e-5 and 3e-5 beyond the start
                    cnt["guard_hit"] += 1
                    assert int(fl[FC["end"]]) == pyprobe.END_REFLECT and fl[FC["hz"]] - ex.Pz < 3e-5, (name, who, idx, m, fl.tolist())
            if later:
                cnt["L1"] += pyprobe.STEP_L1 in kinds
                cnt["L2"] += pyprobe.STEP_L2 in kinds
                cnt["creep"] += "creep" in kinds
                first = by.get(f, [None])[0]
                if first is not None:
                    cnt["first_passed"] += first[2] == pyprobe.STEP_FIRST
                    cnt["first_refused"] += first[2] in LITERAL
                # nodes the flight passes beyond its admissible start and before its end, within NEAR cap of the wall, inside
                j_end = int(fl[FC["i_end"]]) if int(fl[FC["end"]]) != pyprobe.END_EXIT else S["nmax"]
                near = False
                for j in range(ex.i0 + 1, min(j_end, S["nmax"]) + 1):
                    if S["prof"]["z"][j] < ex.adm:
                        continue
                    R = S["prof"]["cap"][j]
                    g = ex.ray.g_node(j)
                    if g < 0 and -g < exact.fr(NEAR) * R * R * (2 - exact.fr(NEAR)):
                        near = True
                        break
                cnt["near_node"] += near
            if int(fl[FC["end"]]) == pyprobe.END_REFLECT:
                cnt["ix_next"] += int(fl[FC["ix"]]) == int(fl[FC["i_end"]]) + 1
    assert not bad, "%s (%s): certified steps over segments with exact max g >= 0: %s" % (name, who, bad[:6])
    assert not bad_out, "%s (%s): certified steps in a flight that starts outside its capillary, before it is back inside: %s" % (name, who, bad_out[:4])
    return dict(steps=steps, counts=cnt, **worst)


def _margin(t, kind, i, kn):
    """the margin a certified step of `kind` from node i compared with (as doubles; a measurement's yardstick, not a decision)"""
    if kind == pyprobe.STEP_L1:
        kd = kn * t["mg_md1"][i]
        return t["mg_mb1"][i] + kd * (t["mg_r2"][i] + kd)
    if kind == pyprobe.STEP_L2:
        kd = kn * t["mg_md2"][i]
        return t["mg_mb2"][i] + kd * (t["mg_r2"][i] + kd)
    return t["adj"]


def report(name, who, m):
    S = flight_case(name)
    cap2 = float(np.max(S["t"]["cap"])) ** 2
    fam = collections.Counter(x["fam"] for x in S["meta"])
    print("flights %-14s %-6s rows %4d flights %5d later %5d | irefl>=1: %s" % (
        name, who, len(S["rows"]), m["counts"]["flights"], m["counts"]["later"], " ".join("%s %d" % kv for kv in m["steps"].items() if kv[1])))
    print("      smallest slack (-max g)/margin %.4g at %s; nearest certified miss -max g = %.3e cm^2 = %.2e cap^2 at %s"
          % (m["slack"], m["slack_at"], m["nearest"], m["nearest"] / cap2, m["nearest_at"]))
    print("      families %s | counts %s" % (" ".join("%s %d" % kv for kv in sorted(fam.items())),
                                            " ".join("%s %d" % (k, m["counts"][k]) for k in tuple(FLOORS) + ("outside", "outside_back"))))


CHAIN_COLS = ("how", "rc", "irefl", "n_flights")
FLIGHT_AGREE = tuple(c for c in pyprobe.FLIGHT_COLS if c not in ("C0", "spare0", "spare1"))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def check_literal_agreement(name, out, code, out_lit, code_lit, who):
    """the certified chain and the literal chain of the same rows are the same chain: every flight's start (irefl, i, lv, bnd, first,
    P, d) and end (kind, segment, normal, cosalfa, ix, hit point) and the chain's end, bit for bit"""
    S = flight_case(name)
    cols = [H[k] for k in CHAIN_COLS]
    fcols = [pyprobe.FLIGHTS_HEAD + pyprobe.FLIGHTS_FL * f + FC[c] for f in range(pyprobe.FLIGHTS_NB) for c in FLIGHT_AGREE]
    same = _bits_equal(out[:, cols + fcols], out_lit[:, cols + fcols])
    rows = np.flatnonzero(~same.all(axis=1) | (code != code_lit))
    assert rows.size == 0, (name, who, [(int(r), S["meta"][r]["fam"], S["meta"][r]["cap"], S["meta"][r]["delta"],
                                         out[r, cols].tolist(), out_lit[r, cols].tolist()) for r in rows[:4]])


def check_endings(name, out, who):
    """no row ran out of passes; a row ran out of flights exactly when FLIGHTS_NB flights were begun and every one ended in a hit"""
    S = flight_case(name)
    how = out[:, H["how"]].astype(int)
    assert not (how == pyprobe.CHAIN_PASSES).any(), (name, who, "rows ran out of passes", np.flatnonzero(how == pyprobe.CHAIN_PASSES)[:8])
    assert (out[:, H["n_trail"]] < pyprobe.FLIGHTS_K).all()
    for idx in range(len(out)):
        nf = int(out[idx, H["n_flights"]])
        ends = [int(flight_block(out[idx], f)[FC["end"]]) for f in range(nf)]
        full = nf == pyprobe.FLIGHTS_NB and all(e == pyprobe.END_REFLECT for e in ends) and int(out[idx, H["irefl"]]) <= S["nmax"]
        assert (how[idx] == pyprobe.CHAIN_FLIGHTS) == full, (name, who, idx, how[idx], nf, ends)
        assert (how[idx] == pyprobe.CHAIN_ENTRANCE) == (nf == 0), (name, who, idx)
        assert all(e == pyprobe.END_REFLECT for e in ends[:-1]), (name, who, idx, ends)
    return int((how == pyprobe.CHAIN_FLIGHTS).sum())


def check_state(name, out, who):
    """what pc_event_post and pc_trace_begin leave at the start of every flight"""
    S = flight_case(name)
    n = 0
    for idx in np.flatnonzero(entered(out)):
        row = out[idx]
        by = trail_by_flight(row)
        bnd = int(row[H["bnd"]])
        prev = None
        for f in range(int(row[H["n_flights"]])):
            fl = flight_block(row, f)
            at = (name, who, int(idx), f, S["meta"][idx]["fam"])
            assert int(fl[FC["irefl"]]) == f and int(fl[FC["first"]]) == 1 and int(fl[FC["bnd"]]) == bnd, at
            assert int(fl[FC["lv"]]) == (0 if bnd else (2 if f == 0 else pyprobe.LV_LATER)), at
            i = int(fl[FC["i"]])
            if prev is None:
                assert i == int(row[H["i0"]]) and _bits_equal(fl[FC["Px"]:FC["Pz"] + 1], S["rows"][idx, 0:3]).all(), at
                assert _bits_equal(fl[FC["dx"]:FC["dz"] + 1], row[H["dx"]:H["dz"] + 1]).all(), at
            else:
                assert i == int(prev[FC["ix"]]), at + (i, prev[FC["ix"]])
                assert int(prev[FC["ix"]]) in (int(prev[FC["i_end"]]), int(prev[FC["i_end"]]) + 1), at
                assert _bits_equal(fl[FC["Px"]:FC["Pz"] + 1], prev[FC["hx"]:FC["hz"] + 1]).all(), at
                want = exact.mirrored(prev[FC["dx"]:FC["dz"] + 1], prev[FC["nx"]:FC["nz"] + 1], prev[FC["cosalfa"]])
                assert _bits_equal(fl[FC["dx"]:FC["dz"] + 1], np.array(want)).all(), at + (fl[FC["dx"]:FC["dz"] + 1].tolist(), want)
                n += 1
            passes = by.get(f, [])
            if i >= S["nmax"]:
                assert not passes and int(fl[FC["end"]]) == pyprobe.END_EXIT, at
            else:
                assert passes and passes[0][2] in (pyprobe.STEP_FIRST,) + LITERAL and passes[0][0] == i, at + (passes[:2],)
                assert all(p[2] != pyprobe.STEP_FIRST for p in passes[1:]), at
            prev = fl
    return n


def check_first_passes_where_it_must(name, out, who):
    """later flights whose first segment is, exactly, inside by twice the margin at both ends of the tested range pass the
    first-segment certificate; returns how many such flights there were"""
    S = flight_case(name)
    z, adj2 = S["prof"]["z"], 2 * exact.fr(S["t"]["adj"])
    n = 0
    for idx in np.flatnonzero(entered(out)):
        if S["meta"][idx]["cap"] not in ("centre", "middle") or S["t"]["mono"]:
            continue
        row = out[idx]
        by = trail_by_flight(row)
        for f in range(1, int(row[H["n_flights"]])):
            fl = flight_block(row, f)
            i = int(fl[FC["i"]])
            if i >= S["nmax"] or not fl[FC["dz"]] > 0 or not by.get(f):
                continue
            ex = exact_flight(name, row, f)
            zlo = max(z[i], exact.fr(ex.Pz + 1.0e-5))
            if zlo >= z[i + 1]:
                must = True
            else:
                must = ex.ray.g_at(zlo) < -adj2 and ex.ray.g_node(i + 1) < -adj2
            if must:
                n += 1
                assert by[f][0][2] == pyprobe.STEP_FIRST, (name, who, int(idx), f, S["meta"][idx]["fam"], by[f][:2])
    return n


def check_limit(name, out, code, who):
    """the chain ends with rc 1 from pc_event_post exactly when irefl exceeds nmax"""
    S = flight_case(name)
    how, irefl, rc = out[:, H["how"]].astype(int), out[:, H["irefl"]].astype(int), out[:, H["rc"]].astype(int)
    lim = how == pyprobe.CHAIN_LIMIT
    assert np.array_equal(lim, irefl > S["nmax"]), (name, who, np.flatnonzero(lim != (irefl > S["nmax"]))[:8])
    assert (rc[lim] == 1).all() and (irefl[lim] == S["nmax"] + 1).all() and np.array_equal(rc, code), (name, who)
    assert ((how == pyprobe.CHAIN_EXIT) <= (rc == 1)).all() and ((how == pyprobe.CHAIN_EVENT) <= (rc == -1)).all(), (name, who)
    return int(lim.sum())


@functools.lru_cache(maxsize=None)
def host_measure(name):
    return check_soundness(name, host_run(name)[0], "host")


def total_counts(measure):
    tot = dict.fromkeys(FLOORS, 0)
    for name in PROFILES:
        for k in tot:
            tot[k] += measure(name)["counts"][k]
    return tot


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PROFILES)
def test_certified_steps_of_every_flight_skip_only_segments_strictly_inside(name):
    report(name, "host", host_measure(name))


@pytest.mark.parametrize("name", PROFILES)
def test_literal_chain_is_the_same_chain_bit_for_bit(name):
    out, code = host_run(name)
    lit, code_lit = host_run(name, literal=True)
    check_literal_agreement(name, out, code, lit, code_lit, "host")
    assert all(k in LITERAL for r in lit for _, _, _, k, _ in pyprobe.flights_trail(r))
    check_endings(name, lit, "host literal")


@pytest.mark.parametrize("name", PROFILES)
def test_state_at_the_start_of_every_flight(name):
    out, code = host_run(name)
    check_state(name, out, "host")
    check_state(name, host_run(name, literal=True)[0], "host literal")


@pytest.mark.parametrize("name", PROFILES)
def test_chain_ends_at_the_reflection_limit_exactly_when_irefl_exceeds_nmax(name):
    out, code = host_run(name)
    n = check_limit(name, out, code, "host")
    nfl = check_endings(name, out, "host")
    print("flights %-14s host   %d rows end at the reflection limit, %d after %d flights" % (name, n, nfl, pyprobe.FLIGHTS_NB))
    if name in ("nmax1", "nmax4"):
        lim = out[:, H["how"]] == pyprobe.CHAIN_LIMIT
        fam = np.array([m["fam"] == "limit" for m in flight_case(name)["meta"]])
        assert (lim & fam).sum() >= 16 and (~lim & fam & entered(out)).sum() >= 16, (name, int(lim.sum()))


def test_first_segment_certificate_passes_where_it_must():
    n = {name: check_first_passes_where_it_must(name, host_run(name)[0], "host") for name in PROFILES}
    print("flight grids: later flights that must pass the first-segment certificate: %s" % " ".join("%s %d" % kv for kv in n.items() if kv[1]))
    assert sum(n.values()) >= 1000, n


def test_grids_hold_what_the_exact_side_must_count():
    tot = total_counts(host_measure)
    print("flight grids: %d rows | %s" % (sum(len(flight_case(n)["rows"]) for n in PROFILES), " ".join("%s %d (>= %d)" % (k, tot[k], FLOORS[k]) for k in FLOORS)))
    assert all(tot[k] >= FLOORS[k] for k in FLOORS), tot


def test_probe_refuses_invalid_rows():
    S = flight_case("nmax4")
    x = S["rows"][:2].copy()
    for col, v in (("literal", 2.0), ("K", pyprobe.FLIGHTS_K + 1.0), ("K", 1.5), ("NB", 0.0), ("NB", pyprobe.FLIGHTS_NB + 1.0), ("x", math.nan)):
        y = x.copy()
        y[1, pyprobe.FLIGHTS_COLS.index(col)] = v
        with pytest.raises(RuntimeError):
            pyprobe.run_flights(S["p"], y, device=False)
    # a short pass or flight budget is reported as such, never as another ending
    y = x.copy()
    y[:, pyprobe.FLIGHTS_COLS.index("K")] = 1.0
    out, _ = pyprobe.run_flights(S["p"], y, device=False)
    assert (out[:, H["how"]] == pyprobe.CHAIN_PASSES).all() and (out[:, H["n_trail"]] == 1).all()
