"""Soundness of the march certificates -- pc_march_first_ok, pc_march_ok at strides 1, PC_L1 and PC_L2, the creep loop of
pc_event_pre and the `bnd` flag of pc_launch_init (pc_device.h), on the tables pc_build_tables makes (pc_problem.h) -- against
rational arithmetic.  Product code is called unchanged through probe op MARCH (tests/devmath/probe_ops.h) in the host compile; the
exact side (tests/devmath/exact.py: fractions.Fraction, no tolerance anywhere) decides alone; the grids (tests/devmath/grid.py) aim
photons at the places where a certificate could be wrong.  The same checks run on the device's outputs in
tests/test_gpu_devmath_march.py.  No trace kernel is involved.

What is asserted, per profile:
  soundness       every segment a certified step skipped has exact max g < 0 over its admissible range (strictly)
  literal         the same rows with Pm.literal = 1 end in the same state, hit and rc, bit for bit
  classification  bnd == 0 only for capillaries whose circle lies strictly inside the outer hexagon at every node (exactly)
  tables          md, mb, r2, adj, adjf are at least their exact values; infinite exactly where a block does not fit
  not vacuous     the rows are what they were built to be; centred rays take the widest stride that fits; crossing rows are
                  visited literally no later than the crossed segment; at least 200 crossing and 200 near-miss rows
The measured figures (steps by kind, smallest slack, nearest certified miss) are printed (run with -s) and stand in DESIGN.md §3.
"""
import functools
import math

import numpy as np
import pytest

from tests.devmath import exact, grid, pyprobe
from tests.emul import pyemul

H = {k: j for j, k in enumerate(pyprobe.MARCH_HEAD_COLS)}
CERTIFIED = (pyprobe.STEP_FIRST, pyprobe.STEP_SINGLE, pyprobe.STEP_L1, pyprobe.STEP_L2)
LITERAL = (pyprobe.STEP_MISS, pyprobe.STEP_HIT, pyprobe.STEP_DONE)
PROFILES = tuple(grid.march_profiles())
NEAR = 1e-6                 # |delta| of a near-miss row


@functools.lru_cache(maxsize=None)
def march_case(name):
    g = grid.march_grids()[name]
    t = pyemul.march_tables(g["problem"])
    return dict(name=name, p=g["problem"], rows=g["rows"], meta=g["meta"], t=t, prof=exact.march_profile(t), nmax=len(t["z"]) - 1)


def run_rows(name, device=False, literal=False):
    S = march_case(name)
    x = S["rows"].copy()
    x[:, pyprobe.MARCH_COLS.index("literal")] = 1.0 if literal else 0.0
    return pyprobe.run_march(S["p"], x, device=device)


@functools.lru_cache(maxsize=None)
def host_run(name, literal=False):
    return run_rows(name, device=False, literal=literal)


_EXACT = {}


def exact_row(name, idx, row_out):
    """the exact side of one row: max g per segment from the entrance segment on, over its admissible range (the first segment:
    beyond P.z + 1e-5, exact.admissible_from); cached per process on the direction and (kx, ky) the probe reports"""
    key = (name, idx, row_out[H["dx"]:H["dz"] + 1].tobytes(), row_out[H["kx"]:H["ky"] + 1].tobytes(), int(row_out[H["i0"]]))
    if key not in _EXACT:
        S = march_case(name)
        P = S["rows"][idx, 0:3]
        ray = exact.MarchRay(S["prof"], P, row_out[H["dx"]:H["dz"] + 1], row_out[H["kx"]:H["ky"] + 1])
        i0 = int(row_out[H["i0"]])
        adm = exact.admissible_from(P[2])
        mg = {}
        for j in range(i0, S["nmax"]):
            r = ray.max_g(j, adm if j == i0 else None)
            mg[j] = None if r is None else r[0]
        _EXACT[key] = dict(ray=ray, i0=i0, maxg=mg)
    return _EXACT[key]


def entered(out):
    return out[:, H["state"]] == pyprobe.ST_MARCH


def _margin(S, kind, i, kn):
    """the margin a certified step of `kind` from node i compared with (as doubles; a measurement's yardstick, not a decision)"""
    t = S["t"]
    if kind == pyprobe.STEP_L1:
        kd = kn * t["mg_md1"][i]
        return t["mg_mb1"][i] + kd * (t["mg_r2"][i] + kd)
    if kind == pyprobe.STEP_L2:
        kd = kn * t["mg_md2"][i]
        return t["mg_mb2"][i] + kd * (t["mg_r2"][i] + kd)
    return t["adj"]


def check_soundness(name, out, who):
    """every certified step (first-segment, single, PC_L1, PC_L2, creep) skipped only segments with exact max g < 0; returns
    the measurements of the profile"""
    S = march_case(name)
    steps = dict.fromkeys(pyprobe.STEP_NAMES + ("creep",), 0)
    worst = dict(slack=math.inf, slack_at=None, nearest=math.inf, nearest_at=None)
    bad = []
    for idx in np.flatnonzero(entered(out)):
        ex = exact_row(name, idx, out[idx])
        kn = float(np.hypot(out[idx, H["kx"]], out[idx, H["ky"]]))
        for ib, ia, kind, creep in pyprobe.march_trail(out[idx]):
            steps[pyprobe.STEP_NAMES[kind]] += 1
            if kind in CERTIFIED:
                assert ia - ib == {pyprobe.STEP_FIRST: 1, pyprobe.STEP_SINGLE: 1, pyprobe.STEP_L1: S["t"]["L1"],
                                   pyprobe.STEP_L2: S["t"]["L2"]}[kind], (name, who, idx, ib, ia, kind)
                skipped, k2 = range(ib, ia), kind
            elif kind in LITERAL and creep:
                steps["creep"] += 1
                skipped, k2 = range(ib, ib + creep), pyprobe.STEP_SINGLE
            else:
                continue
            top = None
            for j in skipped:
                g = ex["maxg"][j]
                if g is None:            # the admissible range of the first segment is empty
                    continue
                if not g < 0:
                    bad.append((idx, S["meta"][idx]["fam"], S["meta"][idx]["cap"], S["meta"][idx]["delta"], ib, ia,
                                pyprobe.STEP_NAMES[kind], j, float(g)))
                top = g if top is None or g > top else top
            if top is not None and top < 0:
                m = _margin(S, k2, ib, kn)
                sl = float(-top) / m if m > 0 and math.isfinite(m) else math.inf
                if sl < worst["slack"]:
                    worst["slack"], worst["slack_at"] = sl, (idx, pyprobe.STEP_NAMES[kind], ib)
                if float(-top) < worst["nearest"]:
                    worst["nearest"], worst["nearest_at"] = float(-top), (idx, pyprobe.STEP_NAMES[kind], ib)
    assert not bad, "%s (%s): certified steps over segments with exact max g >= 0: %s" % (name, who, bad[:6])
    return dict(steps=steps, **worst)


def report(name, who, m):
    S = march_case(name)
    cap2 = float(np.max(S["t"]["cap"])) ** 2
    print("march %-9s %-6s rows %4d  steps %s" % (name, who, len(S["rows"]), " ".join("%s %d" % kv for kv in m["steps"].items() if kv[1])))
    print("      smallest slack (-max g)/margin %.4g at %s; nearest certified miss -max g = %.3e cm^2 = %.2e cap^2 at %s"
          % (m["slack"], m["slack_at"], m["nearest"], m["nearest"] / cap2, m["nearest_at"]))


END_COLS = ("how", "i", "rc", "Px", "Py", "Pz", "nx", "ny", "nz", "cosalfa")


def check_literal_agreement(name, out, code, out_lit, code_lit, who):
    """the certified march and the literal march of the same rows end the same way: how, segment, rc, hit point, normal and
    cosine bit for bit (the hit of a row that ends in REFLECT; the start point otherwise)"""
    cols = [H[k] for k in END_COLS]
    a, b = np.ascontiguousarray(out[:, cols]), np.ascontiguousarray(out_lit[:, cols])
    same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    rows = np.flatnonzero(~same.all(axis=1) | (code != code_lit))
    S = march_case(name)
    assert rows.size == 0, (name, who, [(int(r), S["meta"][r]["fam"], S["meta"][r]["delta"], a[r].tolist(), b[r].tolist()) for r in rows[:4]])
    assert not (out[:, H["how"]] == pyprobe.END_STEPS).any() and not (out_lit[:, H["how"]] == pyprobe.END_STEPS).any(), \
        (name, who, "a row ran out of steps")


def check_classification(name, out, who):
    """bnd == 0 only where the capillary's circle lies strictly inside the outer hexagon at every node.  Between two nodes the
    centre, the radius and the hexagon's size are all linear in z, and each of the twelve conditions is linear in them: it holds
    along a segment when it holds at both ends."""
    S = march_case(name)
    p = S["prof"]
    seen = {}
    for idx in np.flatnonzero(entered(out) & (out[:, H["bnd"]] == 0)):
        k = (float(out[idx, H["kx"]]), float(out[idx, H["ky"]]))
        if k not in seen:
            kx, ky = exact.fr(k[0]), exact.fr(k[1])
            seen[k] = all(exact.circle_inside_hexagon(kx * zh, ky * zh, c, e) for zh, c, e in zip(p["zh"], p["cap"], p["ext"]))
        assert seen[k], (name, who, idx, S["meta"][idx]["cap"], k)
    # the grid's own names: the boundary shell and the mono-capillary are classed boundary, the three inner ones are not
    for idx in np.flatnonzero(entered(out)):
        want = 1 if (S["meta"][idx]["cap"] == "boundary" or S["t"]["mono"]) else 0
        assert int(out[idx, H["bnd"]]) == want, (name, who, idx, S["meta"][idx]["cap"])
    return len(seen)


def check_tables(name):
    S = march_case(name)
    t = S["t"]
    b = exact.march_table_bounds(t)
    n = S["nmax"] + 1
    # the derived tables the exact side takes as given are what the setup made of the profile
    assert np.array_equal(t["zh"], grid.march_grids()[name]["profile"]["ext"] / t["hexscale"])
    assert exact.fr(t["adj"]) >= b["adj"], (name, "adj", t["adj"], float(b["adj"]))
    assert exact.fr(t["adjf"]) >= exact.fr(t["adj"]), (name, "adjf", t["adjf"], t["adj"])
    assert exact.fr(t["two_rmaxf"]) >= exact.fr(t["two_rmax"]) >= 2 * max(S["prof"]["cap"]), (name, "two_rmax")
    for L, mb, md, tmb, tmd in ((t["L1"], "mg_mb1", "mg_md1", "mb1", "md1"), (t["L2"], "mg_mb2", "mg_md2", "mb2", "md2")):
        for i in range(n):
            e = b["L"][L][i]
            if e is None:
                assert math.isinf(t[mb][i]) and t[mb][i] > 0 and math.isinf(t[md][i]) and t[md][i] > 0, (name, L, i, "must be +inf")
                assert math.isinf(t[tmb][i]) and math.isinf(t[tmd][i]), (name, L, i)
                continue
            assert math.isfinite(t[mb][i]) and math.isfinite(t[md][i]), (name, L, i, "block fits: finite margins")
            assert exact.fr(t[md][i]) >= e["md"], (name, L, i, "md", t[md][i], float(e["md"]))
            assert exact.fr(t[mb][i]) >= exact.fr(t[tmb][i]) >= e["mb"], (name, L, i, "mb", t[mb][i], t[tmb][i], float(e["mb"]))
            assert exact.fr(t["mg_r2"][i]) >= e["r2"], (name, L, i, "r2")
            assert t[md][i] == t[tmd][i], (name, L, i, "packed md")
    for i in range(n):
        assert exact.fr(t["mg_r2"][i]) >= b["r2"][i], (name, i, "r2 of the clipped PC_L2 block")


def block_max(name, idx, row_out):
    """largest exact max g over the segments of the row's would-be block, from the start point on"""
    S = march_case(name)
    ex = exact_row(name, idx, row_out)
    ja, jb = S["meta"][idx]["block"]
    P = exact.fr(S["rows"][idx, 2])
    vals = []
    for j in range(max(ja, ex["i0"]), jb):
        r = ex["ray"].max_g(j, P if j == ex["i0"] else None)
        if r is not None:
            vals.append(r[0])
    return max(vals) if vals else None


def check_built(name, out):
    """By the exact side alone: a row built to cross the wall inside its would-be block does (max g > 0 there), a row built to
    miss it by delta cap does (max g < 0 there, and -max g = delta cap (2 R - delta cap) for a radius R of the block, within a
    factor 2 for what doubles lose in placing the ray).  Returns (crossing rows, near-miss rows)."""
    S = march_case(name)
    assert entered(out).all(), (name, "rows not let in", [(int(r), S["meta"][r]["fam"], S["meta"][r]["cap"], S["meta"][r]["delta"],
                                                           int(out[r, H["rc0"]])) for r in np.flatnonzero(~entered(out))[:6]])
    cap = S["t"]["cap"]
    cross = near = 0
    for idx, m in enumerate(S["meta"]):
        if m["delta"] == 0.0:
            continue
        top = block_max(name, idx, out[idx])
        assert top is not None, (name, idx, m)
        if m["delta"] < 0:
            assert top > 0, (name, idx, m["fam"], m["cap"], m["delta"], float(top))
            cross += 1
        else:
            ja, jb = m["block"]
            R = cap[ja:jb + 1]
            gap = m["delta"] * float(cap[m["tnode"]] if m["fam"] != "mid" else 0.5 * (cap[m["tnode"]] + cap[m["tnode"] + 1]))
            lo, hi = gap * (2 * R.min() - gap), gap * (2 * R.max() - gap)
            assert top < 0 and 0.5 * lo <= float(-top) <= 2 * hi, (name, idx, m["fam"], m["cap"], m["delta"], float(top), lo, hi)
            near += m["delta"] <= NEAR
    return cross, near


def expected_widest(S):
    """the trail of a centred axis-parallel photon from z = 0 when every step takes the widest stride that fits: first segment,
    then from node i stride PC_L2 where its margin is finite, else PC_L1 where that is, else one segment"""
    t, i, tr = S["t"], 1, [(0, 1, pyprobe.STEP_FIRST)]
    while i < S["nmax"]:
        if math.isfinite(t["mg_mb2"][i]):
            L, kind = t["L2"], pyprobe.STEP_L2
        elif math.isfinite(t["mg_mb1"][i]):
            L, kind = t["L1"], pyprobe.STEP_L1
        else:
            L, kind = 1, pyprobe.STEP_SINGLE
        tr.append((i, i + L, kind))
        i += L
    return tr


def check_widest(name, out, who):
    S = march_case(name)
    rows = [i for i, m in enumerate(S["meta"]) if m["fam"] == "axis" and m["cap"] == "centre" and S["rows"][i, 2] == 0.0]
    assert rows
    for idx in rows:
        got = [(a, b, k) for a, b, k, _ in pyprobe.march_trail(out[idx])]
        assert got == expected_widest(S), (name, who, got)
        assert out[idx, H["how"]] == pyprobe.END_EXIT and out[idx, H["rc"]] == 1


def check_crossings_visited(name, out, who):
    """a row built to cross: the first segment with exact max g >= 0 is reached by a literal visit, or the march ended in one
    before it; never by a certified step"""
    S = march_case(name)
    n = beyond = 0
    for idx, m in enumerate(S["meta"]):
        if not m["delta"] < 0:
            continue
        ex = exact_row(name, idx, out[idx])
        jc = min(j for j, g in ex["maxg"].items() if g is not None and g >= 0)
        visits = [ib + creep for ib, ia, kind, creep in pyprobe.march_trail(out[idx]) if kind in LITERAL]
        assert visits and min(visits) <= jc, (name, who, idx, m["fam"], m["delta"], jc, visits)
        # Not asserted: that the march stops there.  A root that doubles place on the wrong side of a seam is admitted by neither of
        # the two segments (in the reference's arithmetic as here; the literal march of the same row goes on in the same way, which
        # check_literal_agreement asserts), and a photon flying backwards never hits.  Counted and printed instead.
        beyond += int(out[idx, H["dz"]] > 0 and int(out[idx, H["i"]]) > jc + 1)
        assert jc in visits or max(visits) < jc, (name, who, idx, jc, visits)
        n += 1
    print("march %-9s %-6s %d crossing rows, %d of them marched on past the crossed segment (root lost at a seam)" % (name, who, n, beyond))
    return n


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PROFILES)
def test_tables_are_at_least_their_exact_values(name):
    check_tables(name)


@pytest.mark.parametrize("name", PROFILES)
def test_certified_steps_skip_only_segments_strictly_inside(name):
    out, code = host_run(name)
    report(name, "host", check_soundness(name, out, "host"))


@pytest.mark.parametrize("name", PROFILES)
def test_literal_march_agrees_at_the_adversarial_points(name):
    out, code = host_run(name)
    lit, code_lit = host_run(name, literal=True)
    check_literal_agreement(name, out, code, lit, code_lit, "host")
    steps = [k for r in lit for _, _, k, _ in pyprobe.march_trail(r)]
    assert all(k in LITERAL for k in steps)


@pytest.mark.parametrize("name", PROFILES)
def test_non_boundary_capillaries_lie_inside_the_hexagon(name):
    out, code = host_run(name)
    assert check_classification(name, out, "host") == (0 if march_case(name)["t"]["mono"] else 3)


@pytest.mark.parametrize("name", PROFILES)
def test_rows_are_what_they_were_built_to_be(name):
    out, code = host_run(name)
    check_built(name, out)
    check_crossings_visited(name, out, "host")


def test_grids_hold_enough_crossing_and_near_miss_rows():
    cross = near = total = 0
    for name in PROFILES:
        c, n = check_built(name, host_run(name)[0])
        cross, near, total = cross + c, near + n, total + len(march_case(name)["rows"])
    print("march grids: %d rows, %d crossing, %d near-miss (0 < delta <= %g)" % (total, cross, near, NEAR))
    assert cross >= 200 and near >= 200


@pytest.mark.parametrize("name", ["cylinder", "bulge"])
def test_centred_rays_take_the_widest_stride_that_fits(name):
    check_widest(name, host_run(name)[0], "host")
