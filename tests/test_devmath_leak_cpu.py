"""Soundness of the leak path's skip certificates -- pc_wall_step with pc_wall_reach, the certain misses of pc_wall_probe, the
block skipping of pc_outer_intersect and the cube rounding of pc_hex_index (pc_leak.h), on the tables pc_build_tables makes
(stp, istp, dr, mg, hexd, ext) -- against rational arithmetic.  Product code is called unchanged through probe ops WALL, OUTER and
HEX (tests/devmath/probe_ops.h) in the host compile; op WALL's host compile carries the unit counters of pc_leak.h
(PC_LEAK_STATS, a library of its own), which say what kind every unit of a search was.  The exact side (tests/devmath/exact.py:
fractions.Fraction, no tolerance) decides alone; the grids (tests/devmath/grid.py) aim photons at cell edges, corners, the avoided
capillary, block ends of the probe and step counts that are whole numbers.  The same checks run on the device's outputs in
tests/test_gpu_devmath_leak.py.  No trace kernel is involved.

What is asserted:
  wall step  every certified stretch [pz before, pz after] lies strictly inside cell (q_i, r_i), ends at or before the last node and,
             inside the stack, keeps |p - K zz|^2 - cap^2 > 0 (exact minimum of the quadratic per segment)
  probe      every block of segments a probe unit skipped has exact min |p - K_new zh|^2 - cap^2 > 0: each literal visit would miss
  literal    the same rows with Pm.literal = 1 end in the same head bit for bit (WALL and OUTER)
  OUTER      the returned point lies in the bracket of the first node of the backward scan that is exactly not outside
  HEX        (q, r) is the exact cell; on an edge or corner (within 8 running-error bounds) one of the cells that meet there
  tables     dr.d1 / d2 at least the exact chord deviation of cap, infinite exactly where the block does not fit; stp == cap/10
  not vacuous  by the exact side alone: every row is what it was built to be; >= 200 rows within 1e-6 cap of the avoided capillary
             on each side, >= 200 within 1e-6 zh of a corner or an edge, >= 100 one-node dips; after the run: units of every kind
The measured figures (units by kind, smallest slack, nearest certified miss) are printed (run with -s); they stand in DESIGN.md
section 3 and profiles/leak_cert.txt.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.devmath import exact, grid, pyprobe
from tests.emul import pyemul

H = {k: j for j, k in enumerate(pyprobe.WALL_HEAD_COLS)}
TR = {k: j for j, k in enumerate(pyprobe.WALL_TRAIL_COLS)}
PROFILES = tuple(grid.leak_profiles())
NEAR = 1e-6
LIT, HINT, UNITS = (pyprobe.WALL_COLS.index(k) for k in ("literal", "hint", "max_units"))


@functools.lru_cache(maxsize=None)
def wall_case(name):
    g = grid.wall_grids()[name]
    t = pyemul.march_tables(g["problem"])
    t.update(pyemul.leak_tables(g["problem"]))
    return dict(name=name, p=g["problem"], rows=g["rows"], meta=g["meta"], t=t, nmax=len(t["z"]) - 1, prof=g["profile"])


def wall_rows(name, literal, unit_cap):
    """the rows of a profile for one mode: certified rows keep their cap (LEAK_UNITS; 256 for dz < 0), literal rows get unit_cap"""
    x = wall_case(name)["rows"].copy()
    if literal:
        x[:, LIT] = 1.0
        x[x[:, 5] > 0, UNITS] = float(unit_cap)
    return x


@functools.lru_cache(maxsize=None)
def host_wall(name, literal=False, unit_cap=pyprobe.WALL_UNITS_HOST):
    return pyprobe.run_wall(wall_case(name)["p"], wall_rows(name, literal, unit_cap), device=False)


@functools.lru_cache(maxsize=None)
def ray_of(name, idx):
    S = wall_case(name)
    return exact.WallRay(S["t"], S["rows"][idx, 0:3], S["rows"][idx, 3:6])


# ---------------------------------------------------------------------------------------------------------------------------
# the exact side alone

@functools.lru_cache(maxsize=None)
def built(name):
    """What every row of a profile's grid is, by the exact side alone; asserts it is what it was built to be.  Returns per row a
    dict: cell (the exact cell of the start, None when it returns at once), near_cap (+1 / -1: closest approach to the avoided
    capillary within 1e-6 cap outside / inside), near_edge (leaves within 1e-6 zh of a corner, or runs within 1e-6 zh of an edge)."""
    S = wall_case(name)
    out = []
    for idx, m in enumerate(S["meta"]):
        ray = ray_of(name, idx)
        info = dict(cell=None, near_cap=0, near_edge=False)
        out.append(info)
        P = S["rows"][idx, 0:3]
        fam, delta = m["fam"], m["delta"]
        if fam == "begin":
            continue
        zs = exact.fr(P[2])
        cells, _, _ = _cells_at(ray, zs)
        assert cells, (name, idx, m)
        cell = max(cells, key=cells.get)
        info["cell"] = cell
        who = (name, idx, fam, m["cell"], delta)
        if fam == "cap":
            za, zb = exact.fr(m["block"][0]), exact.fr(m["block"][1])
            assert ray.min_cell_slack(za, min(zb, exact.fr(m["zt"])), *cell) > 0, who + ("leaves the cell before the graze",)
            f, at = ray.min_gap2(za, zb, exact.cell_K(*cell), ray.zz)
            _graze(info, f, delta, ray.at(ray.cap, exact.fr(m["zt"])), who)
        elif fam in ("nbr", "mono"):
            za, zb = exact.fr(m["block"][0]), ray.z[min(S["nmax"], m["tnode"] + 1)]
            f, at = ray.min_gap2(max(za, ray.z[ray.seg(za)]), zb, exact.cell_K(*m["nbr"]), ray.zh)
            _graze(info, f, delta, ray.cap[m["tnode"]], who)
            if fam == "nbr":
                ex = ray.first_exit(zs, *cell)
                assert ex is not None and ex[2] == m["ic"], who + ("crossing segment", ex and ex[2], m["ic"])
        elif fam == "corner":
            ex = ray.first_exit(zs, *cell)
            assert ex is not None, who
            second = ex[1][1]
            assert Fraction(abs(delta)) / 5 <= second <= 5 * Fraction(abs(delta)), who + (float(second),)
            info["near_edge"] = second <= Fraction(NEAR)
        elif fam == "edge":
            zb = exact.fr(m["zb"])
            s0, s1 = ray.min_cell_slack(zs, zs, *cell), ray.min_cell_slack(zb, zb, *cell)
            ok = all(Fraction(abs(delta)) / 2 <= s / exact.COSPI_6 <= 2 * Fraction(abs(delta)) for s in (s0, s1))
            assert ok, who + (float(s0), float(s1))
            info["near_edge"] = max(s0, s1) / exact.COSPI_6 <= Fraction(NEAR)
        elif fam == "xnode":
            ex = ray.first_exit(zs, *cell)
            jn = m["tnode"]
            assert ex is not None, who
            off = (ex[0] - ray.z[jn]) / (ray.z[jn + 1] - ray.z[jn])
            assert (off > 0) == (delta > 0) and Fraction(abs(delta)) / 2 <= abs(off) <= 2 * Fraction(abs(delta)), who + (float(off),)
    return out


def _cells_at(ray, z):
    x, y = ray.xy(z)
    zz = ray.at(ray.zz, z)
    qf, rf = (x / (2 * exact.COSPI_6) - y / 3) / zz, y * exact.TWO_THIRDS / zz
    cells = {}
    for q in range(exact.math_floor(qf) - 1, exact.math_floor(qf) + 3):
        for r in range(exact.math_floor(rf) - 1, exact.math_floor(rf) + 3):
            m = min(zz - abs(v) for v in exact.hex_forms(x, y, zz, q, r))
            if m >= 0:
                cells[(q, r)] = m / zz
    return cells, qf, rf


def _graze(info, f, delta, cap_t, who):
    """the exact minimum f of |u|^2 - cap^2 against what the row was built for: its sign, and for a miss its size, delta cap
    (2 cap + delta cap) within a factor 2"""
    want = Fraction(delta) * cap_t * (2 * cap_t + Fraction(delta) * cap_t)
    if delta > 0:
        assert f > 0 and want / 2 <= f <= 2 * want, who + (float(f), float(want))
    else:
        assert f < 0, who + (float(f), float(want))         # it crosses; how deep is measured (near_cap), not asserted
    lim = Fraction(NEAR) * cap_t * 2 * cap_t * (1 + Fraction(NEAR))
    if abs(f) <= lim:
        info["near_cap"] = 1 if f > 0 else -1


# ---------------------------------------------------------------------------------------------------------------------------
# checks on product outputs (host compile or device)

def kinds_of(name):
    """the kind columns of the host compile's certified run: they carry over to any run whose shared columns equal its bit for bit"""
    out = host_wall(name)[0]
    return out[:, pyprobe.WALL_HEAD:].reshape(out.shape[0], pyprobe.WALL_K, pyprobe.WALL_ENTRY)[:, :, pyprobe.WALL_SHARED:]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


_SOUND = {}


def check_wall_soundness(name, out, who):
    """items 1 and 2 on the certified run `out`; the kinds are the host compile's (asserted equal in the shared columns)"""
    S = wall_case(name)
    t, nmax = S["t"], S["nmax"]
    host = host_wall(name)[0]
    assert same_bits(pyprobe.wall_shared(out), pyprobe.wall_shared(host)).all(), (name, who, "differs from the host compile")
    kinds = kinds_of(name)
    ns, mono = t["n_shells"], t["mono"]
    counts = dict(certified=0, literal=0, skip0=0, skip1=0, skip2=0, miss=0, hit=0, beyond_trail=0)
    worst = dict(edge=math.inf, edge_at=None, cap=math.inf, cap_at=None, probe=math.inf, probe_at=None)
    bad = []
    rmax = float(np.max(t["cap"]))
    for idx in range(out.shape[0]):
        if out[idx, H["begin"]] == pyprobe.LS_INWALL_END:
            continue
        key = (name, idx)
        if key not in _SOUND:
            _SOUND[key] = _sound_row(S, idx, pyprobe.wall_trail(host[idx]), kinds[idx], ns, mono, nmax)
        c, w, b = _SOUND[key]
        for k, v in c.items():
            counts[k] += v
        counts["beyond_trail"] += max(0, int(out[idx, H["units"]]) - pyprobe.WALL_K)
        for k in ("edge", "cap", "probe"):
            if w[k] < worst[k]:
                worst[k], worst[k + "_at"] = w[k], (idx, S["meta"][idx]["fam"], S["meta"][idx]["delta"])
        bad += b
    assert not bad, "%s (%s): unsound certificates: %s" % (name, who, bad[:6])
    worst["probe"] = worst["probe"] / (1e-7 * rmax) if math.isfinite(worst["probe"]) else math.inf
    return dict(counts=counts, **worst)


def _sound_row(S, idx, trail, kinds, ns, mono, nmax):
    ray = ray_of(S["name"], idx)
    m = S["meta"][idx]
    c = dict(certified=0, literal=0, skip0=0, skip1=0, skip2=0, miss=0, hit=0)
    w = dict(edge=math.inf, cap=math.inf, probe=math.inf)
    bad = []
    L1, L2 = S["t"]["L1"], S["t"]["L2"]
    for u, e in enumerate(trail):
        kind, s0, s1, s2, visit = (int(v) for v in kinds[u])
        if kind == pyprobe.KIND_LITERAL:
            c["literal"] += 1
        elif kind == pyprobe.KIND_CERTIFIED:
            c["certified"] += 1
            q, r = int(e[TR["q_i"]]), int(e[TR["r_i"]])
            za, zb = exact.fr(e[TR["pz_b"]]), exact.fr(e[TR["pz_a"]])
            tag = (idx, m["fam"], m["cell"], m["delta"], u, float(za), float(zb))
            if not (zb > za and zb <= ray.z[nmax]):
                bad.append(tag + ("range",))
                continue
            sl = ray.min_cell_slack(za, zb, q, r)
            if not sl > 0:
                bad.append(tag + ("cell", float(sl)))
            w["edge"] = min(w["edge"], float(sl * exact.COSPI_6) / 1e-6)
            if abs(q) <= ns and abs(r) <= ns and abs(q + r) <= ns:
                f, at = ray.min_gap2(za, zb, exact.cell_K(q, r), ray.zz)
                if not f > 0:
                    bad.append(tag + ("capillary", float(f)))
                else:
                    capz, zz = float(ray.at(ray.cap, at)), float(ray.at(ray.zz, at))
                    w["cap"] = min(w["cap"], (math.sqrt(float(f) + capz * capz) - capz) / (1e-6 * zz))
        else:
            c["skip0"] += s0
            c["skip1"] += s1
            c["skip2"] += s2
            c["miss"] += visit == 6
            c["hit"] += visit == 7
            i0 = int(e[TR["z_id_b"]])
            i1 = i0 + s0 + L1 * s1 + L2 * s2
            if i1 > i0:
                K = (Fraction(0), Fraction(0)) if mono else exact.cell_K(int(e[TR["q_new"]]), int(e[TR["r_new"]]))
                tag = (idx, m["fam"], m["cell"], m["delta"], u, i0, i1)
                if i1 > nmax:
                    bad.append(tag + ("range",))
                    continue
                f, at = ray.min_gap2(ray.z[i0], ray.z[i1], K, ray.zh)
                if not f > 0:
                    bad.append(tag + ("probe", float(f)))
                else:
                    capz = float(ray.at(ray.cap, at))
                    w["probe"] = min(w["probe"], math.sqrt(float(f) + capz * capz) - capz)
    return c, w, bad


def check_wall_literal(name, out, lit, who):
    """item 3: every row that ended under its cap in both modes ends in the same head bit for bit; returns the number of rows whose
    literal run hit its cap"""
    S = wall_case(name)
    cols = [H[k] for k in pyprobe.WALL_END_COLS if k not in ("hx", "hy", "hz", "iesc")]
    done = (out[:, H["how"]] == pyprobe.WALL_FINISHED) & (lit[:, H["how"]] == pyprobe.WALL_FINISHED)
    same = same_bits(out[:, cols], lit[:, cols]).all(axis=1) & same_bits(out[:, :4], lit[:, :4]).all(axis=1)
    # hx, hy, hz and iesc are results only where the probe found the wall (iesc == 1: pc_wall_probe reads them then and only then).
    # Elsewhere they are what the last pc_segment call left behind -- the coordinates of a root it then rejected, its reason as a
    # negative code -- and a skipped block makes no such call (it sets iesc = -3).  Compared: iesc by what its readers test (1, 0,
    # anything else), the point where iesc == 1.
    ia, ib = out[:, H["iesc"]], lit[:, H["iesc"]]
    same &= (np.where(ia == 1, 1, np.where(ia == 0, 0, -1)) == np.where(ib == 1, 1, np.where(ib == 0, 0, -1)))
    hit = (ia == 1) & (ib == 1)
    hcols = [H["hx"], H["hy"], H["hz"]]
    same &= ~hit | same_bits(out[:, hcols], lit[:, hcols]).all(axis=1)
    rows = np.flatnonzero(done & ~same)
    assert rows.size == 0, (name, who, [(int(r), S["meta"][r]["fam"], S["meta"][r]["cell"], S["meta"][r]["delta"],
                                         out[r, cols].tolist(), lit[r, cols].tolist()) for r in rows[:3]])
    fwd = S["rows"][:, 5] > 0
    assert (out[fwd, H["how"]] == pyprobe.WALL_FINISHED).all(), (name, who, "a certified row needs more than %d units" % grid.LEAK_UNITS,
                                                                 np.flatnonzero(fwd & (out[:, H["how"]] != 0))[:6])
    return int((lit[fwd, H["how"]] == pyprobe.WALL_CAPPED).sum())


def check_wall_outcomes(name, out, who):
    """after the run: the begin cell is the exact one, every family ends as it was built to, units of every kind occur"""
    S = wall_case(name)
    info = built(name)
    kinds = kinds_of(name)
    for idx, m in enumerate(S["meta"]):
        o = out[idx]
        if m["fam"] == "begin":
            want = pyprobe.LS_INWALL_END if m["expect"] != "in" else (pyprobe.LS_WALL_PROBE if S["t"]["mono"] else pyprobe.LS_WALL_STEP)
            assert o[H["begin"]] == want and (m["expect"] == "in" or o[H["wt"]] == -2), (name, who, idx, m, o[:6])
            continue
        assert o[H["begin"]] != pyprobe.LS_INWALL_END, (name, who, idx, m["fam"], m["cell"], m["delta"], "not let in")
        if not S["t"]["mono"]:
            assert (int(o[H["q_i"]]), int(o[H["r_i"]])) == info[idx]["cell"], (name, who, idx, m["fam"], o[1:3], info[idx]["cell"])
        if m["fam"] in ("exit", "grid") and not S["t"]["mono"]:
            assert o[H["wt"]] == 2, (name, who, idx, m, o[H["wt"]])
        if m["fam"] == "side":
            assert o[H["wt"]] == 3, (name, who, idx, m, o[H["wt"]])
        if m["fam"] in ("cap", "nbr", "mono") and m["delta"] < 0 and o[H["units"]] <= pyprobe.WALL_K:
            k = kinds[idx, :int(o[H["units"]])]
            assert ((k[:, 0] == pyprobe.KIND_LITERAL) | (k[:, 4] > 0)).any(), (name, who, idx, m["fam"], "no literal step or visit")


def report(name, who, m):
    S = wall_case(name)
    line1 = "leak %-9s %-6s rows %4d  units %s" % (name, who, len(S["rows"]), " ".join("%s %d" % kv for kv in m["counts"].items() if kv[1]))
    line2 = ("      smallest slack of a certified stretch: cell edge %.4g, capillary %.4g (x 1e-6 zh); nearest certified miss of the probe "
             "%.4g (x 1e-7 rmax)" % (m["edge"], m["cap"], m["probe"]))
    print(line1)
    print(line2)
    return [line1, line2]


# ---- OUTER

@functools.lru_cache(maxsize=None)
def outer_case(name):
    g = grid.outer_grids()[name]
    t = pyemul.march_tables(g["problem"])
    ex = [exact.outer_scan(t, r[0:3], r[3:6]) if m["fam"] in ("dip", "cross") else (None, None) for r, m in zip(g["rows"], g["meta"])]
    return dict(name=name, p=g["problem"], rows=g["rows"], meta=g["meta"], t=t, exact=ex)


def outer_rows(name, literal):
    x = outer_case(name)["rows"].copy()
    x[:, 6] = 1.0 if literal else 0.0
    return x


@functools.lru_cache(maxsize=None)
def host_outer(name, literal=False):
    return pyprobe.run_outer(outer_case(name)["p"], outer_rows(name, literal), device=False)


def outer_built(name):
    """by the exact side alone: number of rows with a dip at exactly the one node they were aimed at; rows built to miss do"""
    S = outer_case(name)
    dips = 0
    for (j, clear), m, r in zip(S["exact"], S["meta"], S["rows"]):
        if m["fam"] not in ("dip", "cross") or m["delta"] == 0.0:
            continue
        if m["fam"] == "cross":
            assert j == m["node"], (name, m, j)
        elif m["delta"] < 0:
            assert j is None, (name, m, j)
        else:
            assert j == m["node"], (name, m, j)
            # exactly one node: with that node taken out of the scan nothing else is inside
            x = np.delete(np.arange(len(S["t"]["z"])), j)
            t2 = {k: S["t"][k][x] for k in ("z", "ext", "hexd")}
            assert exact.outer_scan(t2, r[0:3], r[3:6])[0] is None, (name, m)
            dips += 1
    return dips


def check_outer(name, out, lit, who):
    S = outer_case(name)
    z = S["t"]["z"]
    assert same_bits(out, lit).all(), (name, who, "literal scan differs", np.argwhere(~same_bits(out, lit))[:4].tolist())
    n = 0
    for idx, ((j, clear), m) in enumerate(zip(S["exact"], S["meta"])):
        if clear is None or clear < 8:
            continue
        n += 1
        if j is None:
            assert out[idx, 0] == 0, (name, who, idx, m, out[idx])
        else:
            # oz is formed as cz + bz (z - cz) / bz: where it is the bracket's end node itself, three roundings may leave it ulps off
            slack = 4 * np.spacing(z[-1])
            assert out[idx, 0] == 1 and z[j] - slack <= out[idx, 3] <= z[j + 1] + slack, (name, who, idx, m, out[idx], z[j], z[j + 1])
    return n


# ---- HEX

@functools.lru_cache(maxsize=None)
def hex_case():
    rows, meta = grid.hex_rows()
    ex = []
    for r in rows:
        cells, qf, rf = exact.hex_cells(*r)
        ex.append((cells, exact.hex_error_bound(r[0], r[1], r[2], qf, rf)))
    return dict(rows=rows, meta=meta, exact=ex, p=grid.wall_grids()["cylinder"]["problem"])


@functools.lru_cache(maxsize=None)
def host_hex():
    return pyprobe.run_hex(hex_case()["p"], hex_case()["rows"], device=False)


def check_hex(out, who):
    S = hex_case()
    near = 0
    for idx, ((cells, bound), m, r) in enumerate(zip(S["exact"], S["meta"], S["rows"])):
        got = (int(out[idx, 0]), int(out[idx, 1]))
        assert got[0] == out[idx, 0] and got[1] == out[idx, 1], (who, idx, out[idx])
        best = max(cells, key=cells.get)
        if len(cells) == 1 and cells[best] > 8 * bound:
            assert got == best, (who, idx, m, r.tolist(), got, best, float(cells[best]), float(bound))
        else:
            near += 1
            # a cell that meets the point's cell there: its own three forms exceed 1 by no more than 8 bounds
            x, y, zz = (exact.fr(v) for v in r)
            over = max(abs(v) for v in exact.hex_forms(x, y, zz, *got)) / zz - 1
            assert over <= 8 * bound, (who, idx, m, r.tolist(), got, sorted(cells), float(over))
            assert m.get("purpose") or cells[best] <= 8 * bound, (who, idx, m)
    assert near <= 0.05 * len(S["rows"]), (who, near, len(S["rows"]))
    return near


# ---- tables

def check_leak_tables(name):
    S = wall_case(name)
    t = S["t"]
    b = exact.leak_table_bounds(t)
    for L, col in ((t["L1"], "d1"), (t["L2"], "d2")):
        for i, e in enumerate(b[L]):
            if e is None:
                assert math.isinf(t[col][i]) and t[col][i] > 0, (name, col, i, "must be +inf")
            else:
                assert math.isfinite(t[col][i]) and exact.fr(t[col][i]) >= e, (name, col, i, t[col][i], float(e))
    assert np.array_equal(t["stp"], t["cap"] / 10.0), (name, "stp")
    ok = t["cap"] > 0
    assert np.array_equal(t["istp"][ok], 10.0 / t["cap"][ok]), (name, "istp")


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PROFILES)
def test_leak_tables_are_at_least_their_exact_values(name):
    check_leak_tables(name)


@pytest.mark.parametrize("name", PROFILES)
def test_wall_rows_are_what_they_were_built_to_be(name):
    built(name)


def test_wall_grids_hold_enough_rows_at_the_capillary_and_at_edges():
    out_side = in_side = edge = total = 0
    for name in PROFILES:
        b = built(name)
        out_side += sum(i["near_cap"] > 0 for i in b)
        in_side += sum(i["near_cap"] < 0 for i in b)
        edge += sum(i["near_edge"] for i in b)
        total += len(b)
    print("leak grids: %d WALL rows; closest approach to the avoided capillary within %g cap: %d outside, %d inside; within %g zh of a "
          "corner or an edge: %d" % (total, NEAR, out_side, in_side, NEAR, edge))
    assert out_side >= 200 and in_side >= 200 and edge >= 200


@pytest.mark.parametrize("name", PROFILES)
def test_certified_stretches_and_skipped_blocks_are_sound(name):
    out, code = host_wall(name)
    m = check_wall_soundness(name, out, "host")
    report(name, "host", m)
    c = m["counts"]
    if not wall_case(name)["t"]["mono"]:
        assert c["certified"] >= 1 and c["literal"] >= 1, (name, c)
        if wall_case(name)["nmax"] >= wall_case(name)["t"]["L2"] + 2:
            assert c["skip1"] >= 1 and c["skip2"] >= 1, (name, c)


@pytest.mark.parametrize("name", PROFILES)
def test_wall_rows_end_as_they_were_built_to(name):
    check_wall_outcomes(name, host_wall(name)[0], "host")


def test_literal_wall_search_agrees_at_the_adversarial_points():
    capped = total = 0
    for name in PROFILES:
        out, lit = host_wall(name)[0], host_wall(name, True)[0]
        assert check_wall_literal(name, out, lit, "host") == 0, (name, "a literal row needs more than 5e7 units")
        over = int((lit[:, H["units"]] > pyprobe.WALL_UNITS_DEVICE).sum())
        capped, total = capped + over, total + len(lit)
        assert not any((pyprobe.wall_trail(r)[:, TR["kind"]] == pyprobe.KIND_CERTIFIED).any() for r in lit), (name, "a certified unit in literal mode")
    print("leak grids: %d of %d WALL rows need more than %d units in literal mode (compared on the host compile only)"
          % (capped, total, pyprobe.WALL_UNITS_DEVICE))
    assert capped <= 0.05 * total


@pytest.mark.parametrize("name", grid.OUTER_PROFILES)
def test_outer_scan_finds_the_exact_first_node(name):
    out, lit = host_outer(name)[0], host_outer(name, True)[0]
    n = check_outer(name, out, lit, "host")
    print("outer %-9s rows %d, %d of them clear of hexd by 8 bounds" % (name, len(out), n))


def test_outer_grids_hold_enough_one_node_dips():
    dips = sum(outer_built(name) for name in grid.OUTER_PROFILES)
    print("outer grids: %d rows with a dip at exactly one node" % dips)
    assert dips >= 100


def test_hex_index_is_the_exact_cell():
    near = check_hex(host_hex()[0], "host")
    print("hex: %d rows, %d on an edge or corner within 8 bounds" % (len(hex_case()["rows"]), near))


def test_refused_rows():
    """a non-finite value, dz == 0 or too many units never reach the product"""
    S = wall_case("cylinder")
    x = S["rows"][:1].copy()
    for col, v in ((5, 0.0), (0, np.nan), (2, np.inf), (UNITS, float(pyprobe.WALL_UNITS_HOST + 1)), (LIT, 2.0), (HINT, 1e6)):
        y = x.copy()
        y[0, col] = v
        with pytest.raises(RuntimeError):
            pyprobe.run_wall(S["p"], y, device=False)


def test_a_hint_changes_nothing():
    """pc_wall_begin finds the same node from a hint (the segment of the reflection, or one some nodes off) as by bisection"""
    S = wall_case("taper")
    x = S["rows"][::7].copy()
    ref = pyprobe.run_wall(S["p"], x, device=False)[0]
    seg = np.clip(np.searchsorted(S["t"]["z"], x[:, 2], side="right") - 1, 0, S["nmax"] - 1)
    for hint in (seg, np.maximum(seg - 3, 0), np.minimum(seg + 4, S["nmax"] - 1), np.zeros_like(seg)):
        y = x.copy()
        y[:, HINT] = hint
        got = pyprobe.run_wall(S["p"], y, device=False)[0]
        assert same_bits(got, ref).all()
