"""The geometric half of a reflection -- pc_segment, pc_reflect_geom, pc_refl_geom3 and the direction update of pc_event_post
(pc_device.h) -- in the host compile and in the oracle, element by element against the reference's definitions in exact
arithmetic (mpmath, tests/devmath/exact.py) on the inputs where they can go wrong (tests/devmath/grid.py).  The same checks run
on the device in tests/test_gpu_devmath_geom.py.  Every measured maximum is printed (run with -s).

Status codes.  A status is asserted where every quantity the reference compares (the discriminant, zr - z0, z1 - zr, zr - last -
1e-5, d_proj - 1e-10, alfa) lies further from its threshold than CODE_MARGIN times the first-order running error bound of the
reference's own evaluation of it (exact.segment: one 2^-53 per operation, the cancellations in q = p0 - c0, in a and in b^2 -
4ac included).  Measured over the whole segment grid: the host compile's |hz - hz*| reaches 0.59 of that bound, the oracle's
0.59 (rays parallel to the wall); CODE_MARGIN = 8 is 13 times that.  Points inside the margin are reported, not asserted on.

Placed on purpose inside the margin: tangent rays with the discriminant at 0, +-1 and +-64 ulp of b^2 (0, 0.05 and 3.5 bounds); rays parallel to the wall with a at 0, +-1
ulp of the slope (2 to 4 ulp of rr^2, the finest step of the direction's doubles) and relative 1e-15 ... 1e-13 of rr^2; roots at z0 and z1 and +-1, +-8 ulp around them; the 1e-5 and 1e-10 guards at 0 and
+-1 ulp (and the 1e-10 guard's +-1e-12 where z0's spacing does not resolve it); alfa = -1e-16.  Outside: tangent rays at
relative 1e-12 ... 1e-3, parallel rays at 1e-12 ... 1e-6, the guards at +-1e-12 and +-1e-8, both roots valid, start on the
wall, dz < 0.  test_margins_leave_the_grids_decided prints which is which as the exact side finds them.
"""
import functools

import numpy as np

from tests.devmath import exact, grid, pyprobe

EPS = exact.EPS
CODE_MARGIN = 8.0        # in units of exact.segment's running error bound; measured error / bound: host 0.59, oracle 0.59
MARGIN_CAP = 0.02        # at most this share of a grid's points may lie inside the margin
M_ORACLE = 4.0           # host compile and device within this factor of the oracle's largest error per bucket
FLOOR_ULPS = 4.0         # absolute floor per point, used only where the oracle's bucket maximum lies below it (the oracle happens to be
#                          exact): ulps of the coordinate scale (z1 for hz, z1 and |P| + R for h); for the angle the same displacement
#                          of the hit seen from the axis, floor_h / min(R0, R1)
NORMAL_LEN = 4.0 * EPS   # | |n| - 1 |: the three products n_k f (2^-53 each, shared), the rounding of eps and of f
K_GEOM = 4.0             # measured errors of pc_reflect_geom / pc_refl_geom3 against exact.geom's running error bound
BOUNCE_LEN = 4.0 * EPS   # growth of | |d| - 1 | per bounce for unit normals and alfa <= 0.3: 2^-52 for the three fma of the update
#                          plus 2 alfa (3 * 2^-53) for the cosine's own rounding; measured below
UNKNOWN = -99
REGULAR = ("bulk", "switch", "both_roots", "on_wall")


def oracle_segment(r):
    """oracle.segment on a probe row, its arguments formed as polycap_capil_trace forms them (src/polycap-capil.c:1246-1258)"""
    from oracle import pyoracle as O
    z0, z1, R0, R1, zh0, zh1, kx, ky, Px, Py, Pz, dx, dy, dz = (float(v) for v in r)
    with np.errstate(all="ignore"):
        one = np.float64(1.0)
        c0, c1 = (kx * zh0, ky * zh0, z0), (kx * zh1, ky * zh1, z1)
        p0 = (Px + dx * (z0 - Pz) / (dz * one), Py + dy * (z0 - Pz) / (dz * one), z0)
        p1 = (Px + dx * (z1 - Pz) / (dz * one), Py + dy * (z1 - Pz) / (dz * one), z1)
    rc, h, n = O.segment(c0, c1, R0, R1, p0, p1, (dx, dy, dz), (Px, Py, Pz))
    return rc, list(h) + list(n)


def _ratio(guards):
    m = np.inf
    for _, v, err in guards:
        if err > 0:
            m = min(m, float(abs(v) / err))
    return m


def _bucket(fam, ex):
    """conditioning bucket of a point with exact status 1: the decade of the selected root's condition number; the families that
    sit on a cancellation by construction are kept apart from the regular points (and rays parallel to the wall by the decade of
    |a| / rr^2: there a itself is rounding noise, which the condition number of the root does not see)"""
    dec = int(np.floor(np.log10(float(ex["cond"])))) if np.isfinite(float(ex["cond"])) else 99
    if fam in REGULAR:
        return "regular  cond 1e%+03d" % dec
    if fam == "parallel":
        r = float(abs(ex["a"]) / ex["rr2"])
        return "parallel |a|/rr2 " + ("0" if r == 0 else "1e%+03d" % int(np.floor(np.log10(r))))
    if fam == "tangent":
        return "tangent  cond 1e%+03d" % dec
    return "seams    cond 1e%+03d" % dec


@functools.lru_cache(maxsize=None)
def segment_case():
    """the segment grid with its exact side and the oracle's results, computed once"""
    rows, fam = grid.segment_rows()
    n = rows.shape[0]
    finite = np.all(np.isfinite(rows), axis=1)
    ex = [exact.segment(r) if f else None for r, f in zip(rows, finite)]
    status = np.array([UNKNOWN if (e is None or e["status"] is None) else e["status"] for e in ex])
    ratio = np.array([0.0 if e is None else _ratio(e["guards"]) for e in ex])
    clear = (status != UNKNOWN) & (ratio > CODE_MARGIN)
    oc, oo = zip(*[oracle_segment(r) for r in rows])
    oc, oo = np.array(oc), np.array(oo)
    hit = status == 1
    bucket = np.array([_bucket(f, e) if h else "" for f, e, h in zip(fam, ex, hit)])
    return dict(p=grid.problem("deck"), rows=rows, fam=fam, ex=ex, status=status, ratio=ratio, clear=clear, oracle_code=oc,
                oracle_out=oo, hit=hit, bucket=bucket, n=n)


def segment_errors(S, out, code):
    """[n, 4] = |hz - hz*|, |h - h*|, angle(n, n*), | |n| - 1 | where the exact status and `code` are 1, else NaN"""
    e = np.full((S["n"], 4), np.nan)
    for i in np.flatnonzero(S["hit"] & (code == 1)):
        e[i] = exact.segment_errors(S["ex"][i], out[i])
    return e


@functools.lru_cache(maxsize=None)
def oracle_envelope():
    """per bucket the oracle's largest |hz - hz*|, |h - h*| and angle"""
    S = segment_case()
    eo = segment_errors(S, S["oracle_out"], S["oracle_code"])
    env = {}
    for b in sorted(set(S["bucket"]) - {""}):
        k = (S["bucket"] == b) & np.isfinite(eo[:, 0])
        if not k.any():          # a bucket of points inside the margin where the oracle itself finds no hit
            continue
        env[b] = dict(n=int(k.sum()), err=eo[k, :3].max(axis=0))
    return env, eo


def check_segment_status(out, code, who):
    """`who`'s statuses against the exact ones where the margins decide, against the oracle's for inputs the reference rejects or
    mangles (dz < 0, dz = 0, NaN), and the setup's rejection of a NaN profile"""
    S = segment_case()
    fam, st, clear = S["fam"], S["status"], S["clear"]
    near = ~clear & (st != UNKNOWN)
    print("SEGMENT %-6s statuses %s; %d of %d inside the margin, %d of them differ from the exact status" % (
        who, dict(zip(*np.unique(code, return_counts=True))), near.sum(), S["n"], (code != st)[near].sum()))
    assert np.array_equal(code[clear], st[clear]), (who, [(fam[i], code[i], st[i], S["ratio"][i]) for i in np.flatnonzero(clear & (code != st))[:8]])
    profile = np.isin(fam, ["nan_z0", "nan_z1", "nan_cap0", "nan_cap1"])
    assert np.all(code[profile] == pyprobe.SETUP_REJECT)      # pc_build_tables refuses the profile: no kernel ever sees it
    rej = (np.char.startswith(fam, "nan_") | np.char.startswith(fam, "dz_")) & ~profile
    assert rej.sum() == 15
    for i in np.flatnonzero(rej):
        print("SEGMENT %-6s %-12s status %3d oracle %3d" % (who, fam[i], code[i], S["oracle_code"][i]))
    assert np.array_equal(code[rej], S["oracle_code"][rej])
    assert np.all(code[fam == "dz_negative"] == -1)


def check_segment_accuracy(out, code, who):
    """`who`'s hit and normal within M_ORACLE of the oracle's own error per conditioning bucket, and |n| = 1"""
    S = segment_case()
    env, eo = oracle_envelope()
    e = segment_errors(S, out, code)
    # wherever the margins decide the status the hit exists on both sides
    assert np.all(np.isfinite(e[S["hit"] & S["clear"], 0]))
    worst = {}
    r = S["rows"]
    fz = FLOOR_ULPS * 2 * EPS * np.abs(r[:, 1])
    fh = FLOOR_ULPS * 2 * EPS * np.hypot(r[:, 1], np.hypot(r[:, 8], r[:, 9]) + np.maximum(r[:, 2], r[:, 3]))
    floor = np.stack([fz, fh, fh / np.minimum(r[:, 2], r[:, 3])], axis=1)
    for b, v in env.items():
        k = (S["bucket"] == b) & np.isfinite(e[:, 0])
        mine = e[k, :3].max(axis=0) if k.any() else np.zeros(3)
        print("SEGMENT %-28s n %5d | hz oracle %.2e %-6s %.2e | h oracle %.2e %-6s %.2e | angle oracle %.2e %-6s %.2e" % (
            b, k.sum(), v["err"][0], who, mine[0], v["err"][1], who, mine[1], v["err"][2], who, mine[2]))
        worst[b] = mine
        # the floor counts only where the oracle's own maximum lies below it (there the oracle happens to be exact)
        env_k = np.broadcast_to(v["err"][None, :], floor[k].shape)
        bound = np.where(env_k >= floor[k], M_ORACLE * env_k, np.maximum(M_ORACLE * env_k, floor[k]))
        over = e[k, :3] > bound
        assert not over.any(), (who, b, mine, v, r[k][over.any(axis=1)][:3].tolist())
    ln = e[np.isfinite(e[:, 3]), 3]
    rr = (S["rows"][:, 3] - S["rows"][:, 2]) / (S["rows"][:, 1] - S["rows"][:, 0])
    for name, k in (("series", np.abs(rr) < 0.9e-2), ("1/sqrt", np.abs(rr) > 1.1e-2)):
        k = k & np.isfinite(e[:, 3])
        assert k.sum() > 80
        print("SEGMENT %-6s | |n| - 1 | <= %.2e (%s branch, %d points)" % (who, e[k, 3].max(), name, k.sum()))
    assert ln.max() <= NORMAL_LEN, (who, ln.max())
    return worst


@functools.lru_cache(maxsize=None)
def geom_case():
    rows, fam, alfa = grid.geom_rows()
    ex = [exact.geom(r) for r in rows]
    b_alfa = np.array([float(e["bound"]["alfa"]) for e in ex])
    a = np.array([float(e["own"]["alfa"]) for e in ex])
    status = np.where(a < 0, -1, 1)
    clear = (np.abs(a) > CODE_MARGIN * b_alfa) | (b_alfa == 0)
    return dict(p=grid.problem("deck"), rows=rows, fam=fam, target=alfa, ex=ex, alfa=a, status=status, clear=clear, n=rows.shape[0])


GEOM_KEYS = ("alfa", "st2", "es2", "ep2", "sd2", "c2", "fs", "fp")


def check_geom(out, code, who):
    G = geom_case()
    ex, fam = G["ex"], G["fam"]
    near = ~G["clear"]
    print("GEOM %-6s statuses %s; %d of %d inside the margin (%s), %d of them differ" % (
        who, dict(zip(*np.unique(code, return_counts=True))), near.sum(), G["n"], sorted(set(fam[near])), (code != G["status"])[near].sum()))
    assert np.array_equal(code[G["clear"]], G["status"][G["clear"]])
    assert np.all(code[(fam == "alfa_negative") & G["clear"]] == -1)
    ok = (code == 1) & np.array([e["own"]["sd2"] > 0 for e in ex])
    # normal incidence (n = d: |n x d| = 0) has no s direction: the reference's fractions are 0/0 there, and these are 0/0 or
    # the quotient of two rounding residues; nothing to hold them against
    deg = (code == 1) & ~ok
    assert set(fam[deg]) <= {"normal_incidence", "axes"}
    K = np.zeros((G["n"], len(GEOM_KEYS)))
    for i in np.flatnonzero(ok):
        for j, key in enumerate(GEOM_KEYS):
            b = float(ex[i]["bound"][key])
            err = exact.absdiff(out[i, j], ex[i]["own"][key])
            K[i, j] = err / b if b > 0 else (0.0 if err == 0 else np.inf)
    dec = np.floor(np.log10(np.maximum(np.abs(G["alfa"]), 1e-300)))
    for d in sorted(set(dec[ok].tolist())):
        k = ok & (dec == d)
        print("GEOM %-6s alfa 1e%+03d n %4d | error / bound: %s" % (who, d, k.sum(), "  ".join("%s %.2f" % (key, K[k, j].max()) for j, key in enumerate(GEOM_KEYS))))
    assert K[ok].max() <= K_GEOM, (who, K[ok].max(), np.unravel_index(np.argmax(np.where(ok[:, None], K, 0)), K.shape))
    fs, fp = out[ok, 6], out[ok, 7]
    s = np.array([exact.absdiff(a, 1 - exact._m(b)) for a, b in zip(fs, fp)])
    print("GEOM %-6s |fs + fp - 1| <= %.2e; fs in [%.17g, %.17g], fp in [%.17g, %.17g]" % (who, s.max(), fs.min(), fs.max(), fp.min(), fp.max()))
    assert s.max() <= 4 * EPS
    assert fs.min() >= 0.0 and fs.max() <= 1.0 and fp.min() >= 0.0 and fp.max() <= 1.0, (
        who, fam[ok][np.argmin(fp)], G["rows"][ok][np.argmin(fp)].tolist(), fp.min(), fs.max())
    # sd2 and st2 are two routes to sin^2 theta: |n x d|^2 = |n|^2 |d|^2 - (n.d)^2
    lag = np.array([float(abs((e["own"]["len_d"] * e["own"]["len_n"]) ** 2 - 1)) for e in ex])
    bb = np.array([float(e["bound"]["sd2"] + e["bound"]["st2"]) for e in ex])
    diff = np.abs(out[:, 4] - out[:, 1])
    print("GEOM %-6s |sd2 - st2| <= %.2e (unit vectors: %.2e)" % (who, diff[ok].max(), diff[ok & (lag < 8 * EPS)].max()))
    assert np.all(diff[ok] <= K_GEOM * bb[ok] + lag[ok])
    # against the reference's definitions, which normalise d, n and E: what the lengths handed on cost
    lE = np.array([float(abs(exact._dot(exact._v(r[3:6]), exact._v(r[3:6])) - 1)) for r in G["rows"]])
    for key, j, ref in (("alfa", 0, "cos"), ("st2", 1, "sin2"), ("fs", 6, "fs"), ("fp", 7, "fp")):
        d = np.array([exact.absdiff(out[i, j], ex[i]["ref"][ref]) for i in np.flatnonzero(ok)])
        b = np.array([float(ex[i]["bound"][key]) for i in np.flatnonzero(ok)])
        slack = (lag[ok] if key in ("alfa", "st2") else lE[ok]) * 2
        print("GEOM %-6s %-4s against the reference's definition: <= %.2e (unit inputs: %.2e)" % (who, key, d.max(), d[slack < 16 * EPS].max()))
        assert np.all(d <= K_GEOM * b + slack)
    return K


def check_bounce(out, code, who):
    G = geom_case()
    ex, rows = G["ex"], G["rows"]
    ok = code >= 0
    # a valid energy of the deck: the reflection is refused exactly where alfa < 0
    assert np.array_equal(code[G["clear"]] < 0, G["alfa"][G["clear"]] < 0)
    assert (ok & G["clear"]).sum() > 4000
    # E' = |E| component by component (the reference loses the signs, src/polycap-capil.c:546-559)
    assert np.array_equal(out[ok, 3:6], np.abs(rows[ok, 3:6]))
    assert np.array_equal(out[~ok, 0:6], rows[~ok, 0:6])
    K, dev, grow = [], [], []
    for i in np.flatnonzero(ok):
        o, r, b = ex[i]["own"], ex[i]["ref"], ex[i]["bound"]
        errs = [(exact.absdiff(out[i, k], o["mirror"][k]), float(b["mirror"][k])) for k in range(3)]
        K.append(max((e / bk if bk > 0 else (0.0 if e == 0 else np.inf)) for e, bk in errs))
        nlen = float(abs(o["len_n"] ** 2 - 1))
        dev.append(max(exact.absdiff(out[i, k], r["mirror"][k]) - K_GEOM * float(b["mirror"][k]) - 2 * abs(G["alfa"][i]) * nlen * 1.0000001 * abs(rows[i, 6 + k])
                       for k in range(3)))
        grow.append((abs(exact.vec_len_minus_one(out[i, 0:3]) - float(o["len_d"] - 1)), 2 * EPS + 2 * abs(G["alfa"][i]) * float(b["alfa"]) + 2 * G["alfa"][i] ** 2 * nlen))
    K, dev, grow = np.array(K), np.array(dev), np.array(grow)
    print("BOUNCE %-6s d' against d - 2 (d.n) n: error / bound <= %.2f; against the exact mirror image beyond bound and |n|: %.2e; "
          "| |d'| - |d| | <= %.2e (%.2f of its bound)" % (who, K.max(), dev.max(), grow[:, 0].max(), (grow[:, 0] / grow[:, 1]).max()))
    assert K.max() <= K_GEOM and dev.max() <= 0.0
    assert np.all(grow[:, 0] <= K_GEOM * grow[:, 1])
    # the probe's own |d'| - 1 (one sqrt) is the exact one to an ulp
    own = np.array([exact.vec_len_minus_one(out[i, 0:3]) for i in np.flatnonzero(ok)])
    assert np.abs(out[ok, 6] - own).max() <= 4 * EPS


def bounce_chain(device, n=400, bounces=64, seed=5):
    """n random unit directions through `bounces` reflections off unit normals at grazing cosines 1e-6 ... 0.3, each bounce one
    probe call on the previous output: (| |d_k| - 1 | max per bounce [bounces], largest step of |d|)"""
    p = grid.problem("deck")
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    E = np.zeros((n, 3)); E[:, 0] = 1.0
    prev = np.array([exact.vec_len_minus_one(v) for v in d])
    drift, step = [], 0.0
    for _ in range(bounces):
        u = rng.normal(size=(n, 3))
        u -= (u * d).sum(axis=1)[:, None] * d / (d * d).sum(axis=1)[:, None]
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
        a = 10.0 ** rng.uniform(-6, np.log10(0.3), n)
        nn = a[:, None] * d + np.sqrt(1 - a * a)[:, None] * u
        nn /= np.sqrt((nn * nn).sum(axis=1))[:, None]
        out, code = pyprobe.run_geom(p, "bounce", np.hstack([d, E, nn]), device=device)
        assert np.all(code >= 0)
        d, E = out[:, 0:3].copy(), out[:, 3:6].copy()
        cur = np.array([exact.vec_len_minus_one(v) for v in d])
        step = max(step, np.abs(cur - prev).max())
        drift.append(np.abs(cur).max())
        prev = cur
    return np.array(drift), step


def check_bounce_chain(device, who):
    drift, step = bounce_chain(device)
    print("BOUNCE %-6s 64 bounces of 400 directions: largest step of |d| %.2e, | |d| - 1 | after 1 / 8 / 64 bounces %.2e / %.2e / %.2e" % (
        who, step, drift[0], drift[7], drift[63]))
    assert step <= BOUNCE_LEN
    assert np.all(drift <= BOUNCE_LEN * np.arange(1, 65) + 2 * EPS)


# ---------------------------------------------------------------------------------------------------------------------------

def test_margins_leave_the_grids_decided():
    """With the exact side alone: at most MARGIN_CAP of each grid lies inside the status margin, the points placed on a threshold
    do, and the exact statuses cover every exit of the reference (1, -1, -2, -3, -6; -4 and -5 repeat tests the selected root
    of two has already passed: only the double root of an exactly tangent ray can reach them)."""
    S, G = segment_case(), geom_case()
    decided = S["status"] != UNKNOWN
    inside = decided & ~S["clear"]
    for f in sorted(set(S["fam"])):
        k = S["fam"] == f
        if not np.char.startswith(f, "nan_"):
            print("margin %-12s %4d points, %3d inside; exact statuses %s" % (f, k.sum(), (inside & k).sum(), dict(zip(*np.unique(S["status"][k], return_counts=True)))))
    for f in ("tangent", "parallel", "seam_z0", "seam_z1", "guard_1e-5", "guard_1e-10"):
        for i in np.flatnonzero(S["fam"] == f):
            g = min((t for t in S["ex"][i]["guards"] if t[2] > 0), key=lambda t: abs(t[1]) / t[2], default=None)
            if g:
                print("margin %-12s %-7s status %3d nearest guard %-16s value %+.3e = %.3g bounds" % (
                    f, "inside" if inside[i] else "outside", S["status"][i], g[0], float(g[1]), float(abs(g[1]) / g[2])))
    assert inside.sum() <= MARGIN_CAP * S["n"], inside.sum()
    assert (~decided).sum() <= 16 + 2          # NaN rows, dz = 0, a = 0
    assert not inside[np.isin(S["fam"], REGULAR)].any()
    for f, least in (("tangent", 3), ("parallel", 3), ("seam_z0", 3), ("seam_z1", 3), ("guard_1e-5", 3), ("guard_1e-10", 3)):
        k = S["fam"] == f
        assert (inside & k).sum() >= least and (f.startswith("seam") or (S["clear"] & k).sum() >= 4), f
    assert {1, -1, -2, -3, -6} <= set(S["status"].tolist())
    assert (~G["clear"]).sum() <= MARGIN_CAP * G["n"]
    assert (~G["clear"] & (G["fam"] == "alfa_negative")).any() and (G["clear"] & (G["fam"] == "alfa_negative")).sum() >= 10


def test_oracle_statuses_are_the_exact_ones():
    """the oracle (the reference's arithmetic) returns the exact status wherever the margins decide: the exact side and the
    margin are right about the reference"""
    S = segment_case()
    assert np.array_equal(S["oracle_code"][S["clear"]], S["status"][S["clear"]])
    assert S["clear"][S["hit"]].sum() > 6000


def test_segment_status_host():
    S = segment_case()
    out, code = pyprobe.run_geom(S["p"], "segment", S["rows"], device=False)
    check_segment_status(out, code, "host")


def test_segment_hit_and_normal_host():
    """pc_segment in the host compile: hit and normal within M_ORACLE of the oracle's own error against the exact values per
    conditioning bucket; | |n| - 1 | <= NORMAL_LEN on both sides of the series switch."""
    S = segment_case()
    out, code = pyprobe.run_geom(S["p"], "segment", S["rows"], device=False)
    check_segment_accuracy(out, code, "host")
    # p0 is the ray at z0
    k = S["hit"]
    p0 = np.array([[float(v) for v in S["ex"][i]["p0"]] for i in np.flatnonzero(k)])
    scale = np.abs(S["rows"][k, 8:10]) + np.abs(S["rows"][k, 11:13] / S["rows"][k, 13:14] * (S["rows"][k, 0:1] - S["rows"][k, 10:11]))
    assert np.all(np.abs(out[k, 6:8] - p0) <= 4 * EPS * scale)


def test_reflection_geometry_host():
    """pc_reflect_geom and pc_refl_geom3 in the host compile: every quantity within K_GEOM of its running error bound, fs + fp =
    1, both in [0, 1] (E along s and along p included), sd2 against st2."""
    G = geom_case()
    out, code = pyprobe.run_geom(G["p"], "geom", G["rows"], device=False)
    check_geom(out, code, "host")


def test_bounce_host():
    G = geom_case()
    out, code = pyprobe.run_geom(G["p"], "bounce", G["rows"], device=False)
    check_bounce(out, code, "host")


def test_bounce_chain_host():
    check_bounce_chain(False, "host")


def test_geometry_probe_rejects_bad_calls():
    """widths and op numbers are checked before anything is read"""
    import ctypes as C
    from tests.emul import pyemul
    p = grid.problem("deck")
    x = np.zeros((4, 9)); out = np.zeros((4, 8)); code = np.zeros(4, dtype=np.int32); e = np.zeros(4, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    f = pyemul.lib().emul_probe_run_geom
    args = lambda op, wi, wo: (C.byref(p.s), op, 4, e.ctypes.data_as(ip), x.ctypes.data_as(pyprobe.c_double_p), wi,
                               out.ctypes.data_as(pyprobe.c_double_p), wo, code.ctypes.data_as(ip))
    assert f(*args(14, 9, 8)) == 0
    assert f(*args(14, 14, 8)) == -2 and f(*args(13, 9, 8)) == -2 and f(*args(14, 9, 2)) == -2
    assert f(*args(3, 8, 2)) == -2 and f(*args(16, 9, 8)) == -2
    e[2] = p.n_energies
    assert f(*args(14, 9, 8)) == -2
