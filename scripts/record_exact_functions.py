"""Records tests/golden/exact_functions.json: what the library's public host functions make of exact sums, output bit for output bit
-- pc_hip_fixed_to_double, pc_hip_efficiencies, pc_hip_efficiency_stderr, pc_hip_relay_efficiencies, pc_hip_scan_efficiencies,
pc_hip_tally_stderr, pc_hip_select_transmission -- over a few hundred fixed integer inputs each (200 to 240).

    python scripts/record_exact_functions.py /path/to/parent/libpolycap.so

The library is the build of the commit the table is to characterise, kept outside the tree.  Inputs are stored as integers (a sum is
one 128-bit integer), outputs as float.hex().  tests/test_exact_cpu.py asserts the table against the tree's own build, so that a change
to the arithmetic of exact sums (polycap_amd/csrc/hip/pc_exact.h and its callers) shows every last bit it moves.  None of the
functions uses a device."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "exact_functions.json")

T64, T128 = 2 ** 64, 2 ** 128
# sums at their seams: zero, lo at 2^64 - 1, the first hi, the scales, the top
SUMS = [0, 1, 2 ** 32, 2 ** 62 - 1, 2 ** 62, 2 ** 62 + 1, T64 - 1, T64, T64 + 1, 3 * T64 - 1, 2 ** 100, 2 ** 126, 2 ** 126 + T64 - 1, 2 ** 127, T128 - 1]
COUNTS = [0, 1, 2, 3, 7, 1000, 10 ** 6, 2 ** 31, 2 ** 40, 2 ** 62]


def sum128(r):
    k = r.random()
    if k < 0.25:
        return r.choice(SUMS)
    if k < 0.5:
        return r.getrandbits(r.randrange(1, 64))                      # hi = 0
    if k < 0.6:
        return (r.getrandbits(r.randrange(1, 64)) << 64) | (T64 - 1)  # lo at 2^64 - 1
    return r.getrandbits(r.randrange(65, 129))                        # hi != 0


def counters6(r, n=None):
    """six counters whose first three add up to n started photons"""
    if n is None:
        n = r.choice(COUNTS) if r.random() < 0.5 else r.getrandbits(r.randrange(1, 50))
    a = r.randrange(0, n + 1)
    b = r.randrange(0, n - a + 1)
    return [a, b, n - a - b, r.getrandbits(40), r.choice([0, 0, 3]), r.getrandbits(41)]


def moments(r, n, scale_bits):
    """sums A, B of n weights in units of 2^-scale_bits: plausible ones (0 <= w <= 1), and squares below the mean squared (the clamp)"""
    S = 2 ** scale_bits
    A = r.randrange(0, n * S + 1) if n else 0
    k = r.random()
    if k < 0.3:
        B = A * A // (n * S) // r.choice([1, 2, 1000]) if n else 0     # at or below N m^2: the clamp
    elif k < 0.8:
        B = r.randrange(0, A + 1)                                       # w^2 <= w
    else:
        B = sum128(r)
    return A, B


def cases():
    r = random.Random(20240229)
    out = []

    def add(fn, inputs):
        out.append(dict(fn=fn, inputs=inputs))

    for v in SUMS:
        add("pc_hip_fixed_to_double", dict(lo=v % T64, hi=v // T64))
    for _ in range(225):
        v = sum128(r)
        add("pc_hip_fixed_to_double", dict(lo=v % T64, hi=v // T64))

    for k in range(240):
        ne = 1 + k % 3
        n = [0, 1, 2][k] if k < 3 else None
        add("pc_hip_efficiencies", dict(num=[r.choice([0, 1, 2 ** 53 - 1, r.getrandbits(r.randrange(1, 54))]) for _ in range(ne)], counters=counters6(r, n)))

    for k in range(240):
        ne = 1 + k % 3
        c = counters6(r, COUNTS[k] if k < len(COUNTS) else None)
        n = c[0] + c[1] + c[2]
        ab = [moments(r, n, 62) if k >= 2 * len(COUNTS) else (sum128(r), sum128(r)) for _ in range(ne)]
        if k % 16 == 0:
            ab[0] = (0, 0)
        add("pc_hip_efficiency_stderr", dict(A=[x[0] for x in ab], B=[x[1] for x in ab], counters=c))

    for k in range(240):
        ne = 1 + k % 3
        n = COUNTS[k] if k < len(COUNTS) else (r.choice(COUNTS) if r.random() < 0.3 else r.getrandbits(r.randrange(1, 50)))
        n = -5 if k == 239 else n                                       # a negative count is "nothing started"
        ab = [moments(r, max(n, 0), 62) if k % 4 else (sum128(r), sum128(r)) for _ in range(ne)]
        c8 = [r.getrandbits(30) for _ in range(7)] + [n]
        add("pc_hip_relay_efficiencies", dict(A=[x[0] for x in ab], B=None if k % 3 == 0 else [x[1] for x in ab], counters=c8))

    for k in range(200):
        ne, P = 1 + k % 2, 1 + k % 3
        cnt, A, B = [], [], []
        for p in range(P):
            kind = r.random()
            if kind < 0.15:
                c = [0] * 6                                             # nothing started at this point
            elif kind < 0.3:
                c = [0, r.getrandbits(20), 0, 0, 0, r.getrandbits(21)]  # nothing entered a capillary
            else:
                c = counters6(r, r.choice([1, 2]) if kind < 0.4 else None)
            n = c[0] + c[1] + c[2]
            ab = [moments(r, n, 62) for _ in range(ne)]
            cnt.append(c); A.append([x[0] for x in ab]); B.append([x[1] for x in ab])
        add("pc_hip_scan_efficiencies", dict(counters=cnt, A=A, B=None if k % 5 == 0 else B))

    for k in range(240):
        cells = 1 + k % 3
        n = COUNTS[k] if k < len(COUNTS) else (r.choice(COUNTS) if r.random() < 0.3 else r.getrandbits(r.randrange(1, 40)))
        sums, squares = [], []
        for _ in range(cells):
            # a cell's sum is a uint64 in units of 2^-32, its squares a pair in units of 2^-64
            s = r.choice([0, 1, T64 - 1, min(n, 2 ** 31) * 2 ** 32, r.getrandbits(r.randrange(1, 65))])
            q = r.choice([0, s * s // max(n, 1) // 2, min(s * 2 ** 32, T128 - 1), sum128(r)])
            sums.append(s); squares.append(q)
        add("pc_hip_tally_stderr", dict(sums=sums, squares=squares, n_started=n))

    for k in range(240):
        ne = 1 + k % 2
        pw = [r.choice([0, 1, T64 - 1, r.getrandbits(r.randrange(1, 65))]) for _ in range(ne)]
        rw = [r.choice([0, 1, T64 - 1, r.getrandbits(r.randrange(1, 65))]) for _ in range(ne)]
        if k % 10 == 0:
            pw[0] = rw[0] = 0                                           # zero passed + rejected
        p2 = [r.choice([0, min(w * 2 ** 32, T128 - 1), sum128(r)]) for w in pw]
        r2 = [r.choice([0, min(w * 2 ** 32, T128 - 1), sum128(r)]) for w in rw]
        add("pc_hip_select_transmission", dict(pw=pw, rw=rw, p2=p2, r2=r2))
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    lib = os.path.abspath(sys.argv[1])
    if lib.startswith(ROOT + os.sep + "polycap_amd"):
        raise SystemExit("the library to record from is the tree's own: give the parent commit's build")
    os.environ["POLYCAP_AMD_LIB"] = lib          # read when polycap_amd is first imported
    sys.path.insert(0, ROOT)
    from tests.exact.pyexact import call
    table = {}
    for c in cases():
        table.setdefault(c["fn"], []).append([c["inputs"], [x.hex() for x in call(c["fn"], c["inputs"])]])
    # {function: [[inputs, outputs], ...]}, eight cases to a line
    blocks = []
    for fn, rows in table.items():
        rows = [json.dumps(c, separators=(",", ":")) for c in rows]
        blocks.append(json.dumps(fn) + ":[\n" + ",\n".join(",".join(rows[k:k + 8]) for k in range(0, len(rows), 8)) + "\n]")
    with open(OUT, "w") as f:
        f.write("{" + ",\n".join(blocks) + "}\n")
    print("%d cases -> %s" % (sum(len(v) for v in table.values()), OUT))


if __name__ == "__main__":
    main()
