"""Scans of many energies: the logging kernel (context option "scan_log" = 1) against the immediate weight sweep (0, the default).

    python scripts/bench_scan_log.py [out.txt]

xos1 (smooth) and ellip_l9 with 5 A roughness at 12, 40 and 291 energies (the decks' own 291; linspace(5, 30, n) keV below); a
21 x 21 lateral grid of +-0.03 cm, 2000 slots per point, max_attempts 1 (441 x 2000 started photons per scan).  Per case one
context, one warm-up scan of each kind, then scan_log 0 and 1 alternating 5 times: kernel time of each (median, min, max; device
events around the launch) and the totals compared every time: counters always equal; the exact sums are equal bit for bit without
roughness, and with roughness the efficiencies agree to 1e-10 relative (the logging kernel lumps a log's roughness factors into one
exponential: ~4e-14 per weight).  Prints one JSON line per case and a table; with an argument the table is also written there.
Run it under a time limit:  timeout -k 10 900 python scripts/bench_scan_log.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
NPP, SIDE, HALF_WIDTH, REPS = 2000, 21, 0.03, 5


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def case(deck, ne, rough):
    kw = dict(sig_rough=5.0) if rough else {}
    if ne != 291:
        kw["energies"] = np.linspace(5.0, 30.0, ne)
    prob = polycap_amd.problem_from_inp(os.path.join(EXAMPLE, deck + ".inp"), **kw)
    assert prob.n_energies == ne
    ax = np.linspace(-HALF_WIDTH, HALF_WIDTH, SIDE)
    pts = polycap_amd.scan_points(x=ax + prob.source[5], y=ax + prob.source[6])
    t = {0: [], 1: []}
    with polycap_amd.TraceContext(prob) as ctx:
        for log in (0, 1):                                          # warm-up of both kernels at the timed shape
            ctx.set_option("scan_log", log)
            ctx.scan(1, pts, NPP, max_attempts=1)
        for i in range(REPS):
            r = {}
            for log in (0, 1):
                ctx.set_option("scan_log", log)
                r[log] = ctx.scan(7, pts, NPP, max_attempts=1)
                t[log].append(r[log]["kernel_ms"])
            assert (r[0]["kernel"], r[1]["kernel"]) == ("pc_trace_kernel", "pc_trace_log_kernel"), (r[0]["kernel"], r[1]["kernel"])
            assert np.array_equal(r[0]["counters"], r[1]["counters"]), i
            if rough:
                assert np.allclose(r[0]["efficiencies"], r[1]["efficiencies"], rtol=1e-10, atol=0.0), i
            else:
                assert np.array_equal(r[0]["sumw_fixed"], r[1]["sumw_fixed"]), i
    started = int(r[1]["counters"][:, 5].sum())
    out = dict(deck=deck, rough=bool(rough), energies=ne, points=len(pts), slots_per_point=NPP, started=started,
               exit=int(r[1]["counters"][:, 0].sum()), immediate_ms=spread(t[0]), logging_ms=spread(t[1]),
               speedup_median=float(np.median(t[0]) / np.median(t[1])),
               totals="counters equal, efficiencies to 1e-10" if rough else "bit-identical")
    print(json.dumps(out), flush=True)
    return out


def table(rows):
    lines = ["%-10s %5s %8s | %28s | %28s | %7s | %s" % ("deck", "rough", "energies", "scan_log 0: median [min, max] ms",
                                                         "scan_log 1: median [min, max] ms", "0 / 1", "totals")]
    for o in rows:
        a, b = o["immediate_ms"], o["logging_ms"]
        lines.append("%-10s %5s %8d | %10.2f [%7.2f, %7.2f] | %10.2f [%7.2f, %7.2f] | %6.2fx | %s" % (
            o["deck"], "5 A" if o["rough"] else "-", o["energies"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
            o["speedup_median"], o["totals"]))
    return "\n".join(lines)


if __name__ == "__main__":
    rows = [case(deck, ne, rough) for deck, rough in (("xos1", False), ("ellip_l9", True)) for ne in (12, 40, 291)]
    text = table(rows)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
