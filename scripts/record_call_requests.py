"""Records tests/golden/call_requests.json: what polycap_source_get_transmission_efficiencies parses an accepted environment into, case
by case -- the text dump of every field of its struct pc_run_request, as tests/request/request_host.c prints it.

    python scripts/record_call_requests.py /path/to/parent/checkout

The checkout is the built tree of the commit the table is to characterise, kept outside this tree.  The dumper is this tree's
tests/request/request_host.c, compiled over that commit's file that holds the parsers (pc_request.c; pc_source.c where they were still
static in it) and linked against that commit's libpolycap.so for the rest.  tests/test_request_cpu.py asserts the table line for line
against the tree's own pc_request.c, so that a later change to the parsing shows every field it moves.  No case uses a device."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "call_requests.json")

SPOT = "dist=0.5,1,2;window=-0.02,0.02,-0.02,0.02;bins=256x128"
HIST = "axis=x,d=0.5,range=-0.01:0.01,bins=2048;axis=r,d=0.5,centre=0.001:-0.002,range=0:0.02,bins=1024;axis=nrefl,range=0:256,bins=256"
JOINT = "axis=x,d=0.5,range=-0.01:0.01,bins=64*axis=slope_x,range=-0.005:0.005,bins=32;" \
        "axis=start_x,range=-0.3:0.3,bins=128*axis=start_y,range=-0.3:0.3,bins=96"
SELECT = "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not"
DRAW = "n=100000,energy=3,phase=12345"
BIG = 2000000          # POLYCAP_RUN_PARTS is read from this many photons on

CASES = []


def case(name, env, ne=291, leak_calc=False, n_photons=1000):
    CASES.append(dict(name=name, ne=ne, leak_calc=leak_calc, n_photons=n_photons, env=env))


case("nothing-set", {})
case("nothing-set-leak", {}, leak_calc=True)
case("nothing-set-big", {}, n_photons=BIG)
# the lenient variables: valid, and unparsable (the default)
for v in ["8", "abc", ""]:
    case("run-parts-%s-big" % (v or "empty"), {"POLYCAP_RUN_PARTS": v}, n_photons=BIG)
case("run-parts-below-the-threshold", {"POLYCAP_RUN_PARTS": "8"}, n_photons=BIG - 1)
case("run-parts-leak", {"POLYCAP_RUN_PARTS": "8"}, leak_calc=True, n_photons=BIG)
case("run-parts-without-images", {"POLYCAP_RUN_PARTS": "8", "POLYCAP_IMAGES": "0"}, n_photons=BIG)
for v in ["0", "1", "abc", ""]:
    case("compact-%s" % (v or "empty"), {"POLYCAP_COMPACT": v})
case("compact-leak", {"POLYCAP_COMPACT": "1"}, leak_calc=True)
for v in ["16", "0x10", "abc", ""]:
    case("block-shift-%s" % (v or "empty"), {"POLYCAP_BLOCK_SHIFT": v})
for v in ["0", "1", "abc", ""]:
    case("rccl-%s" % (v or "empty"), {"POLYCAP_RCCL": v})
for v in ["1000", "abc", "4294967296"]:
    case("max-attempts-%s" % v, {"POLYCAP_MAX_ATTEMPTS": v})
for v in ["12345", "0x10", "18446744073709551615", "abc", ""]:
    case("seed-%s" % (v or "empty"), {"POLYCAP_SEED": v})
for v in ["0", "1", "abc", ""]:
    case("images-%s" % (v or "empty"), {"POLYCAP_IMAGES": v})
for v in ["1", "0", ""]:
    case("timing-%s" % (v or "empty"), {"POLYCAP_TIMING": v})
# device lists
case("devices-one", {"POLYCAP_HIP_DEVICES": "3"})
case("devices-repeated", {"POLYCAP_HIP_DEVICES": "0,1,0,1"})
case("devices-64", {"POLYCAP_HIP_DEVICES": ",".join(str(k % 8) for k in range(64))})
case("devices-empty", {"POLYCAP_HIP_DEVICES": ""})
# the flags
for name in ("POLYCAP_STDERR", "POLYCAP_TALLY_STDERR", "POLYCAP_BEAM"):
    for v in "01":
        case("%s-%s" % (name[8:].lower().replace("_", "-"), v), {name: v})
# the grammars, each with energies=all and with a list
case("spot-all", {"POLYCAP_SPOT": SPOT + ";energies=all"})
case("spot-list", {"POLYCAP_SPOT": SPOT + ";energies=0,290,17"})
case("spot-no-energies", {"POLYCAP_SPOT": SPOT})
case("spot-energies-twice", {"POLYCAP_SPOT": "energies=1,2;" + SPOT + ";energies=all"})
case("spot-empty-is-unset", {"POLYCAP_SPOT": ""})
case("hist-all", {"POLYCAP_HIST": HIST + ";energies=all"})
case("hist-list", {"POLYCAP_HIST": "energies=5,4;" + HIST})
case("hist-one-energy", {"POLYCAP_HIST": "axis=z,range=0:1,bins=2;energies=0"}, ne=1)
case("joint-all", {"POLYCAP_JOINT": JOINT + ";energies=all"})
case("joint-list", {"POLYCAP_JOINT": JOINT + ";energies=7,8,9"})
case("select", {"POLYCAP_SELECT": SELECT})
case("select-records", {"POLYCAP_SELECT": SELECT, "POLYCAP_SELECT_RECORDS": "500"})
case("select-records-max", {"POLYCAP_SELECT": "axis=start_x,range=-1:1", "POLYCAP_SELECT_RECORDS": "2147483647"})
case("draw-implicit-selection", {"POLYCAP_DRAW": DRAW})
case("draw-n-only", {"POLYCAP_DRAW": "n=1"})
case("draw-with-select", {"POLYCAP_DRAW": DRAW, "POLYCAP_SELECT": SELECT})
case("draw-leak", {"POLYCAP_DRAW": "phase=4294967295,n=2147483647,energy=290"}, leak_calc=True)
# POLYCAP_SPOT_SHARE through its two readers: as part of POLYCAP_SPOT, and under its own name without it
case("share-with-spot", {"POLYCAP_SPOT": SPOT, "POLYCAP_SPOT_SHARE": "0.25"})
case("share-with-spot-and-beam", {"POLYCAP_SPOT": SPOT, "POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": "1"})
case("share-with-beam", {"POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": "0.125"})
case("share-with-hist", {"POLYCAP_HIST": HIST, "POLYCAP_SPOT_SHARE": "1e-3"})
case("share-with-joint", {"POLYCAP_JOINT": JOINT, "POLYCAP_SPOT_SHARE": "0x1p-4"})
case("share-with-select", {"POLYCAP_SELECT": SELECT, "POLYCAP_SPOT_SHARE": "0.5"})
case("share-with-draw", {"POLYCAP_DRAW": DRAW, "POLYCAP_SPOT_SHARE": "0.75"})
case("share-default-with-beam", {"POLYCAP_BEAM": "1"})
case("share-empty-with-beam", {"POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": ""})
case("share-not-read", {"POLYCAP_SPOT_SHARE": "7"})
case("share-not-read-with-beam-0", {"POLYCAP_BEAM": "0", "POLYCAP_SPOT_SHARE": "7"})
case("everything", {"POLYCAP_STDERR": "1", "POLYCAP_TALLY_STDERR": "1", "POLYCAP_BEAM": "1", "POLYCAP_SPOT": SPOT + ";energies=1,2,3",
                    "POLYCAP_SPOT_SHARE": "0.01", "POLYCAP_HIST": HIST + ";energies=all", "POLYCAP_JOINT": JOINT + ";energies=4",
                    "POLYCAP_SELECT": SELECT, "POLYCAP_SELECT_RECORDS": "100", "POLYCAP_DRAW": DRAW, "POLYCAP_HIP_DEVICES": "1,0",
                    "POLYCAP_IMAGES": "0", "POLYCAP_RUN_PARTS": "2", "POLYCAP_COMPACT": "0", "POLYCAP_BLOCK_SHIFT": "12", "POLYCAP_RCCL": "1",
                    "POLYCAP_MAX_ATTEMPTS": "99", "POLYCAP_SEED": "7", "POLYCAP_TIMING": "1"}, n_photons=BIG)


def stdin_of(cases):
    """the cases as tests/request/request_host.c reads them"""
    return "".join("%d %d %d %d\n" % (c["ne"], c["leak_calc"], c["n_photons"], len(c["env"])) +
                   "".join("%s=%s\n" % kv for kv in c["env"].items()) for c in cases)


def blocks_of(stdout):
    """the lines the dumper printed for every case"""
    blocks = []
    for line in stdout.splitlines():
        if line.startswith("case "):
            blocks.append([])
        elif line != "end":
            blocks[-1].append(line)
    return blocks


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    if parent == ROOT or parent.startswith(ROOT + os.sep):
        raise SystemExit("the checkout to record from is this tree: give the parent commit's, built, outside it")
    host, lib = os.path.join(parent, "polycap_amd", "csrc", "host"), os.path.join(parent, "polycap_amd", "lib")
    source = os.path.join(host, "pc_request.c")
    if not os.path.exists(source):
        source = os.path.join(host, "pc_source.c")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "request_host")
        # what the parsers call is exported by that commit's library; the rest of that file is never called, and what it alone
        # refers to inside the library may stay unresolved
        subprocess.check_call(["gcc", "-std=c11", "-O1", '-DREQUEST_HOST_SOURCE="%s"' % source,
                               "-I", os.path.join(parent, "include"), "-I", host, os.path.join(ROOT, "tests", "request", "request_host.c"),
                               "-Wl,--unresolved-symbols=ignore-all", "-L", lib, "-lpolycap", "-lm", "-Wl,-rpath," + lib, "-o", exe])
        env = {k: v for k, v in os.environ.items() if not k.startswith("POLYCAP_")}
        env["HIP_VISIBLE_DEVICES"] = ""
        r = subprocess.run([exe], input=stdin_of(CASES), env=env, capture_output=True, text=True, timeout=120, check=True)
    blocks = blocks_of(r.stdout)
    assert len(blocks) == len(CASES) and len({c["name"] for c in CASES}) == len(CASES)
    for c, dump in zip(CASES, blocks):
        if dump[0].startswith("error "):
            raise SystemExit("case %s is not accepted: %s" % (c["name"], dump[0]))
        c["dump"] = dump
    with open(OUT, "w") as f:
        json.dump(CASES, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(CASES), OUT))


if __name__ == "__main__":
    main()
