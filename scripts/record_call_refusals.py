"""Records tests/golden/call_refusals.json: what polycap_source_get_transmission_efficiencies answers to a bad environment, case by
case -- the complete error string and the Python exception type.  Every refusal here happens before a device is used.

    python scripts/record_call_refusals.py /path/to/parent/libpolycap.so

The library is the build of the commit the table is to characterise, kept outside the tree; each case runs in a child process with
POLYCAP_AMD_LIB pointing at it.  tests/test_call_refusals_cpu.py asserts the table string for string against the tree's own build, so
that a later change to the host code of the call (the grammars, the order of validation) shows every message it moves.  A case given
changed="new message" holds a message that is reworded on purpose by such a change: the recorded one stays in the table as "recorded"."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "call_refusals.json")
DECK = os.path.join("tests", "golden", "example", "xos1.inp")          # 291 energies

SPOT = "dist=0.5;window=-0.02,0.02,-0.02,0.02;bins=16x16"
HIST = "axis=x,d=0.5,range=-0.01:0.01,bins=64"
PAIR = "axis=x,d=0.5,range=-0.01:0.01,bins=16*axis=y,d=0.5,range=-0.01:0.01,bins=16"
SELECT = "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not"
EXAMPLE_JOINT = "axis=x,d=0.5,range=-0.01:0.01,bins=256*axis=slope_x,range=-0.005:0.005,bins=256;" \
                "axis=start_x,range=-0.3:0.3,bins=512*axis=start_y,range=-0.3:0.3,bins=512;energies=all"
W = ";window=-0.02,0.02,-0.02,0.02"

# what tests/test_spot_cpu.py, test_hist_cpu.py, test_joint_cpu.py, test_select_cpu.py, test_gather_cpu.py, test_stderr_cpu.py and
# test_beam_cpu.py provoke through the public call
SPOT_VALUES = [
    "dist=1;window=0.02,-0.02,-0.02,0.02;bins=16x16;energies=all", "dist=1" + W + ";bins=0x5;energies=all",
    "dist=1" + W + ";bins=16x16;energies=0,1000", "dist=" + ",".join(["1"] * 65) + W + ";bins=16x16",
    "dist=1,2" + W + ";bins=16384x8192", "dist=1" + W, "dist=1" + W + ";bins=4x4;energies=0,0",
    # one refusal per key, and the items' form
    "dist=abc" + W + ";bins=4x4", "dist=1;window=1,2,3;bins=4x4", "dist=1" + W + ";bins=16", "dist=1" + W + ";bins=4x4;energies=0,x",
    "dist=1" + W + ";bins=4x4;energies=", "dist=1" + W + ";bins=4x4;colour=red", "dist=1" + W + ";bins",
]
HIST_VALUES = [
    "", "energies=all", "axis=q,range=0:1,bins=4", "axis=x,range=0:1", "axis=x,bins=4", "axis=x,range=0,1,bins=4", "axis=x,range=0:1:2,bins=4",
    "axis=x,range=1:0,bins=4", "axis=x,range=0:1,bins=0", "axis=x,range=0:1,bins=four", "axis=x,d=-1,range=0:1,bins=4",
    "axis=nrefl,d=0.5,range=0:256,bins=256", "axis=x,centre=0.1:0,range=0:1,bins=4", "axis=r,centre=0.1,range=0:1,bins=4",
    "axis=x,range=0:1,bins=4,width=3", "axis=x,range=0:1,bins=4;window=1", "axis=x,range=0:1,bins=4;energies=",
    "axis=x,range=0:1,bins=4;energies=0,x", "axis=x,range=0:1,bins=4;energies=291", "axis=x,range=0:1,bins=4;energies=1,1",
    "axis=x,range=0:1,bins=65536", ";".join(["axis=z,range=0:1,bins=2"] * 17),
    ";".join(["axis=z,range=0:1,bins=2"] * 18), "axis=x,d=far,range=0:1,bins=4", "axis=x,range=0:1,bins=4,flag", "axis=start_x,range=0:1,bins=4",
]
JOINT_VALUES = [
    "", "energies=all", "axis=x,d=0.5,range=-0.01:0.01,bins=256", EXAMPLE_JOINT.replace("start_y", "start_z"),
    "axis=x,range=0:1,bins=4*axis=y,range=0:1", "axis=x,range=0:1,bins=4*axis=y,range=0:1,bins=4*axis=z,range=0:1,bins=4",
    "axis=x,range=0:1,bins=4*axis=y,range=0:1,bins=4;window=1", "axis=x,range=0:1,bins=4*axis=y,range=0:1,bins=4;energies=0,x",
    "axis=x,range=0:1,bins=4*axis=y,range=0:1,bins=4;energies=1,1", "axis=x,range=0:1,bins=4*axis=nrefl,d=0.5,range=0:256,bins=256",
    "axis=x,range=1:0,bins=4*axis=y,range=0:1,bins=4", "axis=x,range=0:1,bins=1024*axis=y,range=0:1,bins=1024",
    ";".join(["axis=z,range=0:1,bins=2*axis=nrefl,range=0:1,bins=2"] * 9),
    ";".join(["axis=z,range=0:1,bins=2*axis=nrefl,range=0:1,bins=2"] * 10), "axis=x,d=far,range=0:1,bins=4*axis=y,range=0:1,bins=4",
    "axis=x,range=0:1,bins=4*axis=r,centre=1,range=0:1,bins=4", "axis=x,range=0:1,bins=4*axis=y,range=0,1,bins=4",
    "axis=x,range=0:1,bins=4*axis=y,range=0:1,bins=4.5",
]
SELECT_VALUES = [
    "", ";;", "energies=all", "axis=r,range=0:1;window=1", SELECT.replace("nrefl", "n_refl"), "axis=x", "axis=x,range=0:1,bins=4",
    "axis=x,range=0:1,never", "axis=x,range=0", "axis=x,range=0:1x", "axis=x,range=0:1,d=far", "axis=r,range=0:1,centre=0",
    "axis=x,range=0:1;axis=nrefl,d=0.5,range=0:40", "axis=x,range=1:0", "axis=x,centre=0.1:0,range=0:1", ";".join(["axis=z,range=0:1"] * 9),
]
DRAW_VALUES = [
    "", "n=10,colour=red", "n", "n=10," + "x" * 64, "energy=3", "energy=3,phase=1", "n=0", "n=2147483648", "n=ten", "n=10,energy=291",
    "n=10,energy=-1", "n=10,energy=x", "n=10,phase=4294967296", "n=10,phase=-1", "n=10,phase=", "n=10,",
]
FLAG_VALUES = ["2", "yes", "", "01", " 1", "1.0", "-1", "on", "true"]
BAD_SHARES = ["1.5", "0", "abc", "0.5x"]
BAD_DEVICES = "1,x"
LEAK_WITHOUT_IMAGES = {"POLYCAP_IMAGES": "0"}

CASES = []


def case(name, env, leak_calc=False, changed=None):
    CASES.append(dict(name=name, env=env, leak_calc=leak_calc, **({"changed": changed} if changed else {})))


for i, v in enumerate(SPOT_VALUES):
    case("spot-%d" % i, {"POLYCAP_SPOT": v})
for i, v in enumerate(HIST_VALUES):
    case("hist-%d" % i, {"POLYCAP_HIST": v})
for i, v in enumerate(JOINT_VALUES):
    case("joint-%d" % i, {"POLYCAP_JOINT": v})
for i, v in enumerate(SELECT_VALUES):
    case("select-%d" % i, {"POLYCAP_SELECT": v})
for name in ("POLYCAP_STDERR", "POLYCAP_TALLY_STDERR", "POLYCAP_BEAM"):
    for i, v in enumerate(FLAG_VALUES):
        case("%s-%d" % (name[8:].lower(), i), {name: v})
for v in ["0", "-1", "abc", "2147483648"]:
    case("records-" + v, {"POLYCAP_SELECT": SELECT, "POLYCAP_SELECT_RECORDS": v})
case("records-without-select", {"POLYCAP_SELECT_RECORDS": "500"})
for i, v in enumerate(BAD_SHARES):
    # with POLYCAP_SPOT set a bad share is refused as part of POLYCAP_SPOT, without it under its own name
    case("share-spot-%d" % i, {"POLYCAP_SPOT": SPOT, "POLYCAP_SPOT_SHARE": v})
    case("share-beam-%d" % i, {"POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": v})
    case("share-hist-%d" % i, {"POLYCAP_HIST": HIST, "POLYCAP_SPOT_SHARE": v})
    case("share-joint-%d" % i, {"POLYCAP_JOINT": PAIR, "POLYCAP_SPOT_SHARE": v})
    case("share-select-%d" % i, {"POLYCAP_SELECT": SELECT, "POLYCAP_SPOT_SHARE": v})
case("devices", {"POLYCAP_HIP_DEVICES": BAD_DEVICES})
case("devices-too-many", {"POLYCAP_HIP_DEVICES": ",".join(["0"] * 65)})
case("leak-without-images", LEAK_WITHOUT_IMAGES, leak_calc=True)
# empty values: POLYCAP_SPOT and POLYCAP_HIP_DEVICES count as unset (so the next check in the order answers, and the share is not read);
# POLYCAP_HIST and POLYCAP_JOINT count as set (hist-0, joint-0 above)
case("empty-spot-is-unset", {"POLYCAP_SPOT": "", "POLYCAP_SPOT_SHARE": "2", "POLYCAP_HIP_DEVICES": BAD_DEVICES})
case("empty-devices-is-unset", dict(LEAK_WITHOUT_IMAGES, POLYCAP_HIP_DEVICES=""), leak_calc=True)
case("empty-share-is-unset", {"POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": "", "POLYCAP_HIP_DEVICES": BAD_DEVICES})
case("empty-select", {"POLYCAP_SELECT": "", "POLYCAP_SPOT_SHARE": "2"})
# two bad variables: the order of validation
case("order-stderr-before-tally-stderr", {"POLYCAP_STDERR": "2", "POLYCAP_TALLY_STDERR": "3"})
case("order-tally-stderr-before-beam", {"POLYCAP_TALLY_STDERR": "2", "POLYCAP_BEAM": "3"})
case("order-beam-before-spot", {"POLYCAP_BEAM": "2", "POLYCAP_SPOT": "dist=1"})
case("order-spot-before-hist", {"POLYCAP_SPOT": "dist=1", "POLYCAP_HIST": ""})
case("order-spot-grammar-before-share", {"POLYCAP_SPOT": "dist=1", "POLYCAP_SPOT_SHARE": "2"})
case("order-share-before-spot-validation", {"POLYCAP_SPOT": SPOT.replace("16x16", "0x5"), "POLYCAP_SPOT_SHARE": "2"})
case("order-spot-share-before-hist", {"POLYCAP_SPOT": SPOT, "POLYCAP_SPOT_SHARE": "2", "POLYCAP_HIST": ""})
case("order-hist-before-joint", {"POLYCAP_HIST": "", "POLYCAP_JOINT": ""})
case("order-joint-before-records", {"POLYCAP_JOINT": "", "POLYCAP_SELECT": SELECT, "POLYCAP_SELECT_RECORDS": "0"})
case("order-records-before-select", {"POLYCAP_SELECT": "axis=x", "POLYCAP_SELECT_RECORDS": "0"})
case("order-select-before-share", {"POLYCAP_SELECT": "axis=x", "POLYCAP_SPOT_SHARE": "2"})
case("order-hist-before-share", {"POLYCAP_HIST": "", "POLYCAP_SPOT_SHARE": "2"})
case("order-share-before-devices", {"POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": "2", "POLYCAP_HIP_DEVICES": BAD_DEVICES})
case("order-devices-before-images", dict(LEAK_WITHOUT_IMAGES, POLYCAP_HIP_DEVICES=BAD_DEVICES), leak_calc=True)
case("order-stderr-before-images", dict(LEAK_WITHOUT_IMAGES, POLYCAP_STDERR="2"), leak_calc=True)
# POLYCAP_DRAW: an empty value counts as set; one refusal per key and the items' form; and it is refused last
for i, v in enumerate(DRAW_VALUES):
    case("draw-%d" % i, {"POLYCAP_DRAW": v})
case("order-devices-before-draw", {"POLYCAP_DRAW": "n=0", "POLYCAP_HIP_DEVICES": BAD_DEVICES})
case("order-images-before-draw", dict(LEAK_WITHOUT_IMAGES, POLYCAP_DRAW=""), leak_calc=True)
case("order-share-before-draw", {"POLYCAP_DRAW": "n=0", "POLYCAP_BEAM": "1", "POLYCAP_SPOT_SHARE": "2"})
case("bad-draw-makes-no-selection", {"POLYCAP_DRAW": "n=0", "POLYCAP_SPOT_SHARE": "2"})

CHILD = """
import json, sys
from polycap_amd import capi
src = capi.Source.new_from_file(%r)
try:
    src.get_transmission_efficiencies(1, 1000, leak_calc=%r)
    print(json.dumps(dict(exception=None, message=None)))
except Exception as e:
    print(json.dumps(dict(exception=type(e).__name__, message=str(e))))
"""


def run_case(c, lib):
    env = {k: v for k, v in os.environ.items() if not k.startswith("POLYCAP_")}
    env.update(c["env"], POLYCAP_AMD_LIB=lib, HIP_VISIBLE_DEVICES="")          # no device: a case that is not refused must not run
    r = subprocess.run([sys.executable, "-c", CHILD % (DECK, c["leak_calc"])], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise SystemExit("case %s: the child failed\n%s" % (c["name"], r.stderr))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    lib = os.path.abspath(sys.argv[1])
    if lib.startswith(ROOT + os.sep + "polycap_amd"):
        raise SystemExit("the library to record from is the tree's own: give the parent commit's build")
    table = []
    for c in CASES:
        got = run_case(c, lib)
        if got["exception"] != "ValueError":
            raise SystemExit("case %s is not refused before a device is used: %r" % (c["name"], got))
        entry = dict(name=c["name"], env=c["env"], leak_calc=c["leak_calc"], exception=got["exception"], message=got["message"])
        if "changed" in c:
            entry.update(message=c["changed"], recorded=got["message"], changed=True)
        table.append(entry)
    assert len({e["name"] for e in table}) == len(table)
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(table), OUT))


if __name__ == "__main__":
    main()
