"""What polycap_source_get_transmission_efficiencies makes of its environment (polycap_amd/csrc/host/pc_request.c), without a device
and without the library: tests/request/request_host.c is a program of its own over pc_request.c, pc_error.c and the host parts of the
tallies' headers.  tests/golden/call_requests.json holds accepted environments and the dump of every field of the struct pc_run_request
they parse to, recorded from the commit before pc_request.c existed (scripts/record_call_requests.py); tests/golden/call_refusals.json
holds the refused ones and their messages (tests/test_call_refusals_cpu.py asserts the same table through the library).  The program is
run once plain, and once under the sanitizers with leak detection: that run is what checks the frees behind every refusal."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HOST = os.path.join(ROOT, "polycap_amd", "csrc", "host")
HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "request")
CODES = {"ValueError": 1}          # POLYCAP_ERROR_INVALID_ARGUMENT

with open(os.path.join(ROOT, "tests", "golden", "call_requests.json")) as f:
    REQUESTS = json.load(f)
with open(os.path.join(ROOT, "tests", "golden", "call_refusals.json")) as f:
    REFUSALS = [dict(e, ne=291, n_photons=1000) for e in json.load(f)]          # as scripts/record_call_refusals.py made the call


def build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    objs = []
    for cc, std, src in (("gcc", "-std=c11", os.path.join(HOST, "pc_request.c")), ("gcc", "-std=c11", os.path.join(HOST, "pc_error.c")),
                         ("gcc", "-std=c11", os.path.join(HERE, "request_host.c")), ("g++", "-std=c++17", os.path.join(HERE, "request_validators.cpp"))):
        objs.append(os.path.join(str(tmp), name + "." + os.path.basename(src) + ".o"))
        subprocess.check_call([cc, std, *flags, "-I", INCLUDE, "-I", HOST, "-I", HIPD, "-c", src, "-o", objs[-1]])
    subprocess.check_call(["g++", *flags, *objs, "-lm", "-o", exe])
    return exe


def run(exe, cases, extra_env=None):
    """the lines the program prints for every case, and what it wrote to stderr"""
    text = "".join("%d %d %d %d\n" % (c["ne"], c["leak_calc"], c["n_photons"], len(c["env"])) +
                   "".join("%s=%s\n" % kv for kv in c["env"].items()) for c in cases)
    env = {k: v for k, v in os.environ.items() if not k.startswith("POLYCAP_")}
    env.update(extra_env or {})
    r = subprocess.run([exe], input=text, env=env, capture_output=True, text=True, timeout=120)
    blocks = []
    for line in r.stdout.splitlines():
        if line.startswith("case "):
            blocks.append([])
        elif line != "end":
            blocks[-1].append(line)
    return r, blocks


def check(blocks):
    assert len(blocks) == len(REQUESTS) + len(REFUSALS)
    for c, got in zip(REQUESTS, blocks):
        assert got == c["dump"], c["name"]
    for c, got in zip(REFUSALS, blocks[len(REQUESTS):]):
        assert got == ["error %d %s" % (CODES[c["exception"]], c["message"])], c["name"]


def test_the_table_covers_what_it_is_meant_to():
    names = [c["name"] for c in REQUESTS]
    assert len(set(names)) == len(names) >= 40
    used = set().union(*(c["env"] for c in REQUESTS))
    assert used >= {"POLYCAP_RUN_PARTS", "POLYCAP_COMPACT", "POLYCAP_BLOCK_SHIFT", "POLYCAP_RCCL", "POLYCAP_MAX_ATTEMPTS", "POLYCAP_SEED", "POLYCAP_IMAGES",
                    "POLYCAP_TIMING", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT", "POLYCAP_SPOT_SHARE", "POLYCAP_HIST", "POLYCAP_JOINT", "POLYCAP_SELECT",
                    "POLYCAP_SELECT_RECORDS", "POLYCAP_DRAW", "POLYCAP_STDERR", "POLYCAP_TALLY_STDERR", "POLYCAP_BEAM"}
    assert any(len(c["env"].get("POLYCAP_HIP_DEVICES", "").split(",")) == 64 for c in REQUESTS)
    assert any(c["leak_calc"] for c in REQUESTS) and {c["n_photons"] for c in REQUESTS} >= {1999999, 2000000}
    assert all(c["dump"] and not c["dump"][0].startswith("error") for c in REQUESTS)


def test_every_environment_parses_to_what_was_recorded(tmp_path):
    r, blocks = run(build(tmp_path, "request_host", ["-O2"]), REQUESTS + REFUSALS)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check(blocks)


def test_parsing_is_clean_under_the_sanitizers_and_leaks_nothing(tmp_path):
    """both tables in one process, the refusals' failure paths included: any report of AddressSanitizer, UndefinedBehaviorSanitizer or
    LeakSanitizer fails (they exit non-zero and write to stderr)"""
    exe = build(tmp_path, "request_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r, blocks = run(exe, REQUESTS + REFUSALS, {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and r.stderr == "", r.stderr
    check(blocks)
