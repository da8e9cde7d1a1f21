"""Static instruction counts of the launching-wave trace kernel, from a reduced translation unit that compiles in seconds.

    python scripts/analysis/producer_listing.py                 # pc_trace_producer_kernel<0, false, false>
    python scripts/analysis/producer_listing.py --all           # the six instantiations the library launches (MODE 0 and 1)
    python scripts/analysis/producer_listing.py --runs 8        # also: runs of >= 8 consecutive register copies, by line
    python scripts/analysis/producer_listing.py --root DIR      # the sources of another checkout of this repository
    python scripts/analysis/producer_listing.py --probe         # scripts/analysis/event_probe.hip (the EVENT visit and the
                                                                # hot march step around one photon, alone)
    python scripts/analysis/producer_listing.py --keep DIR      # leave the .hip and .s files in DIR

The unit is pc_kernels.hip -- a list of includes in dependency order -- up to and including its
`#include "pc_producer_kernel.h"`, plus explicit instantiations; the kernel's code is the same as in the full build (same flags,
nothing after that line is visible to it).  The few plain kernels of the headers in front of that line (pc_images.h,
pc_trace_kernel.h) compile along and are left out of the listing.  Nothing is run: the
compile is for the device only.  Per kernel: vector-ALU instructions (mnemonics that start with v_), how many of them are
plain register copies or selects (v_mov_b32, v_mov_b64, v_cndmask_b32, v_accvgpr_read/write/mov, in their _e32 / _e64
encodings only: DPP and SDWA forms move data between lanes and are not counted as copies), and the registers, spills and
scratch bytes of the kernel's descriptor.

--runs N lists every run of at least N copies in a row (`first line-last line count`, with the loop nesting the assembler
comments give).  A photon that lives in two register sets shows as runs of 20-30 copies inside the tracing loop (Depth=1):
one at the head of a phase, one before the back edge.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MOVES = ("v_mov_b32", "v_mov_b64", "v_cndmask_b32", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_accvgpr_mov_b32")
INSTANCES = ["0, false, false", "0, true, false", "0, false, true", "1, false, false", "1, true, false", "1, false, true"]


def flags(root):
    hipd = os.path.join(root, "polycap_amd", "csrc", "hip")
    return ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
            "-I" + os.path.join(root, "include"), "-I" + hipd, "-S", "--cuda-device-only"]


def reduced_unit(root, instances):
    lines = open(os.path.join(root, "polycap_amd", "csrc", "hip", "pc_kernels.hip")).read().split("\n")
    cut = next(k for k, l in enumerate(lines) if l.startswith('#include "pc_producer_kernel.h"'))
    return "\n".join(lines[:cut + 1] + ["template __global__ void pc_trace_producer_kernel<%s>(pc_kargs);" % i for i in instances]) + "\n"


def is_move(op):
    return any(op == m or op == m + "_e32" or op == m + "_e64" for m in MOVES)


def is_inst(line):
    return line.startswith("\t") and not line.startswith(("\t.", "\t;"))


def count(asm):
    """[(kernel name, counts, body lines, first line number)] for every kernel of the assembly text."""
    meta = asm[asm.rindex("amdhsa.kernels:"):asm.rindex("amdhsa.target:")]
    out = []
    for blk in re.split(r"\n  - ", meta)[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        sym = g("symbol").replace(".kd", "").strip("'\"")
        start = asm.index("\n" + sym + ":") + 1
        body = asm[start:]
        body = body[:body.index(".Lfunc_end")].split("\n")
        ops = [l.split()[0] for l in body if is_inst(l)]
        valu = [o for o in ops if o.startswith("v_")]
        out.append((g("name"), dict(valu=len(valu), moves=sum(is_move(o) for o in valu), insts=len(ops),
                                    vgpr=g("vgpr_count"), agpr=g("agpr_count"), vspill=g("vgpr_spill_count"),
                                    sspill=g("sgpr_spill_count"), scratch=g("private_segment_fixed_size")),
                    body, asm.count("\n", 0, start) + 1))
    return out


def move_runs(body, line0, least):
    """(first line, last line, copies, loop depth) of every run of at least `least` copies with no other instruction between."""
    runs, run, depth = [], [], 0
    for n, l in enumerate(body + ["\ts_endpgm"]):
        m = re.search(r"Depth[= ](\d+)", l)
        if l.startswith(".LBB"):
            depth = int(m.group(1)) if m else 0
        if not is_inst(l):
            continue
        if is_move(l.split()[0]):
            run.append(n)
        else:
            if len(run) >= least:
                runs.append((line0 + run[0], line0 + run[-1], len(run), depth))
            run = []
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--runs", type=int, default=0)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--keep")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    d = a.keep or tempfile.mkdtemp(prefix="producer_listing_")
    os.makedirs(d, exist_ok=True)
    if a.probe:
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_probe.hip")
    else:
        src = os.path.join(d, "producer_unit.hip")
        open(src, "w").write(reduced_unit(root, INSTANCES if a.all else INSTANCES[:1]))
    s = os.path.join(d, os.path.basename(src)[:-4] + ".s")
    subprocess.check_call(["hipcc"] + flags(root) + [src, "-o", s], stderr=subprocess.DEVNULL)
    demangle = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for name, c, body, line0 in count(open(s).read()):
        if not a.probe and "pc_trace_producer_kernel" not in name:
            continue
        if demangle:
            name = subprocess.check_output([demangle, name]).decode().strip()
        print("%-56s VALU %5d  mov/cndmask %4d  all %5d  vgpr %s agpr %s vspill %s sspill %s scratch %s" % (
            name.replace("void ", "").replace("(pc_kargs)", "")[:56], c["valu"], c["moves"], c["insts"], c["vgpr"], c["agpr"],
            c["vspill"], c["sspill"], c["scratch"]))
        if a.runs:
            for first, last, n, depth in move_runs(body, line0, a.runs):
                print("    lines %5d-%5d  %2d copies in a row  (loop depth %d)" % (first, last, n, depth))
    if not a.keep:
        shutil.rmtree(d)


if __name__ == "__main__":
    sys.exit(main())
