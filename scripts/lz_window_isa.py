#!/usr/bin/env python3
"""Static instruction counts of the persistent LZ window kernels, from the compiler's assembly.

usage: lz_window_isa.py [--format lz4|snappy] [--commit REV] [-D...]

Compiles api/<format>_api.hip for the device only with the product's flags (plus any -D given), once as it is and once
with -DNVCOMP_LZW_RUNS=0 -- the kernel then holds only the instance of the decode loop without the run executor, the one
the mix runs -- and prints for <format>_decompress_window_kernel<true> of each: lines of assembly, vector ALU instructions
(v_*), all vector-side instructions (v_*, ds_*, global_*, flat_*, buffer_*, scratch_*), v_mov_b32 / v_mov_b64, s_waitcnt,
materialised ballots (v_cndmask_b32 v, 0, 1, mask whose only use is the v_cmp_ne_u32 0, v behind it), and the SGPR spill /
VGPR / scratch figures of the kernel's metadata. --commit counts the sources of that revision instead of the working tree.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR = ("v_", "ds_", "global_", "flat_", "buffer_", "scratch_")


def kernel_text(asm, name):
    """The body of the first function whose demangled-ish symbol holds `name` and the bool argument `true` (Lb1E)."""
    sym = None
    for m in re.finditer(r"^(_Z\w*%s\w*Lb1E\w*):" % name, asm, re.M):
        sym = m.group(1)
        break
    if sym is None:
        raise SystemExit(f"no kernel {name}<true> in the assembly")
    start = asm.index(sym + ":")
    end = asm.index(".Lfunc_end", start)
    meta = re.search(r"\.name:\s+%s\n(.*?)(?=\n  - \.|\Z)" % re.escape(sym), asm, re.S)
    block = asm[asm.rfind("  - .", 0, meta.start()) if meta else 0: meta.end() if meta else 0]
    return asm[start:end], block


def count(body, meta):
    ins = [ln.split()[0] for ln in body.splitlines()
           if ln.startswith("\t") and not ln.lstrip().startswith((".", ";")) and ln.strip()]
    lines = body.splitlines()
    ballots = 0
    for i, ln in enumerate(lines):
        m = re.match(r"\s+v_cndmask_b32(?:_e64)? (v\d+), 0, 1, ", ln)
        if m and any(re.match(r"\s+v_cmp_ne_u32(?:_e32|_e64)? .*\b0, %s\b" % m.group(1), nxt) for nxt in lines[i + 1: i + 12]):
            ballots += 1
    def field(key):
        m = re.search(r"\.%s:\s+(\d+)" % key, meta)
        return int(m.group(1)) if m else None
    return {
        "asm_lines": len(lines),
        "valu": sum(1 for x in ins if x.startswith("v_")),
        "vector_all": sum(1 for x in ins if x.startswith(VECTOR)),
        "v_mov_b32": sum(1 for x in ins if x.startswith("v_mov_b32")),
        "v_mov_b64": sum(1 for x in ins if x.startswith("v_mov_b64")),
        "s_waitcnt": sum(1 for x in ins if x == "s_waitcnt"),
        "materialised_ballots": ballots,
        "sgpr_spills": field("sgpr_spill_count"),
        "vgpr_spills": field("vgpr_spill_count"),
        "vgprs": field("vgpr_count"),
        "scratch_bytes": field("private_segment_fixed_size"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", default="lz4", choices=("lz4", "snappy"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--keep", default=None, help="directory to keep the .s files in")
    a, extra = ap.parse_known_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = REPO
        if a.commit:
            root = os.path.join(tmp, "src")
            os.makedirs(root)
            tar = subprocess.run(["git", "-C", REPO, "archive", a.commit, "nvcomp_amd/csrc", "include"], check=True,
                                 stdout=subprocess.PIPE).stdout
            subprocess.run(["tar", "-x", "-C", root], input=tar, check=True)
        src = os.path.join(root, "nvcomp_amd", "csrc")
        for label, flags in (("kernel", []), ("non_runs_loop", ["-DNVCOMP_LZW_RUNS=0"])):
            out = os.path.join(a.keep or tmp, f"{a.format}_{label}.s")
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                            "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-S",
                            "-I" + os.path.join(root, "include"), "-I" + src, "-Wno-unused-function", *flags, *extra,
                            os.path.join(src, "api", f"{a.format}_api.hip"), "-o", out], check=True)
            body, meta = kernel_text(open(out).read(), f"{a.format}_decompress_window_kernel")
            print(json.dumps({"format": a.format, "what": label, "commit": a.commit or "worktree", **count(body, meta)}))


if __name__ == "__main__":
    sys.exit(main())
