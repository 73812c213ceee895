#!/usr/bin/env python3
"""Static instruction counts of the persistent LZ window kernels, from the compiler's assembly.

usage: lz_window_isa.py [--format lz4|snappy] [--commit REV] [-D...]
       lz_window_isa.py --diff REV [--api NAME ...] [--rename OLD=NEW ...] [-D...]

Compiles api/<format>_api.hip for the device only with the product's flags (plus any -D given), once as it is and once
with -DNVCOMP_LZW_RUNS=0 -- the kernel then holds only the instance of the decode loop without the run executor, the one
the mix runs -- and prints for <format>_decompress_window_kernel<true> of each: lines of assembly, vector ALU instructions
(v_*), all vector-side instructions (v_*, ds_*, global_*, flat_*, buffer_*, scratch_*), v_mov_b32 / v_mov_b64, s_waitcnt,
materialised ballots (v_cndmask_b32 v, 0, 1, mask whose only use is the v_cmp_ne_u32 0, v behind it), and the SGPR spill /
VGPR / scratch figures of the kernel's metadata. --commit counts the sources of that revision instead of the working tree.

--diff REV compiles api/NAME.hip (default: lz4_api snappy_api) from REV and from the working tree, each with the product's
flags for that file plus any -D given, and compares the text of every function of the two -- the kernels with their
.amdhsa_kernel descriptor, and the functions they call -- ignoring lines that hold the per-build __hip_cuid_ symbol and
the per-file numbering of local labels. One line per function: identical, different (instructions a / b), only in REV,
only in worktree; the exit status is 1 when any is different. This is how a refactor shows that it left the code alone.
--rename OLD=NEW replaces OLD by NEW in REV's assembly first: a refactor that renames a kernel's parameter type renames the
kernel's symbol (--rename 6Launch=7Tickets for lzl::Launch -> lzl::Tickets), which would otherwise read as two functions.
"""
import argparse
import concurrent.futures
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


# What csrc/Makefile adds to CXXFLAGS for single files.
PRODUCT_FLAGS = {"lz4_api": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
                 "snappy_api": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
                 "bitcomp_native_api": ["-fhip-fp32-correctly-rounded-divide-sqrt"]}


def checkout(rev, tmp):
    """The sources of `rev` unpacked under `tmp`, or the repository itself for the working tree."""
    if not rev:
        return REPO
    root = os.path.join(tmp, "src")
    os.makedirs(root)
    tar = subprocess.run(["git", "-C", REPO, "archive", rev, "nvcomp_amd/csrc", "include"], check=True,
                         stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", root], input=tar, check=True)
    return root


def compile_asm(root, api, flags, out):
    src = os.path.join(root, "nvcomp_amd", "csrc")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                    *PRODUCT_FLAGS.get(api, []), "--cuda-device-only", "-S",
                    "-I" + os.path.join(root, "include"), "-I" + src, "-Wno-unused-function", *flags,
                    os.path.join(src, "api", f"{api}.hip"), "-o", out], check=True)
    return open(out).read()


def functions(asm):
    """{symbol: text} of every function; a kernel's text ends with its .amdhsa_kernel descriptor."""
    asm = "\n".join(ln for ln in asm.splitlines() if "__hip_cuid_" not in ln)
    asm = re.sub(r"[ \t]+;", " ;", asm)  # comments are aligned behind labels, whose width follows the function's number
    asm = re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+_", r"\1_", asm)  # .LBB<function number>_<block>, and BB<n>_<block> in comments
    asm = re.sub(r"(\.Lfunc_(?:begin|end))\d+", r"\1", asm)
    out = {}
    for m in re.finditer(r"^\t\.type\t(\w+),@function\n", asm, re.M):
        sym = m.group(1)
        out[sym] = asm[asm.index(sym + ":", m.end()): asm.index(".Lfunc_end", m.end())]
        desc = re.search(r"^\t\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % sym, asm, re.M | re.S)
        if desc:
            out[sym] += desc.group(0)
    return out


def instructions(body):
    return sum(1 for ln in body.splitlines() if ln.startswith("\t") and not ln.lstrip().startswith((".", ";")) and ln.strip())


def diff(rev, apis, extra, keep, renames=()):
    with tempfile.TemporaryDirectory() as tmp:
        roots = {rev: checkout(rev, tmp), "worktree": REPO}
        jobs = [(api, side) for api in apis for side in roots]
        with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            texts = dict(zip(jobs, pool.map(lambda j: functions(compile_asm(
                roots[j[1]], j[0], extra, os.path.join(keep or tmp, f"{j[0]}_{j[1].replace('/', '_')}.s"))), jobs)))
    different = 0
    for api in apis:
        old, new = texts[api, rev], texts[api, "worktree"]
        for a, b in (r.split("=", 1) for r in renames):
            old = {sym.replace(a, b): text.replace(a, b) for sym, text in old.items()}
        for sym in sorted(set(old) | set(new)):
            name = subprocess.run(["c++filt", "-p", sym], stdout=subprocess.PIPE, text=True).stdout.strip()
            if sym not in new:
                verdict = f"only in {rev}"
            elif sym not in old:
                verdict = "only in worktree"
            elif old[sym] == new[sym]:
                verdict = "identical"
            else:
                verdict = f"different (instructions {instructions(old[sym])} / {instructions(new[sym])})"
                different += 1
            print(f"{api}: {name}: {verdict}")
    return 1 if different else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", default="lz4", choices=("lz4", "snappy"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--diff", default=None, metavar="REV")
    ap.add_argument("--api", nargs="+", default=["lz4_api", "snappy_api"])
    ap.add_argument("--keep", default=None, help="directory to keep the .s files in")
    ap.add_argument("--rename", nargs="+", default=[], metavar="OLD=NEW", help="--diff: applied to REV's assembly")
    a, extra = ap.parse_known_args()
    if a.diff:
        return diff(a.diff, a.api, extra, a.keep, a.rename)
    with tempfile.TemporaryDirectory() as tmp:
        root = checkout(a.commit, tmp)
        for label, flags in (("kernel", []), ("non_runs_loop", ["-DNVCOMP_LZW_RUNS=0"])):
            asm = compile_asm(root, f"{a.format}_api", [*flags, *extra], os.path.join(a.keep or tmp, f"{a.format}_{label}.s"))
            body, meta = kernel_text(asm, f"{a.format}_decompress_window_kernel")
            print(json.dumps({"format": a.format, "what": label, "commit": a.commit or "worktree", **count(body, meta)}))


if __name__ == "__main__":
    sys.exit(main())
