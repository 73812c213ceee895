"""The stdout contract the reference's benchmark scripts rely on, met by this library's harness programs.

The reference's benchmarks/benchmark.sh and benchmarks/benchmark_all_algorithms.sh run
`./bin/benchmark_<algo>_chunked -f FILE [-t TYPE] [-a VARIANT] [-r R -d D -b B]` and cut four numbers out of every
program's stdout with awk: field 3 of the line starting `uncompressed `, field 5 of the line holding `compressed ratio:`,
field 4 of the lines starting `compression throughput ` and `decompression throughput `. A user switching libraries keeps
those scripts, so the programs of benchmarks/*.cpp must print those lines for every command line the scripts compose.

The programs are built here against the kernels' host emulation (tests/emu): same sources, same stdout, no GPU. The
contract on the GPU build is checked by tests/test_programs.py::test_chunked_harness_on_gpu.
"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = ["lz4", "snappy", "cascaded", "bitcomp", "deflate", "ans"]


@pytest.fixture(scope="module")
def emu_bench_dir(tmp_path_factory):
    """A directory laid out like the reference's benchmarks/: ./bin/benchmark_<algo>_chunked, built for the emulator."""
    import conftest

    conftest.emu_library()
    root = tmp_path_factory.mktemp("bench")
    os.makedirs(root / "bin")
    jobs = []
    for algo in ALGOS:
        cmd = ["g++", "-O1", "-std=c++17", "-Itests/emu", "-Iinclude", "-Ibenchmarks", "-Iexamples",
               f"benchmarks/benchmark_{algo}_chunked.cpp", "-o", str(root / "bin" / f"benchmark_{algo}_chunked"),
               "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
        jobs.append(subprocess.Popen(cmd, cwd=REPO, stderr=subprocess.PIPE))
    for j in jobs:
        _, err = j.communicate()
        assert j.returncode == 0, err.decode()[-2000:]
    return root


def _datasets(dirpath, names):
    from nvcomp_amd import datasets

    gens = [datasets.int32_column, datasets.silesia_style, datasets.float_columns, datasets.table_rows]
    for i, name in enumerate(names):
        data = gens[i % len(gens)](96 * 1024 + 40 * i, i)
        np.asarray(data).tofile(os.path.join(dirpath, name))


def _field(stdout, pattern, n):
    """awk '/pattern/{print $n}': field n (1-based, split on blanks) of every line matching the regular expression."""
    return [line.split()[n - 1] for line in stdout.splitlines() if re.search(pattern, line) and len(line.split()) >= n]


def _run(bench_dir, algo, path, *flags):
    """One program as the scripts start it (from the benchmarks directory); the four numbers they read from its stdout."""
    r = subprocess.run([f"./bin/benchmark_{algo}_chunked", "-f", str(path), *flags], cwd=str(bench_dir),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (algo, flags, r.stderr[-2000:])
    fields = [_field(r.stdout, "^uncompressed ", 3), _field(r.stdout, "compressed ratio:", 5),
              _field(r.stdout, "^compression throughput ", 4), _field(r.stdout, "^decompression throughput ", 4)]
    for f in fields:
        assert len(f) == 1, (algo, flags, r.stdout[-2000:])
    return int(fields[0][0]), float(fields[1][0]), float(fields[2][0]), float(fields[3][0])


def test_harness_stdout_for_benchmark_sh(emu_bench_dir, tmp_path):
    """benchmark.sh's command line, `-f FILE` alone: bytes = the file's size, a ratio, two throughputs."""
    data = tmp_path / "data"
    os.makedirs(data)
    _datasets(str(data), ["a_column.bin", "b_mix.bin"])
    for algo in ("lz4", "snappy", "ans"):
        ratios = []
        for name in ("a_column.bin", "b_mix.bin"):
            size, ratio, comp, decomp = _run(emu_bench_dir, algo, data / name)
            assert size == os.path.getsize(data / name)
            assert ratio > 0.9 and comp >= 0 and decomp >= 0, (algo, name, ratio, comp, decomp)
            ratios.append(ratio)
        assert ratios[0] > 1.5, "the int32 column compresses with every one of these codecs"


# benchmark_all_algorithms.sh: its four datasets and, per dataset, the flags it adds for the typed codecs
ALL_ALGORITHMS_FLAGS = {
    "mortgage-2009Q2-col0-long.bin": {"lz4": ["-t", "int"], "bitcomp": ["-t", "uchar"],
                                      "cascaded": ["-r", "1", "-d", "0", "-b", "1", "-t", "longlong"]},
    "silesia.tar": {"lz4": ["-t", "char"], "bitcomp": ["-t", "ulonglong"],
                    "cascaded": ["-r", "0", "-d", "0", "-b", "1", "-t", "char"]},
    "texturecache.tar": {"lz4": ["-t", "char"], "bitcomp": ["-t", "ushort"],
                         "cascaded": ["-r", "1", "-d", "0", "-b", "1", "-t", "short"]},
    "geometrycache.tar": {"lz4": ["-t", "char"], "bitcomp": ["-t", "ulonglong"],
                          "cascaded": ["-r", "1", "-d", "0", "-b", "1", "-t", "int"]},
}


def test_harness_stdout_for_all_algorithms_flags(emu_bench_dir, tmp_path):
    """benchmark_all_algorithms.sh's command lines: every program on its four datasets, LZ4 and Bitcomp typed (-t),
    Bitcomp in both variants (-a 0 / 1), Cascaded with its per-dataset scheme (-r -d -b -t)."""
    data = tmp_path / "data"
    os.makedirs(data)
    names = list(ALL_ALGORITHMS_FLAGS)
    _datasets(str(data), names)
    for name in names:
        flags = ALL_ALGORITHMS_FLAGS[name]
        runs = [("lz4", flags["lz4"]), ("snappy", []), ("cascaded", flags["cascaded"]),
                ("bitcomp", ["-a", "0"] + flags["bitcomp"]), ("bitcomp", ["-a", "1"] + flags["bitcomp"]),
                ("deflate", []), ("ans", [])]
        for algo, extra in runs:
            size, ratio, comp, decomp = _run(emu_bench_dir, algo, data / name, *extra)
            # (the throughputs are those of the host EMULATION, printed with four decimals: a workgroup-per-chunk decode
            # of 512 - 1 024 coroutines can round to 0.0000 GB/s -- the fields must parse, not impress)
            assert size == os.path.getsize(data / name)
            assert ratio > 0.5 and comp >= 0 and decomp >= 0, (name, algo, extra, ratio, comp, decomp)
