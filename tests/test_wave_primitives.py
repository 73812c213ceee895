"""The wave64 primitives every kernel is built from (common/wave.h), on known inputs.

test_wave_primitives is the library's exported self-test kernel. The tests below it run the kernels of
tests/wave/wave_ops_kernels.hip, one per family of primitives, and compare every output lane with the lane model of
tests/wave_model.py. The kernels are built four times: on the card and on the host emulation (`backend`), each against
the library's header (common/wave.h) and against the device API's copies (nvcomp/device/detail/wave*.hpp) (`ops`). The
model sees every case before it is launched and refuses inputs outside a primitive's contract, so nothing that would
not terminate reaches either.

Coverage: every function defined in common/wave.h and in the four device-detail headers is called by those kernels
(test_every_primitive_is_accounted_for enumerates the headers); NOT_EXERCISED would name the exceptions, and has none.
touch, sched_fence, nap, nap_short, sync and sync_wave have no value of their own: they are called in kernels whose
results must still be right.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wave_model as model


def test_wave_primitives(backend):
    d = backend.dev
    rng = np.random.RandomState(1)
    v = rng.randint(0, 1 << 20, size=64).astype(np.uint32)
    din = d.upload(v.view(np.uint8))
    dout = d.upload(np.zeros(640, dtype=np.uint32).view(np.uint8))
    scratch = d.upload(np.zeros(4096, dtype=np.uint8))
    fn = backend.lib.nvcompAmdSelfTestWave
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    assert fn(d.ptr(din), d.ptr(dout), d.ptr(scratch), d.stream()) == 0
    d.synchronize()
    out = d.download(dout).view(np.uint32).reshape(10, 64)
    lanes = np.arange(64)
    assert np.array_equal(out[0], np.cumsum(v.astype(np.uint64)).astype(np.uint32))
    assert (out[1] == v.max()).all()
    assert (out[2] == np.uint32(v.astype(np.uint64).sum() & 0xFFFFFFFF)).all()
    assert np.array_equal(out[3], v[(lanes * 7 + 3) & 63])
    assert (out[4] == v[37]).all()
    ballot = sum(1 << i for i in range(64) if v[i] & 1)
    assert (out[5] == (ballot & 0xFFFFFFFF)).all() and (out[6] == (ballot >> 32)).all()
    exp = v.copy()
    exp[11] = 0xABCD
    assert np.array_equal(out[7], exp)
    assert np.array_equal(out[8], ((v + 1) & 0xFF)[::-1])
    assert (out[9] == 0).all()


# ---- the four builds of tests/wave/wave_ops_kernels.hip --------------------------------------------------------------

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join("tests", "wave", "wave_ops_kernels.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LIBRARY_HEADER = os.path.join(REPO, "nvcomp_amd", "csrc", "common", "wave.h")
DEVICE_HEADERS = [os.path.join(REPO, "include", "nvcomp", "device", "detail", n)
                  for n in ("wave.hpp", "wave_ext.hpp", "wave_lz.hpp", "wave_lzc.hpp")]
NOT_EXERCISED = {}  # name -> why no kernel calls it

IN_WORDS, OUT_ROWS = 4 * 64 + 8, 8
LANES = np.arange(64, dtype=np.uint32)
M32 = 0xFFFFFFFF
_libs = {}


def build_command(tier, variant, so):
    macro = ["-DWAVE_OPS_DEVICE_HEADERS"] if variant == "device" else []
    if tier == "emu":
        return ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", "-Invcomp_amd/csrc",
                *macro, SRC, "-o", so, "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
    # -Wno-inline-asm: common/wave.h names M0 as clobbered on purpose (see write_lane_scalar there)
    return [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Werror", "-shared", "-fPIC",
            "-Invcomp_amd/csrc", "-Iinclude", *macro, SRC, "-o", so]


def built(tier, variant, tmp_path_factory):
    """Path of the test kernels built for a tier ("emu" / "gpu") and a header variant (once per session)."""
    if (tier, variant) not in _libs:
        so = str(tmp_path_factory.mktemp(f"waveops_{tier}_{variant}") / "waveops.so")
        if tier == "emu":
            import conftest

            conftest.emu_library()
        r = subprocess.run(build_command(tier, variant, so), cwd=REPO, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _libs[tier, variant] = so
    return _libs[tier, variant]


class Ops:
    def __init__(self, backend, variant, so):
        self.backend, self.dev, self.variant, self.lib = backend, backend.dev, variant, C.CDLL(so)
        self.library = variant == "library"

    def run(self, family, cases, extra=()):
        """Launch one family on `cases` (dicts with lane operands a..d and a list u of uniform words): [case, row, lane]."""
        table = np.zeros((len(cases), IN_WORDS), dtype=np.uint32)
        for i, c in enumerate(cases):
            for j, key in enumerate("abcd"):
                if key in c:
                    table[i, 64 * j: 64 * j + 64] = np.asarray(c[key], dtype=np.uint64).astype(np.uint32)
            u = [int(x) & M32 for x in c.get("u", [])]
            table[i, 256: 256 + len(u)] = u
        din = self.dev.upload(table.view(np.uint8))
        dout = self.dev.upload(np.full(len(cases) * OUT_ROWS * 64, 0xEEEEEEEE, dtype=np.uint32).view(np.uint8))
        fn = getattr(self.lib, "waveops_" + family)
        fn.argtypes = [C.c_void_p] * (2 + len(extra)) + [C.c_uint, C.c_void_p]
        fn.restype = C.c_int
        assert fn(self.dev.ptr(din), self.dev.ptr(dout), *[self.dev.ptr(e) for e in extra], len(cases), self.dev.stream()) == 0
        self.dev.synchronize()
        return self.dev.download(dout).view(np.uint32).reshape(len(cases), OUT_ROWS, 64)


@pytest.fixture(params=["library", "device"])
def ops(request, backend, tmp_path_factory):
    """The test kernels against common/wave.h ("library") or against nvcomp/device/detail/wave*.hpp ("device")."""
    return Ops(backend, request.param, built(backend.name, request.param, tmp_path_factory))


@pytest.fixture
def lib_ops(backend, tmp_path_factory):
    return Ops(backend, "library", built(backend.name, "library", tmp_path_factory))


def expect(primitive, case, got, want):
    """Every lane of `got` equals the model's `want` (a lane vector, or one value for all lanes)."""
    got = np.asarray(got, dtype=np.uint32).reshape(-1)
    want = np.broadcast_to(np.asarray(want, dtype=np.uint64).astype(np.uint32), got.shape)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        lane = int(bad[0])
        raise AssertionError(f"{primitive}: case '{case}', lane {lane}: got 0x{int(got[lane]):08x}, the model says "
                             f"0x{int(want[lane]):08x} ({bad.size} of 64 lanes differ)")


def lane_vectors():
    rng = np.random.RandomState(7)
    out = {"zero": np.zeros(64, np.uint32), "all_ones": np.full(64, M32, np.uint32), "index": LANES.copy(),
           "descending": (63 - LANES).astype(np.uint32)}
    for p in (0, 15, 16, 31, 32, 47, 48, 63):
        v = np.zeros(64, np.uint32)
        v[p] = 0x80000001 + p
        out[f"one_at_{p}"] = v
    for b in (16, 32, 48):
        out[f"step_up_at_{b}"] = np.where(LANES >= b, 1000, 1).astype(np.uint32)
        out[f"step_down_at_{b}"] = np.where(LANES >= b, 1, 0x7FFFFFFF).astype(np.uint32)
    out["random32"] = rng.randint(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
    out["random_small"] = rng.randint(0, 16, size=64).astype(np.uint32)
    return out


def masks(with_zero=True):
    rng = np.random.RandomState(11)
    out = {"zero": 0} if with_zero else {}
    out.update({"all": (1 << 64) - 1, "bit0": 1, "bit31": 1 << 31, "bit32": 1 << 32, "bit63": 1 << 63,
                "low_half": M32, "high_half": M32 << 32, "even_bits": 0x5555555555555555, "odd_bits": 0xAAAAAAAAAAAAAAAA})
    for i in range(4):
        out[f"random{i}"] = int(rng.randint(0, 1 << 32, dtype=np.uint64)) | (int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 32)
    return out


def index_patterns():
    return {"identity": LANES.copy(), "reversal": (63 - LANES).astype(np.uint32), "7l+3": ((7 * LANES + 3) & 63).astype(np.uint32),
            "all_lane0": np.zeros(64, np.uint32), "all_lane63": np.full(64, 63, np.uint32)}


def last_writer_cases():
    rng = np.random.RandomState(13)
    rnd = lambda: rng.randint(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
    out = {"disjoint_bytes": (rnd(), (np.uint32(0xFF) << (8 * (LANES % 4))).astype(np.uint32)),
           "overlapping": (rnd(), rnd() & rnd()), "dense_overlap": (rnd(), rnd() | rnd()),
           "no_writer": (rnd(), np.zeros(64, np.uint32)),
           "bits_outside_mask": (np.full(64, M32, np.uint32), rnd() & rnd() & rnd())}
    for name, writers in (("lone_lane0", {0: M32}), ("lone_lane63", {63: M32}), ("writers_15_16", {15: 0x00FFFF00, 16: 0x0000FFFF}),
                          ("writers_31_32", {31: 0xFFFF0000, 32: 0x00FFFF00}), ("writers_47_48", {47: 0x0F0F0F0F, 48: 0x00FF00FF}),
                          ("one_per_row", {3: 0xFF, 19: 0xFF00, 35: 0xFF0000, 51: 0xFF000000})):
        m = np.zeros(64, np.uint32)
        for lane, bits in writers.items():
            m[lane] = bits
        out[name] = (rnd(), m)
    return out


# ---- scans, reductions, moves ---------------------------------------------------------------------------------------

def test_scans_and_reductions(ops):
    rng = np.random.RandomState(3)
    names, cases = [], []
    for name, v in lane_vectors().items():
        names.append(name)
        cases.append({"a": v, "b": rng.permutation(v)})
    for name, (val, mask) in last_writer_cases().items():
        names.append("last_writer/" + name)
        cases.append({"a": val, "b": mask, "c": val, "d": mask})
    zero = np.zeros(64, np.uint32)
    expected = [(model.scan_add_inclusive(c["a"]), model.reduce_add(c["a"]), model.reduce_max(c["a"]), model.umax(c["a"], c["b"]),
                 model.scan_max_inclusive(c["a"]), *model.scan_last_writer(c.get("c", zero), c.get("d", zero))) for c in cases]
    out = ops.run("scan", cases)
    for name, e, o in zip(names, expected, out):
        expect("scan_add_inclusive", name, o[0], e[0])
        expect("reduce_add", name, o[1], e[1])  # one value: identical in all 64 lanes
        expect("reduce_max", name, o[2], e[2])
        expect("umax", name, o[3], e[3])
        if ops.library:
            expect("scan_max_inclusive", name, o[4], e[4])
            expect("scan_last_writer (value)", name, o[5], e[5])
            expect("scan_last_writer (mask)", name, o[6], e[6])


def test_moves(ops):
    vectors, patterns = lane_vectors(), index_patterns()
    names, cases = [], []
    for name, v in vectors.items():
        names.append(name)
        cases.append({"a": v, "b": patterns["7l+3"], "c": patterns["reversal"]})
    for name, idx in patterns.items():
        names.append("index/" + name)
        is_permutation = sorted(idx.tolist()) == list(range(64))
        cases.append({"a": vectors["random32"], "b": idx, "c": idx if is_permutation else patterns["identity"]})
    with pytest.raises(model.ContractError):
        model.permute_to(vectors["random32"], patterns["all_lane0"])
    expected = [(model.shuffle(c["a"], c["b"]), model.prev_lane(c["a"]), model.next_lane(c["a"]), model.permute_to(c["a"], c["c"]))
                for c in cases]
    out = ops.run("move", cases)
    for name, e, o in zip(names, expected, out):
        expect("shuffle", name, o[0], e[0])
        expect("prev_lane", name, o[1], e[1])
        if ops.library:
            expect("next_lane", name, o[2], e[2])
            expect("permute_to", name, o[3], e[3])


def test_lane_reads_and_writes(ops):
    rng = np.random.RandomState(5)
    names, cases, expected = [], [], []
    for r in (0, 31, 32, 63):
        for w1, w2 in ((0, 63), (31, 32), (32, 31), (63, 0)):
            v = rng.randint(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
            x, y, u32, lo, hi = (int(t) for t in rng.randint(1, 1 << 32, size=5, dtype=np.uint64))
            hi |= 0x80000000  # uniform64: a high word that is not zero
            names.append(f"read{r}_write{w1}_then{w2}")
            cases.append({"a": v, "b": np.full(64, u32), "c": np.full(64, lo), "d": np.full(64, hi), "u": [r, x, w1, y, w2, 0x1234567]})
            q = model.uniform64(cases[-1]["c"], cases[-1]["d"])
            expected.append((model.read_lane(v, r), model.write_lane(v, x, w1), model.uniform(cases[-1]["b"]),
                             model.write_lane_scalar(model.write_lane_scalar(v, x, w1), y, w2), q & M32, q >> 32,
                             (v.astype(np.uint64) + 0x1234567) & M32))
    for bad in (64, 1 << 31):
        with pytest.raises(model.ContractError):
            model.read_lane(cases[0]["a"], bad)
        with pytest.raises(model.ContractError):
            model.write_lane(cases[0]["a"], 1, bad)
    with pytest.raises(model.ContractError):
        model.uniform(LANES)
    out = ops.run("lane", cases)
    for name, e, o in zip(names, expected, out):
        expect("read_lane", name, o[0], e[0])
        expect("write_lane", name, o[1], e[1])
        expect("uniform", name, o[2], e[2])
        if ops.library:
            expect("write_lane_scalar (twice)", name, o[3], e[3])
            expect("uniform64 (low word)", name, o[4], e[4])
            expect("uniform64 (high word)", name, o[5], e[5])
            expect("uniform_ptr (load through it)", name, o[6], e[6])


def test_masks(ops):
    names, cases = [], []
    for name, m in masks().items():
        names.append(name)
        cases.append({"a": model.lane_in(m) * (LANES + np.uint32(0x100)), "u": [m & M32, m >> 32], "mask": m})
    with pytest.raises(model.ContractError):
        model.ctz64(0)
    expected = []
    for c in cases:
        m = c["mask"]
        b = model.ballot(c["a"] != 0)
        assert b == m
        # ctz64: the kernel does not call it on an empty mask and writes ~0 instead
        expected.append((b & M32, b >> 32, model.prefix_popc(m), model.popc64(m), model.ctz64(m) if m else M32, model.lane_in(m)))
    out = ops.run("mask", cases)
    for name, e, o in zip(names, expected, out):
        expect("ballot (low word)", name, o[0], e[0])
        expect("ballot (high word)", name, o[1], e[1])
        expect("prefix_popc", name, o[2], e[2])
        expect("popc64", name, o[3], e[3])
        expect("ctz64", name, o[4], e[4])
        if ops.library:
            expect("lane_in", name, o[5], e[5])


def test_two_waves(ops):
    """lane_id / fresh_lane_id in both waves of a workgroup, sync(), and (library) the flag pairs handing data from wave 0
    to wave 1. A consumer that never saw its flag wrote 0xdead0000."""
    rng = np.random.RandomState(17)
    cases = [{k: rng.randint(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32) for k in "abc"} for _ in range(4)]
    out = ops.run("two_waves", cases)
    for i, (c, o) in enumerate(zip(cases, out)):
        expect("lane_id (wave 0)", i, o[0], model.lane_id())
        expect("fresh_lane_id (wave 0)", i, o[1], model.fresh_lane_id())
        expect("lane_id (wave 1)", i, o[2], model.lane_id())
        expect("fresh_lane_id (wave 1)", i, o[3], model.fresh_lane_id())
        expect("sync (store, then a cross-lane load)", i, o[4], c["c"][::-1])
        if ops.library:
            expect("lds_store_release / lds_load_acquire / nap", i, o[5], c["a"][::-1])
            expect("lds_store_relaxed / lds_load_relaxed / nap_short", i, o[6], c["b"][::-1])


# ---- per-lane arithmetic --------------------------------------------------------------------------------------------

def rand32(rng, n=64):
    return rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def cycle(values):
    return np.resize(np.asarray(values, dtype=np.uint64), 64).astype(np.uint32)


def arith_cases():
    """(primitive, case name, kernel operation, model function, operands)"""
    rng = np.random.RandomState(19)
    top = (1 << 24) - 1
    out = []
    a = rng.randint(0, 1 << 24, size=64).astype(np.uint32)
    b = rng.randint(0, 1 << 24, size=64).astype(np.uint32)
    out.append(("mul24", "random", 0, model.mul24, (a, b)))
    a, b = a.copy(), b.copy()
    a[:8] = [0, 0, 1, 1, top, top, top, 0]
    b[:8] = [0, 12345, 1, top, top, 1, 2, top]
    out.append(("mul24", "edges", 0, model.mul24, (a, b)))
    for name, hi, lo in (("random", rand32(rng), rand32(rng)), ("hi_only", rand32(rng), np.zeros(64, np.uint32)),
                         ("all_ones", np.full(64, M32, np.uint32), np.full(64, M32, np.uint32))):
        for half in (0, 1):
            out.append(("align_bits", f"{name}/shifts_{32 * half}", 1, model.align_bits, (hi, lo, (LANES + 64 * half) % 32)))
    shifts = cycle(list(range(8)) + [28, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF])
    out.append(("align_bytes", "random", 2, model.align_bytes, (rand32(rng), rand32(rng), shifts)))
    out.append(("align_bytes", "zero_above", 2, model.align_bytes, (np.zeros(64, np.uint32), rand32(rng), shifts)))  # lz_copy's use
    out.append(("align_bytes", "minus_end", 2, model.align_bytes, (np.zeros(64, np.uint32), rand32(rng), (0 - LANES).astype(np.uint32))))
    halves = [0, 1, 254, 255, 256, 0xFFFF]
    words = [x | (y << 16) for x in halves for y in halves]
    pairs = [(p, q) for p in words for q in words]
    for i in range(0, len(pairs), 64):
        chunk = (pairs[i: i + 64] + pairs[:64])[:64]
        out.append(("pk_add_sat255", f"pairs_{i}", 3, model.pk_add_sat255, (cycle([p for p, _ in chunk]), cycle([q for _, q in chunk]))))
    v = rand32(rng)
    v[:3] = [0, 1, 0x80000000]
    out.append(("bit_reverse", "edges_and_random", 4, model.bit_reverse, (v,)))
    sel = cycle([0x06040200, 0x03020100, 0x07060504, 0x0C0C0C0C, 0x0D0E0FFF, 0x0C070D00, 0x80FF0C04, 0x00000000])
    out.append(("perm_bytes", "listed_selectors", 5, model.perm_bytes, (rand32(rng), rand32(rng), sel)))
    domain = np.array(list(range(8)) + list(range(12, 256)), dtype=np.uint32)
    for i in range(3):
        s = domain[rng.randint(0, domain.size, size=(64, 4))]
        sel = s[:, 0] | (s[:, 1] << 8) | (s[:, 2] << 16) | (s[:, 3] << 24)
        out.append(("perm_bytes", f"random_selectors_{i}", 5, model.perm_bytes, (rand32(rng), rand32(rng), sel)))
    return out


def test_arithmetic(ops):
    zero = np.zeros(64, np.uint32)
    for bad in (lambda: model.mul24(np.full(64, 1 << 24), zero), lambda: model.align_bits(zero, zero, np.full(64, 32)),
                lambda: model.perm_bytes(zero, zero, np.full(64, 0x00000800)), lambda: model.perm_bytes(zero, zero, np.full(64, 0x0B000000))):
        with pytest.raises(model.ContractError):
            bad()
    table = [t for t in arith_cases() if ops.library or t[0] == "mul24"]
    expected = [fn(*operands) for _, _, _, fn, operands in table]
    cases = [dict(zip("abc", operands), u=[op]) for _, _, op, _, operands in table]
    out = ops.run("arith", cases)
    for (primitive, name, _, _, _), e, o in zip(table, expected, out):
        expect(primitive, name, o[0], e)


# ---- the serial walks -----------------------------------------------------------------------------------------------

def chain_walk_cases():
    rng = np.random.RandomState(23)
    ones = np.ones(64, np.uint32)
    far = ones.copy()
    far[60] = 200
    out = {"64_iterations": (ones, 64, 0, 0), "single_at_r63": (rand32(rng) >> 1 | 1, 64, 63, 5),
           "k63_one_iteration": (np.full(64, 64), 64, 10, 63), "limit_1": (ones * 7, 1, 0, 0), "overshoot_200": (far, 64, 57, 3),
           "huge_step": (np.full(64, 0x7FFFFFFF), 64, 0, 0)}
    for i in range(8):
        step = rng.randint(1, 9, size=64).astype(np.uint32)
        limit = int(rng.randint(1, 65))
        r = int(rng.randint(0, limit))
        _, iterations, _ = model.chain_walk(step, limit, r, 0, np.zeros(64))
        out[f"random{i}"] = (step, limit, r, int(rng.randint(0, 64 - iterations + 1)))
    return out


def test_chain_walk(lib_ops):
    rng = np.random.RandomState(29)
    zero, ones = np.zeros(64, np.uint32), np.ones(64, np.uint32)
    for bad in ((zero, 64, 0, 0), (ones, 64, 0, 1), (ones, 65, 0, 0), (ones, 10, 10, 0), (ones, 64, 63, 64)):
        with pytest.raises(model.ContractError):  # a zero step, k + iterations > 64, limit > 64, r >= limit, k >= 64
            model.chain_walk(*bad, zero)
    names, cases, expected = [], [], []
    for name, (step, limit, r, k) in chain_walk_cases().items():
        rec = rand32(rng)
        names.append(name)
        expected.append(model.chain_walk(step, limit, r, k, rec))  # raises on anything that would not end
        cases.append({"a": step, "b": rec, "u": [limit, r, k]})
    out = lib_ops.run("chain_walk", cases)
    for name, (r, k, rec), o in zip(names, expected, out):
        expect("chain_walk (rec)", name, o[0], rec)
        expect("chain_walk (r)", name, o[1], r)
        expect("chain_walk (k)", name, o[2], k)


def select_walk_cases():
    rng = np.random.RandomState(31)
    ones = np.ones(64, np.uint32)
    skip = np.full(64, 2, np.uint32)
    skip[3] = 10
    long0 = ones.copy()
    long0[0] = 63
    far = ones.copy()
    far[63] = 63
    out = {"only_lane63_start63": (1 << 63, ones * 5, 63), "only_lane63_start0": (1 << 63, far, 0), "high_half": (M32 << 32, ones * 3, 0),
           "low_half": (M32, ones * 4, 0), "64_takes": ((1 << 64) - 1, ones, 0), "length63_at_lane0": ((1 << 64) - 1, long0, 0),
           "skipped_inside_match": ((1 << 3) | (1 << 5) | (1 << 20), skip, 0), "end_above_64": ((1 << 40) | (1 << 50), ones * 63, 7),
           "start_on_candidate": (0b1010 << 30, ones * 2, 31)}
    for name, m in masks(with_zero=False).items():
        out["mask/" + name] = (m, rng.randint(1, 6, size=64).astype(np.uint32), 0)
    for i in range(8):
        m = int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 32 | int(rng.randint(0, 1 << 32, dtype=np.uint64))
        m &= int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 32 | int(rng.randint(0, 1 << 32, dtype=np.uint64)) if i % 2 else M32 << 32 | M32
        m |= 1 << int(rng.randint(0, 64))
        length = rng.randint(1, 64 if i < 4 else 8, size=64).astype(np.uint32)
        out[f"random{i}"] = (m, length, int(rng.randint(0, m.bit_length())))
    return out


def test_select_walk(lib_ops):
    zero, ones = np.zeros(64, np.uint32), np.ones(64, np.uint32)
    for bad in ((1, zero, 0), (1, ones * 64, 0), (0, ones, 0), (1, ones, 1), (1 << 63, ones, 64)):
        with pytest.raises(model.ContractError):  # a zero length, a length of 64, no candidate, none at or above start, start 64
            model.select_walk(*bad)
    table = select_walk_cases()
    expected = {name: model.select_walk(*t) for name, t in table.items()}  # raises on anything that would not end
    assert bin(expected["64_takes"][0]).count("1") == 64 and expected["end_above_64"][1] > 64
    assert expected["skipped_inside_match"][0] == (1 << 3) | (1 << 20)
    cases = [{"a": length, "u": [m & M32, m >> 32, start]} for m, length, start in table.values()]
    out = lib_ops.run("select_walk", cases)
    for (name, (taken, end)), o in zip(expected.items(), out):
        expect("select_walk (taken, low word)", name, o[0], taken & M32)
        expect("select_walk (taken, high word)", name, o[1], taken >> 32)
        expect("select_walk (end)", name, o[2], end)


# ---- LDS read-modify-write, kernel arguments ------------------------------------------------------------------------

def test_lds_atomics(lib_ops):
    rng = np.random.RandomState(37)
    targets = {"one_word": np.full(64, 5, np.uint32), "two_words": np.where(LANES & 1, 9, 40).astype(np.uint32),
               "word_per_lane": rng.permutation(64).astype(np.uint32)}
    table = []
    for name, index in targets.items():
        table.append(("lds_or", name, 0, model.lds_or, index, (np.uint32(1) << (LANES % 32)).astype(np.uint32) | (rand32(rng) & rand32(rng))))
        table.append(("lds_add", name, 1, model.lds_add, index, rand32(rng)))
        table.append(("lds_sub", name, 2, model.lds_sub, index, rand32(rng)))
    words = [rand32(rng) & rand32(rng) for _ in table]
    expected = [fn(w, index, v) for (_, _, _, fn, index, v), w in zip(table, words)]
    cases = [{"a": index, "b": v, "c": w, "u": [op]} for (_, _, op, _, index, v), w in zip(table, words)]
    out = lib_ops.run("lds_atomic", cases)
    for (primitive, name, *_), e, o in zip(table, expected, out):
        expect(primitive, name, o[0], e)


def test_kernel_args(lib_ops):
    d = lib_ops.dev
    fn = lib_ops.lib.waveops_kernel_args
    fn.argtypes = [C.c_uint, C.c_uint, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    for f8, f16, f32, f64 in ((0xA7, 0xBEEF, 0x89ABCDEF, 0xFEDCBA9876543210), (1, 2, 3, 4 << 32)):
        dout = d.upload(np.full(5 * 64, 0xEEEEEEEE, dtype=np.uint32).view(np.uint8))
        assert fn(f8, f16, f32, f64, d.ptr(dout), d.stream()) == 0
        d.synchronize()
        o = d.download(dout).view(np.uint32).reshape(5, 64)
        for field, row, want in (("8-bit", 0, f8), ("16-bit", 1, f16), ("32-bit", 2, f32), ("64-bit, low word", 3, f64 & M32),
                                 ("64-bit, high word", 4, f64 >> 32)):
            expect(f"kernel_args ({field} field)", hex(f64), o[row], want)


# ---- memory accessors -----------------------------------------------------------------------------------------------

LOADS = {"gload_u8": (0, 1), "gload_u16": (1, 2), "gload_u32": (2, 4), "gload_u64": (3, 8), "gload_u32x3": (4, 12), "gload_u32x4": (5, 16)}
STORES = {"gstore_u8": (7, 1), "gstore_u32": (8, 4), "gstore_u32x4": (9, 16)}
ALIGNED = {"gload_u32x4_aligned": (6, 16), "gstore_u32x4_aligned": (10, 16), "gstore_u32x4_aligned_nt": (11, 16)}
SLOT, GUARD = 64, 16


def test_accessors(lib_ops):
    """Every accessor at byte offsets 0..15 (the aligned and non-temporal forms at 0): loads against known bytes, stores
    against the slot they may write, 16 guard bytes on each side included."""
    rng = np.random.RandomState(41)
    d = lib_ops.dev
    src = rng.randint(0, 256, size=16 * 64 + 32).astype(np.uint8)
    table = [(name, op, size, off) for name, (op, size) in {**LOADS, **STORES}.items() for off in range(16)]
    table += [(name, op, size, 0) for name, (op, size) in ALIGNED.items()]
    cases = [{"a": rand32(rng), "b": rand32(rng), "c": rand32(rng), "d": rand32(rng), "u": [op, off]} for _, op, _, off in table]
    dsrc = d.upload(src)
    ddst = d.upload(np.full(len(table) * 64 * SLOT, 0xA5, dtype=np.uint8))
    out = lib_ops.run("access", cases, extra=(dsrc, ddst))
    dst = d.download(ddst).reshape(len(table), 64, SLOT)
    for (name, op, size, off), c, o, slots in zip(table, cases, out, dst):
        want = np.full((64, SLOT), 0xA5, dtype=np.uint8)
        if "gload" in name:
            data = np.stack([src[16 * lane + off: 16 * lane + off + size] for lane in range(64)])
            data = np.pad(data, ((0, 0), (0, -size % 4))).copy().view(np.uint32)
            for word in range(data.shape[1]):
                expect(f"{name} (word {word})", f"offset {off}", o[word], data[:, word])
        else:
            value = np.stack([c[k] for k in "abcd"], axis=1).copy().view(np.uint8)[:, :size]
            want[:, GUARD + off: GUARD + off + size] = value
        bad = np.argwhere(slots != want)
        assert bad.size == 0, (f"{name}: case 'offset {off}', lane {bad[0][0]}: byte {bad[0][1] - GUARD - off} relative to the "
                               f"address is 0x{slots[tuple(bad[0])]:02x}, the model says 0x{want[tuple(bad[0])]:02x}")


REGION = 2112
COPY_LENGTHS = (0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 1279, 1285)


def test_lz_copies(lib_ops):
    """lz::wave_copy at the lengths around its three loops, lz::ld_u32 / st_u32 and lz::copy16, source and destination
    misaligned by 0..3 each; the whole destination region is compared, so a byte outside the copy shows."""
    rng = np.random.RandomState(43)
    d = lib_ops.dev
    src = rng.randint(0, 256, size=2048).astype(np.uint8)
    table = [("lz::wave_copy", 0, n, s, t) for n in COPY_LENGTHS for s in range(4) for t in range(4)]
    table += [(name, op, 0, s, t) for name, op in (("lz::ld_u32 / lz::st_u32", 1), ("lz::copy16", 2)) for s in range(4) for t in range(4)]
    cases = [{"u": [op, n, s, t]} for _, op, n, s, t in table]
    dsrc = d.upload(src)
    ddst = d.upload(np.full(len(table) * REGION, 0xA5, dtype=np.uint8))
    lib_ops.run("lz_copy", cases, extra=(dsrc, ddst))
    dst = d.download(ddst).reshape(len(table), REGION)
    for (name, op, n, s, t), got in zip(table, dst):
        want = np.full(REGION, 0xA5, dtype=np.uint8)
        to = want[GUARD + t:]
        if op == 0:
            to[:n] = src[s: s + n]
        else:
            size, stride = (4, 8) if op == 1 else (16, 32)
            for lane in range(64):
                to[stride * lane: stride * lane + size] = src[s + size * lane: s + size * lane + size]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{name}: case 'length {n}, source + {s}, destination + {t}': byte {int(bad[0]) - GUARD - t} of the "
                               f"destination is 0x{got[bad[0]]:02x}, the model says 0x{want[bad[0]]:02x} ({bad.size} bytes differ)")


def test_is_lds(backend, tmp_path_factory):
    dev_ops = Ops(backend, "device", built(backend.name, "device", tmp_path_factory))
    out = dev_ops.run("is_lds", [{}, {}])
    for i, o in enumerate(out):
        expect("is_lds (a pointer into the block's dynamic LDS)", i, o[0], 1)
        expect("is_lds (a pointer to the input table)", i, o[1], 0)
        expect("is_lds (a pointer to the output table)", i, o[2], 0)


# ---- the builds and the coverage ------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["library", "device"])
def test_kernels_compile_for_gfx950(variant, tmp_path_factory):
    """The command line the card's tests use (-Werror included), on a machine with the compiler and without the card."""
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    assert os.path.getsize(built("gpu", variant, tmp_path_factory)) > 0


def defined_functions(path, marker):
    """Names of the functions a header defines with `marker` in front (__forceinline__ on the card, inline on the host)."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b" + marker + r"\s[^(;{}#]*?\b(\w+)\s*\(", text))


def compiled_text(device_headers):
    """The kernel source as one of the two header variants sees it (only this file's own two conditions are evaluated)."""
    known = {"#if WAVE_OPS_LIBRARY": not device_headers, "#if defined(WAVE_OPS_DEVICE_HEADERS)": device_headers}
    keep, stack = [], []  # stack: per open #if, [its value (None: not one of the two), whether the #else was passed]
    for line in open(os.path.join(REPO, SRC)).read().splitlines():
        s = line.strip()
        if s.startswith("#if"):
            stack.append([known.get(s), False])
        elif s.startswith("#else"):
            stack[-1][1] = True
        elif s.startswith("#endif"):
            stack.pop()
        elif all(value is None or value != passed_else for value, passed_else in stack):
            keep.append(line)
    assert not stack
    return "\n".join(keep)


def test_every_primitive_is_accounted_for():
    """Every function of common/wave.h and of the four device-detail headers is called by the test kernels in the build
    that sees it, or named in NOT_EXERCISED with the reason; and the emulation defines every one of them."""
    library = defined_functions(LIBRARY_HEADER, "__forceinline__")
    device = set().union(*(defined_functions(h, "__forceinline__") for h in DEVICE_HEADERS))
    assert {"select_walk", "chain_walk", "kernel_args", "uniform_ptr", "gstore_u32x4_aligned_nt", "prefix_popc"} <= library
    assert {"fresh_lane_id", "lane_id", "ballot", "read_lane", "uniform", "scan_add_inclusive", "reduce_max", "reduce_add", "popc64",
            "mul24", "prefix_popc", "shuffle", "prev_lane", "write_lane", "ctz64", "is_lds"} <= device
    for names, text, where in ((library, compiled_text(False), "common/wave.h"), (device, compiled_text(True), "nvcomp/device/detail")):
        called = set(re.findall(r"\bW::(\w+)\s*\(", text))
        missing = sorted(names - called - set(NOT_EXERCISED))
        assert not missing, f"{where} defines {missing}: no kernel of {SRC} calls them and NOT_EXERCISED does not list them"
    assert not set(NOT_EXERCISED) - library - device, "NOT_EXERCISED names functions that no header defines"
    emulated = defined_functions(os.path.join(REPO, "tests", "emu", "common", "wave.h"), "inline")
    assert not library - emulated, f"tests/emu/common/wave.h lacks {sorted(library - emulated)}"
    no_lane_value = {"kernel_args", "uniform_ptr", "touch", "sched_fence", "sync", "sync_wave", "nap", "nap_short"}
    for name in sorted(library - no_lane_value):  # what computes lane values: the model has every one of them
        if not name.startswith(("gload_", "gstore_", "lds_store_", "lds_load_")):
            assert hasattr(model, name), f"tests/wave_model.py has no {name}"
