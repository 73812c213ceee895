"""Helpers of tests/test_scale_parity.py: batches of a small unique set replicated on the device, and a checker that
names what differs.

A batch is `replicas` copies of `U` unique chunks. Every replica lies in one slab at `r * slots.stride`; inside a replica
chunk `i` owns the slot [slots.off[i], slots.off[i] + slots.cap[i]), followed by `slots.guard` bytes of GUARD_BYTE that
nothing may touch. The expected content of one replica is a host image (`Expect`): the bytes every chunk must hold, a
mask of the bytes that are determined (a compressor may leave the rest of its slot as it likes) and the sizes the call
must report. The check_* functions take torch tensors on ANY device, so the CPU tier plants faults in a synthetic batch
and asserts that they are found and named (a checker that compares nothing looks like a pass otherwise).
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

GUARD = 64
GUARD_BYTE = 0xA5
# Every replica starts at a multiple of this many bytes from the slab's base (torch aligns the base to at least 256), so
# chunk i of every replica has the same address modulo 4 096: see test_scale_parity.py, "placement".
PLACEMENT = 4096


def pool_threads() -> int:
    """Threads of the host reference: the CPUs this process may use, 16 at most."""
    return min(16, len(os.sched_getaffinity(0)))


def pool_map(fn: Callable, items: Sequence) -> list:
    """fn over items on the host pool (the ctypes calls and zlib release the GIL)."""
    with ThreadPoolExecutor(max_workers=pool_threads()) as ex:
        return list(ex.map(fn, items))


class Mismatch(AssertionError):
    """A failed comparison: `kind` is "byte", "size", "status" or "guard"; `replica`, `chunk` and `offset` (the byte
    inside the chunk's slot, or inside its guard) say where the first one is."""

    def __init__(self, what: str, kind: str, replica: int, chunk: int, offset: Optional[int], detail: str) -> None:
        self.kind, self.replica, self.chunk, self.offset = kind, replica, chunk, offset
        at = "" if offset is None else f", byte offset {offset}"
        super().__init__(f"{what}: first wrong {kind}: replica {replica}, chunk {chunk}{at}: {detail}")


@dataclass
class Slots:
    """Where the U chunks of ONE replica lie."""

    off: np.ndarray   # int64: slot starts inside a replica
    cap: np.ndarray   # int64: slot capacities (what the API is told)
    guard: int        # bytes of GUARD_BYTE behind every slot (0: none)
    stride: int       # bytes from one replica to the next, a multiple of PLACEMENT

    @property
    def count(self) -> int:
        return len(self.off)

    def pointers(self, base: int, replicas: int) -> np.ndarray:
        """uint64 addresses of all replicas * U slots, replica-major."""
        rep = np.arange(replicas, dtype=np.uint64)[:, None] * np.uint64(self.stride)
        return (self.off.astype(np.uint64)[None, :] + rep + np.uint64(base)).reshape(-1)

    def image(self, chunks: Optional[Sequence[np.ndarray]] = None) -> np.ndarray:
        """One replica on the host: zeros, the guards, and `chunks` (if given) at the starts of their slots."""
        img = np.zeros(self.stride, dtype=np.uint8)
        if self.guard:
            idx = (self.off + self.cap)[:, None] + np.arange(self.guard, dtype=np.int64)[None, :]
            img[idx.reshape(-1)] = GUARD_BYTE
        if chunks is not None:
            assert len(chunks) == self.count
            for o, cap, c in zip(self.off, self.cap, chunks):
                assert c.size <= cap
                img[o: o + c.size] = c
        return img


def pack_slots(caps: Sequence[int], align: int = 1, guard: int = 0) -> Slots:
    """Slots one behind the other, each start rounded up to `align`, each followed by `guard` bytes."""
    caps = np.asarray(caps, dtype=np.int64)
    span = caps + guard
    if align > 1:
        span = (span + align - 1) // align * align
    off = np.zeros(len(caps), dtype=np.int64)
    off[1:] = np.cumsum(span)[:-1]
    total = int(span.sum())
    return Slots(off, caps, guard, max(PLACEMENT, (total + PLACEMENT - 1) // PLACEMENT * PLACEMENT))


@dataclass
class Expect:
    """What one replica of an output slab must hold after a call."""

    image: np.ndarray   # uint8[stride]: expected bytes at the starts of the slots
    mask: np.ndarray    # uint8[stride]: 0xFF where `image` is binding, 0 elsewhere
    sizes: np.ndarray   # int64[U]: the sizes the call must report


def expect(slots: Slots, outputs: Sequence[np.ndarray]) -> Expect:
    image = np.zeros(slots.stride, dtype=np.uint8)
    mask = np.zeros(slots.stride, dtype=np.uint8)
    assert len(outputs) == slots.count
    for o, cap, c in zip(slots.off, slots.cap, outputs):
        assert c.size <= cap, "an expected output does not fit its slot"
        image[o: o + c.size] = c
        mask[o: o + c.size] = 0xFF
    return Expect(image, mask, np.array([c.size for c in outputs], dtype=np.int64))


def _first(flags) -> int:
    """Index of the first true element of a 1-D bool tensor that has one."""
    import torch

    return int(torch.nonzero(flags.reshape(-1))[0, 0])


def check_sizes(actual, expected, replicas: int, what: str) -> None:
    """actual: int64 tensor of replicas * U reported sizes, replica-major; expected: int64 tensor of U."""
    import torch

    n_u = expected.numel()
    assert actual.numel() == replicas * n_u and n_u > 0 and replicas > 0, f"{what}: the checker was given nothing to compare"
    got = actual.reshape(replicas, n_u)
    if torch.equal(got, expected[None, :].expand(replicas, n_u)):
        return
    at = _first(got != expected[None, :])
    r, c = divmod(at, n_u)
    raise Mismatch(what, "size", r, c, None, f"reported {int(got[r, c])}, expected {int(expected[c])}")


def check_statuses(statuses, replicas: int, n_u: int, what: str) -> None:
    """statuses: int32 tensor of replicas * U; every one must be 0 (nvcompSuccess)."""
    assert statuses.numel() == replicas * n_u and n_u > 0 and replicas > 0, f"{what}: the checker was given nothing to compare"
    if bool((statuses == 0).all()):
        return
    bad = statuses != 0
    r, c = divmod(_first(bad), n_u)
    raise Mismatch(what, "status", r, c, None, f"status {int(statuses[r * n_u + c])} ({int(bad.sum())} of {statuses.numel()} chunks failed)")


def check_bytes(slab, image, mask, slots: Slots, replicas: int, what: str) -> None:
    """Every replica of `slab` (uint8, replicas * slots.stride) against one expected replica `image` where `mask` is set;
    `image` and `mask` are uint8 tensors of slots.stride on the slab's device."""
    import torch

    stride = slots.stride
    assert slab.numel() >= replicas * stride and image.numel() == stride and mask.numel() == stride
    assert replicas > 0 and bool(mask.any()), f"{what}: the checker was given nothing to compare"
    for r in range(replicas):
        diff = torch.bitwise_and(torch.bitwise_xor(slab[r * stride: (r + 1) * stride], image), mask)
        if not bool(diff.any()):
            continue
        pos = _first(diff != 0)
        c = int(np.searchsorted(slots.off, pos, side="right")) - 1
        raise Mismatch(what, "byte", r, c, pos - int(slots.off[c]),
                       f"holds 0x{int(slab[r * stride + pos]):02x}, expected 0x{int(image[pos]):02x}")


def check_guards(slab, slots: Slots, replicas: int, what: str) -> None:
    """All guards of all replicas in ONE gather and comparison."""
    import torch

    assert slots.guard > 0 and replicas > 0, f"{what}: the checker was given nothing to compare"
    starts = (slots.off + slots.cap)[None, :] + np.arange(replicas, dtype=np.int64)[:, None] * slots.stride
    starts = torch.from_numpy(starts.reshape(-1)).to(slab.device)
    idx = starts[:, None] + torch.arange(slots.guard, dtype=torch.int64, device=slab.device)[None, :]
    got = slab[idx.reshape(-1)]
    if bool((got == GUARD_BYTE).all()):
        return
    at = _first(got != GUARD_BYTE)
    slot, k = divmod(at, slots.guard)
    r, c = divmod(slot, slots.count)
    raise Mismatch(what, "guard", r, c, k, f"guard byte {k} behind the slot (capacity {int(slots.cap[c])}) holds 0x{int(got[at]):02x}")


def ragged_sizes(count: int, top: int, elem: int, seed: int) -> np.ndarray:
    """`count` chunk sizes drawn from 1 .. top bytes in whole elements of `elem` bytes, one in 64 of them empty, and the
    largest and the smallest present."""
    rng = np.random.RandomState(seed)
    sizes = rng.randint(1, top // elem + 1, size=count).astype(np.int64) * elem
    sizes[rng.randint(0, count, size=max(1, count // 64))] = 0
    sizes[1], sizes[2] = top, elem
    return sizes


def cut(data: np.ndarray, sizes: Sequence[int], elem: int = 1) -> List[np.ndarray]:
    """Consecutive pieces of `data` of the given sizes; a piece starts at a multiple of `elem`."""
    out, pos = [], 0
    for s in sizes:
        s = int(s)
        assert pos + s <= data.size, "not enough data for the ragged batch"
        out.append(data[pos: pos + s])
        pos += (s + elem - 1) // elem * elem
    return out
