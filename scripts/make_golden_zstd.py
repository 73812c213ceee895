#!/usr/bin/env python3
"""Golden Zstandard frames for tests/test_zstd.py: tests/golden/zstd_*.zst and tests/golden/zstd_manifest.json.

The originals come from the tree only -- nvcomp_amd/datasets.py with fixed seeds and the committed
tests/golden/ExampleTable.txt.gz / ExampleFloatData.csv.gz -- and are rebuilt by tests/test_zstd.py from the recipe the
manifest records (and checked against its SHA-256). The frames are written by CPU libzstd (nvcomp_amd/zstd_cpu.py):
levels -5 / 1 / 3 / 9 / 19, the checksum on, the content size off, streamed frames with flushes (many blocks: repeat
modes, treeless literals), concatenated, skippable and empty frames, a frame with a Dictionary_ID written into its
header by hand, two small frames written by hand (RLE literals; RLE sequence tables), and windowLog 20 / 24
chunks of 1 / 2 MiB whose repeats lie 160 / 256 KiB back. Every file stays under 100 KiB. Run once; the files are committed."""
import gzip
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def original(recipe) -> np.ndarray:
    """The bytes a recipe names (tests/test_zstd.py carries the same function)."""
    from nvcomp_amd import datasets

    kind = recipe["source"]
    if kind == "gz":
        raw = gzip.open(os.path.join(GOLDEN, recipe["file"])).read()
        return np.frombuffer(raw[recipe["offset"]: recipe["offset"] + recipe["size"]], dtype=np.uint8).copy()
    if kind == "dataset":
        return datasets.CLASSES[recipe["class"]](recipe["size"], recipe["seed"])
    if kind == "far":  # `period` bytes (noise head, zeros behind), repeated up to `size`
        unit = np.zeros(recipe["period"], dtype=np.uint8)
        unit[: recipe["noise"]] = datasets.noise(recipe["noise"], recipe["seed"])
        return np.resize(unit, recipe["size"])
    if kind == "concat":
        return np.concatenate([original(r) for r in recipe["parts"]] or [np.zeros(0, np.uint8)])
    if kind == "hex":
        return np.frombuffer(bytes.fromhex(recipe["hex"]), dtype=np.uint8).copy()
    raise ValueError(kind)


def handmade_rle_literals(size=100, byte=0x51):
    """One compressed block: RLE literals (2-byte header), no sequences. libzstd's encoder writes RLE literals only
    where a block's literals are all one byte, which its match finder leaves no room for."""
    body = bytes([1 | 1 << 2 | (size & 15) << 4, size >> 4, byte, 0])
    frame = (0xFD2FB528).to_bytes(4, "little") + bytes([0x20, size])
    frame += (1 | 2 << 1 | len(body) << 3).to_bytes(3, "little") + body
    return np.frombuffer(frame, dtype=np.uint8), bytes([byte]) * size


def handmade_rle_sequences(nseq=10):
    """One compressed block whose LL, OF and ML tables are all RLE (codes 4, 0, 10: four literals, then a 13-byte match
    at repeat offset 1 -- no extra bits, no state bits: the bit stream is its padding byte alone)."""
    from nvcomp_amd import datasets

    lits = bytes(datasets.noise(4 * nseq, 41))
    regen = len(lits)
    body = bytes([0 | 1 << 2 | (regen & 15) << 4, regen >> 4]) + lits
    body += bytes([nseq, 1 << 6 | 1 << 4 | 1 << 2, 4, 0, 10, 0x01])
    out = b""
    for k in range(nseq):
        out += lits[4 * k: 4 * k + 4] + lits[4 * k + 3: 4 * k + 4] * 13
    frame = (0xFD2FB528).to_bytes(4, "little") + bytes([0x20, len(out)])
    frame += (1 | 2 << 1 | len(body) << 3).to_bytes(3, "little") + body
    return np.frombuffer(frame, dtype=np.uint8), out


def main():
    from nvcomp_amd import datasets, zstd_cpu as z

    if z.load() is None:
        sys.exit("libzstd cannot be loaded")
    table = {"source": "gz", "file": "ExampleTable.txt.gz", "offset": 0, "size": 65536}
    floats = {"source": "gz", "file": "ExampleFloatData.csv.gz", "offset": 0, "size": 65536}
    entries = []

    def add(name, recipe, comp, how, **flags):
        data = original(recipe)
        comp = np.asarray(comp, dtype=np.uint8)
        assert comp.size < 100 * 1024, (name, comp.size)
        if not flags.get("dict_id"):
            assert np.array_equal(z.decompress(comp, max(data.size, 1)), data), name
        path = os.path.join(GOLDEN, f"zstd_{name}.zst")
        comp.tofile(path)
        entries.append({"file": os.path.basename(path), "how": how, "recipe": recipe, "bytes": int(data.size),
                        "sha256": hashlib.sha256(data.tobytes()).hexdigest(), "zst_bytes": int(comp.size), **flags})

    for lvl in (-5, 1, 3, 9, 19):
        add(f"table_l{lvl}", table, z.compress(original(table), lvl), f"ZSTD_compress2 level {lvl}")
    add("floats_l3_checksum", floats, z.compress(original(floats), 3, checksum=True), "level 3, checksumFlag 1")
    add("floats_l19_nosize", floats, z.compress(original(floats), 19, content_size=False), "level 19, contentSizeFlag 0")
    text = {"source": "gz", "file": "ExampleTable.txt.gz", "offset": 65536, "size": 98304}
    add("table_streamed_4k", text, z.compress_streamed(original(text), 3, 4096), "level 3, ZSTD_e_flush every 4 KiB")
    add("table_streamed_512", text, z.compress_streamed(original(text), 1, 512, checksum=True),
        "level 1, ZSTD_e_flush every 512 B, checksum")
    mixed = {"source": "dataset", "class": "float_csv", "size": 98304, "seed": 7}
    add("float_csv_streamed_l19", mixed, z.compress_streamed(original(mixed), 19, 8192), "level 19, flush every 8 KiB")
    ints = {"source": "dataset", "class": "int32", "size": 65536, "seed": 3}
    add("int32_l3", ints, z.compress(original(ints), 3), "level 3")
    add("int32_streamed", ints, z.compress_streamed(original(ints), 3, 2048), "level 3, flush every 2 KiB")
    low = {"source": "dataset", "class": "lowcard", "size": 65536, "seed": 5}
    add("lowcard_l9", low, z.compress(original(low), 9), "level 9")
    zeros = {"source": "dataset", "class": "zeros", "size": 200000, "seed": 0}
    add("zeros", zeros, z.compress(original(zeros), 3), "level 3 (RLE blocks)")
    noise = {"source": "dataset", "class": "noise", "size": 40000, "seed": 11}
    add("noise", noise, z.compress(original(noise), 3), "level 3 (raw blocks)")
    half = {"source": "concat", "parts": [{"source": "dataset", "class": "noise", "size": 3000, "seed": 12},
                                          {"source": "dataset", "class": "text", "size": 3000, "seed": 12}]}
    add("noise_text", half, z.compress(original(half), 1), "level 1 (raw literals beside matches)")
    # several frames in one chunk: a skippable frame, an empty frame, frames with and without content size
    parts = [{"source": "dataset", "class": "text", "size": 20000, "seed": 1},
             {"source": "concat", "parts": []},
             {"source": "dataset", "class": "table", "size": 30000, "seed": 2}]
    multi = np.concatenate([z.compress(original(parts[0]), 3), z.skippable_frame(b"nvcomp skippable frame", 7),
                            z.compress(original(parts[1]), 3), z.compress(original(parts[2]), 9, content_size=False,
                                                                             checksum=True)])
    add("concat", {"source": "concat", "parts": parts}, multi, "frames: level 3 | skippable | empty | level 9 no size")
    empty = {"source": "concat", "parts": []}
    add("empty", empty, z.compress(original(empty), 3), "an empty frame")
    add("dict_id", table, z.with_dictionary_id(z.compress(original(table), 3)),
        "level 3, then Dict_ID_flag 3 and an ID written into the header", dict_id=True)
    far1 = {"source": "far", "size": 1 << 20, "period": 160 * 1024, "noise": 20000, "seed": 21}
    add("far_wl20", far1, z.compress(original(far1), 3, window_log=20), "level 3, windowLog 20: repeats 160 KiB back")
    far2 = {"source": "far", "size": 2 << 20, "period": 256 * 1024, "noise": 24000, "seed": 22}
    add("far_wl24", far2, z.compress(original(far2), 3, window_log=24), "level 3, windowLog 24: repeats 256 KiB back")
    comp, data = handmade_rle_literals()
    add("handmade_rle_literals", {"source": "hex", "hex": data.hex()}, comp, "by hand: RLE literals, no sequences")
    comp, data = handmade_rle_sequences()
    add("handmade_rle_tables", {"source": "hex", "hex": data.hex()}, comp, "by hand: LL / OF / ML tables in RLE mode")
    manifest = {"libzstd": z.version(), "frames": entries}
    with open(os.path.join(GOLDEN, "zstd_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print(f"{len(entries)} frames, {sum(e['zst_bytes'] for e in entries)} bytes")


if __name__ == "__main__":
    main()
