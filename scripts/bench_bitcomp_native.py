#!/usr/bin/env python3
"""Native Bitcomp API throughput on the card (include/nvcomp/native/bitcomp.h), timed with HIP events around each call,
in GB/s of UNCOMPRESSED bytes, on a buffer of --mib MiB (default 1 GiB) of the float columns (nvcomp_amd.datasets):

  lossless uint32 / fp32                 compress, uncompress
  lossy fp16 / fp32 / fp64, two deltas   compress, uncompress (fp16 and fp64: the fp32 columns converted)
  partial uncompress of 1 MiB            time, and the bytes of the compressed buffer it had to read (from the offset table)

Every lossless result is compared with the input and every lossy one with |x - x'| <= delta / 2 + ulp. One JSON line per
configuration; exits non-zero on a mismatch. The batched yardstick to put next to it: python bench.py --full --algo bitcomp."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    args = ap.parse_args()

    import torch

    import nvcomp_amd
    from nvcomp_amd import bitcomp_native as bn
    from nvcomp_amd import datasets

    lib = nvcomp_amd.load_library()
    dev = nvcomp_amd.TorchDevice("cuda:0")
    stream = torch.cuda.current_stream()
    n = args.mib << 20
    unique = torch.from_numpy(datasets.float_columns(64 << 20, 5).view(np.float32).copy()).cuda()
    f32 = unique.repeat((n // 4 + unique.numel() - 1) // unique.numel())[: n // 4].contiguous()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "bytes": n}), flush=True)

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3)
        return float(np.median(times)), float(min(times))

    configs = [("lossless uint32", bn.DataType.UNSIGNED_32BIT, bn.Mode.LOSSLESS, None, f32),
               ("lossless fp32", bn.DataType.FP32_DATA, bn.Mode.LOSSLESS, None, f32)]
    for delta in (1e-3, 1e-1):
        configs.append((f"lossy fp16 delta={delta}", bn.DataType.FP16_DATA, bn.Mode.LOSSY_FP_TO_SIGNED, delta, None))
        configs.append((f"lossy fp32 delta={delta}", bn.DataType.FP32_DATA, bn.Mode.LOSSY_FP_TO_SIGNED, delta, f32))
        configs.append((f"lossy fp64 delta={delta}", bn.DataType.FP64_DATA, bn.Mode.LOSSY_FP_TO_SIGNED, delta, None))
    ok = True
    for name, dtype, mode, delta, data in configs:
        if args.only not in name:
            continue
        if data is None:  # the same values in the other width, the buffer still n bytes
            elem = bn.ELEM_BYTES[dtype]
            wide = torch.cat([f32, f32]) if elem == 2 else f32  # n / elem elements
            data = wide[: n // elem].to(torch.float16 if elem == 2 else torch.float64).contiguous()
            del wide
        assert data.numel() * data.element_size() == n
        src = data.view(torch.uint8)
        plan = bn.Plan(n, dtype, mode, bn.Algorithm.DEFAULT, dev, lib)
        comp = dev.empty(plan.max_buflen())
        out = dev.empty(n)
        if delta is None:
            c_med, c_best = timed(lambda: plan.compress_into(src.data_ptr(), comp.data_ptr()))
        else:
            c_med, c_best = timed(lambda: plan.compress_lossy_into(src.data_ptr(), comp.data_ptr(), delta))
        size = plan.compressed_size(comp)
        d_med, d_best = timed(lambda: plan.uncompress_into(comp.data_ptr(), out.data_ptr()))
        torch.cuda.synchronize()
        back = out.view(data.dtype)
        if delta is None:
            good = bool(torch.equal(out, src))
        else:
            inside = data.double().abs() / delta < 2.0 ** (8 * bn.ELEM_BYTES[dtype] - 1) - 1  # not saturated
            err = ((back.double() - data.double()).abs() * inside).max().item()
            good = err <= delta / 2 + float(torch.finfo(data.dtype).eps) * float(data.abs().max().item())
        ok &= good
        rec = {"config": name, "compressed_bytes": size, "ratio": round(n / size, 3),
               "compress_gbps": round(n / c_med / 1e9, 1), "compress_gbps_best": round(n / c_best / 1e9, 1),
               "uncompress_gbps": round(n / d_med / 1e9, 1), "uncompress_gbps_best": round(n / d_best / 1e9, 1),
               "compress_ms": round(c_med * 1e3, 4), "uncompress_ms": round(d_med * 1e3, 4),
               "hbm_fraction_uncompress": round((n + size) / d_med / 1e9 / HBM_PEAK_GBPS, 3), "verified": good}
        if name == "lossless uint32":
            part = 1 << 20
            start = n // 2 + 4096
            small = dev.empty(part)
            p_med, p_best = timed(lambda: plan.partial_uncompress_into(comp.data_ptr(), small.data_ptr(), start, part))
            torch.cuda.synchronize()
            good_part = bool(torch.equal(small, src[start: start + part]))
            ok &= good_part
            first, last = start // bn.SEGMENT_BYTES, (start + part - 1) // bn.SEGMENT_BYTES
            table = comp[bn.HEADER_BYTES + 8 * first: bn.HEADER_BYTES + 8 * (last + 2)].cpu().numpy().view(np.uint64)
            rec["partial_1mib"] = {"median_us": round(p_med * 1e6, 2), "best_us": round(p_best * 1e6, 2),
                                   "segments": last - first + 1,
                                   "compressed_bytes_read": int(table[-1] - table[0]) + bn.HEADER_BYTES + 8 * (last - first + 2),
                                   "verified": good_part}
        print(json.dumps(rec), flush=True)
        plan.destroy()
        del comp, out, src, data
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
