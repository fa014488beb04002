#!/usr/bin/env python3
"""Times "every member of a gzip file" (include/bz2_mi355x.h section 6) on one GPU.

    tools/gz_members_time.py [--mib 256] [--calls 5] [--workload W1,W2,W3]

Workloads, all of --mib MiB of the bench corpus (corpus.py), members written by zlib at level 6:
  W1   members of 64 KiB (a BGZF-like file: 4 096 members at 256 MiB)
  W2   the same bytes as members of 16 MiB: every member takes the split path
  W3   W1 with one stored member in the middle that holds 64 nested .gz files: the cost of decoding a member again

Per workload one JSON line with the medians of --calls calls behind a warm-up call, in seconds:
  device      df_gpu_decode_members_device, file and output in HBM
  host        gzip_decompress_members, host to host
  python      gzip.decompress on one host thread
  floor       df_gpu_decode_batch_device (kind 2) over the same members handed in as separate, already aligned entries:
              the same decode without search, gather, zero skip and compaction
  stages      df_gpu_last_decode_members_timings of the last device call (host clock around waited launches)
  timings     df_gpu_last_timings of that call; stats: df_gpu_last_decode_members_stats
The bytes of every path are compared with the corpus before anything is timed."""
import argparse
import gzip
import importlib
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def members_of(data, size):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(member, [data[a:a + size] for a in range(0, len(data), size)]))


def median_of(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def run(pkg, eng, name, mems, data, calls):
    import torch
    f = b"".join(mems)
    t_in = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    need, v = eng.gzip_decode_members_device(t_in.data_ptr(), len(f), None, 0)
    assert (need, v) == (len(data), 0), (need, v, len(data))
    out = torch.empty(need + 64, dtype=torch.uint8, device="cuda")

    def device():
        assert eng.gzip_decode_members_device(t_in.data_ptr(), len(f), out.data_ptr(), need) == (need, 0)

    device()
    torch.cuda.synchronize()
    assert out[:need].cpu().numpy().tobytes() == data, "device bytes differ"
    assert pkg.gzip_decompress_members(f) == (data, 0), "host bytes differ"
    res = {"workload": name, "members": len(mems), "file_bytes": len(f), "bytes": len(data)}
    res["device"] = median_of(device, calls)
    res["stats"] = eng.gzip_decode_members_stats()
    res["stages"] = eng.gzip_decode_members_timings()
    res["timings"] = eng.deflate_timings()
    res["split_stats"] = eng.deflate_decode_split_stats()
    res["host"] = median_of(lambda: pkg.gzip_decompress_members(f), calls)
    res["python"] = median_of(lambda: gzip.decompress(f), max(3, calls // 2))
    # the floor: the members as separate entries at multiples of 16
    buf, off = bytearray(), []
    for m in mems:
        off.append(len(buf))
        buf += m + bytes(-len(m) % 16)
    t_b = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    lens = [len(m) for m in mems]
    o_off, o_len, ver = eng.deflate_decode_batch_device(2, t_b.data_ptr(), off, lens, None, 0)
    cap = o_off[-1] + o_len[-1]
    out_b = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    res["floor"] = median_of(lambda: eng.deflate_decode_batch_device(2, t_b.data_ptr(), off, lens, out_b.data_ptr(), cap), calls)
    res["floor_timings"] = eng.deflate_timings()
    res["gbps_device"] = len(data) / res["device"] / 1e9
    res["gbps_host"] = len(data) / res["host"] / 1e9
    res["gbps_python"] = len(data) / res["python"] / 1e9
    res["over_floor"] = res["device"] / res["floor"] - 1.0
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--workload", default="W1,W2,W3")
    a = ap.parse_args()
    import corpus
    pkg = importlib.import_module("rust-compression_amd")
    data = corpus.corpus_bytes(a.mib << 20)
    eng = pkg.GpuEngine(0, 1)
    want = a.workload.split(",")
    small = members_of(data, 65536) if ("W1" in want or "W3" in want) else None
    if "W1" in want:
        run(pkg, eng, "W1", small, data, a.calls)
    if "W2" in want:
        run(pkg, eng, "W2", members_of(data, 16 << 20), data, a.calls)
    if "W3" in want:
        nested = b"".join(member(data[k * 1000:k * 1000 + 500]) for k in range(64))
        half = len(small) // 2
        mems = small[:half] + [member(nested, 0)] + small[half:]
        run(pkg, eng, "W3", mems, data[:half * 65536] + nested + data[half * 65536:], a.calls)
    eng.close()


if __name__ == "__main__":
    main()
