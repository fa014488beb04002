#!/usr/bin/env python3
"""Times the BGZF writer (include/bz2_mi355x.h section 7) and, with --read, the BGZF reader (section 8) on one GPU.

    tools/bgzf_time.py [--mib 1024] [--calls 5] [--host-mib 64] [--other-lib PATH]
    tools/bgzf_time.py --read [--mib 256] [--calls 5] [--host-mib 64]

The input is --mib MiB of the bench corpus (corpus.py) in HBM.  The runs alternate, --calls times behind a warm-up of each:
  a   df_gpu_bgzf_encode_device at the default block size (65 280 bytes)
  b   df_gpu_encode_batch_device (kind 2) over the same 65 280-byte chunks handed in as separate inputs (65 280 is a multiple
      of 16, so the batch call takes them where they lie): the same pipeline with padded offsets and the plain gzip wrap
  c   df_gpu_encode_device (kind 2): the whole input as one stream of one member
--other-lib PATH runs b and c through another build of the library (a parent commit's libbz2_mi355x.so) in the same process,
and adds b_this: b through this build, to tell the cost of the BGZF forms from a difference between two builds' workspaces.
One JSON line: per run the times in seconds, their median and the file's bytes; the stage timers (df_gpu_last_timings) and
df_gpu_last_bgzf_stats of the last a; the decode of a's file through df_gpu_decode_members_device; and host to host over the
first --host-mib MiB: bgzf_compress against one Python thread that builds the same kind of file with zlib (level 6).
a's file is decoded on the device and compared with the input before anything is timed.

--read: the file is this library's own (df_gpu_bgzf_encode_device over --mib MiB of the corpus, in HBM); it is read whole by
df_gpu_bgzf_read_device and the bytes compared with the corpus before anything is timed.  Then, alternating call by call,
--calls times behind one warm call of each:
  whole     df_gpu_bgzf_read_device over [0, total) with the index in hand
  members   df_gpu_decode_members_device over the same buffer (section 6: two decode passes and a copy)
  index     df_gpu_bgzf_index_device (search and chain)
  r64m, r1m, r1b, r100   range reads of 64 MiB, 1 MiB, one block's 65 280 bytes and 100 bytes from the middle of the file
  sizes     the sizes-only call (no launch)
and, on the host, host_index (bgzf_index over the file's bytes) and, over the first --host-mib MiB, bgzf_decompress against
gzip_decompress_members and Python's gzip.decompress.  One JSON line: the times in seconds, their medians, the stage timers
(df_gpu_last_timings) and df_gpu_last_bgzf_read_stats behind `whole`, `members` and `r64m`."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 65280


def python_bgzf(data):
    """one thread, zlib level 6: the file bgzip writes, block by block"""
    out = []
    for a in range(0, len(data), B):
        chunk = data[a:a + B]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(chunk) + c.flush()
        out.append(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(d) + 25) + d
                   + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)


class Raw:
    """the two older calls through a library of their own (the C ABI alone)"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        vp, sz, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)
        self.L.bz_gpu_engine_create.argtypes = [C.POINTER(vp), C.c_int, sz]
        self.L.bz_gpu_engine_destroy.argtypes = [vp]
        self.L.df_gpu_encode_batch_device.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, vp, sz, u64p, u64p]
        self.L.df_gpu_encode_device.argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
        self.L.df_gpu_last_timings.argtypes = [vp, C.POINTER(C.c_double)]
        self.L.df_encode_batch_bound.restype = sz
        self.L.df_encode_batch_bound.argtypes = [u64p, sz]
        self.L.df_encode_bound.restype = sz
        self.L.df_encode_bound.argtypes = [sz]
        self.h = vp()
        assert self.L.bz_gpu_engine_create(C.byref(self.h), 0, 1) == 0

    def batch(self, d_in, off, lens, d_out, cap):
        k = len(off)
        o_off, o_len = (C.c_uint64 * k)(), (C.c_uint64 * k)()
        rc = self.L.df_gpu_encode_batch_device(self.h, 2, d_in, off, lens, k, d_out, cap, o_off, o_len)
        assert rc == 0, rc
        return o_off[k - 1] + o_len[k - 1]

    def stream(self, d_in, n, d_out, cap):
        got = C.c_size_t(0)
        rc = self.L.df_gpu_encode_device(self.h, 2, d_in, n, d_out, cap, C.byref(got))
        assert rc == 0, rc
        return got.value

    def timings(self):
        t = (C.c_double * 6)()
        self.L.df_gpu_last_timings(self.h, t)
        return list(t)

    def close(self):
        self.L.bz_gpu_engine_destroy(self.h)


def read_main(a):
    import gzip
    import corpus
    import torch
    pkg = importlib.import_module("rust-compression_amd")
    data = corpus.corpus_bytes(a.mib << 20)
    n = len(data)
    eng = pkg.GpuEngine(0, 1)
    t_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    file = torch.empty(pkg.bgzf_bound(n) + 64, dtype=torch.uint8, device="cuda")
    size, offs = eng.bgzf_encode_device(t_in.data_ptr(), n, file.data_ptr(), pkg.bgzf_bound(n), offsets=True)
    back = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    ix = eng.bgzf_index_device(file.data_ptr(), size)
    assert ix.verdict == 0 and ix.coff[:-1] == offs and ix.total == n, "the device index is not the writer's table"
    assert eng.bgzf_read_device(file.data_ptr(), size, ix, 0, n, back.data_ptr(), n) == (n, 0)
    assert torch.equal(back[:n], t_in), "the file does not read back as the input"
    host_file = file[:size].cpu().numpy().tobytes()
    mid = (n // 2) // B * B + 12345

    def ranged(length):
        def run():
            got = eng.bgzf_read_device(file.data_ptr(), size, ix, mid, length, back.data_ptr(), length)
            assert got == (min(length, n - mid), 0)
        return run
    runs = {
        "whole": lambda: eng.bgzf_read_device(file.data_ptr(), size, ix, 0, n, back.data_ptr(), n),
        "members": lambda: eng.gzip_decode_members_device(file.data_ptr(), size, back.data_ptr(), n),
        "index": lambda: eng.bgzf_index_device(file.data_ptr(), size),
        "r64m": ranged(64 << 20), "r1m": ranged(1 << 20), "r1b": ranged(B), "r100": ranged(100),
        "sizes": lambda: eng.bgzf_read_device(file.data_ptr(), size, ix, 0, n, None, 0),
        "host_index": lambda: pkg.bgzf_index(host_file),
    }
    res = {"bytes": n, "file_bytes": size, "blocks": ix.blocks, "times": {k: [] for k in runs}, "stages": {}, "stats": {}}
    for fn in runs.values():
        fn()
    for _ in range(a.calls):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            res["times"][k].append(time.perf_counter() - t)
            if k in ("whole", "members", "r64m", "r1b"):
                res["stages"][k] = eng.deflate_timings()
                res["stats"][k] = eng.bgzf_read_stats() if k != "members" else eng.gzip_decode_members_stats()
    ranged(64 << 20)()
    assert torch.equal(back[:min(64 << 20, n - mid)], t_in[mid:mid + (64 << 20)]), "the range does not read back as the input"
    res["median"] = {k: statistics.median(v) for k, v in res["times"].items()}
    part_n = min(a.host_mib << 20, n) // B * B
    k = part_n // B
    part_file = host_file[:offs[k]]          # (offs holds count + 1 entries: the first k blocks, no marker)
    want = data[:part_n]
    host = {"bytes": part_n, "file_bytes": len(part_file)}
    for name, fn in (("bgzf_decompress", lambda: pkg.bgzf_decompress(part_file)),
                     ("gzip_decompress_members", lambda: pkg.gzip_decompress_members(part_file)[0]),
                     ("bgzf_read_1mib", lambda: pkg.bgzf_read(part_file, part_n // 2, 1 << 20))):
        assert fn() == (want if name != "bgzf_read_1mib" else want[part_n // 2:part_n // 2 + (1 << 20)]), name
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        host[name] = statistics.median(ts)
    t = time.perf_counter()
    assert gzip.decompress(part_file) == want
    host["python_gzip"] = time.perf_counter() - t
    res["host"] = host
    print(json.dumps(res), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--read", action="store_true")
    a = ap.parse_args()
    if a.read:
        return read_main(a)
    import corpus
    import torch
    pkg = importlib.import_module("rust-compression_amd")
    data = corpus.corpus_bytes(a.mib << 20)
    n = len(data)
    eng = pkg.GpuEngine(0, 1)
    own = os.path.join(ROOT, "rust-compression_amd", "libbz2_mi355x.so")
    raw = Raw(a.other_lib or own)
    t_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    count = pkg.bgzf_block_count(n)
    off = (C.c_uint64 * count)(*[k * B for k in range(count)])
    lens = (C.c_uint64 * count)(*[min(B, n - k * B) for k in range(count)])
    cap_a, cap_b, cap_c = pkg.bgzf_bound(n), raw.L.df_encode_batch_bound(lens, count), raw.L.df_encode_bound(n)
    out = torch.empty(max(cap_a, cap_b, cap_c) + 64, dtype=torch.uint8, device="cuda")

    runs = {
        "a": lambda: eng.bgzf_encode_device(t_in.data_ptr(), n, out.data_ptr(), cap_a),
        "b": lambda: raw.batch(t_in.data_ptr(), off, lens, out.data_ptr(), cap_b),
        "c": lambda: raw.stream(t_in.data_ptr(), n, out.data_ptr(), cap_c),
    }
    if a.other_lib:
        mine = Raw(own)
        runs["b_this"] = lambda: mine.batch(t_in.data_ptr(), off, lens, out.data_ptr(), cap_b)
    res = {"bytes": n, "blocks": count, "other_lib": a.other_lib, "times": {k: [] for k in runs}, "file_bytes": {}}
    for k, fn in runs.items():          # warm-up: workspaces, and the sizes
        res["file_bytes"][k] = fn()
    # a's file, decoded on the device, is the input
    size_a = runs["a"]()
    back = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    assert eng.gzip_decode_members_device(out.data_ptr(), size_a, back.data_ptr(), n) == (n, 0)
    assert torch.equal(back[:n], t_in), "the file does not decode to the input"
    file_a = out[:size_a].clone()
    for _ in range(a.calls):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            res["times"][k].append(time.perf_counter() - t)
            if k == "a":
                res["stages_a"] = eng.deflate_timings()
                res["stats_a"] = eng.bgzf_stats()
            else:
                res["stages_" + k] = (mine if k == "b_this" else raw).timings()
    res["median"] = {k: statistics.median(v) for k, v in res["times"].items()}
    res["gbps"] = {k: n / v / 1e9 for k, v in res["median"].items()}
    dec = []
    for _ in range(a.calls):
        t = time.perf_counter()
        eng.gzip_decode_members_device(file_a.data_ptr(), size_a, back.data_ptr(), n)
        dec.append(time.perf_counter() - t)
    res["decode_members"] = statistics.median(dec)
    # host to host
    part = data[:a.host_mib << 20]
    f = pkg.bgzf_compress(part)
    assert pkg.gzip_decompress_members(f) == (part, 0)
    hh = []
    for _ in range(3):
        t = time.perf_counter()
        pkg.bgzf_compress(part)
        hh.append(time.perf_counter() - t)
    t = time.perf_counter()
    pf = python_bgzf(part)
    res["host"] = {"bytes": len(part), "bgzf_compress": statistics.median(hh), "python_zlib": time.perf_counter() - t,
                   "file_bytes": len(f), "python_file_bytes": len(pf)}
    print(json.dumps(res), flush=True)
    raw.close()
    if a.other_lib:
        mine.close()
    eng.close()


if __name__ == "__main__":
    main()
