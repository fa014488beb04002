#!/usr/bin/env python3
"""Many small inputs: one bz_encode_batch call against a loop of bz_encode_buffer calls over the same inputs.

    tools/batch_time.py [--workload sample1x256|corpus16k|all] [--runs 3] [--calls 5] [--loops 3] [--oracle 16] [--level 9]

Workloads (level 9, one GPU):
  sample1x256  256 copies of tests/golden/sample1.ref (98 696 bytes each)
  corpus16k    4 096 consecutive 16 KiB slices of the bench corpus (corpus.py), 64 MiB in all
Per workload and run, alternating the two forms (batch, loop, batch, loop, ...): the median of `calls` warm
bz_encode_batch calls, the median of `loops` warm passes of the bz_encode_buffer loop (the parent commit's code), and
the oracle on one CPU thread for a sample of the inputs, scaled to all of them.  The streams of the two forms are
compared byte for byte before anything is timed.  Every call ends with its bytes on the host, so a host clock around
it is the call's time.  Prints one line of JSON per workload.  Needs a GPU (no fallback).

    tools/batch_time.py --decode [--workload ...] [--runs 3] [--calls 5] [--loops 3]

The same two workloads, compressed once with compress_batch: one bz_decode_batch call (decompress_batch) against a loop
of bz_decode_buffer calls (the parent commit's code) over the same streams, alternating, both warm, medians as above;
the outputs of the two forms are compared byte for byte (and with the inputs) before anything is timed.  The line also
carries bz_gpu_last_decode_timings and bz_gpu_last_decode_batch_stats of one bz_gpu_decode_batch_device call over the
same streams in HBM.

    tools/batch_time.py --deflate [--kind deflate|zlib|gzip] [--workload ...] [--runs 3] [--calls 5] [--loops 3]

The same two workloads through the Deflate encoders: one df_encode_batch call (deflate_compress_batch) against a loop of
df_encode_buffer calls (the parent commit's code), alternating, both warm, medians as above; the streams of the two forms
are compared byte for byte before anything is timed.  sample1x256 (98 696 bytes each: two blocks) takes the one-input
path inside the batch call and is the control; corpus16k takes the batch path.  The line also carries
df_gpu_last_timings and df_gpu_last_batch_stats of one df_gpu_encode_batch_device call over the same inputs in HBM.
BZ_DF_BATCH_MIB sets the sub-batch size.

    tools/batch_time.py --deflate --dict-kib N [--kind deflate|zlib] [--workload ...]

Encoding with a preset dictionary of N KiB of another chapter of the bench corpus: one df_encode_batch_dict call
(deflate_compress_batch(.., dict_=)) against the loop of df_encode_buffer_dict calls over the same inputs (the parent
commit's code), both host to host, and -- the control -- the batch call WITHOUT a dictionary over the same inputs; the three
alternate within every run.  The streams of batch and loop are compared byte for byte before anything is timed.  The line
also carries, per form ("dict", "plain"), `calls` df_gpu_encode_batch_device_dict calls over the inputs in HBM, alternating
the forms call by call: wall time, df_gpu_last_timings, df_gpu_last_batch_stats, and the stream bytes.

    tools/batch_time.py --inflate [--kind deflate|zlib|gzip] [--workload ...|text64m] [--runs 3] [--calls 5] [--loops 3]

The same workloads, compressed once with deflate_compress_batch: one df_decode_batch call (deflate_decompress_batch), host
to host, against a loop of Python's zlib.decompress over the same streams on one host thread (the yardstick: a decoder
that shares no code with this one), alternating, medians as above; the outputs are compared with the inputs before
anything is timed.  The line also carries one df_gpu_decode_batch_device call over the streams in HBM: its wall time, the
split between the sizes launch, the writing launch and the checksum kernel (df_gpu_last_timings) and
df_gpu_last_decode_batch_stats.  text64m is ONE entry of 64 MiB of the bench corpus: what a single stream costs.

    tools/batch_time.py --inflate --dict-kib N [--kind deflate|zlib] [--workload ...]

Decoding with a preset dictionary (section 5, clause (c) of the header): the dictionary is N KiB of another chapter of the
bench corpus, the streams are zlib's (level 6) -- made once with zdict= and once without -- and the project's own
(deflate_compress_batch(.., dict_=)).  Per form ("dict", "plain", "own_dict"), in the same run and alternating: deflate_decompress_batch host to host, the loop
of zlib.decompressobj(wbits, zdict=) on one host thread, and one deflate_decode_batch_device call over the streams in HBM
with its launches' times.  With --inflate-one the ONE stream is zlib's, made with the dictionary; --inflate-one --zlib-made
is its control: zlib's stream of the same bytes without a dictionary.

    tools/batch_time.py --inflate-one SIZE_MIB [--calls 5] [--one-wave]

ONE raw Deflate stream of SIZE_MIB MiB of the bench corpus (written by deflate_compress_batch), decoded by the split path
(BZ_DF_INF_SPLIT_KIB / BZ_DF_INF_PIECE_KIB as the environment has them): host to host (deflate_decompress_batch) and
HBM-resident (one deflate_decode_batch_device call: it returns with the device idle; timed by a host clock and by a pair of
hipEvents recorded on the idle device around it), the median of `calls` calls after a warm one each, the phases of the split entry
(df_gpu_last_decode_split_timings), the split stats, and zlib.decompress on one host thread over the same stream.
--one-wave adds ONE HBM-resident call with BZ_DF_INF_SPLIT_KIB=0: this build's one-wave path (12.6 s for 64 MiB; the parent
commit's library is timed by running its own `--inflate --workload text64m`)."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(name):
    if name == "sample1x256":
        with open(os.path.join(ROOT, "tests", "golden", "sample1.ref"), "rb") as f:
            one = f.read()
        return [one] * 256
    if name == "corpus16k":
        import corpus
        data = corpus.corpus_bytes(4096 * 16384)
        return [data[i * 16384:(i + 1) * 16384] for i in range(4096)]
    if name == "text64m":
        import corpus
        return [corpus.corpus_bytes(64 << 20)]
    raise SystemExit("unknown workload %s" % name)


def decode_mode(pkg, a, names):
    L = pkg.lib()

    def loop(streams):
        out = []
        for z in streams:
            p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
            rc = L.bz_decode_buffer(0, z, len(z), C.byref(p), C.byref(n))
            out.append((C.string_at(p, n.value), rc))
            L.bz_free(p)
        return out

    def device_call(streams):
        """one bz_gpu_decode_batch_device call over the streams in HBM: its stage timings and stats"""
        import torch
        off, buf = [], bytearray()
        for z in streams:
            off.append(len(buf))
            buf += z
            buf += bytes(-len(buf) % 4)
        lens = [len(z) for z in streams]
        t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        eng = pkg.GpuEngine(0, 8)
        try:
            o_off, o_len, _ = eng.decode_batch_device(t.data_ptr(), off, lens, None, 0)
            cap = max(x + n for x, n in zip(o_off, o_len))
            o = torch.empty((cap + 64,), dtype=torch.uint8, device="cuda")
            eng.decode_batch_device(t.data_ptr(), off, lens, o.data_ptr(), cap)   # (warm)
            eng.decode_batch_device(t.data_ptr(), off, lens, o.data_ptr(), cap)
            return {k: round(v * 1e3, 3) for k, v in eng.decode_timings().items()}, eng.decode_batch_stats()
        finally:
            eng.close()

    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        streams = pkg.compress_batch(datas, a.level)
        batch = pkg.decompress_batch(streams)        # (warms the engine's workspace too)
        same = batch == loop(streams) and batch == [(d, 0) for d in datas]
        runs = []
        for _ in range(a.runs):
            tb, tl = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                pkg.decompress_batch(streams)
                tb.append(time.perf_counter() - t0)
            for _ in range(a.loops):
                t0 = time.perf_counter()
                loop(streams)
                tl.append(time.perf_counter() - t0)
            runs.append({"batch_ms": round(statistics.median(tb) * 1e3, 2), "loop_ms": round(statistics.median(tl) * 1e3, 2),
                         "batch_all_ms": [round(t * 1e3, 2) for t in tb], "loop_all_ms": [round(t * 1e3, 2) for t in tl]})
        bm = statistics.median(r["batch_ms"] for r in runs)
        lm = statistics.median(r["loop_ms"] for r in runs)
        stage_ms, stats = device_call(streams)
        print(json.dumps({"mode": "decode", "workload": name, "streams": len(streams), "bytes": total,
                          "compressed_bytes": sum(len(z) for z in streams), "level": a.level, "outputs_equal": same,
                          "batch_ms": bm, "loop_ms": lm, "loop_over_batch": round(lm / bm, 2),
                          "batch_GBps": round(total / bm / 1e6, 3), "loop_GBps": round(total / lm / 1e6, 3),
                          "device_call_stage_ms": stage_ms, "device_call_batch_stats": stats, "runs": runs}), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's outputs differ from the loop's or from the inputs")


def deflate_mode(pkg, a, names):
    L = pkg.lib()
    kind = {"deflate": pkg.DEFLATE, "zlib": pkg.ZLIB, "gzip": pkg.GZIP}[a.kind]

    def loop(datas):
        out = []
        for d in datas:
            p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
            rc = L.df_encode_buffer(kind, 0, d, len(d), C.byref(p), C.byref(n))
            if rc != 0:
                raise SystemExit("df_encode_buffer: %d" % rc)
            out.append(C.string_at(p, n.value))
            L.bz_free(p)
        return out

    def device_call(datas):
        """one df_gpu_encode_batch_device call over the inputs in HBM: its stage timings and stats"""
        import torch
        off, buf = [], bytearray()
        for d in datas:
            off.append(len(buf))
            buf += d
            buf += bytes(-len(buf) % 16)
        lens = [len(d) for d in datas]
        t = torch.frombuffer(buf + bytes(16), dtype=torch.uint8).cuda()
        cap = pkg.deflate_encode_batch_bound(lens)
        o = torch.empty((cap + 64,), dtype=torch.uint8, device="cuda")
        eng = pkg.GpuEngine(0, 1)
        try:
            eng.deflate_encode_batch_device(kind, t.data_ptr(), off, lens, o.data_ptr(), cap)   # (warm)
            t0 = time.perf_counter()
            eng.deflate_encode_batch_device(kind, t.data_ptr(), off, lens, o.data_ptr(), cap)
            wall = time.perf_counter() - t0
            return ({k: round(v * 1e3, 3) for k, v in eng.deflate_timings().items()}, eng.deflate_batch_stats(), round(wall * 1e3, 3))
        finally:
            eng.close()

    if a.dict_kib:
        return deflate_dict_mode(pkg, a, names, kind)
    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        batch = pkg.deflate_compress_batch(datas, kind)   # (warms the engine's workspace too)
        same = batch == loop(datas)
        runs = []
        for _ in range(a.runs):
            tb, tl = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                pkg.deflate_compress_batch(datas, kind)
                tb.append(time.perf_counter() - t0)
            for _ in range(a.loops):
                t0 = time.perf_counter()
                loop(datas)
                tl.append(time.perf_counter() - t0)
            runs.append({"batch_ms": round(statistics.median(tb) * 1e3, 2), "loop_ms": round(statistics.median(tl) * 1e3, 2),
                         "batch_all_ms": [round(t * 1e3, 2) for t in tb], "loop_all_ms": [round(t * 1e3, 2) for t in tl]})
        bm = statistics.median(r["batch_ms"] for r in runs)
        lm = statistics.median(r["loop_ms"] for r in runs)
        stage_ms, stats, wall_ms = device_call(datas)
        print(json.dumps({"mode": "deflate", "kind": a.kind, "workload": name, "inputs": len(datas), "bytes": total,
                          "compressed_bytes": sum(len(z) for z in batch), "batch_mib": os.environ.get("BZ_DF_BATCH_MIB", "default"),
                          "streams_equal": same, "batch_ms": bm, "loop_ms": lm, "loop_over_batch": round(lm / bm, 2),
                          "batch_GBps": round(total / bm / 1e6, 3), "loop_GBps": round(total / lm / 1e6, 3),
                          "device_call_ms": wall_ms, "device_call_stage_ms": stage_ms, "device_call_batch_stats": stats,
                          "runs": runs}), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's streams differ from the loop's")


def deflate_dict_mode(pkg, a, names, kind):
    import torch
    L = pkg.lib()
    if kind == pkg.GZIP:
        raise SystemExit("batch_time.py: gzip takes no dictionary")
    dict_ = bench_dictionary(a.dict_kib)

    def loop(datas):
        out = []
        for d in datas:
            p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
            rc = L.df_encode_buffer_dict(kind, 0, d, len(d), dict_, len(dict_), C.byref(p), C.byref(n))
            if rc != 0:
                raise SystemExit("df_encode_buffer_dict: %d" % rc)
            out.append(C.string_at(p, n.value))
            L.bz_free(p)
        return out

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        forms = {"dict": dict_, "plain": b""}
        streams = {f: pkg.deflate_compress_batch(datas, kind, dict_=d) for f, d in forms.items()}   # (warms the engine's workspace too)
        same = streams["dict"] == loop(datas)
        runs = []
        for _ in range(a.runs):
            t = {"dict": [], "plain": [], "loop": []}
            for _ in range(a.calls):
                for f, d in forms.items():
                    t[f].append(timed(lambda: pkg.deflate_compress_batch(datas, kind, dict_=d)))
            for _ in range(a.loops):
                t["loop"].append(timed(lambda: loop(datas)))
            runs.append({k + "_ms": round(statistics.median(v) * 1e3, 2) for k, v in t.items()})
            runs[-1].update({k + "_all_ms": [round(x * 1e3, 2) for x in v] for k, v in t.items()})
        med = {k: statistics.median(r[k + "_ms"] for r in runs) for k in ("dict", "plain", "loop")}
        # the inputs in HBM: the two forms alternating call by call on one engine
        off, buf = [], bytearray()
        for d in datas:
            off.append(len(buf))
            buf += d
            buf += bytes(-len(buf) % 16)
        lens = [len(d) for d in datas]
        tin = torch.frombuffer(buf + bytes(16), dtype=torch.uint8).cuda()
        cap = pkg.deflate_encode_batch_bound(lens)
        o = torch.empty((cap + 64,), dtype=torch.uint8, device="cuda")
        eng = pkg.GpuEngine(0, 1)
        dev = {f: {"wall_ms": [], "stage_ms": []} for f in forms}
        try:
            call = lambda d: eng.deflate_encode_batch_device(kind, tin.data_ptr(), off, lens, o.data_ptr(), cap, dict_=d)
            for d in forms.values():
                call(d)   # (warm)
            for _ in range(a.calls):
                for f, d in forms.items():
                    dev[f]["wall_ms"].append(round(timed(lambda: call(d)) * 1e3, 3))
                    dev[f]["stage_ms"].append({k: round(v * 1e3, 3) for k, v in eng.deflate_timings().items()})
                    dev[f]["batch_stats"] = eng.deflate_batch_stats()
        finally:
            eng.close()
        line = {"mode": "deflate-dict", "kind": a.kind, "workload": name, "dict_kib": a.dict_kib, "inputs": len(datas), "bytes": total,
                "batch_mib": os.environ.get("BZ_DF_BATCH_MIB", "default"), "streams_equal": same,
                "batch_dict_ms": med["dict"], "batch_plain_ms": med["plain"], "loop_dict_ms": med["loop"],
                "loop_over_batch": round(med["loop"] / med["dict"], 2), "dict_over_plain": round(med["dict"] / med["plain"], 2), "runs": runs}
        for f in forms:
            w = dev[f]["wall_ms"]
            line[f] = {"compressed_bytes": sum(len(z) for z in streams[f]), "device_call_ms": statistics.median(w), "device_call_all_ms": w,
                       "device_call_stage_ms": {k: statistics.median(x[k] for x in dev[f]["stage_ms"]) for k in dev[f]["stage_ms"][0]},
                       "device_call_batch_stats": dev[f]["batch_stats"]}
        line["device_dict_over_plain"] = round(line["dict"]["device_call_ms"] / line["plain"]["device_call_ms"], 2)
        print(json.dumps(line), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's streams differ from the loop's")


def inflate_mode(pkg, a, names):
    import zlib
    kind = {"deflate": pkg.DEFLATE, "zlib": pkg.ZLIB, "gzip": pkg.GZIP}[a.kind]
    wbits = {"deflate": -15, "zlib": 15, "gzip": 31}[a.kind]

    def loop(streams, dict_=b""):
        if dict_:
            return [zlib.decompressobj(wbits, zdict=dict_).decompress(z) for z in streams]
        return [zlib.decompress(z, wbits) for z in streams]

    def device_call(streams, dict_=b""):
        """one df_gpu_decode_batch_device call over the streams in HBM: wall time, the launches' times, stats"""
        import torch
        off, buf = [], bytearray()
        for z in streams:
            off.append(len(buf))
            buf += z
            buf += bytes(-len(buf) % 4)
        lens = [len(z) for z in streams]
        t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        eng = pkg.GpuEngine(0, 1)
        kw = {"dict_": dict_} if dict_ else {}
        try:
            o_off, o_len, _ = eng.deflate_decode_batch_device(kind, t.data_ptr(), off, lens, None, 0, **kw)
            cap = max(x + n for x, n in zip(o_off, o_len))
            o = torch.empty((cap + 64,), dtype=torch.uint8, device="cuda")
            eng.deflate_decode_batch_device(kind, t.data_ptr(), off, lens, o.data_ptr(), cap, **kw)   # (warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.deflate_decode_batch_device(kind, t.data_ptr(), off, lens, o.data_ptr(), cap, **kw)
            wall = time.perf_counter() - t0
            tm = eng.deflate_timings()
            stage = {"sizes_launch": tm["hash_chains"], "write_launch": tm["matches"], "checksums": tm["parse"], "total": tm["total"]}
            return {k: round(v * 1e3, 3) for k, v in stage.items()}, eng.deflate_decode_batch_stats(), round(wall * 1e3, 3)
        finally:
            eng.close()

    if a.dict_kib:
        return inflate_dict_mode(pkg, a, names, kind, wbits, loop, device_call)
    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        streams = pkg.deflate_compress_batch(datas, kind)
        batch = pkg.deflate_decompress_batch(streams, kind)      # (warms the engine's workspace too)
        same = batch == [(d, 0) for d in datas] and loop(streams) == datas
        runs = []
        for _ in range(a.runs):
            tb, tl = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                pkg.deflate_decompress_batch(streams, kind)
                tb.append(time.perf_counter() - t0)
            for _ in range(a.loops):
                t0 = time.perf_counter()
                loop(streams)
                tl.append(time.perf_counter() - t0)
            runs.append({"batch_ms": round(statistics.median(tb) * 1e3, 2), "zlib_loop_ms": round(statistics.median(tl) * 1e3, 2),
                         "batch_all_ms": [round(t * 1e3, 2) for t in tb], "zlib_loop_all_ms": [round(t * 1e3, 2) for t in tl]})
        bm = statistics.median(r["batch_ms"] for r in runs)
        lm = statistics.median(r["zlib_loop_ms"] for r in runs)
        stage_ms, stats, wall_ms = device_call(streams)
        print(json.dumps({"mode": "inflate", "kind": a.kind, "workload": name, "streams": len(streams), "bytes": total,
                          "compressed_bytes": sum(len(z) for z in streams), "outputs_equal": same,
                          "batch_ms": bm, "zlib_loop_ms": lm, "zlib_loop_over_batch": round(lm / bm, 2),
                          "batch_GBps": round(total / bm / 1e6, 3), "zlib_loop_GBps": round(total / lm / 1e6, 3),
                          "device_call_ms": wall_ms, "device_call_GBps": round(total / wall_ms / 1e6, 3),
                          "device_call_stage_ms": stage_ms, "device_call_batch_stats": stats, "runs": runs}), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's outputs differ from the inputs")


def bench_dictionary(kib):
    """kib KiB of a chapter of the bench corpus that no workload holds: the same vocabulary, other text"""
    import corpus
    return bytes(corpus.chapter(1, kib * 1024)[:kib * 1024])


def inflate_dict_mode(pkg, a, names, kind, wbits, loop, device_call):
    import zlib
    if kind == pkg.GZIP:
        raise SystemExit("batch_time.py: gzip takes no dictionary")
    dict_ = bench_dictionary(a.dict_kib)
    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        forms = {}
        for form, d in (("dict", dict_), ("plain", b"")):
            streams = []
            for x in datas:
                c = zlib.compressobj(6, zlib.DEFLATED, wbits, zdict=d) if d else zlib.compressobj(6, zlib.DEFLATED, wbits)
                streams.append(c.compress(x) + c.flush())
            forms[form] = (d, streams)
        forms["own_dict"] = (dict_, pkg.deflate_compress_batch(datas, kind, dict_=dict_))
        same = all(pkg.deflate_decompress_batch(z, kind, dict_=d) == [(x, 0) for x in datas] and loop(z, d) == datas for d, z in forms.values())
        times = {form: {"batch": [], "zlib_loop": []} for form in forms}
        for _ in range(a.runs):
            for form, (d, z) in forms.items():      # (alternating the two forms)
                tb, tl = [], []
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    pkg.deflate_decompress_batch(z, kind, dict_=d)
                    tb.append(time.perf_counter() - t0)
                for _ in range(a.loops):
                    t0 = time.perf_counter()
                    loop(z, d)
                    tl.append(time.perf_counter() - t0)
                times[form]["batch"].append(round(statistics.median(tb) * 1e3, 2))
                times[form]["zlib_loop"].append(round(statistics.median(tl) * 1e3, 2))
        line = {"mode": "inflate-dict", "kind": a.kind, "workload": name, "dict_kib": a.dict_kib, "streams": len(datas), "bytes": total,
                "outputs_equal": same}
        for form, (d, z) in forms.items():
            stage_ms, stats, wall_ms = device_call(z, d)
            bm, lm = statistics.median(times[form]["batch"]), statistics.median(times[form]["zlib_loop"])
            line[form] = {"compressed_bytes": sum(len(s) for s in z), "batch_ms": bm, "zlib_loop_ms": lm, "batch_GBps": round(total / bm / 1e6, 3),
                          "zlib_loop_GBps": round(total / lm / 1e6, 3), "batch_runs_ms": times[form]["batch"],
                          "zlib_loop_runs_ms": times[form]["zlib_loop"], "device_call_ms": wall_ms,
                          "device_call_GBps": round(total / wall_ms / 1e6, 3), "device_call_stage_ms": stage_ms, "device_call_batch_stats": stats}
        print(json.dumps(line), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's outputs differ from the inputs")


def inflate_one_mode(pkg, a):
    import zlib
    import torch
    import corpus
    data = corpus.corpus_bytes(int(a.inflate_one * (1 << 20)))
    dict_ = bench_dictionary(a.dict_kib) if a.dict_kib else b""
    kw = {"dict_": dict_} if dict_ else {}
    if dict_ or a.zlib_made:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=dict_) if dict_ else zlib.compressobj(6, zlib.DEFLATED, -15)
        z = c.compress(data) + c.flush()
        unzip = lambda: (zlib.decompressobj(-15, zdict=dict_) if dict_ else zlib.decompressobj(-15)).decompress(z)
    else:
        (z,) = pkg.deflate_compress_batch([data], pkg.DEFLATE)
        unzip = lambda: zlib.decompress(z, -15)
    same = unzip() == data                                                              # (warm)
    tz = []
    for _ in range(3):
        t0 = time.perf_counter()
        unzip()
        tz.append((time.perf_counter() - t0) * 1e3)
    zlib_ms = statistics.median(tz)
    same = same and pkg.deflate_decompress_batch([z], pkg.DEFLATE, **kw) == [(data, 0)]      # (warm)
    th = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        pkg.deflate_decompress_batch([z], pkg.DEFLATE, **kw)
        th.append((time.perf_counter() - t0) * 1e3)
    t = torch.frombuffer(bytearray(z) + bytes(-len(z) % 4 + 4), dtype=torch.uint8).cuda()
    eng = pkg.GpuEngine(0, 1)
    try:
        call = lambda o, cap: eng.deflate_decode_batch_device(pkg.DEFLATE, t.data_ptr(), [0], [len(z)], o, cap, **kw)
        o_off, o_len, _ = call(None, 0)
        o = torch.empty((o_len[0] + 64,), dtype=torch.uint8, device="cuda")
        call(o.data_ptr(), o_len[0])                                                    # (warm)
        td, te, phases = [], [], []
        for _ in range(a.calls):
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()                                      # (hipEvents on the idle device around the synchronous call)
            t0 = time.perf_counter()
            call(o.data_ptr(), o_len[0])
            td.append((time.perf_counter() - t0) * 1e3)
            ev1.record()
            ev1.synchronize()
            te.append(ev0.elapsed_time(ev1))
            phases.append(eng.deflate_decode_split_timings())
        stats = eng.deflate_decode_split_stats()
        same = same and o[:o_len[0]].cpu().numpy().tobytes() == data
        one_wave = None
        if a.one_wave:
            os.environ["BZ_DF_INF_SPLIT_KIB"] = "0"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(o.data_ptr(), o_len[0])
            one_wave = round((time.perf_counter() - t0) * 1e3, 1)
            del os.environ["BZ_DF_INF_SPLIT_KIB"]
    finally:
        eng.close()
    hm, dm = statistics.median(th), statistics.median(td)
    print(json.dumps({"mode": "inflate-one", "bytes": len(data), "compressed_bytes": len(z), "outputs_equal": same, "dict_kib": a.dict_kib,
                      "stream": "zlib level 6" if dict_ or a.zlib_made else "deflate_compress_batch",
                      "split_kib": os.environ.get("BZ_DF_INF_SPLIT_KIB", "default"), "piece_kib": os.environ.get("BZ_DF_INF_PIECE_KIB", "default"),
                      "host_to_host_ms": round(hm, 2), "host_to_host_GBps": round(len(data) / hm / 1e6, 3),
                      "device_call_ms": round(dm, 2), "device_call_GBps": round(len(data) / dm / 1e6, 3),
                      "device_call_all_ms": [round(x, 2) for x in td], "device_call_event_ms": round(statistics.median(te), 2),
                      "phase_ms": {k: round(statistics.median(p[k] for p in phases) * 1e3, 3) for k in phases[0]},
                      "split_stats": stats, "zlib_one_thread_ms": round(zlib_ms, 1), "one_wave_device_call_ms": one_wave}), flush=True)
    if not same:
        raise SystemExit("batch_time.py: the output differs from the input")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deflate", action="store_true", help="time deflate_compress_batch against a loop of df_encode_buffer")
    ap.add_argument("--inflate", action="store_true", help="time deflate_decompress_batch against a loop of zlib.decompress")
    ap.add_argument("--inflate-one", type=float, default=0, metavar="SIZE_MIB", help="time ONE Deflate stream of that many MiB of text")
    ap.add_argument("--one-wave", action="store_true", help="--inflate-one: one more call on the one-wave path")
    ap.add_argument("--zlib-made", action="store_true", help="--inflate-one: the stream is zlib's (level 6), the control of --dict-kib")
    ap.add_argument("--dict-kib", type=int, default=0, metavar="N", help="--deflate / --inflate / --inflate-one: with a preset dictionary of N KiB")
    ap.add_argument("--kind", default="deflate", choices=["deflate", "zlib", "gzip"])
    ap.add_argument("--decode", action="store_true", help="time decompress_batch against a loop of bz_decode_buffer")
    ap.add_argument("--workload", default="all")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--oracle", type=int, default=16, help="inputs the one-thread oracle encodes (0: skip)")
    ap.add_argument("--level", type=int, default=9)
    a = ap.parse_args()
    pkg = importlib.import_module("rust-compression_amd")
    if pkg.device_count() < 1:
        raise SystemExit("batch_time.py: no gfx950 device visible")
    L = pkg.lib()

    def loop(datas):
        out = []
        for d in datas:
            p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
            rc = L.bz_encode_buffer(a.level, 0, d, len(d), C.byref(p), C.byref(n))
            if rc != 0:
                raise SystemExit("bz_encode_buffer: %d" % rc)
            out.append(C.string_at(p, n.value))
            L.bz_free(p)
        return out

    names = ["sample1x256", "corpus16k"] if a.workload == "all" else [a.workload]
    if a.decode:
        return decode_mode(pkg, a, names)
    if a.deflate:
        return deflate_mode(pkg, a, names)
    if a.inflate_one:
        return inflate_one_mode(pkg, a)
    if a.inflate:
        return inflate_mode(pkg, a, names)
    for name in names:
        datas = workload(name)
        total = sum(len(d) for d in datas)
        batch = pkg.compress_batch(datas, a.level)   # (warms the engine's workspace too)
        same = batch == loop(datas)
        t_oracle = None
        if a.oracle:
            from oracle import oracle
            step = max(1, len(datas) // a.oracle)
            sample = datas[::step][:a.oracle]
            t0 = time.perf_counter()
            for d in sample:
                oracle.encode(d, a.level)
            t_oracle = (time.perf_counter() - t0) / sum(len(d) for d in sample) * total
        runs = []
        for _ in range(a.runs):
            tb, tl = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                pkg.compress_batch(datas, a.level)
                tb.append(time.perf_counter() - t0)
            for _ in range(a.loops):
                t0 = time.perf_counter()
                loop(datas)
                tl.append(time.perf_counter() - t0)
            runs.append({"batch_ms": round(statistics.median(tb) * 1e3, 2), "loop_ms": round(statistics.median(tl) * 1e3, 2),
                         "batch_all_ms": [round(t * 1e3, 2) for t in tb], "loop_all_ms": [round(t * 1e3, 2) for t in tl]})
        bm = statistics.median(r["batch_ms"] for r in runs)
        lm = statistics.median(r["loop_ms"] for r in runs)
        print(json.dumps({"workload": name, "inputs": len(datas), "bytes": total, "level": a.level, "streams_equal": same,
                          "batch_ms": bm, "loop_ms": lm, "loop_over_batch": round(lm / bm, 2),
                          "batch_GBps": round(total / bm / 1e6, 3), "loop_GBps": round(total / lm / 1e6, 3),
                          "oracle_one_thread_ms": None if t_oracle is None else round(t_oracle * 1e3, 1),
                          "runs": runs}), flush=True)
        if not same:
            raise SystemExit("batch_time.py: the batch's streams differ from the loop's")


if __name__ == "__main__":
    main()
