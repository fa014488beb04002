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
it is the call's time.  Prints one line of JSON per workload.  Needs a GPU (no fallback)."""
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
    raise SystemExit("unknown workload %s" % name)


def main():
    ap = argparse.ArgumentParser()
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
