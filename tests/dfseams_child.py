"""The child process of tests/test_gpu_deflate_seams.py: every case of tests/golden/df_seams.json through the library in
ONE process (BZ_DF_PART_MIB is read once per process).  Run as `python tests/dfseams_child.py`; needs a GPU."""
import hashlib
import json
import os
import sys

import dfseams as S
from dfseams import FINISH, FLUSH, ROOT, RUN, build_dict, build_pieces, load

SMALL = (b"", b"a", b"seam " * 400, bytes(range(256)) * 40)
BATCH = ("H-258", "B-stored-skip2-L8")


def main():
    """Runs every committed case through the library in THIS process (BZ_DF_PART_MIB is read once per process): a
    marker line on stderr in front of each call, one JSON record per case and path on stdout.  Leaves at the first
    exception.  DFSEAMS_DUMP: a directory that takes the bytes of every stream that is not the recorded one."""
    import importlib
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("rust-compression_amd")
    eng = pkg.GpuEngine(0, 1)
    dump = os.environ.get("DFSEAMS_DUMP")
    A = pkg.Action
    acts = {RUN: A.RUN, FLUSH: A.FLUSH, FINISH: A.FINISH}

    def mark(name, path):
        sys.stderr.write("dfseams case %s path %s\n" % (name, path))
        sys.stderr.flush()

    def emit(name, path, outs, want, extra=None):
        rec = {"case": name, "path": path, "streams": [[len(b), hashlib.sha256(b).hexdigest()] for b in outs]}
        if extra:
            rec.update(extra)
        if dump and rec["streams"] != want:
            for i, b in enumerate(outs):
                with open(os.path.join(dump, "%s.%s.%d.bin" % (name, path, i)), "wb") as fh:
                    fh.write(b)
        sys.stdout.write(json.dumps(rec) + "\n")
        sys.stdout.flush()

    def dev(data, kind, dict_):
        n = len(data)
        tin = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
        cap = pkg.deflate_bound(n)
        tout = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        k = eng.deflate_encode_device(kind, tin.data_ptr(), n, tout.data_ptr(), cap, dict_=dict_)
        blocks = eng.deflate_debug_blocks()
        st = eng.deflate_stats()
        return bytes(tout[:k].cpu().numpy()), {"stats": {x: int(st[x]) for x in ("blocks", "stored", "fixed", "dynamic")},
                                               "debug_blocks": [len(blocks), int(sum(int(b[1]) for b in blocks)),
                                                                int(blocks[0][0]) if blocks else 0]}

    def flushed(name, path, case, pieces, dict_):
        mark(name, path)
        enc = pkg.Inflater(dict_=dict_)
        outs = []
        for data, act in pieces:
            enc.write(data)
            enc.end(acts[act])
            outs.append(bytes(enc.read_all()))
        emit(name, path, outs, case["streams"]["pieces"])

    import time
    t_first = None
    cases = load()["cases"]
    for case in cases:
        name = case["name"]
        pieces, dict_ = build_pieces(case), build_dict(case)
        one = len(pieces) == 1 and pieces[0][1] == FINISH
        for cuts in ("beside", "after"):
            if cuts == "after":
                if not S.runs_after(case):
                    continue
                os.environ["BZ_DF_CUTS"] = "after"
            sfx = "" if cuts == "beside" else "-after"
            if one:
                for k in case["kinds"] if cuts == "beside" else case["kinds"][:1]:
                    mark(name, "dev%d%s" % (k, sfx))
                    t0 = time.time()
                    got, extra = dev(pieces[0][0], k, dict_)
                    if t_first is None:
                        t_first = time.time() - t0
                        extra["first_call_s"] = round(t_first, 3)
                    emit(name, "dev%d%s" % (k, sfx), [got], [case["streams"]["kind%d" % k]], extra)
                if cuts == "beside":
                    mark(name, "host0")
                    emit(name, "host0", [pkg.deflate_compress(pieces[0][0], case["kinds"][0], dict_=dict_)],
                         [case["streams"]["kind%d" % case["kinds"][0]]])
            elif pieces[0][1] == RUN:
                for k in case["kinds"] if cuts == "beside" else case["kinds"][:1]:
                    mark(name, "run%d%s" % (k, sfx))
                    cls = {1: pkg.ZlibEncoder, 2: pkg.GZipEncoder}[k]
                    emit(name, "run%d%s" % (k, sfx), [bytes(cls().encode_all(pieces[0][0], A.RUN))],
                         [case["streams"]["run%d" % k]])
            else:
                flushed(name, "inflater" + sfx, case, pieces, dict_)
            os.environ.pop("BZ_DF_CUTS", None)
    # large inputs inside a batch call: two seam cases among small inputs
    by = {c["name"]: c for c in cases}
    datas = [SMALL[0], build_pieces(by[BATCH[0]])[0][0], SMALL[1], SMALL[2], build_pieces(by[BATCH[1]])[0][0], SMALL[3]]
    mark("batch", "batch")
    outs = pkg.deflate_compress_batch(datas, pkg.DEFLATE)
    emit("batch", "batch", [bytes(b) for b in outs], None)
    eng.close()
    sys.stdout.write(json.dumps({"case": "done", "path": "done"}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
