"""Timing of bz_gpu_lha_write_device against bz_gpu_lzh_encode_batch_device on 4 096 pages of 16 KiB, the host forms, and one
64 MiB member; every archive is read back and compared (profiles/r33_lha_write.md).
usage: python tools/lha_write_time.py [--trace]      (--trace: warm calls and one call per form only, for a kernel trace)"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import lzhshapes  # noqa: E402

pkg = importlib.import_module("rust-compression_amd")
TRACE = "--trace" in sys.argv
PAGE, NPAGES = 16384, 4096


def sync():
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    r = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    t0 = time.perf_counter()
    text = lzhshapes.gen_text(99, 8 << 20)
    stride = (len(text) - PAGE) // (NPAGES - 1)
    pages = [text[k * stride:k * stride + PAGE] for k in range(NPAGES)]
    print("pages: %d of %d bytes, slices of gen_text(99, 8 MiB) at stride %d (%.1f s to make)" % (NPAGES, PAGE, stride, time.perf_counter() - t0), flush=True)
    d_in = torch.frombuffer(bytearray(b"".join(pages)), dtype=torch.uint8).cuda()
    offs = [k * PAGE for k in range(NPAGES)]
    lens = [PAGE] * NPAGES
    names = [b"page%04d.txt" % k for k in range(NPAGES)]
    eng = pkg.GpuEngine(0, 1)
    cap_e = pkg.lzhuf_encode_batch_bound(lens)
    cap_w = pkg.lha_write_bound(names, lens, 2)
    d_e = torch.empty(cap_e + 64, dtype=torch.uint8, device="cuda")
    d_w = torch.empty(cap_w + 64, dtype=torch.uint8, device="cuda")

    def enc(m):
        return eng.lzh_encode_batch_device(m, d_in.data_ptr(), offs, lens, d_e.data_ptr(), cap_e)

    def wr(m):
        return eng.lha_write_device(d_in.data_ptr(), offs, lens, names, d_w.data_ptr(), cap_w, m, 2)

    # the timed forms: the C calls with their arrays made once (the wrappers build 4 096 records per call)
    import ctypes as C
    recs, keep = pkg._lha_entries(names)
    a_off, a_len = (C.c_uint64 * NPAGES)(*offs), (C.c_uint64 * NPAGES)(*lens)
    o_off_, o_len_ = (C.c_uint64 * NPAGES)(), (C.c_uint64 * NPAGES)()
    table, n_out = (pkg._LhaMemberRec * NPAGES)(), C.c_size_t(0)
    L = pkg.lib()

    def enc_c(m):
        assert L.bz_gpu_lzh_encode_batch_device(eng._h, m, d_in.data_ptr(), a_off, a_len, NPAGES, d_e.data_ptr(), cap_e, o_off_, o_len_) == 0

    def wr_c(m):
        assert L.bz_gpu_lha_write_device(eng._h, m, 2, d_in.data_ptr(), a_off, a_len, recs, NPAGES, d_w.data_ptr(), cap_w, C.byref(n_out), table) == 0
        return n_out.value, None

    for m in (5, 7):       # warm, and the archive read back on the device once
        enc(m)
        n, idx = wr(m)
        st = eng.lha_write_stats()
        need = NPAGES * PAGE + 16
        back = torch.empty(need, dtype=torch.uint8, device="cuda")
        o_off, o_len, ver = eng.lha_read_device(d_w.data_ptr(), n, idx, back.data_ptr(), need)
        sync()
        ok = ver == [0] * NPAGES and o_len == lens and bool(torch.equal(back[:NPAGES * PAGE], d_in))
        print("lh%d: archive %d bytes, stats %s, read back clean and equal: %s" % (m, n, st, ok), flush=True)
        assert ok
    if TRACE:
        for m in (5, 7):
            enc_c(m)
            wr_c(m)
        sync()
        return
    for run in range(3):
        for m in (5, 7):
            te, _ = timed(lambda: enc_c(m))
            tw, _ = timed(lambda: wr_c(m))
            print("run %d lh%d: encode_batch_device %.3f ms, lha_write_device %.3f ms (+%.3f)" % (run + 1, m, te, tw, tw - te), flush=True)
    # stored by request: CRC and layout alone
    for run in range(3):
        tw, (n, _) = timed(lambda: wr_c(0))
        print("run %d stored: lha_write_device %.3f ms (%d bytes)" % (run + 1, tw, n), flush=True)
    # ---- host to host: one call against a loop over the members
    for run in range(3):
        t0 = time.perf_counter()
        arc = pkg.lha_compress(list(zip(names, pages)), 5, 2)
        t1 = time.perf_counter()
        streams = pkg.lzhuf_compress_batch(pages, pkg.LzhufMethod.Lh5)
        t2 = time.perf_counter()
        print("run %d host to host lh5: lha_compress %.1f ms (%d bytes), lzhuf_compress_batch %.1f ms" % (run + 1, (t1 - t0) * 1e3, len(arc), (t2 - t1) * 1e3), flush=True)
    got = pkg.lha_extract(arc)
    assert [b for b, _ in got] == pages and all(v == 0 for _, v in got)
    idx = pkg.lha_index(arc)
    assert [arc[m.data_off:m.data_off + m.packed_len] for m in idx] == streams
    print("host archive: extracts clean, member data equal to lzhuf_compress_batch's streams", flush=True)
    t0 = time.perf_counter()
    for p in pages[:128]:
        pkg.lzhuf_compress(p, pkg.LzhufMethod.Lh5)
    per = (time.perf_counter() - t0) / 128
    print("loop of bz_lzh_encode_buffer: %.2f ms per member over 128 members (%.1f s extrapolated to 4 096)" % (per * 1e3, per * NPAGES), flush=True)
    # ---- one 64 MiB text member
    big = (text * 8)[:64 << 20]
    d_big = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()
    cap_b = pkg.lha_write_bound([b"big.txt"], [len(big)], 2)
    cap_be = pkg.lzhuf_encode_batch_bound([len(big)])
    d_bw = torch.empty(cap_b + 64, dtype=torch.uint8, device="cuda")
    d_be = torch.empty(cap_be + 64, dtype=torch.uint8, device="cuda")
    for run in range(3):
        te, _ = timed(lambda: eng.lzh_encode_batch_device(5, d_big.data_ptr(), [0], [len(big)], d_be.data_ptr(), cap_be))
        tw, (n, idx) = timed(lambda: eng.lha_write_device(d_big.data_ptr(), [0], [len(big)], [b"big.txt"], d_bw.data_ptr(), cap_b, 5, 2))
        print("run %d one 64 MiB member lh5: encode %.2f ms, write %.2f ms (%d bytes)" % (run + 1, te, tw, n), flush=True)
    back = torch.empty(len(big) + 16, dtype=torch.uint8, device="cuda")
    o_off, o_len, ver = eng.lha_read_device(d_bw.data_ptr(), n, idx, back.data_ptr(), len(big) + 16)
    sync()
    print("64 MiB member read back: verdict %s, equal %s" % (ver, bool(torch.equal(back[:len(big)], d_big))), flush=True)
    tw, (n, idx) = timed(lambda: eng.lha_write_device(d_big.data_ptr(), [0], [len(big)], [b"big.txt"], d_bw.data_ptr(), cap_b, 0, 1))
    o_off, o_len, ver = eng.lha_read_device(d_bw.data_ptr(), n, idx, back.data_ptr(), len(big) + 16)
    sync()
    print("64 MiB member stored: write %.2f ms, read back verdict %s, equal %s" % (tw, ver, bool(torch.equal(back[:len(big)], d_big))), flush=True)
    eng.close()


main()
