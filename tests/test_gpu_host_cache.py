"""The engines the one-shot calls over host buffers keep between calls (round 4: bz_decode_buffer, bz_dec_*,
df_encode_buffer, df_enc_* park ONE engine per device; bz_release_cached_resources frees it).  An engine made by one
kind of call serves the next call of ANOTHER kind -- decode, Deflate, streaming contexts, in any order --, results
are the oracle's every time, and the calling thread's current device is left as it was.
(the reference's src/bzip2/decoder.rs:583-612 and src/deflate/encoder.rs are what the calls stand for; the cache is the
library's own.)"""
import pytest

pytestmark = pytest.mark.gpu


def _text(n, seed):
    import corpus
    return corpus.chapter(seed, max(n, 1 << 16))[:n]


def test_one_shot_calls_share_the_parked_engine(pkg, oracle):
    data = _text(2_500_000, 5) + b"\x00" * 70_000 + _text(300_000, 6)
    z = oracle.encode(data, 9)
    z1 = oracle.encode(data[:400_000], 1)
    df = oracle.deflate_encode(data[:1_200_000], 0)
    for round_ in range(2):
        # decode -> Deflate -> decode (another stream) -> Deflate again: the engine goes from call to call
        back, verdict = pkg.decompress(z)
        assert verdict == 0 and back == data
        assert pkg.deflate_compress(data[:1_200_000], pkg.DEFLATE) == df
        back, verdict = pkg.decompress(z1)
        assert verdict == 0 and back == data[:400_000]
        assert pkg.deflate_compress(data[:1_200_000], pkg.DEFLATE) == df
        # a truncated stream: the bytes in front of the error, then the verdict -- and the engine is still good
        back, verdict = pkg.decompress(z[:len(z) // 2])
        assert verdict != 0 and data.startswith(back)
        back, verdict = pkg.decompress(z)
        assert verdict == 0 and back == data
        # the streaming contexts take the same engine
        dec = pkg.BZip2Decoder()
        assert dec.decode_all(z) == data
        del dec
        enc = pkg.Inflater()
        assert enc.encode_all(data[:1_200_000]) == df
        del enc
        back, verdict = pkg.decompress(z)
        assert verdict == 0 and back == data
        pkg.release_cached_resources()  # ... and the next round starts without one


def test_batch_calls_share_the_parked_engine(pkg, oracle):
    """The four batch forms in the rotation: each borrows an engine through the same lease as the one-shot calls
    (csrc/host_call.h), so a bzip2 decode batch, a Deflate encode batch, a Deflate decode batch and a one-shot decode that
    ends in a data verdict hand the engines on to one another; results are the oracle's streams or the inputs, entry by
    entry, and the calling thread's current device is left as it was.  The 70 000-byte entry is more than one Deflate
    block: the one-input path inside the Deflate batch."""
    import torch
    torch.cuda.set_device(0)
    datas = [b"", b"a", _text(20_000, 3), _text(70_000, 4)]
    bz = [oracle.encode(d, 9) for d in datas]
    gz = [oracle.deflate_encode(d, pkg.GZIP) for d in datas]
    for round_ in range(2):
        assert pkg.compress_batch(datas) == bz
        assert pkg.decompress_batch(bz) == [(d, 0) for d in datas]
        assert pkg.deflate_compress_batch(datas, pkg.GZIP) == gz
        assert pkg.deflate_decompress_batch(gz, pkg.GZIP) == [(d, 0) for d in datas]
        # a truncated stream: a data verdict, and the engine it ran on is still good for the next batch
        back, verdict = pkg.decompress(bz[3][:len(bz[3]) // 2])
        assert verdict != 0 and datas[3].startswith(back)
        assert pkg.decompress_batch(bz) == [(d, 0) for d in datas]
        pkg.release_cached_resources()  # ... and the next round starts without one
    assert torch.cuda.current_device() == 0


def test_decode_buffer_hands_out_memory_free_takes(pkg, oracle):
    """bz_decode_buffer's result lives in posix_memalign'ed memory (2 MiB-aligned, huge pages asked for) from 4 MiB on and
    in malloc'ed memory below: bz_free (= free) takes both; an empty result is a 1-byte allocation."""
    import ctypes as C
    L = pkg.lib()
    for n in (0, 1, 5_000, 6_000_000):
        data = _text(n, 9) if n else b""
        z = oracle.encode(data, 9)
        for _ in range(2):
            outp, outn = C.POINTER(C.c_uint8)(), C.c_size_t(0)
            assert L.bz_decode_buffer(0, z, len(z), C.byref(outp), C.byref(outn)) == 0
            assert outn.value == n and C.string_at(outp, outn.value) == data
            if n >= (4 << 20):
                assert C.addressof(outp.contents) % (2 << 20) == 0
            L.bz_free(outp)
    pkg.release_cached_resources()


def test_peer_copy_selftest_on_the_boxes_devices(pkg):
    """bz_peer_copy_selftest (round 5; bench.py's preflight at N > 1): a list that names the one device twice copies
    nothing (peer_access -1), bad arguments are refused, and the calling thread's current device is left as it was.  (Two
    different devices need a second GPU: the driver's node; the pairs' arithmetic runs under the sanitizers against the HIP
    shim, tests/host_stub/host_pipeline_stress.cpp.)"""
    import ctypes as C
    import torch
    L = pkg.lib()
    torch.cuda.set_device(0)
    devs = (C.c_int * 2)(0, 0)
    peer = (C.c_int * 2)(9, 9)
    ms = (C.c_double * 2)(-2.0, -2.0)
    assert L.bz_peer_copy_selftest(devs, 2, 1 << 20, peer, ms) == 0
    assert list(peer) == [-1, -1] and list(ms) == [0.0, 0.0]
    assert L.bz_peer_copy_selftest(devs, 0, 1 << 20, None, None) == pkg.BZ_E_PARAM
    assert L.bz_peer_copy_selftest((C.c_int * 1)(77), 1, 1 << 20, None, None) == pkg.BZ_E_PARAM
    assert L.bz_peer_copy_selftest(devs, 2, 0, None, None) == pkg.BZ_E_PARAM
    n = torch.cuda.device_count()
    if n >= 2:  # (a multi-GPU box: the real thing, a round trip per neighbour pair)
        devs = (C.c_int * n)(*range(n))
        peer = (C.c_int * n)()
        ms = (C.c_double * n)()
        assert L.bz_peer_copy_selftest(devs, n, 1 << 20, peer, ms) == 0
        assert all(p in (0, 1) for p in peer) and all(t > 0 for t in ms)
    assert torch.cuda.current_device() == 0


def test_streaming_decoder_reads_behind_the_end_wait_for_the_worker(pkg, oracle):
    """Round 5: bz_dec_end returns at once and bz_dec_read waits behind it.  A stream large enough for the worker thread
    (chunks of 4 MiB and more are decoded beside the caller): written in one piece, ended, then read in small pieces until
    the verdict -- every byte, then 0; a corrupted copy: the bytes in front of the error, then the error
    (the reference's src/bzip2/decoder.rs:583-612: the iterator yields exactly that sequence)."""
    import bz2
    import ctypes as C
    data = _text(30_000_000, 11)
    z = bz2.compress(data, 9)
    assert len(z) > (5 << 20)
    L = pkg.lib()
    for corrupt in (False, True):
        zz = bytearray(z)
        if corrupt:
            zz[len(zz) * 3 // 4] ^= 0x55
        want, verdict = oracle.decode(bytes(zz))
        h = C.c_void_p()
        assert L.bz_dec_create(C.byref(h), 0) == 0
        assert L.bz_dec_write(h, bytes(zz), len(zz)) == 0
        rc_end = L.bz_dec_end(h)
        assert rc_end in (0, verdict)
        buf = (C.c_uint8 * (3 << 20))()
        got = bytearray()
        while True:
            k = L.bz_dec_read(h, buf, len(buf))
            if k <= 0:
                break
            got += bytes(buf[:k])
        L.bz_dec_destroy(h)
        assert k == verdict and bytes(got) == want, (corrupt, k, verdict, len(got), len(want))
        assert (verdict == 0) == (not corrupt)


def _stream_through(L, zz, piece=1 << 20, read_cap=3 << 20, read_between=True):
    """the loop a host runs: write in pieces, read what has come between the writes, end, read to the verdict"""
    import ctypes as C
    h = C.c_void_p()
    assert L.bz_dec_create(C.byref(h), 0) == 0
    buf = (C.c_uint8 * read_cap)()
    got = bytearray()
    zb = bytes(zz)
    for i in range(0, len(zb), piece):
        assert L.bz_dec_write(h, zb[i:i + piece], len(zb[i:i + piece])) == 0
        while read_between:
            k = L.bz_dec_read(h, buf, len(buf))
            if k <= 0:
                break
            got += bytes(buf[:k])
    L.bz_dec_end(h)
    while True:
        k = L.bz_dec_read(h, buf, len(buf))
        if k <= 0:
            break
        got += bytes(buf[:k])
    L.bz_dec_destroy(h)
    return bytes(got), k


def test_streaming_decoder_two_lanes(pkg, oracle, monkeypatch):
    """Round 5: chunks of 4 MiB and more go to the context's two lanes -- the next chunk's scan and Huffman stage run
    beside the rebuilding of this chunk's blocks, a lane whose chunk in front ends with an error gives up before it hands
    out a byte.  Several chunks per stream here (BZ_DEC_CHUNK = 4 MiB): a clean stream, two streams in one file with the
    seam inside a chunk, a block corrupted in the second chunk (the third is in flight on the other lane by then), a
    stream cut off in mid-block, a context destroyed with chunks still in flight: the bytes and the verdict of the oracle's
    decoder every time (the reference's src/bzip2/decoder.rs:583-612: bytes in front of an error, then the error)."""
    import ctypes as C
    monkeypatch.setenv("BZ_DEC_CHUNK", str(4 << 20))
    monkeypatch.setenv("BZ_DEC_FIRST_CHUNK", str(4 << 20))
    data = _text(80_000_000, 21)
    z = pkg.compress(data, 9)
    assert len(z) > (14 << 20)  # four chunks at least
    L = pkg.lib()
    # clean, with and without reads between the writes; one lane gives the same
    for between in (True, False):
        got, verdict = _stream_through(L, z, read_between=between)
        assert verdict == 0 and got == data
    monkeypatch.setenv("BZ_DEC_LANES", "1")
    got, verdict = _stream_through(L, z)
    assert verdict == 0 and got == data
    monkeypatch.delenv("BZ_DEC_LANES")
    # two streams, the seam somewhere inside the third chunk
    cut = 40_500_123
    zz = pkg.compress(data[:cut], 9) + pkg.compress(data[cut:], 5)
    got, verdict = _stream_through(L, zz)
    assert verdict == 0 and got == data
    # a block of the second chunk corrupted / the stream cut off inside the third chunk / junk behind the stream
    for name, bad in (("flip", bytes(z[:6 << 20]) + bytes([z[6 << 20] ^ 0x41]) + bytes(z[(6 << 20) + 1:])),
                      ("cut", bytes(z[:(9 << 20) + 12345])),
                      ("junk", bytes(z) + b"\x00" * 5)):
        want, st = oracle.decode(bad)
        assert st != 0, name
        for between in (True, False):
            got, verdict = _stream_through(L, bad, read_between=between)
            assert verdict == st and got == want, (name, between, verdict, st, len(got), len(want))
    # a context that is dropped while its chunks are in flight (nothing read): no hang, the next context is fine
    h = C.c_void_p()
    assert L.bz_dec_create(C.byref(h), 0) == 0
    assert L.bz_dec_write(h, bytes(z), len(z)) == 0
    L.bz_dec_destroy(h)
    got, verdict = _stream_through(L, z[:5 << 20] + z[5 << 20:])
    assert verdict == 0 and got == data


def test_single_call_forms_share_the_parked_engine(pkg, oracle):
    """The eight host-to-host forms that are one upload, one device call and one download (csrc/one_shot.h:
    df_encode_batch_dict, df_bgzf_encode_buffer, df_decode_batch_dict, df_decode_members_buffer, df_bgzf_read_buffer,
    bz_lzh_decode_batch, bz_lzh_encode_batch, bz_lha_read_buffer) back to back on one device: they take turns on the parked
    engine's input and output buffers.  Each form runs with about 64 KiB first, then about 1 KiB, then a result of no bytes,
    so that a byte or a size left over from the larger call would show; each decoder gets one damaged entry between two
    good ones, and the call behind it is as good as the one in front.  Expected bytes: the inputs themselves, zlib and gzip
    of the standard library, tests/lzhref.py, tests/lhaforge.py and tests/bgzfref.py."""
    import gzip
    import zlib

    import bgzfref
    import lhaforge
    import lzhref
    import torch
    torch.cuda.set_device(0)
    big, small = _text(66_001, 31), _text(1_003, 32)
    sizes = (big, small, b"")
    zl = {d: zlib.compress(d, 6) for d in sizes}
    gz = {d: gzip.compress(d[:len(d) // 2]) + b"\0" * 7 + gzip.compress(d[len(d) // 2:]) for d in sizes}  # two members, padding between
    bg = {d: bgzfref.build(oracle, d)[0] for d in sizes}
    lz = {d: lzhref.encode(d, 5) for d in sizes}
    lz_cut = lz[small][:len(lz[small]) // 2]
    lz_cut_want = lzhref.decode(lz_cut, 5, len(small))[:2]
    assert lz_cut_want[1] != 0
    lha = {d: lhaforge.wrap([(d, lz[d]), (small, lz[small])]) for d in sizes}
    lha_bad = lhaforge.wrap([(small, lz[small]), (small, lz_cut), (big, lz[big])])
    pkg.release_cached_resources()
    for round_ in range(2):  # the second round starts on the engine the first one parked
        # -- the encoders: every stream decodes to its input, the BGZF file and the LZHUF streams are the references'
        for d in sizes:
            got = pkg.deflate_compress_batch([d, small, b""], pkg.ZLIB)
            assert [zlib.decompress(s) for s in got] == [d, small, b""]
        assert pkg.deflate_compress_batch([], pkg.ZLIB) == []
        for d in sizes:
            assert pkg.bgzf_compress(d) == bg[d] and gzip.decompress(bg[d]) == d
        for d in sizes:
            assert pkg.lzhuf_compress_batch([d, small, b""], 5) == [lz[d], lz[small], b""]
        assert pkg.lzhuf_compress_batch([], 5) == []
        # -- the decoders, a damaged entry between two good ones in the first call, a clean call behind it
        got = pkg.deflate_decompress_batch([zl[big], zl[small][:len(zl[small]) // 2], zl[small]], pkg.ZLIB)
        assert got[0] == (big, 0) and got[2] == (small, 0) and got[1][1] != 0 and small.startswith(got[1][0])
        for d in sizes:
            assert pkg.deflate_decompress_batch([zl[d], zl[b""]], pkg.ZLIB) == [(d, 0), (b"", 0)]
        assert pkg.deflate_decompress_batch([zl[b""]], pkg.ZLIB) == [(b"", 0)]  # (a device call that yields no byte)
        assert pkg.deflate_decompress_batch([], pkg.ZLIB) == []
        back, verdict = pkg.gzip_decompress_members(gz[big][:len(gz[big]) - 9])
        assert verdict != 0 and big.startswith(back) and len(back) >= len(big) // 2
        for d in sizes:
            assert pkg.gzip_decompress_members(gz[d]) == (d, 0)
        assert pkg.gzip_decompress_members(b"") == (b"", 0)
        for d in (big, small):
            assert pkg.bgzf_read(bg[d], 0, None) == d
            assert pkg.bgzf_read(bg[d], len(d) // 3, 500) == d[len(d) // 3:len(d) // 3 + 500]
            assert pkg.bgzf_read(bg[d], len(d), 10) == b""
        assert pkg.bgzf_read(bg[b""], 0, None) == b""
        got = pkg.lzhuf_decompress_batch([lz[big], lz_cut, lz[small]], 5, [len(big), len(small), len(small)])
        assert got == [(big, 0), lz_cut_want, (small, 0)]
        for d in sizes:
            assert pkg.lzhuf_decompress_batch([lz[d], b""], 5, [len(d), 0]) == [(d, 0), (b"", 0)]
        assert pkg.lzhuf_decompress_batch([], 5) == []
        got = pkg.lha_extract(lha_bad)
        assert got[0] == (small, 0) and got[2] == (big, 0) and got[1][1] != 0
        for d in sizes:
            assert pkg.lha_extract(lha[d]) == [(d, 0), (small, 0)]
        assert pkg.lha_extract(lha[small], []) == []
    pkg.release_cached_resources()
    assert torch.cuda.current_device() == 0
