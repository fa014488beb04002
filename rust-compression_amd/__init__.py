"""rust-compression_amd -- MI355X-native BZip2 block-encode path (and its inverse, the decode path).

Host-side mirror (Python flavour) of the reference's interface for this one path:

    reference (Rust)                                   here
    ------------------------------------------------   ---------------------------------------
    Action::{Run,Flush,Finish}   src/action.rs:8-13    Action.RUN / FLUSH / FINISH
    CompressionError             src/error.rs:10-15    CompressionError(kind)
    BZip2Encoder::new(level)     bzip2/encoder.rs:58   BZip2Encoder(level)   (ValueError = the panic)
    Encoder::next(iter, action)  traits/encoder.rs:81  BZip2Encoder.next(iter, action) -> int | None
    iter.encode(&mut enc, act)   traits/encoder.rs:12  encode(iterable, enc, action) -> iterator of ints
    BZip2Error                   bzip2/error.rs:5-11   BZip2Error(kind)  (a CompressionError, bzip2/error.rs:45-53)
    BZip2Decoder::new()          bzip2/decoder.rs:588  BZip2Decoder()
    Decoder::next(iter)          traits/decoder.rs:95  BZip2Decoder.next(iter) -> int | None, raises BZip2Error
    Deflater / ZlibDecoder / GZipDecoder               Deflater() / ZlibDecoder() / GZipDecoder(): .next(iter), .decode_all(data)
    (every member of a gzip file: no counterpart)      MultiGZipDecoder(), gzip_decompress_members(data)
    iter.decode(&mut dec)        traits/decoder.rs:15  decode(iterable, dec) -> iterator of ints

Everything below the iterator plumbing happens in the HIP library (csrc/, C ABI in
include/bz2_mi355x.h) loaded with ctypes.  There is no CPU implementation in this package: if the
library or a gfx950 device is missing, calls raise.  PyTorch is used only by GpuEngine's callers
for device memory (tensor.data_ptr()); nothing here imports torch.
"""
import collections
import ctypes as C
import enum
import os
import sys

from . import _build

__all__ = ["Action", "CompressionError", "BZip2Error", "BZip2Encoder", "BZip2Decoder", "encode", "decode",
           "compress", "compress_batch", "encode_batch_bound", "decompress", "decompress_batch", "deflate_decompress", "deflate_decompress_batch", "Deflater", "ZlibDecoder", "GZipDecoder", "gzip_decompress_members", "MultiGZipDecoder", "bgzf_compress", "bgzf_bound", "bgzf_block_count", "BgzfIndex", "bgzf_index", "bgzf_decompress", "bgzf_read", "LzhufMethod", "LzhufDecoder", "lzhuf_decompress", "lzhuf_decompress_batch", "LzhufEncoder", "lha_index", "lha_extract", "LhaArchive", "LhaIndex", "LhaMember", "LhaEntry", "LHA_STORED", "lha_write_bound", "lha_compress", "lzhuf_compress", "lzhuf_compress_batch", "lzhuf_encode_batch_bound", "GpuEngine", "release_cached_resources", "last_call_phases",
           "build", "lib", "device_count", "encode_bound", "shard_window", "rccl_lib", "rccl_unique_id", "RcclComm"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

BZ_OK, BZ_E_DATA, BZ_E_EOF, BZ_E_UNEXPECTED = 0, -1, -2, -3
BZ_E_MAGIC_FIRST, BZ_E_MAGIC = -4, -5
BZ_E_PARAM, BZ_E_NOGPU, BZ_E_NOMEM, BZ_E_CAPACITY = -6, -7, -8, -9


class Action(enum.IntEnum):
    """src/action.rs:8-13"""
    RUN = 0
    FLUSH = 1
    FINISH = 2


class CompressionError(Exception):
    """src/error.rs:10-15 (kinds DataError / UnexpectedEof / Unexpected) + this library's own."""
    KINDS = {BZ_E_DATA: "DataError", BZ_E_EOF: "UnexpectedEof", BZ_E_UNEXPECTED: "Unexpected",
             BZ_E_NOGPU: "NoGpu", BZ_E_NOMEM: "NoMemory", BZ_E_CAPACITY: "Capacity", BZ_E_PARAM: "Param"}

    def __init__(self, code):
        self.code = code
        self.kind = self.KINDS.get(code, "Unexpected")
        msg = lib().bz_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__("%s (%d): %s" % (self.kind, code, msg))


class BZip2Error(CompressionError):
    """src/bzip2/error.rs:5-11.  `kind` is the BZip2Error variant; as a CompressionError the two
    magic variants are DataError (bzip2/error.rs:45-53)."""
    BZ_KINDS = {BZ_E_DATA: "DataError", BZ_E_MAGIC_FIRST: "DataErrorMagicFirst", BZ_E_MAGIC: "DataErrorMagic",
                BZ_E_EOF: "UnexpectedEof", BZ_E_UNEXPECTED: "Unexpected"}

    def __init__(self, code, partial=b""):
        super().__init__(code)
        self.bzip2_kind = self.BZ_KINDS.get(code, "Unexpected")
        if code in (BZ_E_MAGIC_FIRST, BZ_E_MAGIC):
            self.kind = "DataError"
        self.partial = partial  # bytes the iterator yielded before this Err


def build(force=False):
    """Compile csrc/*.hip for gfx950 into rust-compression_amd/libbz2_mi355x.so (in-tree)."""
    return _build.build(force=force)


EXPORTS = [
    "bz_strerror", "bz_version", "bz_device_count",
    "bz_enc_create", "bz_enc_write", "bz_enc_end", "bz_enc_read", "bz_enc_pending", "bz_enc_destroy",
    "bz_encode_buffer", "bz_encode_batch", "bz_encode_batch_bound", "bz_gpu_encode_batch_device", "bz_gpu_last_batch_stats",
    "bz_free", "bz_enc_create_multi", "bz_enc_set_verify", "bz_enc_verify_stats", "bz_enc_phase_stats", "bz_encode_buffer_last_phases",
    "bz_gpu_engine_set_verify", "bz_gpu_verify_stats", "bz_encode_buffer_multi", "bz_release_cached_resources", "bz_peer_copy_selftest",
    "bz_gpu_engine_create", "bz_gpu_engine_destroy", "bz_gpu_engine_reserve", "bz_encode_bound", "bz_gpu_encode_device",
    "bz_gpu_partition", "bz_gpu_partition_slab_begin", "bz_gpu_partition_slab_count",
    "bz_gpu_partition_slab_finish", "bz_gpu_block_count", "bz_gpu_encode_blocks", "bz_gpu_assemble", "bz_gpu_encode_sharded",
    "bz_shard_comm_selftest", "bz_gpu_last_timings", "bz_shard_halo_bytes", "bz_shard_window", "bz_shard_slab_tiles", "bz_gpu_encode_sharded_window", "bz_gpu_last_shard_timings", "bz_gpu_last_shard_phases",
    "bz_gpu_last_bwt_stats", "bz_gpu_cut_stats", "bz_gpu_last_bwt_rounds", "bz_gpu_profile_enable", "bz_gpu_profile_kernels", "bz_gpu_profile_get",
    "bz_gpu_debug_bwt", "bz_gpu_debug_mtf", "bz_gpu_debug_code_lengths", "bz_gpu_debug_block_stats", "bz_gpu_debug_block_sections",
    "bz_gpu_decode_device", "bz_gpu_decode_device_sharded", "bz_gpu_last_decode_timings", "bz_gpu_last_decode_stats", "bz_decode_buffer",
    "bz_gpu_decode_batch_device", "bz_gpu_last_decode_batch_stats", "bz_decode_batch",
    "bz_dec_create", "bz_dec_write", "bz_dec_end", "bz_dec_read", "bz_dec_pending", "bz_dec_destroy",
    "df_encode_bound", "df_gpu_encode_device", "df_gpu_last_timings", "df_gpu_last_stats", "df_gpu_debug_codes",
    "df_gpu_debug_blocks", "df_encode_buffer", "df_gpu_encode_device_dict", "df_encode_buffer_dict", "df_enc_create_dict",
    "df_enc_create", "df_enc_write", "df_enc_end", "df_enc_read", "df_enc_pending", "df_enc_destroy", "df_enc_finished",
    "df_encode_batch_bound", "df_gpu_encode_batch_device", "df_gpu_last_batch_stats", "df_encode_batch",
    "df_gpu_encode_batch_device_dict", "df_encode_batch_dict",
    "df_gpu_decode_batch_device", "df_gpu_last_decode_batch_stats", "df_gpu_last_decode_split_stats", "df_gpu_last_decode_split_timings", "df_decode_batch", "df_decode_buffer",
    "df_gpu_decode_batch_device_dict", "df_decode_batch_dict", "df_decode_buffer_dict",
    "df_gpu_decode_members_device", "df_gpu_last_decode_members_stats", "df_gpu_last_decode_members_timings", "df_decode_members_buffer",
    "df_bgzf_block_count", "df_bgzf_bound", "df_gpu_bgzf_encode_device", "df_gpu_last_bgzf_stats", "df_bgzf_encode_buffer",
    "df_bgzf_index_buffer", "df_gpu_bgzf_index_device", "df_gpu_bgzf_read_device", "df_gpu_last_bgzf_read_stats", "df_bgzf_read_buffer",
    "bz_gpu_lzh_decode_batch_device", "bz_gpu_last_lzh_decode_stats", "bz_lzh_decode_batch", "bz_lzh_decode_buffer",
    "bz_gpu_last_lzh_decode_split_stats", "bz_gpu_last_lzh_decode_split_timings",
    "bz_gpu_lzh_encode_batch_device", "bz_gpu_last_lzh_encode_stats", "bz_lzh_encode_batch_bound", "bz_lzh_encode_batch",
    "bz_lzh_encode_buffer", "bz_gpu_lzh_debug_codes", "bz_gpu_lzh_debug_tables",
    "bz_lha_index_buffer", "bz_gpu_lha_read_device", "bz_gpu_last_lha_read_stats", "bz_lha_read_buffer",
    "bz_lha_write_bound", "bz_gpu_lha_write_device", "bz_gpu_last_lha_write_stats", "bz_lha_write_buffer",
]


# int (*bz_allgather_fn)(void *ctx, const void *send, size_t bytes, void *recv)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so.7.  Two HIP runtimes in one process do not
    work (the second sees no GPU), so when torch is installed its copy is loaded first and this
    library binds to it by soname.  torch itself is NOT imported."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the HIP library (never falls back to anything else)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(_HERE, "libbz2_mi355x.so")
    if not os.path.exists(so):
        so = build()
    _share_hip_runtime_with_torch()
    L = C.CDLL(so)
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.bz_strerror.restype = C.c_char_p
    L.bz_strerror.argtypes = [C.c_int]
    L.bz_version.restype = C.c_char_p
    L.bz_device_count.restype = C.c_int
    L.bz_enc_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.bz_enc_write.argtypes = [vp, C.c_char_p, sz]
    L.bz_enc_end.argtypes = [vp, C.c_int]
    L.bz_enc_read.restype = C.c_long
    L.bz_enc_read.argtypes = [vp, u8p, sz]
    L.bz_enc_pending.restype = sz
    L.bz_enc_pending.argtypes = [vp]
    L.bz_enc_destroy.restype = None
    L.bz_enc_destroy.argtypes = [vp]
    L.bz_encode_buffer.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.bz_encode_batch.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.POINTER(u8p), u64p, u64p]
    L.bz_encode_batch_bound.restype = sz
    L.bz_encode_batch_bound.argtypes = [u64p, sz]
    L.bz_gpu_encode_batch_device.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, vp, sz, u64p, u64p]
    L.bz_gpu_last_batch_stats.argtypes = [vp, u64p]
    L.bz_enc_create_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.c_int]
    L.bz_encode_buffer_multi.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.bz_enc_phase_stats.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_encode_buffer_last_phases.argtypes = [C.POINTER(C.c_double)]
    L.bz_enc_set_verify.argtypes = [vp, C.c_int]
    L.bz_enc_verify_stats.argtypes = [vp, u64p]
    L.bz_gpu_engine_set_verify.argtypes = [vp, C.c_int]
    L.bz_gpu_verify_stats.argtypes = [vp, u64p]
    L.bz_release_cached_resources.restype = None
    L.bz_release_cached_resources.argtypes = []
    L.bz_peer_copy_selftest.argtypes = [C.POINTER(C.c_int), C.c_int, sz, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.bz_free.restype = None
    L.bz_free.argtypes = [vp]
    L.bz_gpu_engine_create.argtypes = [C.POINTER(vp), C.c_int, sz]
    L.bz_gpu_engine_reserve.argtypes = [vp, sz]
    L.bz_gpu_engine_destroy.restype = None
    L.bz_gpu_engine_destroy.argtypes = [vp]
    L.bz_encode_bound.restype = sz
    L.bz_encode_bound.argtypes = [sz]
    L.bz_gpu_encode_device.argtypes = [vp, C.c_int, vp, sz, vp, sz, szp]
    L.bz_gpu_partition.argtypes = [vp, C.c_int, vp, sz, C.c_int, szp, szp, C.POINTER(C.c_int)]
    L.bz_gpu_partition_slab_begin.argtypes = [vp, C.c_int, vp, sz, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64)]
    L.bz_gpu_partition_slab_count.argtypes = [vp, C.c_int64]
    L.bz_gpu_partition_slab_finish.argtypes = [vp, C.c_uint64, C.c_int, szp, u64p, C.POINTER(C.c_int)]
    L.bz_gpu_block_count.restype = sz
    L.bz_gpu_block_count.argtypes = [vp]
    L.bz_gpu_encode_blocks.argtypes = [vp, sz, sz, vp, sz, u64p, u64p, u32p, szp]
    L.bz_gpu_assemble.argtypes = [vp, C.c_int, sz, vp, u64p, u64p, u32p, C.c_int, C.c_int, C.c_int,
                                  C.c_uint, C.c_uint, C.c_uint32, u32p, vp, sz, szp,
                                  C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.bz_gpu_encode_sharded.argtypes = [vp, C.c_int, vp, sz, vp, vp, sz, vp, sz, vp, sz, szp]
    L.bz_shard_halo_bytes.restype = sz
    L.bz_shard_halo_bytes.argtypes = [C.c_int]
    L.bz_shard_window.argtypes = [C.c_int, sz, C.c_int, C.c_int, u64p, szp]
    L.bz_shard_slab_tiles.argtypes = [sz, C.c_int, C.c_int, u64p, u64p]
    L.bz_gpu_encode_sharded_window.argtypes = [vp, C.c_int, vp, C.c_uint64, sz, sz, vp, vp, sz, vp, sz, vp, sz, szp]
    L.bz_gpu_last_shard_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_gpu_last_shard_phases.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_shard_comm_selftest.argtypes = [vp, C.c_int]
    L.bz_gpu_last_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_gpu_last_bwt_stats.argtypes = [vp, u64p]
    L.bz_gpu_last_bwt_rounds.argtypes = [vp, u64p]
    L.bz_gpu_cut_stats.argtypes = [vp, u64p]
    L.bz_gpu_profile_enable.argtypes = [vp, C.c_int]
    L.bz_gpu_profile_kernels.argtypes = [vp]
    L.bz_gpu_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), u64p, C.POINTER(C.c_double), u64p]
    L.bz_gpu_debug_bwt.argtypes = [vp, C.c_char_p, sz, u32p]
    L.bz_gpu_debug_mtf.argtypes = [vp, sz, C.c_char_p, u64p, u32p, C.c_int, C.POINTER(C.c_uint16), sz, u32p, u32p, u32p]
    L.bz_gpu_debug_code_lengths.argtypes = [vp, u32p, sz, u8p, C.POINTER(C.c_int)]
    L.bz_gpu_debug_block_stats.argtypes = [vp, u32p, sz, szp]
    L.bz_gpu_debug_block_sections.argtypes = [vp, u32p, sz, szp]
    L.bz_gpu_decode_device.argtypes = [vp, vp, sz, vp, sz, szp]
    L.bz_gpu_decode_device_sharded.argtypes = [vp, vp, sz, vp, sz, C.c_int, C.c_int, ALLGATHER_FN, vp, szp, szp, szp]
    L.bz_gpu_last_decode_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_gpu_last_decode_stats.argtypes = [vp, u64p]
    L.bz_decode_buffer.argtypes = [C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    i32p = C.POINTER(C.c_int32)
    L.bz_gpu_decode_batch_device.argtypes = [vp, vp, u64p, u64p, sz, vp, sz, u64p, u64p, i32p]
    L.bz_gpu_last_decode_batch_stats.argtypes = [vp, u64p]
    L.bz_decode_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), szp, sz, C.POINTER(u8p), u64p, u64p, i32p]
    L.bz_dec_create.argtypes = [C.POINTER(vp), C.c_int]
    L.bz_dec_write.argtypes = [vp, C.c_char_p, sz]
    L.bz_dec_end.argtypes = [vp]
    L.bz_dec_read.restype = C.c_long
    L.bz_dec_read.argtypes = [vp, u8p, sz]
    L.bz_dec_pending.restype = sz
    L.bz_dec_pending.argtypes = [vp]
    L.bz_dec_destroy.restype = None
    L.bz_dec_destroy.argtypes = [vp]
    L.df_encode_bound.restype = sz
    L.df_encode_bound.argtypes = [sz]
    L.df_gpu_encode_device.argtypes = [vp, C.c_int, vp, sz, vp, sz, szp]
    L.df_gpu_last_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.df_gpu_last_stats.argtypes = [vp, u64p]
    L.df_gpu_debug_codes.argtypes = [vp, vp, sz, u32p, sz, szp]
    L.df_gpu_debug_blocks.argtypes = [vp, u64p, sz, szp]
    L.df_encode_buffer.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.df_gpu_encode_device_dict.argtypes = [vp, C.c_int, vp, sz, C.c_char_p, sz, vp, sz, szp]
    L.df_encode_buffer_dict.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.df_enc_create_dict.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_char_p, sz]
    L.df_enc_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.df_enc_write.argtypes = [vp, C.c_char_p, sz]
    L.df_enc_end.argtypes = [vp, C.c_int]
    L.df_enc_finished.argtypes = [vp]
    L.df_enc_read.restype = C.c_long
    L.df_enc_read.argtypes = [vp, u8p, sz]
    L.df_enc_pending.restype = sz
    L.df_enc_pending.argtypes = [vp]
    L.df_enc_destroy.restype = None
    L.df_enc_destroy.argtypes = [vp]
    L.df_encode_batch_bound.restype = sz
    L.df_encode_batch_bound.argtypes = [u64p, sz]
    L.df_gpu_encode_batch_device.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, vp, sz, u64p, u64p]
    L.df_gpu_last_batch_stats.argtypes = [vp, u64p]
    L.df_encode_batch.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.POINTER(u8p), u64p, u64p]
    L.df_gpu_encode_batch_device_dict.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, C.c_char_p, sz, vp, sz, u64p, u64p]
    L.df_encode_batch_dict.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.c_char_p, sz, C.POINTER(u8p), u64p, u64p]
    L.df_gpu_decode_batch_device.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, vp, sz, u64p, u64p, i32p]
    L.df_gpu_last_decode_batch_stats.argtypes = [vp, u64p]
    L.df_gpu_last_decode_split_stats.argtypes = [vp, u64p]
    L.df_gpu_last_decode_split_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.df_decode_batch.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.POINTER(u8p), u64p, u64p, i32p]
    L.df_gpu_decode_members_device.argtypes = [vp, vp, sz, vp, sz, u64p, i32p]
    L.df_gpu_last_decode_members_stats.argtypes = [vp, u64p]
    L.df_gpu_last_decode_members_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.df_decode_members_buffer.argtypes = [C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.df_bgzf_block_count.restype = sz
    L.df_bgzf_block_count.argtypes = [sz, C.c_uint32]
    L.df_bgzf_bound.restype = sz
    L.df_bgzf_bound.argtypes = [sz, C.c_uint32, C.c_int]
    L.df_gpu_bgzf_encode_device.argtypes = [vp, vp, sz, C.c_uint32, C.c_int, vp, sz, u64p, u64p]
    L.df_gpu_last_bgzf_stats.argtypes = [vp, u64p]
    L.df_bgzf_encode_buffer.argtypes = [C.c_int, C.c_char_p, sz, C.c_uint32, C.c_int, C.POINTER(u8p), szp, u64p]
    L.df_bgzf_index_buffer.argtypes = [C.c_char_p, sz, C.POINTER(u64p), C.POINTER(u64p), szp, i32p]
    L.df_gpu_bgzf_index_device.argtypes = [vp, vp, sz, u64p, u64p, sz, szp, i32p]
    L.df_gpu_bgzf_read_device.argtypes = [vp, vp, sz, u64p, u64p, sz, C.c_uint64, C.c_uint64, vp, sz, u64p, i32p]
    L.df_gpu_last_bgzf_read_stats.argtypes = [vp, u64p]
    L.df_bgzf_read_buffer.argtypes = [C.c_int, C.c_char_p, sz, C.c_uint64, C.c_uint64, C.POINTER(u8p), szp]
    L.df_decode_buffer.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.df_gpu_decode_batch_device_dict.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, C.c_char_p, sz, vp, sz, u64p, u64p, i32p]
    L.df_decode_batch_dict.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.c_char_p, sz, C.POINTER(u8p), u64p, u64p, i32p]
    L.df_decode_buffer_dict.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.bz_gpu_lzh_decode_batch_device.argtypes = [vp, C.c_int, C.c_int, vp, u64p, u64p, u64p, sz, vp, sz, u64p, u64p, i32p]
    L.bz_gpu_last_lzh_decode_stats.argtypes = [vp, u64p]
    L.bz_gpu_last_lzh_decode_split_stats.argtypes = [vp, u64p]
    L.bz_gpu_last_lzh_decode_split_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.bz_lzh_decode_batch.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, u64p, sz, C.POINTER(u8p), u64p, u64p, i32p]
    L.bz_lzh_decode_buffer.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, sz, C.c_uint64, C.POINTER(u8p), szp]
    L.bz_gpu_lzh_encode_batch_device.argtypes = [vp, C.c_int, vp, u64p, u64p, sz, vp, sz, u64p, u64p]
    L.bz_gpu_last_lzh_encode_stats.argtypes = [vp, u64p]
    L.bz_lzh_encode_batch_bound.argtypes = [u64p, sz]
    L.bz_lzh_encode_batch_bound.restype = sz
    L.bz_lzh_encode_batch.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, sz, C.POINTER(u8p), u64p, u64p]
    L.bz_lzh_encode_buffer.argtypes = [C.c_int, C.c_int, C.c_char_p, sz, C.POINTER(u8p), szp]
    L.bz_gpu_lzh_debug_codes.argtypes = [vp, C.c_int, vp, sz, C.POINTER(C.c_uint32), sz, szp]
    L.bz_gpu_lzh_debug_tables.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u8p, u8p, u8p, C.POINTER(C.c_uint32)]
    L.bz_lha_index_buffer.argtypes = [C.c_char_p, sz, vp, sz, szp, i32p, u64p]
    L.bz_gpu_lha_read_device.argtypes = [vp, vp, sz, vp, sz, szp, sz, C.c_int, vp, sz, u64p, u64p, i32p]
    L.bz_gpu_last_lha_read_stats.argtypes = [vp, u64p]
    L.bz_lha_read_buffer.argtypes = [C.c_int, C.c_char_p, sz, szp, sz, C.c_int, C.POINTER(u8p), u64p, u64p, i32p, i32p]
    L.bz_lha_write_bound.argtypes = [C.c_int, vp, u64p, sz]
    L.bz_lha_write_bound.restype = sz
    L.bz_gpu_lha_write_device.argtypes = [vp, C.c_int, C.c_int, vp, u64p, u64p, vp, sz, vp, sz, szp, vp]
    L.bz_gpu_last_lha_write_stats.argtypes = [vp, u64p]
    L.bz_lha_write_buffer.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), szp, vp, sz, C.POINTER(u8p), szp]
    _LIB = L
    return L


def _check(rc):
    if rc != BZ_OK:
        raise CompressionError(rc)


def _settle():
    """Before a device-pointer call: an engine runs on its own HIP stream, the pointers handed in here usually
    belong to torch tensors whose contents (or whose memory, with torch's stream-ordered allocator) may still be
    in use by work queued on torch's streams.  Waits for that work (include/bz2_mi355x.h, "Stream ordering")."""
    t = sys.modules.get("torch")
    if t is not None and t.cuda.is_available() and t.cuda.is_initialized():
        t.cuda.synchronize()


_RCCL_LIB = None
RCCL_EXPORTS = ["bz_rccl_unique_id", "bz_rccl_comm_create", "bz_rccl_comm_destroy", "bz_rccl_comm_count"]


def rccl_lib():
    """The RCCL transport library (libbz2_mi355x_rccl.so, csrc/rccl_comm.hip): only it links librccl.  When
    torch is installed its bundled librccl is loaded first, so that the process has ONE RCCL."""
    global _RCCL_LIB
    if _RCCL_LIB is not None:
        return _RCCL_LIB
    lib()
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
    so = _build.build_rccl()  # (a no-op when the library is newer than its source)
    L = C.CDLL(so)
    L.bz_rccl_unique_id.argtypes = [C.c_char_p]
    L.bz_rccl_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.bz_rccl_comm_destroy.restype = None
    L.bz_rccl_comm_destroy.argtypes = [C.c_void_p]
    L.bz_rccl_comm_count.argtypes = [C.c_void_p]
    _RCCL_LIB = L
    return L


def rccl_unique_id():
    """rank 0: the 128 bytes every rank needs to join the communicator (ship them by any means)"""
    buf = C.create_string_buffer(128)
    _check(rccl_lib().bz_rccl_unique_id(buf))
    return buf.raw


class RcclComm:
    """struct bz_shard_comm over RCCL, implemented inside libbz2_mi355x_rccl.so (no Python in the data path).
    Creating it is collective (ncclCommInitRank): every rank calls it with the id rank 0 drew."""

    def __init__(self, unique_id, rank, world, device):
        self._p = C.c_void_p()
        _check(rccl_lib().bz_rccl_comm_create(C.byref(self._p), bytes(unique_id), rank, world, device))
        self.rank, self.world = rank, world
        self.errors = []

    @property
    def struct(self):
        """the bz_shard_comm the library filled in (GpuEngine.encode_sharded passes its address)"""
        from .sharded import ShardComm
        return ShardComm.from_address(self._p.value)

    def register(self, t):
        return t  # (device pointers are used as they are)

    def count(self):
        """ranks of the communicator as RCCL counts them (ncclCommCount)"""
        n = rccl_lib().bz_rccl_comm_count(self._p)
        if n < 0:
            raise CompressionError(n)
        return n

    def close(self):
        if getattr(self, "_p", None) and self._p.value and _RCCL_LIB is not None:
            _RCCL_LIB.bz_rccl_comm_destroy(self._p)
            self._p = C.c_void_p()

    __del__ = close


def shard_window(level, n, rank, world):
    """(offset, bytes) of the input a rank of bz_gpu_encode_sharded_window has to hold: its slab, the largest block's
    worth of input in front of it and one tile behind (bz_shard_window)."""
    off, nb = C.c_uint64(0), C.c_size_t(0)
    _check(lib().bz_shard_window(level, n, rank, world, C.byref(off), C.byref(nb)))
    return off.value, nb.value


def device_count():
    return lib().bz_device_count()


def encode_bound(n):
    return lib().bz_encode_bound(n)


class BZip2Encoder:
    """`BZip2Encoder` (src/bzip2/encoder.rs:40-159) over the C ABI's streaming context."""

    CHUNK = 1 << 20  # bytes pulled from the input iterator per refill

    def __init__(self, level=9, device=0, devices=None, verify=None):
        if level < 1 or level > 9:
            raise ValueError("invalid level")  # the reference panics (encoder.rs:59-61)
        self._h = C.c_void_p()
        if devices is None:
            _check(lib().bz_enc_create(C.byref(self._h), level, device))
        else:
            devs = (C.c_int * len(devices))(*devices)
            _check(lib().bz_enc_create_multi(C.byref(self._h), level, devs, len(devices)))
        if verify is not None:
            self.set_verify(verify)
        self._buf = (C.c_uint8 * 65536)()
        self._ready = b""
        self._pos = 0

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.bz_enc_destroy(self._h)
            self._h = None

    VERIFY_STATS = ("blocks_checked", "jobs_redone", "jobs_failed_again", "nanoseconds")

    def set_verify(self, on=True):
        """Self-check (bz_enc_set_verify): every job's blocks are decoded on the device and compared with their input
        before their bytes can be read; a job that fails is encoded again without look-back passes."""
        _check(lib().bz_enc_set_verify(self._h, int(bool(on))))

    def verify_stats(self):
        s = (C.c_uint64 * 4)()
        _check(lib().bz_enc_verify_stats(self._h, s))
        return dict(zip(self.VERIFY_STATS, [int(x) for x in s]))

    def phase_stats(self):
        """where the time of this stream went so far (bz_enc_phase_stats)"""
        t = (C.c_double * 8)()
        _check(lib().bz_enc_phase_stats(self._h, t))
        return {k: (int(v) if k == "jobs" else round(v, 3)) for k, v in zip(PHASES, t)}

    @classmethod
    def with_devices(cls, level, devices):
        """The same encoder over several GPUs of this process (bz_enc_create_multi): chunks of the input go round
        two lanes per listed device; the stream is the one `BZip2Encoder(level)` writes."""
        return cls(level, devices=list(devices))

    def _refill(self):
        k = lib().bz_enc_read(self._h, self._buf, len(self._buf))
        if k < 0:
            raise CompressionError(k)
        self._ready = C.string_at(self._buf, k)
        self._pos = 0
        return k

    def next(self, it, action):
        """One `Encoder::next(iter, action)` call: an int byte, or None."""
        if self._pos >= len(self._ready) and self._refill() == 0:
            # pull the input (the reference pulls one byte per call; the bytes are the same)
            while True:
                chunk = bytearray()
                for b in it:
                    chunk.append(b)
                    if len(chunk) >= self.CHUNK:
                        break
                if chunk:
                    _check(lib().bz_enc_write(self._h, bytes(chunk), len(chunk)))
                    if lib().bz_enc_pending(self._h):
                        break
                if len(chunk) < self.CHUNK:
                    _check(lib().bz_enc_end(self._h, int(action)))
                    break
            if self._refill() == 0:
                return None
        b = self._ready[self._pos]
        self._pos += 1
        return b

    # bulk helpers (same semantics, fewer Python-level calls)
    def write(self, data):
        _check(lib().bz_enc_write(self._h, bytes(data), len(data)))

    def end(self, action):
        _check(lib().bz_enc_end(self._h, int(action)))

    def read_all(self):
        out = bytearray(self._ready[self._pos:])
        self._ready, self._pos = b"", 0
        while self._refill():
            out += self._ready
        self._ready, self._pos = b"", 0
        return bytes(out)

    read_available = read_all  # what is complete now (chunks are encoded while the caller goes on writing)

    def encode_all(self, data, action=Action.FINISH):
        """`data.encode(&mut self, action).collect()`"""
        self.write(data)
        self.end(action)
        return self.read_all()


def encode(iterable, encoder, action):
    """`EncodeExt::encode` / `EncodeIterator` (src/traits/encoder.rs:12-79)."""
    it = iter(iterable)
    while True:
        b = encoder.next(it, action)
        if b is None:
            return
        yield b


PHASES = ("caller_copy_in_ms", "caller_wait_staging_ms", "split_serial_ms", "encode_ms", "assemble_serial_ms", "download_ms",
          "jobs", "workers_wait_turn_ms")


def last_call_phases():
    """where the time of the last one-shot call (compress / bz_encode_buffer[_multi]) went (bz_encode_buffer_last_phases)"""
    t = (C.c_double * 8)()
    _check(lib().bz_encode_buffer_last_phases(t))
    return {k: (int(v) if k == "jobs" else round(v, 3)) for k, v in zip(PHASES, t)}


def release_cached_resources():
    """Frees what finished contexts parked for the next one (bz_release_cached_resources)."""
    lib().bz_release_cached_resources()


def _batch_call(fn, head_args, datas, verdicts, mid_args=()):
    """One host-to-host batch entry point (bz_encode_batch and its siblings): the ctypes arrays, the call, the
    result cut into its entries, the buffer freed.  verdicts: the call also fills one verdict per entry, and an entry of
    the result is (bytes, verdict).  mid_args: what the call takes between the inputs and the outputs (a dictionary)."""
    datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
    k = len(datas)
    ins = (C.c_char_p * max(k, 1))(*datas)
    lens = (C.c_size_t * max(k, 1))(*[len(d) for d in datas])
    off = (C.c_uint64 * max(k, 1))()
    ln = (C.c_uint64 * max(k, 1))()
    v = (C.c_int32 * max(k, 1))()
    out = C.POINTER(C.c_uint8)()
    _check(fn(*head_args, ins, lens, k, *mid_args, C.byref(out), off, ln, *((v,) if verdicts else ())))
    try:
        base = C.addressof(out.contents) if k else 0
        parts = [C.string_at(base + off[i], ln[i]) for i in range(k)]
        return [(p, int(v[i])) for i, p in enumerate(parts)] if verdicts else parts
    finally:
        lib().bz_free(out)


def _decode_call(fn, head_args, data, data_verdicts, mid_args=()):
    """One host-to-host one-shot decode (bz_decode_buffer, df_decode_buffer) -> (bytes yielded, verdict code); a status
    that is not one of the decoder's verdicts is raised.  mid_args as in _batch_call."""
    data = bytes(data)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    rc = fn(*head_args, data, len(data), *mid_args, C.byref(out), C.byref(n))
    if rc != BZ_OK and rc not in data_verdicts:
        raise CompressionError(rc)
    try:
        return C.string_at(out, n.value), rc
    finally:
        lib().bz_free(out)


def compress(data, level=9, device=0, devices=None, verify=None):
    """One-shot over host buffers (bz_encode_buffer; `devices`: bz_encode_buffer_multi over that list of GPUs).
    verify=True: through a streaming context with the self-check on (the one-shot entry points take BZ_VERIFY=1
    from the environment); the bytes are the same."""
    if level < 1 or level > 9:
        raise ValueError("invalid level")
    if not isinstance(data, (bytes, bytearray)):
        data = bytes(data)
    if verify is not None:
        return BZip2Encoder(level, device, devices, verify=verify).encode_all(data)
    buf = data if isinstance(data, bytes) else (C.c_char * len(data)).from_buffer(data)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    if devices is None:
        _check(lib().bz_encode_buffer(level, device, buf, len(data), C.byref(out), C.byref(n)))
    else:
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().bz_encode_buffer_multi(level, devs, len(devices), buf, len(data), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().bz_free(out)


def encode_batch_bound(lens):
    """An output capacity that always suffices for GpuEngine.encode_batch_device (bz_encode_batch_bound)."""
    a = (C.c_uint64 * max(len(lens), 1))(*lens)
    return lib().bz_encode_batch_bound(a, len(lens))


def compress_batch(datas, level=9, device=0, verify=None):
    """Many independent inputs in one call (bz_encode_batch) -> list of streams: element i is compress(datas[i], level),
    bit for bit.  Inputs that are certain to be one block (at most 719 985 bytes at level 9) are encoded together in one
    pass of the pipeline, however many there are.  verify given: each input through a streaming context with the
    self-check switched that way (the batch call takes BZ_VERIFY=1 from the environment); the bytes are the same."""
    if level < 1 or level > 9:
        raise ValueError("invalid level")
    datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
    if verify is not None:
        return [BZip2Encoder(level, device, verify=verify).encode_all(d) for d in datas]
    return _batch_call(lib().bz_encode_batch, (level, device), datas, False)


# ---------------------------------------------------------------------------- Deflate / zlib / gzip
DEFLATE, ZLIB, GZIP = 0, 1, 2


class Inflater:
    """`Inflater` (src/deflate/encoder.rs:92-260) over the C ABI's streaming context: the reference's
    name for its Deflate ENCODER.  Action.RUN accumulates, Action.FLUSH writes the bytes so far as a
    byte-aligned segment (non-final block; the window and decompress_len carry over), Action.FINISH ends
    the stream.  ZlibEncoder / GZipEncoder end their container at the first None of the inner Inflater whatever
    the Action (zlib/encoder.rs:138-150): Run / Flush give header + what the Inflater yields + trailer, and the
    encoder then returns None without pulling its caller's iterator."""

    KIND = DEFLATE
    CHUNK = 1 << 20

    def __init__(self, device=0, dict_=b""):
        self._h = C.c_void_p()
        dict_ = bytes(dict_)
        _check(lib().df_enc_create_dict(C.byref(self._h), self.KIND, device, dict_, len(dict_)))
        self._buf = (C.c_uint8 * 65536)()
        self._ready = b""
        self._pos = 0

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.df_enc_destroy(self._h)
            self._h = None

    @classmethod
    def with_dict(cls, dict_, device=0):
        """`Inflater::with_dict` / `ZlibEncoder::with_dict`"""
        return cls(device, dict_)

    def _refill(self):
        k = lib().df_enc_read(self._h, self._buf, len(self._buf))
        if k < 0:
            raise CompressionError(k)
        self._ready = C.string_at(self._buf, k)
        self._pos = 0
        return k

    def next(self, it, action):
        """One `Encoder::next(iter, action)` call: an int byte, or None."""
        if self._pos >= len(self._ready) and self._refill() == 0:
            if self.KIND != DEFLATE and lib().df_enc_finished(self._h):
                return None  # the trailer is out: the wrappers do not touch the iterator any more (zlib/encoder.rs:130-136)
            while True:
                chunk = bytearray()
                for b in it:
                    chunk.append(b)
                    if len(chunk) >= self.CHUNK:
                        break
                if chunk:
                    _check(lib().df_enc_write(self._h, bytes(chunk), len(chunk)))
                if len(chunk) < self.CHUNK:
                    _check(lib().df_enc_end(self._h, int(action)))
                    break
            if self._refill() == 0:
                return None
        b = self._ready[self._pos]
        self._pos += 1
        return b

    def write(self, data):
        _check(lib().df_enc_write(self._h, bytes(data), len(data)))

    def end(self, action):
        _check(lib().df_enc_end(self._h, int(action)))

    def read_all(self):
        out = bytearray(self._ready[self._pos:])
        self._ready, self._pos = b"", 0
        while self._refill():
            out += self._ready
        self._ready, self._pos = b"", 0
        return bytes(out)

    def encode_all(self, data, action=Action.FINISH):
        self.write(data)
        self.end(action)
        return self.read_all()


class ZlibEncoder(Inflater):
    """`ZlibEncoder` (src/zlib/encoder.rs:55-157)."""
    KIND = ZLIB


class GZipEncoder(Inflater):
    """`GZipEncoder` (src/gzip/encoder.rs:50-135)."""
    KIND = GZIP


def deflate_compress(data, kind=DEFLATE, device=0, dict_=b""):
    """One-shot over host buffers (df_encode_buffer / df_encode_buffer_dict)."""
    data, dict_ = bytes(data), bytes(dict_)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    _check(lib().df_encode_buffer_dict(kind, device, data, len(data), dict_, len(dict_), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().bz_free(out)


def deflate_bound(n):
    return lib().df_encode_bound(n)


def deflate_encode_batch_bound(lens):
    """An output capacity that always suffices for GpuEngine.deflate_encode_batch_device (df_encode_batch_bound)."""
    a = (C.c_uint64 * max(len(lens), 1))(*lens)
    return lib().df_encode_batch_bound(a, len(lens))


def _encode_dict(kind, dict_):
    """The dictionary of a batch encode call as the C ABI takes it; an empty one is no dictionary."""
    if kind not in (DEFLATE, ZLIB, GZIP):
        raise ValueError("invalid kind")
    dict_ = bytes(dict_)
    if dict_ and kind == GZIP:
        raise ValueError("gzip encoding takes no preset dictionary (GZipEncoder has no with_dict)")
    return dict_


def deflate_compress_batch(datas, kind=DEFLATE, device=0, dict_=b""):
    """Many independent inputs in one call (df_encode_batch_dict) -> list of streams: element i is
    deflate_compress(datas[i], kind, dict_=dict_), bit for bit -- one preset dictionary (`Inflater::with_dict` /
    `ZlibEncoder::with_dict`, kinds DEFLATE and ZLIB) serves every input.  Inputs of at most 65 535 bytes (one Deflate
    block for certain) are encoded together in one pass of the pipeline, however many there are."""
    dict_ = _encode_dict(kind, dict_)
    return _batch_call(lib().df_encode_batch_dict, (kind, device), datas, False, (dict_, len(dict_)))


BGZF_BLOCK = 65280  # DF_BGZF_BLOCK: htslib's block size, the default and the maximum


def _bgzf_block_bytes(block_bytes):
    if not 0 <= block_bytes <= BGZF_BLOCK:
        raise ValueError("bgzf: block_bytes is 0 (the default, 65 280) or 1 .. 65 280")
    return block_bytes


def bgzf_block_count(n, block_bytes=0):
    """Blocks of a BGZF file of n input bytes (df_bgzf_block_count): ceil(n / B), the EOF marker not counted."""
    return lib().df_bgzf_block_count(n, _bgzf_block_bytes(block_bytes))


def bgzf_bound(n, block_bytes=0, eof=True):
    """An output capacity that always suffices for GpuEngine.bgzf_encode_device (df_bgzf_bound)."""
    return lib().df_bgzf_bound(n, _bgzf_block_bytes(block_bytes), 1 if eof else 0)


def bgzf_compress(data, block_bytes=0, eof=True, device=0, offsets=False):
    """One input as a BGZF file (df_bgzf_encode_buffer): gzip members of at most block_bytes (default 65 280) input bytes,
    side by side, then the 28-byte EOF marker unless eof is false.  Every member decodes with zlib / gzip / htslib.
    offsets=True: -> (file, offsets), count + 1 file offsets: where block k starts, and last where the marker starts."""
    data = bytes(data)
    block_bytes = _bgzf_block_bytes(block_bytes)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    k = (len(data) + (block_bytes or BGZF_BLOCK) - 1) // (block_bytes or BGZF_BLOCK)
    offs = (C.c_uint64 * (k + 1))()
    _check(lib().df_bgzf_encode_buffer(device, data, len(data), block_bytes, 1 if eof else 0, C.byref(out), C.byref(n), offs))
    try:
        z = C.string_at(out, n.value)
    finally:
        lib().bz_free(out)
    return (z, [int(x) for x in offs]) if offsets else z


class BgzfIndex:
    """The block index of a BGZF file (section 8 of the header): count + 1 pairs -- block k starts at file offset coff[k]
    and at uncompressed offset uoff[k]; the last pair is the end of the last complete block.  `verdict` is the chain's
    (BZ_OK, BZ_E_DATA or BZ_E_EOF: the blocks in front of a fault are still indexed).  The two lists are the .gzi table."""

    def __init__(self, coff, uoff, verdict=BZ_OK):
        self.coff = [int(x) for x in coff]
        self.uoff = [int(x) for x in uoff]
        if len(self.coff) != len(self.uoff) or not self.coff:
            raise ValueError("BgzfIndex: coff and uoff hold count + 1 entries each")
        self.verdict = int(verdict)

    @property
    def blocks(self):
        return len(self.coff) - 1

    @property
    def total(self):
        """uncompressed bytes of the indexed blocks"""
        return self.uoff[-1] - self.uoff[0]

    def _block_of(self, upos):
        import bisect
        return bisect.bisect_right(self.uoff, upos, 0, self.blocks) - 1

    def voffset(self, upos):
        """htslib's virtual offset of uncompressed position upos: coff << 16 | offset inside the block.  A position at a
        block's edge belongs to the block that starts there (the last of them, behind empty blocks); upos == the end of the
        last block is the end of the file: (coff[count], 0)."""
        if not self.uoff[0] <= upos <= self.uoff[-1]:
            raise ValueError("BgzfIndex.voffset: position outside the index")
        if upos == self.uoff[-1]:
            return self.coff[-1] << 16
        k = self._block_of(upos)
        return self.coff[k] << 16 | (upos - self.uoff[k])

    def upos(self, voffset):
        """the uncompressed position of a virtual offset (its coff must be a block's start, or the end of the last block)"""
        import bisect
        c, o = voffset >> 16, voffset & 0xFFFF
        k = bisect.bisect_left(self.coff, c)
        if k >= len(self.coff) or self.coff[k] != c:
            raise ValueError("BgzfIndex.upos: no block starts at file offset %d" % c)
        if k == self.blocks:
            if o:
                raise ValueError("BgzfIndex.upos: an offset behind the last block")
            return self.uoff[-1]
        if o >= max(self.uoff[k + 1] - self.uoff[k], 1):
            raise ValueError("BgzfIndex.upos: offset %d is not inside block %d" % (o, k))
        return self.uoff[k] + o

    def _arrays(self):
        """the two lists as the C call takes them; made once (an index is not changed after it is made)"""
        if getattr(self, "_c", None) is None:
            n = len(self.coff)
            self._c = (C.c_uint64 * n)(*self.coff), (C.c_uint64 * n)(*self.uoff)
        return self._c

    def __eq__(self, other):
        return isinstance(other, BgzfIndex) and (self.coff, self.uoff, self.verdict) == (other.coff, other.uoff, other.verdict)

    def __repr__(self):
        return "BgzfIndex(blocks=%d, total=%d, verdict=%d)" % (self.blocks, self.total, self.verdict)


class BgzfError(CompressionError):
    """A BGZF read that ended on a verdict: `partial` holds the bytes of the range in front of the fault."""

    def __init__(self, code, partial=b""):
        super().__init__(code)
        self.partial = partial


def bgzf_index(data):
    """The block index of a BGZF file in host memory (df_bgzf_index_buffer): the BSIZE chain, walked on the host.  Parsing,
    not decoding: no GPU is needed.  A faulty file does not raise: see BgzfIndex.verdict."""
    data = bytes(data)
    pc, pu = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    n = C.c_size_t(0)
    v = C.c_int32(0)
    _check(lib().df_bgzf_index_buffer(data, len(data), C.byref(pc), C.byref(pu), C.byref(n), C.byref(v)))
    try:
        return BgzfIndex(pc[:n.value + 1], pu[:n.value + 1], v.value)
    finally:
        lib().bz_free(pc)
        lib().bz_free(pu)


def bgzf_read(data, ustart, ulen, index=None, device=0):
    """The uncompressed bytes [ustart, ustart + ulen) of a BGZF file in host memory, clamped to its end (df_bgzf_read_buffer):
    only the blocks the range touches are uploaded and decoded.  ulen = None: to the end.  `index` (a BgzfIndex of this
    file) is accepted for symmetry with GpuEngine.bgzf_read_device; the host form walks the chain itself (parsing a file in
    host memory costs less than passing its table).  A fault raises BgzfError (a CompressionError, kind DataError or
    UnexpectedEof) whose `partial` holds the range's bytes in front of it."""
    if ustart < 0 or (ulen is not None and ulen < 0):
        raise ValueError("bgzf_read: a negative range")
    if index is not None and not isinstance(index, BgzfIndex):
        raise TypeError("bgzf_read: index is a BgzfIndex")
    out, rc = _decode_call(lib().df_bgzf_read_buffer, (device,), data, _DF_VERDICTS,
                           (C.c_uint64(ustart), C.c_uint64(0xFFFFFFFFFFFFFFFF if ulen is None else ulen)))
    if rc != BZ_OK:
        raise BgzfError(rc, out)
    return out


def bgzf_decompress(data, device=0):
    """A whole BGZF file (bgzf_read over everything): the bytes of gzip.decompress for every file this reader accepts."""
    return bgzf_read(data, 0, None, device=device)


_DECODER_VERDICTS = (BZ_E_DATA, BZ_E_MAGIC_FIRST, BZ_E_MAGIC)


class BZip2Decoder:
    """`BZip2Decoder` (src/bzip2/decoder.rs:583-612) over the C ABI's streaming context.  Input is
    handed over in chunks; the library decodes whatever records are complete once BZ_DEC_CHUNK bytes
    have come in and at the end, so bytes come out before the input is exhausted for long inputs."""

    CHUNK = 1 << 20  # bytes pulled from the input iterator per refill

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().bz_dec_create(C.byref(self._h), device))
        self._buf = (C.c_uint8 * 65536)()
        self._ready = b""
        self._pos = 0
        self._ended = False

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.bz_dec_destroy(self._h)
            self._h = None

    def _refill(self):
        """bytes fetched; 0 = nothing ready (or, after the end, the clean end); raises the decoder's Err item"""
        k = lib().bz_dec_read(self._h, self._buf, len(self._buf))
        if k < 0:
            raise BZip2Error(k) if k in _DECODER_VERDICTS else CompressionError(k)
        self._ready = C.string_at(self._buf, k)
        self._pos = 0
        return k

    def _end(self):
        if not self._ended:
            self._ended = True
            rc = lib().bz_dec_end(self._h)
            if rc != BZ_OK and rc not in _DECODER_VERDICTS:
                raise CompressionError(rc)  # infrastructure (no GPU, memory ...)

    def next(self, it):
        """One `Decoder::next(iter)` call: an int byte, None at the end, raises BZip2Error for Err."""
        while self._pos >= len(self._ready):
            if self._refill():
                break
            if self._ended:
                return None
            chunk = bytearray()
            for b in it:  # (the reference pulls bytes on demand; the bytes are the same)
                chunk.append(b)
                if len(chunk) >= self.CHUNK:
                    break
            if chunk:
                _check(lib().bz_dec_write(self._h, bytes(chunk), len(chunk)))
            if len(chunk) < self.CHUNK:
                self._end()
        b = self._ready[self._pos]
        self._pos += 1
        return b

    # bulk helpers (same semantics, fewer Python-level calls)
    def write(self, data):
        data = bytes(data)
        if data:
            _check(lib().bz_dec_write(self._h, data, len(data)))

    def read_available(self):
        """decoded bytes that are ready now (raises the Err item once the bytes in front of it are out)"""
        out = bytearray(self._ready[self._pos:])
        self._ready, self._pos = b"", 0
        while True:
            try:
                if not self._refill():
                    break
            except BZip2Error as e:
                e.partial = bytes(out)
                raise
            out += self._ready
            self._ready, self._pos = b"", 0
        return bytes(out)

    def decode_all(self, data):
        """`data.decode(&mut self).collect::<Result<Vec<_>, _>>()`; BZip2Error.partial holds the bytes
        yielded before an Err."""
        self.write(data)
        self._end()
        return self.read_available()


def decode(iterable, decoder):
    """`DecodeExt::decode` / `DecodeIterator` (src/traits/decoder.rs:15-86)."""
    it = iter(iterable)
    while True:
        b = decoder.next(it)
        if b is None:
            return
        yield b


def decompress(data, device=0):
    """One-shot over host buffers (bz_decode_buffer) -> (bytes yielded, verdict code)."""
    return _decode_call(lib().bz_decode_buffer, (device,), data, _DECODER_VERDICTS)


def decompress_batch(datas, device=0):
    """Many independent streams in one call (bz_decode_batch) -> list of (bytes yielded, verdict code): element i is
    decompress(datas[i]).  An entry's verdict is its own -- a bad record hides nothing behind it; CompressionError is
    raised for infrastructure errors only."""
    return _batch_call(lib().bz_decode_batch, (device,), datas, True)


_DF_VERDICTS = (BZ_E_DATA, BZ_E_EOF)


def _decode_dict(kind, dict_):
    """The dictionary of a decode call as the C ABI takes it; an empty one is no dictionary (clause (c) of section 5)."""
    if kind not in (DEFLATE, ZLIB, GZIP):
        raise ValueError("invalid kind")
    dict_ = bytes(dict_)
    if dict_ and kind == GZIP:
        raise ValueError("gzip decoding takes no preset dictionary (GZipDecoder has no with_dict)")
    return dict_


def deflate_decompress(data, kind=DEFLATE, device=0, dict_=b""):
    """One-shot over host buffers (df_decode_buffer_dict) -> (bytes yielded, verdict code): BZ_OK, BZ_E_DATA or BZ_E_EOF
    under the contract of section 5 of the header (RFC 1951 / 1950 / 1952; zlib's inflate is the arbiter).  dict_: the
    preset dictionary of `Deflater::with_dict` / `ZlibDecoder::with_dict` (kinds DEFLATE and ZLIB)."""
    dict_ = _decode_dict(kind, dict_)
    return _decode_call(lib().df_decode_buffer_dict, (kind, device), data, _DF_VERDICTS, (dict_, len(dict_)))


def deflate_decompress_batch(datas, kind=DEFLATE, device=0, dict_=b""):
    """Many independent streams in one call (df_decode_batch_dict) -> list of (bytes yielded, verdict code): element i is
    deflate_decompress(datas[i], kind, dict_=dict_) -- one dictionary serves every entry.  An entry's verdict is its own;
    CompressionError is raised for infrastructure errors only."""
    dict_ = _decode_dict(kind, dict_)
    return _batch_call(lib().df_decode_batch_dict, (kind, device), datas, True, (dict_, len(dict_)))


class Deflater:
    """`Deflater` (src/deflate/decoder.rs) with the `next(it)` / `decode_all(data)` surface of BZip2Decoder, over
    df_decode_buffer: the first `next` collects the input iterator and decodes it in one call; the bytes are handed out,
    then CompressionError (kind DataError / UnexpectedEof, `.partial` = the bytes in front of it) is raised once.
    dict_: `Deflater::with_dict` (deflate/decoder.rs:358-404); an empty one is no dictionary.
    Creating one does not touch the device."""
    KIND = DEFLATE

    def __init__(self, device=0, dict_=b""):
        self._device = device
        self._dict = _decode_dict(self.KIND, dict_)
        self._ready = None
        self._pos = 0
        self._verdict = BZ_OK

    @classmethod
    def with_dict(cls, dict_, device=0):
        """`Deflater::with_dict(dict)` / `ZlibDecoder::with_dict(dict)`."""
        return cls(device, dict_)

    def _decode(self, data):
        return deflate_decompress(data, self.KIND, self._device, self._dict)

    def _error(self):
        e = CompressionError(self._verdict)
        e.partial = self._ready
        self._verdict = BZ_OK
        return e

    def next(self, it):
        """One `Decoder::next(iter)` call: an int byte, None at the end, raises CompressionError for Err."""
        if self._ready is None:
            self._ready, self._verdict = self._decode(bytes(bytearray(it)))
        if self._pos < len(self._ready):
            self._pos += 1
            return self._ready[self._pos - 1]
        if self._verdict != BZ_OK:
            raise self._error()
        return None

    def decode_all(self, data):
        """`data.decode(&mut self).collect::<Result<Vec<_>, _>>()`; CompressionError.partial holds the bytes yielded
        before an Err."""
        self._ready, self._verdict = self._decode(data)
        self._pos = len(self._ready)
        if self._verdict != BZ_OK:
            raise self._error()
        return self._ready


class ZlibDecoder(Deflater):
    """`ZlibDecoder` (src/zlib/decoder.rs); with a dictionary the header must carry FDICT and its Adler-32."""
    KIND = ZLIB


class GZipDecoder(Deflater):
    """`GZipDecoder` (src/gzip/decoder.rs): the first member.  It has no with_dict: a non-empty dictionary is a ValueError."""
    KIND = GZIP


def gzip_decompress_members(data, device=0):
    """Every member of a gzip file, one after the other (df_decode_members_buffer; section 6 of the header) -> (bytes
    yielded, verdict code): what gzip(1) and gzip.decompress yield, zero padding between and behind members skipped;
    BZ_E_DATA / BZ_E_EOF with the bytes in front of the fault."""
    return _decode_call(lib().df_decode_members_buffer, (device,), data, _DF_VERDICTS)


class MultiGZipDecoder(Deflater):
    """Every member of a gzip file (flate2's MultiGzDecoder); GZipDecoder stops behind the first, as the reference's does."""
    KIND = GZIP

    def _decode(self, data):
        return gzip_decompress_members(data, self._device)


class LzhufMethod(enum.IntEnum):
    """`LzhufMethod` (src/lzhuf/mod.rs:14-38): the LHA methods -lh4- .. -lh7-; the values are the C ABI's BZ_LZH_LH4 .. 7."""
    Lh4 = 4
    Lh5 = 5
    Lh6 = 6
    Lh7 = 7

    @property
    def dictionary_bits(self):
        return {4: 12, 5: 13, 6: 15, 7: 16}[int(self)]

    @property
    def offset_bits(self):
        return 4 if self in (LzhufMethod.Lh4, LzhufMethod.Lh5) else 5


LZH_NO_LEN = 0xFFFFFFFFFFFFFFFF  # an original length that is not known (UINT64_MAX)


def _lzh_params(method, prefill):
    if int(method) not in (4, 5, 6, 7):
        raise ValueError("invalid LZHUF method")
    if not -1 <= int(prefill) <= 255:
        raise ValueError("prefill must be -1 (strict) or a byte value")
    return int(method), int(prefill)


def _lzh_len(orig_len):
    return LZH_NO_LEN if orig_len is None else int(orig_len)


def lzhuf_decompress(data, method, orig_len=None, prefill=-1, device=0):
    """One-shot over host buffers (bz_lzh_decode_buffer) -> (bytes yielded, verdict code): BZ_OK, BZ_E_DATA or BZ_E_EOF
    under the contract of section 9 of the header.  orig_len: the original length an LHA member header carries (None: not
    known, the stream ends at a block boundary with fewer than 16 bits left or a zero block length).  prefill: -1 is
    strict (no distance may reach in front of the output), 0..255 the value of every byte in front of it."""
    method, prefill = _lzh_params(method, prefill)
    return _decode_call(lib().bz_lzh_decode_buffer, (method, prefill, device), data, _DF_VERDICTS, (_lzh_len(orig_len),))


def lzhuf_decompress_batch(datas, method, orig_lens=None, prefill=-1, device=0):
    """Many independent streams in one call (bz_lzh_decode_batch) -> list of (bytes yielded, verdict code): element i is
    lzhuf_decompress(datas[i], method, orig_lens[i]).  An entry's verdict is its own; CompressionError is raised for
    infrastructure errors only."""
    method, prefill = _lzh_params(method, prefill)
    datas = list(datas)
    ol = None
    if orig_lens is not None:
        if len(orig_lens) != len(datas):
            raise ValueError("lzhuf_decompress_batch: datas and orig_lens differ in length")
        ol = (C.c_uint64 * max(len(datas), 1))(*[_lzh_len(x) for x in orig_lens])
    return _batch_call(lambda m, f, d, ins, lens, k, *rest: lib().bz_lzh_decode_batch(m, f, d, ins, lens, ol, k, *rest),
                       (method, prefill, device), datas, True)


class LzhufDecoder(Deflater):
    """`LzhufDecoder::new(&method)` (src/lzhuf/decoder.rs) with the `next(it)` / `decode_all(data)` surface of Deflater,
    over bz_lzh_decode_buffer; strict (prefill -1) unless told otherwise.  Creating one does not touch the device."""

    def __init__(self, method, device=0, orig_len=None, prefill=-1):
        self._method, self._prefill = _lzh_params(method, prefill)
        self._orig_len = orig_len
        self._device = device
        self._ready = None
        self._pos = 0
        self._verdict = BZ_OK

    def _decode(self, data):
        return lzhuf_decompress(data, self._method, self._orig_len, self._prefill, self._device)


def _lzh_method(method):
    if int(method) not in (4, 5, 6, 7):
        raise ValueError("invalid LZHUF method")
    return int(method)


def lzhuf_encode_batch_bound(lens):
    """An output capacity that always suffices for GpuEngine.lzh_encode_batch_device (bz_lzh_encode_batch_bound)."""
    a = (C.c_uint64 * max(len(lens), 1))(*lens)
    return lib().bz_lzh_encode_batch_bound(a, len(lens))


def lzhuf_compress(data, method, device=0):
    """One-shot over host buffers (bz_lzh_encode_buffer): `data.encode(&mut LzhufEncoder::new(&method), Action::Finish)`
    collected, byte for byte.  An empty input gives an empty stream."""
    method = _lzh_method(method)
    data = bytes(data)
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    _check(lib().bz_lzh_encode_buffer(method, device, data, len(data), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().bz_free(out)


def lzhuf_compress_batch(datas, method, device=0):
    """Many independent inputs in one call (bz_lzh_encode_batch) -> list of streams: element i is
    lzhuf_compress(datas[i], method), bit for bit.  All inputs share passes of the pipeline, however many there are."""
    return _batch_call(lib().bz_lzh_encode_batch, (_lzh_method(method), device), datas, False)


class LzhufEncoder:
    """`LzhufEncoder::new(&method)` (src/lzhuf/encoder.rs) in the shape of Inflater: `next(it, action)`, `write`, `end`,
    `read_all`, `encode_all`.  Action.RUN accumulates and Action.FINISH ends the stream; Action.FLUSH is NOT offered (the
    reference's flush closes the block and pads to a byte in the middle of a stream; this encoder writes whole streams
    only) and is a parameter error.  The bytes are encoded by one bz_lzh_encode_buffer call when the stream is finished;
    creating an encoder does not touch the device."""

    def __init__(self, method, device=0):
        self._method = _lzh_method(method)
        self._device = device
        self._in = bytearray()
        self._ready = b""
        self._pos = 0
        self._finished = False

    def write(self, data):
        if self._finished:
            raise CompressionError(BZ_E_PARAM)
        self._in += bytes(data)

    def end(self, action):
        if int(action) == int(Action.FLUSH):
            raise CompressionError(BZ_E_PARAM)
        if int(action) not in (int(Action.RUN), int(Action.FINISH)):
            raise ValueError("invalid action")
        if int(action) == int(Action.FINISH) and not self._finished:
            self._ready = self._ready[self._pos:] + lzhuf_compress(bytes(self._in), self._method, self._device)
            self._pos = 0
            self._in = bytearray()
            self._finished = True

    def next(self, it, action):
        """One `Encoder::next(iter, action)` call: an int byte, or None (Action.RUN: nothing is yielded before FINISH)."""
        if self._pos >= len(self._ready) and not self._finished:
            self._in += bytes(bytearray(it))
            self.end(action)
        if self._pos >= len(self._ready):
            return None
        b = self._ready[self._pos]
        self._pos += 1
        return b

    def read_all(self):
        out = self._ready[self._pos:]
        self._ready, self._pos = b"", 0
        return out

    def encode_all(self, data, action=Action.FINISH):
        self.write(data)
        self.end(action)
        return self.read_all()


# ---- LHA archives (section 11 of the header): the member table on the host, every member's bytes in one device call
class _LhaMemberRec(C.Structure):
    """bz_lha_member"""
    _fields_ = [("header_off", C.c_uint64), ("data_off", C.c_uint64), ("packed_len", C.c_uint64), ("orig_len", C.c_uint64),
                ("name_off", C.c_uint64), ("dir_off", C.c_uint64), ("name_len", C.c_uint32), ("dir_len", C.c_uint32),
                ("mtime", C.c_uint32), ("crc16", C.c_uint16), ("method", C.c_uint8), ("level", C.c_uint8), ("os_id", C.c_uint8),
                ("attr", C.c_uint8), ("method_id", C.c_uint8 * 5), ("pad", C.c_uint8)]


LhaMember = collections.namedtuple("LhaMember", "name directory method level packed_len orig_len crc16 mtime os_id data_off header_off attr")
LhaMember.__doc__ = """One member of an LHA archive: `name` and `directory` are raw bytes (a directory's components are
separated by 0xFF), `method` the five bytes of its id (b"-lh5-"), `mtime` the header's raw time field."""


class LhaIndex(tuple):
    """The members of an archive in its order, and `.fault`: BZ_OK when the archive ends cleanly, else (verdict, position of
    the header the fault lies in); the members in front of the fault are listed."""
    fault = BZ_OK
    _records = None


def lha_index(data):
    """The member table of an LHA archive (bz_lha_index_buffer; the host alone, no GPU) -> LhaIndex."""
    data = bytes(data)
    L = lib()
    n, fault, pos = C.c_size_t(0), C.c_int32(0), C.c_uint64(0)
    _check(L.bz_lha_index_buffer(data, len(data), None, 0, C.byref(n), C.byref(fault), C.byref(pos)))
    recs = (_LhaMemberRec * max(n.value, 1))()
    _check(L.bz_lha_index_buffer(data, len(data), recs, n.value, C.byref(n), C.byref(fault), C.byref(pos)))
    idx = LhaIndex(LhaMember(data[r.name_off:r.name_off + r.name_len], data[r.dir_off:r.dir_off + r.dir_len], bytes(r.method_id), r.level,
                             r.packed_len, r.orig_len, r.crc16, r.mtime, r.os_id, r.data_off, r.header_off, r.attr)
                   for r in recs[:n.value])
    idx.fault = BZ_OK if fault.value == BZ_OK else (int(fault.value), int(pos.value))
    idx._records = recs
    return idx


def _lha_selection(index, members):
    """indices (ascending, as the C call wants them) of `members`: None (all), or indices and names (the first member of that
    name) in any order -> (sorted indices, the position of each request in them)"""
    if members is None:
        return None, list(range(len(index)))
    want = []
    for m in members:
        if isinstance(m, (bytes, bytearray, str)):
            name = m.encode() if isinstance(m, str) else bytes(m)
            hits = [i for i, q in enumerate(index) if q.name == name]
            if not hits:
                raise KeyError(m)
            want.append(hits[0])
        else:
            i = int(m)
            if not 0 <= i < len(index):
                raise IndexError("no member %d" % i)
            want.append(i)
    order = sorted(set(want))
    return order, [order.index(i) for i in want]


def lha_extract(data, members=None, prefill=0x20, device=0, check=False):
    """The bytes of the members of an LHA archive in one call (bz_lha_read_buffer) -> list of (bytes, verdict), one per
    request: members = None (all), or indices and names.  A member is BZ_OK only when its CRC-16 is its header's.
    check=True: the first verdict that is not BZ_OK is raised as CompressionError."""
    data = bytes(data)
    index = lha_index(data)
    order, pos = _lha_selection(index, members)
    k = len(index) if order is None else len(order)
    sel = None if order is None else (C.c_size_t * max(k, 1))(*order)
    off, ln, v = (C.c_uint64 * max(k, 1))(), (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
    out = C.POINTER(C.c_uint8)()
    fault = C.c_int32(0)
    if not -1 <= int(prefill) <= 255:
        raise ValueError("prefill must be -1 (strict) or a byte value")
    _check(lib().bz_lha_read_buffer(device, data, len(data), sel, k, int(prefill), C.byref(out), off, ln, v, C.byref(fault)))
    try:
        base = C.addressof(out.contents) if k else 0
        res = [(C.string_at(base + off[j], ln[j]), int(v[j])) for j in pos]
    finally:
        lib().bz_free(out)
    if check:
        for _, verdict in res:
            if verdict != BZ_OK:
                raise CompressionError(verdict)
    return res


class LhaArchive:
    """An LHA archive in host memory: `.members` (LhaIndex), `.read(index or name)` -> (bytes, verdict), `.read_all()`.
    Creating one builds the table on the host and does not touch the device."""

    def __init__(self, data, prefill=0x20, device=0):
        self._data = bytes(data)
        self._prefill, self._device = prefill, device
        self.members = lha_index(self._data)

    def read(self, member):
        return lha_extract(self._data, [member], self._prefill, self._device)[0]

    def read_all(self):
        return lha_extract(self._data, None, self._prefill, self._device)


# ---- LHA archives, writing (section 12 of the header): every member in one device call
class _LhaEntryRec(C.Structure):
    """bz_lha_entry"""
    _fields_ = [("name", C.c_char_p), ("name_len", C.c_uint32), ("dir", C.c_char_p), ("dir_len", C.c_uint32), ("mtime", C.c_uint32),
                ("attr", C.c_uint8), ("os_id", C.c_uint8), ("is_dir", C.c_uint8), ("pad", C.c_uint8)]


_LhaEntryBase = collections.namedtuple("LhaEntry", "name directory mtime attr os_id is_dir")


class LhaEntry(_LhaEntryBase):
    """What a member's header says beside its sizes and CRC: `name` and `directory` are raw bytes (a directory's components
    are separated by 0xFF; str is encoded as UTF-8), `mtime` the header's raw time field (levels 0 and 1: MS-DOS time and
    date; level 2: Unix time), `is_dir` a -lhd- member without data."""
    __slots__ = ()

    def __new__(cls, name, directory=b"", mtime=0, attr=0x20, os_id=0x55, is_dir=False):
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in (name, directory)]
        return super().__new__(cls, raw[0], raw[1], int(mtime), int(attr), int(os_id), bool(is_dir))


LHA_STORED = 0   # the `method` of lha_compress / lha_write_device that writes every member as -lh0- (BZ_LHA_STORED)


def _lha_method(method):
    if int(method) not in (0, 4, 5, 6, 7):
        raise ValueError("invalid LHA method")
    return int(method)


def _lha_entries(entries):
    """-> (the bz_lha_entry array, what keeps its bytes alive)"""
    ents = [e if isinstance(e, LhaEntry) else LhaEntry(e) for e in entries]
    recs = (_LhaEntryRec * max(len(ents), 1))()
    for r, e in zip(recs, ents):
        r.name, r.name_len, r.dir, r.dir_len = e.name, len(e.name), e.directory, len(e.directory)
        r.mtime, r.attr, r.os_id, r.is_dir = e.mtime, e.attr, e.os_id, int(e.is_dir)
    return recs, ents


def lha_write_bound(entries, lens, level=2):
    """An output capacity that always suffices for GpuEngine.lha_write_device (bz_lha_write_bound; the host alone).  0: an
    entry has no header at that level."""
    recs, keep = _lha_entries(entries)
    if len(lens) != len(keep):
        raise ValueError("lha_write_bound: the arrays differ in length")
    return lib().bz_lha_write_bound(int(level), recs, (C.c_uint64 * max(len(keep), 1))(*lens), len(keep))


def lha_compress(members, method=LzhufMethod.Lh5, level=2, device=0):
    """An LHA archive of `members`, a list of (name, data) or (LhaEntry, data), in one call (bz_lha_write_buffer) -> bytes.
    method: a LzhufMethod, or LHA_STORED; a member whose stream would not be shorter than its bytes is stored."""
    members = list(members)
    recs, keep = _lha_entries([m[0] for m in members])
    datas = [bytes(m[1]) for m in members]
    k = len(datas)
    ins = (C.c_char_p * max(k, 1))(*datas)
    lens = (C.c_size_t * max(k, 1))(*[len(d) for d in datas])
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
    _check(lib().bz_lha_write_buffer(_lha_method(method), int(level), device, ins, lens, recs, k, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().bz_free(out)


class GpuEngine:
    """Device-resident engine (section 2 of the C ABI).  Pointers are plain ints
    (e.g. torch.Tensor.data_ptr())."""

    STAGES = ("rle1_crc_split", "bwt", "mtf_zle", "huffman", "emit_assemble", "total")

    def __init__(self, device=0, max_blocks_in_flight=64):
        self._h = C.c_void_p()
        _check(lib().bz_gpu_engine_create(C.byref(self._h), device, max_blocks_in_flight))

    def close(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.bz_gpu_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def set_verify(self, on=True):
        """Self-check of the device-resident calls (bz_gpu_engine_set_verify)."""
        _check(lib().bz_gpu_engine_set_verify(self._h, int(bool(on))))

    def verify_stats(self):
        s = (C.c_uint64 * 4)()
        _check(lib().bz_gpu_verify_stats(self._h, s))
        return dict(zip(BZip2Encoder.VERIFY_STATS, [int(x) for x in s]))

    def encode_device(self, level, d_in, n, d_out, cap):
        _settle()
        out_len = C.c_size_t(0)
        _check(lib().bz_gpu_encode_device(self._h, level, d_in, n, d_out, cap, C.byref(out_len)))
        return out_len.value

    BATCH_STATS = ("inputs_batched", "inputs_one_by_one", "blocks", "sub_batches")

    def encode_batch_device(self, level, d_in, in_off, in_len, d_out, cap):
        """Many inputs, one stream each (bz_gpu_encode_batch_device): input i is the in_len[i] bytes at d_in + in_off[i]
        (offsets multiples of 16, in ascending order); returns (out_off, out_len), stream i at d_out + out_off[i]."""
        _settle()
        k = len(in_off)
        if len(in_len) != k:
            raise ValueError("encode_batch_device: in_off and in_len differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        _check(lib().bz_gpu_encode_batch_device(self._h, level, d_in, a_off, a_len, k, d_out, cap, o_off, o_len))
        return list(o_off[:k]), list(o_len[:k])

    def batch_stats(self):
        """The last encode_batch_device call: [0] inputs split by the batch front end, [1] inputs that took the one-input
        path, [2] blocks of the former, [3] sub-batches the pipeline ran them in (bz_gpu_last_batch_stats)."""
        s = (C.c_uint64 * 4)()
        _check(lib().bz_gpu_last_batch_stats(self._h, s))
        return [int(x) for x in s]

    def partition(self, level, d_in, n, mode=Action.FINISH):
        _settle()
        nb, cons, tail = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        _check(lib().bz_gpu_partition(self._h, level, d_in, n, int(mode), C.byref(nb), C.byref(cons), C.byref(tail)))
        return nb.value, cons.value, tail.value

    TILE = 4096  # input bytes per split tile

    def slab_begin(self, level, d_in, n, tile0, tile1):
        _settle()
        last = C.c_int64(-1)
        _check(lib().bz_gpu_partition_slab_begin(self._h, level, d_in, n, tile0, tile1, C.byref(last)))
        return last.value

    def slab_count(self, carry_run):
        _check(lib().bz_gpu_partition_slab_count(self._h, carry_run))

    def slab_finish(self, start_in, is_last):
        nb, nxt, tail = C.c_size_t(0), C.c_uint64(0), C.c_int(0)
        _check(lib().bz_gpu_partition_slab_finish(self._h, start_in, int(is_last), C.byref(nb), C.byref(nxt), C.byref(tail)))
        return nb.value, nxt.value, tail.value

    def encode_blocks(self, first, stride, n_blocks, d_packed, cap_words):
        _settle()
        # the library writes one entry per block of ITS last partition: size the arrays from that count
        have = lib().bz_gpu_block_count(self._h)
        if n_blocks != have:
            raise ValueError("encode_blocks: %d blocks asked for, the last partition made %d" % (n_blocks, have))
        k = max(0, (n_blocks - first + stride - 1) // stride) if n_blocks > first else 0
        woff = (C.c_uint64 * max(k, 1))()
        blen = (C.c_uint64 * max(k, 1))()
        crc = (C.c_uint32 * max(k, 1))()
        used = C.c_size_t(0)
        _check(lib().bz_gpu_encode_blocks(self._h, first, stride, d_packed, cap_words, woff, blen, crc, C.byref(used)))
        return list(woff[:k]), list(blen[:k]), list(crc[:k]), used.value

    def assemble(self, level, d_packed, word_off, bit_len, crc, d_out, cap, header=True, trailer=True, pad=True,
                 carry_bits=0, carry_byte=0, combined_crc=0):
        _settle()
        k = len(word_off)
        woff = (C.c_uint64 * max(k, 1))(*word_off)
        blen = (C.c_uint64 * max(k, 1))(*bit_len)
        crcs = (C.c_uint32 * max(k, 1))(*crc)
        out_len, comb = C.c_size_t(0), C.c_uint32(0)
        ocb, ocy = C.c_uint(0), C.c_uint(0)
        _check(lib().bz_gpu_assemble(self._h, level, k, d_packed, woff, blen, crcs, int(header), int(trailer), int(pad),
                                     carry_bits, carry_byte, combined_crc, C.byref(comb), d_out, cap,
                                     C.byref(out_len), C.byref(ocb), C.byref(ocy)))
        return out_len.value, comb.value, ocb.value, ocy.value

    def encode_sharded(self, level, d_in, n, comm, d_out, cap, packed=None, gather=None):
        """One rank of a multi-GPU encode (bz_gpu_encode_sharded).  `comm` carries a `struct` attribute
        holding a bz_shard_comm (sharded.TorchComm).  packed / gather: optional (pointer, words)
        device buffers for this rank's bit strings / everybody's on rank 0.  -> stream bytes (0 on ranks > 0)."""
        _settle()
        out_len = C.c_size_t(0)
        pp, pw = packed if packed else (None, 0)
        gp, gw = gather if gather else (None, 0)
        _check(lib().bz_gpu_encode_sharded(self._h, level, d_in, n, C.byref(comm.struct), pp, pw, gp, gw, d_out, cap,
                                           C.byref(out_len)))
        return out_len.value

    def encode_sharded_window(self, level, d_window, window_off, window_bytes, n, comm, d_out, cap, packed=None, gather=None):
        """encode_sharded for a rank that holds only the input bytes [window_off, window_off + window_bytes) of the
        n-byte input at d_window (shard_window() says which bytes a rank needs)."""
        _settle()
        out_len = C.c_size_t(0)
        pp, pw = packed if packed else (None, 0)
        gp, gw = gather if gather else (None, 0)
        _check(lib().bz_gpu_encode_sharded_window(self._h, level, d_window, window_off, window_bytes, n, C.byref(comm.struct),
                                                  pp, pw, gp, gw, d_out, cap, C.byref(out_len)))
        return out_len.value

    def shard_timings(self):
        """ms of the last sharded encode on this rank: waiting for the cut, this rank's link of the chain, gather, assembly"""
        t = (C.c_double * 4)()
        _check(lib().bz_gpu_last_shard_timings(self._h, t))
        return dict(zip(("wait_for_cut_ms", "chain_link_ms", "gather_ms", "assemble_ms"), [round(x, 3) for x in t]))

    def shard_phases(self):
        """shard_timings() and: entry -> ready for the cut (nothing of it waits for another rank's cuts), the cuts alone
        once the hop is there, the whole call"""
        t = (C.c_double * 8)()
        _check(lib().bz_gpu_last_shard_phases(self._h, t))
        return dict(zip(("wait_for_cut_ms", "chain_link_ms", "gather_ms", "assemble_ms", "before_the_cut_ms", "cuts_ms", "_", "call_ms"),
                        [round(x, 3) for x in t]))

    DEC_STAGES = ("scan_huffman", "mtf", "inverse_bwt", "rle1_crc", "total")

    def decode_device(self, d_in, n, d_out, cap):
        """-> (bytes decoded, verdict).  d_out = None: sizes only."""
        _settle()
        out_len = C.c_size_t(0)
        rc = lib().bz_gpu_decode_device(self._h, d_in, n, d_out, cap, C.byref(out_len))
        if rc != BZ_OK and rc not in _DECODER_VERDICTS:
            raise CompressionError(rc)
        return out_len.value, rc

    def decode_batch_device(self, d_in, in_off, in_len, d_out, cap):
        """Many independent streams (bz_gpu_decode_batch_device): entry i is the in_len[i] bytes at d_in + in_off[i]
        (offsets multiples of 4, in ascending order -- what encode_batch_device returns); -> (out_off, out_len, verdicts),
        the bytes of entry i at d_out + out_off[i] (multiples of 16).  d_out = None: sizes only."""
        _settle()
        k = len(in_off)
        if len(in_len) != k:
            raise ValueError("decode_batch_device: in_off and in_len differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        verdicts = (C.c_int32 * max(k, 1))()
        _check(lib().bz_gpu_decode_batch_device(self._h, d_in, a_off, a_len, k, d_out, cap, o_off, o_len, verdicts))
        return list(o_off[:k]), list(o_len[:k]), [int(v) for v in verdicts[:k]]

    def decode_batch_stats(self):
        """The last decode_batch_device call: [0] entries decoded by the batch path, [1] entries that took the
        one-stream path, [2] blocks rebuilt for the former, [3] groups (bz_gpu_last_decode_batch_stats)."""
        s = (C.c_uint64 * 4)()
        _check(lib().bz_gpu_last_decode_batch_stats(self._h, s))
        return [int(x) for x in s]

    def decode_device_sharded(self, d_in, n, d_out, cap, rank, world, allgather):
        """One rank of a multi-GPU decode.  `allgather(send: bytes) -> bytes` returns the concatenation of
        every rank's `send`, in rank order (sharded.allgather_bytes wraps torch.distributed).
        -> (bytes in this rank's slice, offset of the slice in the decoded file, total bytes, verdict)"""
        _settle()
        def cb(_ctx, send, nbytes, recv):
            try:
                got = allgather(C.string_at(send, nbytes))
                if len(got) != nbytes * world:
                    return 1
                C.memmove(recv, got, len(got))
                return 0
            except Exception:  # the C side turns this into BZ_E_UNEXPECTED
                return 1
        fn = ALLGATHER_FN(cb)
        out_len, off, tot = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = lib().bz_gpu_decode_device_sharded(self._h, d_in, n, d_out, cap, rank, world, fn, None,
                                                C.byref(out_len), C.byref(off), C.byref(tot))
        if rc != BZ_OK and rc not in _DECODER_VERDICTS:
            raise CompressionError(rc)
        return out_len.value, off.value, tot.value, rc

    DEFLATE_STAGES = ("hash_chains", "matches", "parse", "blocks_tables", "emit_checksums", "total")

    def deflate_encode_device(self, kind, d_in, n, d_out, cap, dict_=b""):
        _settle()
        out_len = C.c_size_t(0)
        dict_ = bytes(dict_)
        _check(lib().df_gpu_encode_device_dict(self._h, kind, d_in, n, dict_, len(dict_), d_out, cap, C.byref(out_len)))
        return out_len.value

    DEFLATE_BATCH_STATS = ("inputs_batched", "inputs_one_by_one", "sub_batches", "stored", "fixed", "dynamic", "limited_tables",
                           "dynamic_without_distances")

    def deflate_encode_batch_device(self, kind, d_in, in_off, in_len, d_out, cap, dict_=b""):
        """Many inputs, one stream each (df_gpu_encode_batch_device_dict): input i is the in_len[i] bytes at d_in + in_off[i]
        (offsets multiples of 16, in ascending order); returns (out_off, out_len), stream i at d_out + out_off[i].  dict_
        (host bytes): one preset dictionary for every input, kinds DEFLATE and ZLIB (a kind outside 0..2 is the C call's
        BZ_E_PARAM, as ever)."""
        dict_ = _encode_dict(kind, dict_) if kind in (DEFLATE, ZLIB, GZIP) else bytes(dict_)
        _settle()
        k = len(in_off)
        if len(in_len) != k:
            raise ValueError("deflate_encode_batch_device: in_off and in_len differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        _check(lib().df_gpu_encode_batch_device_dict(self._h, kind, d_in, a_off, a_len, k, dict_, len(dict_), d_out, cap, o_off, o_len))
        return list(o_off[:k]), list(o_len[:k])

    def deflate_batch_stats(self):
        """The last deflate_encode_batch_device call, in the order of DEFLATE_BATCH_STATS (df_gpu_last_batch_stats);
        the block counts are those of the batch-path inputs."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_batch_stats(self._h, s))
        return [int(x) for x in s]

    BGZF_STATS = ("blocks", "sub_batches", "stored", "fixed", "dynamic", "limited_tables", "strict_replaced", "file_bytes")

    def bgzf_encode_device(self, d_in, n, d_out, cap, block_bytes=0, eof=True, offsets=False):
        """The n bytes at d_in (16-byte aligned) as a BGZF file at d_out, any alignment (df_gpu_bgzf_encode_device); returns
        the file's length, or with offsets=True (length, offsets): count + 1 file offsets, where block k starts and last
        where the EOF marker starts.  block_bytes outside 0 .. 65 280 is the C call's BZ_E_PARAM."""
        _settle()
        out_len = C.c_uint64(0)
        k = bgzf_block_count(n, block_bytes) if 0 <= block_bytes <= BGZF_BLOCK else 0
        offs = (C.c_uint64 * (k + 1))()
        _check(lib().df_gpu_bgzf_encode_device(self._h, d_in, n, block_bytes, 1 if eof else 0, d_out, cap, C.byref(out_len), offs))
        return (out_len.value, [int(x) for x in offs]) if offsets else out_len.value

    def bgzf_stats(self):
        """The last bgzf_encode_device call, in the order of BGZF_STATS (df_gpu_last_bgzf_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_bgzf_stats(self._h, s))
        return [int(x) for x in s]

    BGZF_READ_STATS = ("blocks_decoded", "in_place", "edge_blocks", "candidates", "never_landed_on", "decoded_bytes", "delivered_bytes", "launches")

    def bgzf_index_device(self, d_in, in_len, cap_blocks=None):
        """The block index of the BGZF file d_in[in_len] in device memory, 16-byte aligned (df_gpu_bgzf_index_device) -> a
        BgzfIndex whose verdict is the chain's.  cap_blocks: room for that many blocks (BZ_E_CAPACITY raises); None:
        room for one block per 4 KiB of file, and a second call with the count the first one reports if that is too few."""
        _settle()
        cap = in_len // 4096 + 64 if cap_blocks is None else cap_blocks
        n = C.c_size_t(0)
        v = C.c_int32(0)
        while True:
            coff, uoff = (C.c_uint64 * (cap + 1))(), (C.c_uint64 * (cap + 1))()
            rc = lib().df_gpu_bgzf_index_device(self._h, d_in, in_len, coff, uoff, cap, C.byref(n), C.byref(v))
            if rc != BZ_E_CAPACITY or cap_blocks is not None or n.value <= cap:
                break
            cap = n.value
        _check(rc)
        return BgzfIndex(coff[:n.value + 1], uoff[:n.value + 1], v.value)

    def bgzf_read_device(self, d_in, in_len, index, ustart, ulen, d_out, cap):
        """The uncompressed bytes [ustart, ustart + ulen), clamped to the index's end, of the BGZF file at d_in (16-byte aligned)
        at d_out, any alignment (df_gpu_bgzf_read_device) -> (out_len, verdict).  index: a BgzfIndex, or a (coff, uoff) pair of
        count + 1 entries each, relative to d_in.  d_out = None: sizes only."""
        if not isinstance(index, BgzfIndex):
            index = BgzfIndex(index[0], index[1])
        _settle()
        coff, uoff = index._arrays()
        n = C.c_uint64(0)
        v = C.c_int32(0)
        _check(lib().df_gpu_bgzf_read_device(self._h, d_in, in_len, coff, uoff, index.blocks, ustart, ulen, d_out, cap, C.byref(n), C.byref(v)))
        return int(n.value), int(v.value)

    def bgzf_read_stats(self):
        """The last bgzf_read_device call and, [3] and [4], the last bgzf_index_device call, in the order of BGZF_READ_STATS
        (df_gpu_last_bgzf_read_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_bgzf_read_stats(self._h, s))
        return [int(x) for x in s]

    DEFLATE_DECODE_BATCH_STATS = ("clean", "errors", "stored", "fixed", "dynamic", "decoded_bytes", "consumed_bytes", "launches")

    def deflate_decode_batch_device(self, kind, d_in, in_off, in_len, d_out, cap, dict_=b""):
        """Many streams in one call (df_gpu_decode_batch_device_dict): entry i is the in_len[i] bytes at d_in + in_off[i]
        (offsets multiples of 4, ascending -- what deflate_encode_batch_device returns); returns (out_off, out_len, verdicts),
        entry i's bytes at d_out + out_off[i].  d_out = None: sizes only.  dict_ (host bytes): one preset dictionary for every
        entry, kinds DEFLATE and ZLIB (a kind outside 0..2 is the C call's BZ_E_PARAM, as ever)."""
        dict_ = _decode_dict(kind, dict_) if kind in (DEFLATE, ZLIB, GZIP) else bytes(dict_)
        _settle()
        k = len(in_off)
        if len(in_len) != k:
            raise ValueError("deflate_decode_batch_device: in_off and in_len differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        verdicts = (C.c_int32 * max(k, 1))()
        _check(lib().df_gpu_decode_batch_device_dict(self._h, kind, d_in, a_off, a_len, k, dict_, len(dict_), d_out, cap, o_off, o_len, verdicts))
        return list(o_off[:k]), list(o_len[:k]), [int(v) for v in verdicts[:k]]

    LZH_DECODE_STATS = ("clean", "errors", "blocks", "literals", "matches", "decoded_bytes", "consumed_bytes", "launches")

    def lzh_decode_batch_device(self, method, d_in, in_off, in_len, d_out, cap, orig_len=None, prefill=-1):
        """Many LZHUF streams in one call (bz_gpu_lzh_decode_batch_device; section 9 of the header): entry i is the
        in_len[i] bytes at d_in + in_off[i] (offsets multiples of 4, ascending); returns (out_off, out_len, verdicts), entry
        i's bytes at d_out + out_off[i].  d_out = None: sizes only.  orig_len: None, or one length per entry (None: not
        known).  A method outside 4..7 or a prefill outside -1..255 is the C call's BZ_E_PARAM."""
        _settle()
        k = len(in_off)
        if len(in_len) != k or (orig_len is not None and len(orig_len) != k):
            raise ValueError("lzh_decode_batch_device: the per-entry arrays differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        a_ol = None if orig_len is None else (C.c_uint64 * max(k, 1))(*[_lzh_len(x) for x in orig_len])
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        verdicts = (C.c_int32 * max(k, 1))()
        _check(lib().bz_gpu_lzh_decode_batch_device(self._h, int(method), int(prefill), d_in, a_off, a_len, a_ol, k, d_out, cap, o_off, o_len,
                                                    verdicts))
        return list(o_off[:k]), list(o_len[:k]), [int(v) for v in verdicts[:k]]

    def lzh_decode_stats(self):
        """The last lzh_decode_batch_device call, in the order of LZH_DECODE_STATS (bz_gpu_last_lzh_decode_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().bz_gpu_last_lzh_decode_stats(self._h, s))
        return [int(x) for x in s]

    LHA_READ_STATS = ("clean", "errors", "stored", "directories", "not_decodable", "crc_mismatches", "bytes_out", "launches")

    def lha_read_device(self, d_in, in_len, index, d_out, cap, members=None, prefill=0x20):
        """Members of the LHA archive at d_in (in_len bytes of device memory, 16-byte aligned) in one call
        (bz_gpu_lha_read_device; section 11 of the header).  index: what lha_index gave for the same bytes; members: None
        (all) or ascending indices.  Returns (out_off, out_len, verdicts) in selection order, member k's bytes at d_out +
        out_off[k].  d_out = None: sizes and verdicts only."""
        _settle()
        n = len(index)
        k = n if members is None else len(members)
        sel = None if members is None else (C.c_size_t * max(k, 1))(*members)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        verdicts = (C.c_int32 * max(k, 1))()
        _check(lib().bz_gpu_lha_read_device(self._h, d_in, in_len, index._records, n, sel, k, int(prefill), d_out, cap, o_off, o_len, verdicts))
        return list(o_off[:k]), list(o_len[:k]), [int(v) for v in verdicts[:k]]

    def lha_read_stats(self):
        """The last lha_read_device call, in the order of LHA_READ_STATS (bz_gpu_last_lha_read_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().bz_gpu_last_lha_read_stats(self._h, s))
        return [int(x) for x in s]

    LHA_WRITE_STATS = ("members", "compressed", "stored_by_rule", "stored_by_request", "directories", "bytes_in", "archive_bytes", "launches")

    def lha_write_device(self, d_in, in_off, in_len, entries, d_out, cap, method=LzhufMethod.Lh5, level=2):
        """An LHA archive of the inputs d_in + in_off[i] (in_len[i] bytes of device memory each; d_in and the offsets 16-byte
        aligned, ascending, disjoint) at d_out in one call (bz_gpu_lha_write_device; section 12 of the header).  entries: one
        LhaEntry (or name) per input.  Returns (out_len, LhaIndex): the archive's length and the member table that lha_index
        would build from its bytes (names and directories are the entries')."""
        _settle()
        recs, keep = _lha_entries(entries)
        k = len(keep)
        if len(in_off) != k or len(in_len) != k:
            raise ValueError("lha_write_device: the per-member arrays differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        table = (_LhaMemberRec * max(k, 1))()
        n = C.c_size_t(0)
        _check(lib().bz_gpu_lha_write_device(self._h, _lha_method(method), int(level), d_in, a_off, a_len, recs, k, d_out, cap, C.byref(n), table))
        idx = LhaIndex(LhaMember(e.name, e.directory, bytes(r.method_id), r.level, r.packed_len, r.orig_len, r.crc16, r.mtime, r.os_id, r.data_off,
                                 r.header_off, r.attr) for r, e in zip(table, keep))
        idx._records = table
        return n.value, idx

    def lha_write_stats(self):
        """The last lha_write_device call, in the order of LHA_WRITE_STATS (bz_gpu_last_lha_write_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().bz_gpu_last_lha_write_stats(self._h, s))
        return [int(x) for x in s]

    LZH_DECODE_SPLIT_STATS = ("entries_split", "candidates", "chain_pieces", "false_pieces", "pieces_decoded_again", "jump_rounds",
                              "gathered_bytes", "fallbacks")

    def lzh_decode_split_stats(self):
        """The entries of the last lzh_decode_batch_device call that went across many waves, in the order of
        LZH_DECODE_SPLIT_STATS (bz_gpu_last_lzh_decode_split_stats; section 9 (g) of the header)."""
        s = (C.c_uint64 * 8)()
        _check(lib().bz_gpu_last_lzh_decode_split_stats(self._h, s))
        return [int(x) for x in s]

    def lzh_decode_split_timings(self):
        """Seconds the last call's split entries spent in: search, sizes, pieces decoded again, writing, jump, gather."""
        s = (C.c_double * 6)()
        _check(lib().bz_gpu_last_lzh_decode_split_timings(self._h, s))
        return [float(x) for x in s]

    LZH_ENCODE_STATS = ("inputs", "sub_batches", "blocks", "literals", "matches", "input_bytes", "stream_bytes", "limited_tables")

    def lzh_encode_batch_device(self, method, d_in, in_off, in_len, d_out, cap):
        """Many inputs, one LZHUF stream each (bz_gpu_lzh_encode_batch_device; section 10 of the header): input i is the
        in_len[i] bytes at d_in + in_off[i] (offsets multiples of 16, ascending); returns (out_off, out_len), stream i at
        d_out + out_off[i] (multiples of 4).  A method outside 4..7 is the C call's BZ_E_PARAM."""
        _settle()
        k = len(in_off)
        if len(in_len) != k:
            raise ValueError("lzh_encode_batch_device: in_off and in_len differ in length")
        a_off = (C.c_uint64 * max(k, 1))(*in_off)
        a_len = (C.c_uint64 * max(k, 1))(*in_len)
        o_off = (C.c_uint64 * max(k, 1))()
        o_len = (C.c_uint64 * max(k, 1))()
        _check(lib().bz_gpu_lzh_encode_batch_device(self._h, int(method), d_in, a_off, a_len, k, d_out, cap, o_off, o_len))
        return list(o_off[:k]), list(o_len[:k])

    def lzh_encode_stats(self):
        """The last lzh_encode_batch_device call, in the order of LZH_ENCODE_STATS (bz_gpu_last_lzh_encode_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().bz_gpu_last_lzh_encode_stats(self._h, s))
        return [int(x) for x in s]

    def lzh_debug_codes(self, method, d_in, n):
        """The LZSS codes of the n bytes at d_in under `method` (bz_gpu_lzh_debug_codes): numpy uint32 [count, 2] of
        (len, pos); len 0: the literal pos, else a match of len bytes at distance pos + 1."""
        import numpy as np
        _settle()
        buf = np.zeros((n + 1, 2), dtype=np.uint32)
        cnt = C.c_size_t(0)
        _check(lib().bz_gpu_lzh_debug_codes(self._h, int(method), d_in, n, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n + 1, C.byref(cnt)))
        return buf[:cnt.value]

    def lzh_debug_tables(self, method, c_freq, p_freq):
        """The block stage's table builder on 510 c-counts and 17 p-counts (bz_gpu_lzh_debug_tables) ->
        (c_len[510], p_len[17], t_len[19], header bits, flags, limited tables)."""
        _settle()
        if len(c_freq) != 510 or len(p_freq) != 17:
            raise ValueError("lzh_debug_tables: 510 c-counts and 17 p-counts")
        cf = (C.c_uint32 * 510)(*c_freq)
        pf = (C.c_uint32 * 17)(*p_freq)
        cl, pl, tl = (C.c_uint8 * 510)(), (C.c_uint8 * 17)(), (C.c_uint8 * 19)()
        res = (C.c_uint32 * 3)()
        _check(lib().bz_gpu_lzh_debug_tables(self._h, int(method), cf, pf, cl, pl, tl, res))
        return list(cl), list(pl), list(tl), int(res[0]), int(res[1]), int(res[2])

    def deflate_decode_batch_stats(self):
        """The last deflate_decode_batch_device call, in the order of DEFLATE_DECODE_BATCH_STATS
        (df_gpu_last_decode_batch_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_decode_batch_stats(self._h, s))
        return [int(x) for x in s]

    def deflate_decode_split_stats(self):
        """The entries of the last deflate_decode_batch_device call that were split across many waves: [0] entries split
        [1] pieces with a candidate [2] pieces confirmed without repair [3] repair rounds [4] output bytes of the serial tail
        [5] bytes left unresolved by the writing launch [6] jump rounds [7] kernel launches (df_gpu_last_decode_split_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_decode_split_stats(self._h, s))
        return [int(x) for x in s]

    GZIP_MEMBERS_STATS = ("members", "candidates", "never_confirmed", "redecodes", "zero_bytes", "split_members", "sub_batches", "launches")
    GZIP_MEMBERS_STAGES = ("search", "gather", "zero_skip", "compaction")

    def gzip_decode_members_device(self, d_in, in_len, d_out, cap):
        """Every member of the gzip file d_in[in_len] (16-byte aligned), side by side at d_out (df_gpu_decode_members_device)
        -> (out_len, verdict).  d_out = None: sizes only, out_len is the capacity the real call needs."""
        _settle()
        n = C.c_uint64(0)
        v = C.c_int32(0)
        _check(lib().df_gpu_decode_members_device(self._h, d_in, in_len, d_out, cap, C.byref(n), C.byref(v)))
        return int(n.value), int(v.value)

    def gzip_decode_members_stats(self):
        """The last gzip_decode_members_device call, in the order of GZIP_MEMBERS_STATS (df_gpu_last_decode_members_stats)."""
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_decode_members_stats(self._h, s))
        return [int(x) for x in s]

    def gzip_decode_members_timings(self):
        """Seconds per stage of the last gzip_decode_members_device call (df_gpu_last_decode_members_timings)."""
        t = (C.c_double * 4)()
        _check(lib().df_gpu_last_decode_members_timings(self._h, t))
        return dict(zip(self.GZIP_MEMBERS_STAGES, t))

    DEFLATE_DECODE_SPLIT_PHASES = ("search", "sizes", "repair", "writing", "jump_rounds", "gather", "checksum")

    def deflate_decode_split_timings(self):
        """Seconds per phase of the split entries of the last deflate_decode_batch_device call
        (df_gpu_last_decode_split_timings)."""
        t = (C.c_double * 7)()
        _check(lib().df_gpu_last_decode_split_timings(self._h, t))
        return dict(zip(self.DEFLATE_DECODE_SPLIT_PHASES, t))

    def deflate_timings(self):
        t = (C.c_double * 6)()
        _check(lib().df_gpu_last_timings(self._h, t))
        return dict(zip(self.DEFLATE_STAGES, t))

    def deflate_stats(self):
        s = (C.c_uint64 * 8)()
        _check(lib().df_gpu_last_stats(self._h, s))
        return dict(blocks=s[0], stored=s[1], fixed=s[2], dynamic=s[3], limited_tables=s[4], stream_bytes=s[5],
                    dynamic_without_distances=s[6])

    def deflate_debug_codes(self, d_in, n):
        """numpy uint32 [count, 2] of (len, pos); len 0: literal pos"""
        import numpy as np
        buf = np.zeros((n + 1, 2), dtype=np.uint32)
        cnt = C.c_size_t(0)
        _check(lib().df_gpu_debug_codes(self._h, d_in, n, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n + 1, C.byref(cnt)))
        return buf[:cnt.value]

    def deflate_debug_blocks(self):
        cnt = C.c_size_t(0)
        _check(lib().df_gpu_debug_blocks(self._h, None, 0, C.byref(cnt)))
        buf = (C.c_uint64 * (4 * max(cnt.value, 1)))()
        _check(lib().df_gpu_debug_blocks(self._h, buf, cnt.value, C.byref(cnt)))
        return [tuple(buf[4 * i + k] for k in range(4)) for i in range(cnt.value)]

    def decode_timings(self):
        t = (C.c_double * 5)()
        _check(lib().bz_gpu_last_decode_timings(self._h, t))
        return dict(zip(self.DEC_STAGES, t))

    def decode_stats(self):
        s = (C.c_uint64 * 4)()
        _check(lib().bz_gpu_last_decode_stats(self._h, s))
        return dict(zip(("candidates", "blocks", "streams", "forced_blocks"), [int(x) for x in s]))

    def timings(self):
        t = (C.c_double * 6)()
        _check(lib().bz_gpu_last_timings(self._h, t))
        return dict(zip(self.STAGES, t))

    def profile(self, on=True):
        _check(lib().bz_gpu_profile_enable(self._h, int(on)))

    def kernel_profile(self):
        """{kernel: {launches, seconds, bytes}} accumulated since profile(True)."""
        out = {}
        for i in range(lib().bz_gpu_profile_kernels(self._h)):
            name, n, s, b = C.c_char_p(), C.c_uint64(0), C.c_double(0), C.c_uint64(0)
            _check(lib().bz_gpu_profile_get(self._h, i, C.byref(name), C.byref(n), C.byref(s), C.byref(b)))
            out[name.value.decode()] = {"launches": n.value, "seconds": s.value, "bytes": b.value}
        return out

    def cut_stats(self):
        """Partitions of this engine whose block cuts came from the candidate tables / that fell back to the chain kernel."""
        s = (C.c_uint64 * 2)()
        _check(lib().bz_gpu_cut_stats(self._h, s))
        return {"from_tables": int(s[0]), "fell_back": int(s[1])}

    def bwt_stats(self):
        s = (C.c_uint64 * 4)()
        _check(lib().bz_gpu_last_bwt_stats(self._h, s))
        r = (C.c_uint64 * 64)()
        _check(lib().bz_gpu_last_bwt_rounds(self._h, r))
        unordered = [int(x) for x in r]
        while unordered and unordered[-1] == 0:
            unordered.pop()
        return {"rounds": s[0], "resorted_elements": s[1], "batches": s[2], "unordered_after_round": unordered,
                "fused_fallbacks": s[3]}  # sorts of this engine that fell back to the three-kernel passes (it stays on them)

    def block_stats(self):
        n = C.c_size_t(0)
        _check(lib().bz_gpu_debug_block_stats(self._h, None, 0, C.byref(n)))
        buf = (C.c_uint32 * (8 * max(n.value, 1)))()
        _check(lib().bz_gpu_debug_block_stats(self._h, buf, n.value, C.byref(n)))
        keys = ("nblock", "block_crc", "orig_ptr", "mtf_count", "in_use_count", "group_num", "n_selectors")
        out = []
        for i in range(n.value):
            d = dict(zip(keys, buf[i * 8:i * 8 + 7]))
            d["max_len"] = buf[i * 8 + 7] & 0xFFFF
            d["lm_tables"] = buf[i * 8 + 7] >> 16
            out.append(d)
        return out

    def block_sections(self):
        """Per block of the last encode: the figures of the reference's debug lines "pass k: size is .., grp uses are .." and
        "bits: mapping .., selectors .., code lengths .., codes .." (src/bzip2/encoder.rs:483-498, :556-636)."""
        n = C.c_size_t(0)
        _check(lib().bz_gpu_debug_block_sections(self._h, None, 0, C.byref(n)))
        buf = (C.c_uint32 * (32 * max(n.value, 1)))()
        _check(lib().bz_gpu_debug_block_sections(self._h, buf, n.value, C.byref(n)))
        out = []
        for i in range(n.value):
            w = buf[i * 32:(i + 1) * 32]
            out.append({"pass_size": list(w[0:4]), "fave": [list(w[4 + 6 * k:10 + 6 * k]) for k in range(4)],
                        "bits_mapping": w[28], "bits_selectors": w[29], "bits_lengths": w[30], "bits_codes": w[31]})
        return out

    # stage probes
    def debug_bwt(self, block):
        block = bytes(block)
        sa = (C.c_uint32 * len(block))()
        _check(lib().bz_gpu_debug_bwt(self._h, block, len(block), sa))
        return list(sa)

    def debug_mtf(self, columns, heads=-1):
        """The MTF + zero-run stage on a batch of last columns: [(symbols, mtf_count, in_use_count, mtf_freq)] per column.
        heads: 1 / 0 force the form that ranks only the run heads / every position, -1 follows BZ_MTF_HEADS."""
        columns = [bytes(c) for c in columns]
        nb = len(columns)
        off, lens, pos = (C.c_uint64 * nb)(), (C.c_uint32 * nb)(), 0
        for i, c in enumerate(columns):
            off[i], lens[i] = pos, len(c)
            pos += len(c)
        stride = max(len(c) for c in columns) + 1
        sym = (C.c_uint16 * (nb * stride))()
        cnt, use, freq = (C.c_uint32 * nb)(), (C.c_uint32 * nb)(), (C.c_uint32 * (nb * 258))()
        _check(lib().bz_gpu_debug_mtf(self._h, nb, b"".join(columns), off, lens, int(heads), sym, stride, cnt, use, freq))
        out = []
        for i in range(nb):
            out.append((list(sym[i * stride:i * stride + cnt[i]]), int(cnt[i]), int(use[i]), list(freq[i * 258:(i + 1) * 258])))
        return out

    def debug_code_lengths(self, freq):
        n = len(freq)
        f = (C.c_uint32 * n)(*freq)
        out = (C.c_uint8 * n)()
        lm = C.c_int(0)
        _check(lib().bz_gpu_debug_code_lengths(self._h, f, n, out, C.byref(lm)))
        return list(out), bool(lm.value)
