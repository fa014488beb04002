//! The C ABI of libbz2_mi355x.so (include/bz2_mi355x.h), as far as the codec types need it.
//! Linking is set up by build.rs.
#![allow(non_camel_case_types)]
use core::ffi::c_void;

pub type bz_enc = c_void;
pub type bz_dec = c_void;
pub type df_enc = c_void;

pub const BZ_OK: i32 = 0;
pub const BZ_E_PARAM: i32 = -6; // invalid level: the reference panics (src/bzip2/encoder.rs:59-61)
pub const BZ_E_NOGPU: i32 = -7; // no gfx950 device / HIP runtime unusable: the path has no CPU fallback
pub const BZ_E_NOMEM: i32 = -8;

pub const DF_KIND_DEFLATE: i32 = 0;
pub const DF_KIND_ZLIB: i32 = 1;
pub const DF_KIND_GZIP: i32 = 2;

/// `bz_lha_member`: one member of an LHA archive as `bz_lha_index_buffer` lists it (72 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct LhaMember {
    pub header_off: u64,
    pub data_off: u64,
    pub packed_len: u64,
    pub orig_len: u64,
    pub name_off: u64,
    pub dir_off: u64,
    pub name_len: u32,
    pub dir_len: u32,
    pub mtime: u32,
    pub crc16: u16,
    pub method: u8, // 0 stored, 1 directory, 4 .. 7 -lh4- .. -lh7-, 255 not decodable
    pub level: u8,
    pub os_id: u8,
    pub attr: u8,
    pub method_id: [u8; 5],
    pub pad: u8,
}

/// `bz_lha_entry`: what `bz_lha_write_buffer` writes into a member's header beside its sizes and CRC (40 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct LhaEntry {
    pub name: *const u8,
    pub name_len: u32,
    pub dir: *const u8, // components separated by 0xFF; may be empty
    pub dir_len: u32,
    pub mtime: u32,
    pub attr: u8,
    pub os_id: u8,
    pub is_dir: u8,
    pub pad: u8,
}

extern "C" {
    pub fn bz_device_count() -> i32;
    pub fn bz_strerror(code: i32) -> *const core::ffi::c_char;

    // section 1: BZip2Encoder (src/bzip2/encoder.rs:40-159)
    pub fn bz_enc_create(out: *mut *mut bz_enc, level: i32, device: i32) -> i32;
    pub fn bz_enc_create_multi(out: *mut *mut bz_enc, level: i32, devices: *const i32, n_devices: i32) -> i32;
    pub fn bz_enc_write(e: *mut bz_enc, data: *const u8, n: usize) -> i32;
    pub fn bz_enc_end(e: *mut bz_enc, action: i32) -> i32;
    pub fn bz_enc_read(e: *mut bz_enc, out: *mut u8, cap: usize) -> isize;
    pub fn bz_enc_pending(e: *const bz_enc) -> usize;
    pub fn bz_enc_destroy(e: *mut bz_enc);
    pub fn bz_enc_set_verify(e: *mut bz_enc, on: i32) -> i32;
    pub fn bz_enc_verify_stats(e: *mut bz_enc, out: *mut u64) -> i32;
    // many inputs, one stream each, in one pass of the pipeline; *out is released with bz_free
    pub fn bz_encode_batch(level: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64) -> i32;
    pub fn bz_free(p: *mut c_void);

    // section 3: BZip2Decoder (src/bzip2/decoder.rs:583-612)
    pub fn bz_dec_create(out: *mut *mut bz_dec, device: i32) -> i32;
    pub fn bz_dec_write(d: *mut bz_dec, data: *const u8, n: usize) -> i32;
    pub fn bz_dec_end(d: *mut bz_dec) -> i32;
    pub fn bz_dec_read(d: *mut bz_dec, out: *mut u8, cap: usize) -> isize;
    pub fn bz_dec_destroy(d: *mut bz_dec);
    // many streams in one call: bytes and verdict per entry; *out is released with bz_free
    pub fn bz_decode_batch(device: i32, ins: *const *const u8, lens: *const usize, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64, verdict: *mut i32) -> i32;

    // section 4: Inflater / ZlibEncoder / GZipEncoder
    pub fn df_enc_create(out: *mut *mut df_enc, kind: i32, device: i32) -> i32;
    pub fn df_enc_create_dict(out: *mut *mut df_enc, kind: i32, device: i32, dict: *const u8, dict_len: usize) -> i32;
    pub fn df_enc_write(e: *mut df_enc, data: *const u8, n: usize) -> i32;
    pub fn df_enc_end(e: *mut df_enc, action: i32) -> i32;
    pub fn df_enc_finished(e: *const df_enc) -> i32;
    pub fn df_enc_read(e: *mut df_enc, out: *mut u8, cap: usize) -> isize;
    pub fn df_enc_destroy(e: *mut df_enc);
    pub fn df_encode_batch_bound(in_len: *const u64, count: usize) -> usize;
    pub fn df_gpu_encode_batch_device(g: *mut c_void, kind: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, count: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64) -> i32;
    pub fn df_gpu_last_batch_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_encode_batch(kind: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64) -> i32;
    pub fn df_gpu_encode_batch_device_dict(g: *mut c_void, kind: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, count: usize, dict: *const u8, dict_len: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64) -> i32;
    pub fn df_encode_batch_dict(kind: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, dict: *const u8, dict_len: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64) -> i32;

    // section 5: Deflater / ZlibDecoder / GZipDecoder (many streams in one call; *out is released with bz_free)
    pub fn df_gpu_decode_batch_device(g: *mut c_void, kind: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, count: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64, h_verdict: *mut i32) -> i32;
    pub fn df_gpu_last_decode_batch_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_gpu_last_decode_split_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_gpu_last_decode_split_timings(g: *mut c_void, out_seconds: *mut f64) -> i32;
    pub fn df_decode_batch(kind: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64, verdict: *mut i32) -> i32;
    pub fn df_decode_buffer(kind: i32, device: i32, input: *const u8, in_len: usize, out: *mut *mut u8, out_len: *mut usize) -> i32;
    // ... with one preset dictionary (host memory) for every entry: Deflater::with_dict / ZlibDecoder::with_dict
    pub fn df_gpu_decode_batch_device_dict(g: *mut c_void, kind: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, count: usize, dict: *const u8, dict_len: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64, h_verdict: *mut i32) -> i32;
    pub fn df_decode_batch_dict(kind: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, dict: *const u8, dict_len: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64, verdict: *mut i32) -> i32;
    pub fn df_decode_buffer_dict(kind: i32, device: i32, input: *const u8, in_len: usize, dict: *const u8, dict_len: usize, out: *mut *mut u8, out_len: *mut usize) -> i32;

    // section 9: LZHUF decode (LzhufDecoder); h_orig_len / orig_lens may be null, an entry of u64::MAX is "not known"
    pub fn bz_gpu_lzh_decode_batch_device(g: *mut c_void, method: i32, prefill: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, h_orig_len: *const u64, count: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64, h_verdict: *mut i32) -> i32;
    pub fn bz_gpu_last_lzh_decode_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn bz_lzh_decode_batch(method: i32, prefill: i32, device: i32, ins: *const *const u8, lens: *const usize, orig_lens: *const u64, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64, verdict: *mut i32) -> i32;
    pub fn bz_lzh_decode_buffer(method: i32, prefill: i32, device: i32, input: *const u8, in_len: usize, orig_len: u64, out: *mut *mut u8, out_len: *mut usize) -> i32;
    // section 10: LZHUF encode (LzhufEncoder)
    pub fn bz_gpu_lzh_encode_batch_device(g: *mut c_void, method: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, count: usize, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64) -> i32;
    pub fn bz_gpu_last_lzh_encode_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn bz_lzh_encode_batch_bound(in_len: *const u64, count: usize) -> usize;
    pub fn bz_lzh_encode_batch(method: i32, device: i32, ins: *const *const u8, lens: *const usize, count: usize, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64) -> i32;
    pub fn bz_lzh_encode_buffer(method: i32, device: i32, input: *const u8, in_len: usize, out: *mut *mut u8, out_len: *mut usize) -> i32;
    // (test hooks: the LZSS codes of one input; the block stage's table builder on given counts)
    pub fn bz_gpu_lzh_debug_codes(g: *mut c_void, method: i32, d_in: *const c_void, n: usize, out_pairs: *mut u32, cap: usize, count: *mut usize) -> i32;
    pub fn bz_gpu_lzh_debug_tables(g: *mut c_void, method: i32, c_freq: *const u32, p_freq: *const u32, c_len: *mut u8, p_len: *mut u8, t_len: *mut u8, res: *mut u32) -> i32;

    // section 11: LHA archives, reading (members: *mut / *const LhaMember, the C struct bz_lha_member)
    pub fn bz_lha_index_buffer(input: *const u8, in_len: usize, members: *mut LhaMember, cap: usize, count: *mut usize, fault: *mut i32, fault_pos: *mut u64) -> i32;
    pub fn bz_gpu_lha_read_device(g: *mut c_void, d_in: *const c_void, in_len: usize, h_members: *const LhaMember, nmembers: usize, h_sel: *const usize, nsel: usize, prefill: i32, d_out: *mut c_void, cap: usize, h_out_off: *mut u64, h_out_len: *mut u64, h_verdict: *mut i32) -> i32;
    pub fn bz_gpu_last_lha_read_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn bz_lha_read_buffer(device: i32, input: *const u8, in_len: usize, sel: *const usize, nsel: usize, prefill: i32, out: *mut *mut u8, out_off: *mut u64, out_len: *mut u64, verdict: *mut i32, fault: *mut i32) -> i32;
    // section 12: LHA archives, writing (entries: *const LhaEntry, the C struct bz_lha_entry)
    pub fn bz_lha_write_bound(level: i32, e: *const LhaEntry, in_len: *const u64, count: usize) -> usize;
    pub fn bz_gpu_lha_write_device(g: *mut c_void, method: i32, level: i32, d_in: *const c_void, h_in_off: *const u64, h_in_len: *const u64, h_entries: *const LhaEntry, count: usize, d_out: *mut c_void, cap: usize, out_len: *mut usize, h_members: *mut LhaMember) -> i32;
    pub fn bz_gpu_last_lha_write_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn bz_lha_write_buffer(method: i32, level: i32, device: i32, ins: *const *const u8, lens: *const usize, entries: *const LhaEntry, count: usize, out: *mut *mut u8, out_len: *mut usize) -> i32;

    // section 6: every member of a gzip file (MultiGZipDecoder)
    pub fn df_gpu_decode_members_device(g: *mut c_void, d_in: *const c_void, in_len: usize, d_out: *mut c_void, cap: usize, out_len: *mut u64, verdict: *mut i32) -> i32;
    pub fn df_gpu_last_decode_members_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_gpu_last_decode_members_timings(g: *mut c_void, out_seconds: *mut f64) -> i32;
    pub fn df_decode_members_buffer(device: i32, input: *const u8, in_len: usize, out: *mut *mut u8, out_len: *mut usize) -> i32;

    // section 7: writing BGZF (gzip members of at most 65 280 input bytes; *out is released with bz_free)
    pub fn df_bgzf_block_count(n: usize, block_bytes: u32) -> usize;
    pub fn df_bgzf_bound(n: usize, block_bytes: u32, eof: i32) -> usize;
    pub fn df_gpu_bgzf_encode_device(g: *mut c_void, d_in: *const c_void, n: usize, block_bytes: u32, eof: i32, d_out: *mut c_void, cap: usize, out_len: *mut u64, h_block_off: *mut u64) -> i32;
    pub fn df_gpu_last_bgzf_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_bgzf_encode_buffer(device: i32, input: *const u8, n: usize, block_bytes: u32, eof: i32, out: *mut *mut u8, out_len: *mut usize, block_off: *mut u64) -> i32;

    // section 8: reading BGZF (the index from BSIZE, range reads; *coff, *uoff and *out are released with bz_free)
    pub fn df_bgzf_index_buffer(input: *const u8, in_len: usize, coff: *mut *mut u64, uoff: *mut *mut u64, count: *mut usize, verdict: *mut i32) -> i32;
    pub fn df_gpu_bgzf_index_device(g: *mut c_void, d_in: *const c_void, in_len: usize, h_coff: *mut u64, h_uoff: *mut u64, cap_blocks: usize, count: *mut usize, verdict: *mut i32) -> i32;
    pub fn df_gpu_bgzf_read_device(g: *mut c_void, d_in: *const c_void, in_len: usize, h_coff: *const u64, h_uoff: *const u64, count: usize, ustart: u64, ulen: u64, d_out: *mut c_void, cap: usize, out_len: *mut u64, verdict: *mut i32) -> i32;
    pub fn df_gpu_last_bgzf_read_stats(g: *mut c_void, out: *mut u64) -> i32;
    pub fn df_bgzf_read_buffer(device: i32, input: *const u8, in_len: usize, ustart: u64, ulen: u64, out: *mut *mut u8, out_len: *mut usize) -> i32;
}
