//! What the reference has no place for: which device, and why a call failed when the reason is not
//! one of `CompressionError`'s three variants.
use core::sync::atomic::{AtomicI32, Ordering};

use alloc::vec::Vec;

#[cfg(feature = "bzip2")]
use crate::bzip2::error::BZip2Error;
use crate::error::CompressionError;
use crate::ffi;

static LAST_STATUS: AtomicI32 = AtomicI32::new(0);

/// A status of the C ABI that the crate's error types cannot express.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Status {
    /// no usable gfx950 (MI355X) device or HIP runtime: this crate has no CPU path
    NoGpu,
    /// device or host memory exhausted
    NoMemory,
    /// `level` outside 1..=9 (the reference panics: `BZip2Encoder::new`)
    InvalidParameter,
    /// any other status (the raw BZ_E_* code)
    Other(i32),
}

impl Status {
    pub fn from_code(rc: i32) -> Self {
        match rc {
            ffi::BZ_E_NOGPU => Status::NoGpu,
            ffi::BZ_E_NOMEM => Status::NoMemory,
            ffi::BZ_E_PARAM => Status::InvalidParameter,
            other => Status::Other(other),
        }
    }
}

/// gfx950 devices this process can use (0: none -- every codec call will fail loudly).
pub fn device_count() -> usize {
    let n = unsafe { ffi::bz_device_count() };
    if n > 0 { n as usize } else { 0 }
}

/// The last non-zero status any codec of this process received from the library (0: none yet).
/// `CompressionError::Unexpected` from an encoder usually means "look here": e.g. `Status::NoGpu`.
pub fn last_status() -> Option<Status> {
    match LAST_STATUS.load(Ordering::Relaxed) {
        0 => None,
        rc => Some(Status::from_code(rc)),
    }
}

/// Many independent inputs in one call (`bz_encode_batch`, device 0): element `i` of the result is the stream
/// `inputs[i].iter().cloned().encode(&mut BZip2Encoder::new(level), Action::Finish)` collects, bit for bit.  Inputs that
/// are certain to be one block are encoded together, however many there are.  Panics on a level outside 1..=9, as
/// `BZip2Encoder::new` does.
pub fn encode_batch(level: usize, inputs: &[&[u8]]) -> Result<Vec<Vec<u8>>, CompressionError> {
    assert!((1..=9).contains(&level), "invalid level");
    let ptrs: Vec<*const u8> = inputs.iter().map(|x| x.as_ptr()).collect();
    let lens: Vec<usize> = inputs.iter().map(|x| x.len()).collect();
    let mut off: Vec<u64> = Vec::new();
    off.resize(inputs.len(), 0);
    let mut len = off.clone();
    let mut out: *mut u8 = core::ptr::null_mut();
    let rc = unsafe {
        ffi::bz_encode_batch(level as i32, 0, ptrs.as_ptr(), lens.as_ptr(), inputs.len(), &mut out, off.as_mut_ptr(), len.as_mut_ptr())
    };
    if rc != ffi::BZ_OK {
        return Err(CompressionError::from_status(rc));
    }
    let streams = (0..inputs.len())
        .map(|i| unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec())
        .collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(streams)
}

/// Many independent inputs in one call (`df_encode_batch`, device 0), `kind` 0 raw Deflate, 1 zlib, 2 gzip: element `i` of
/// the result is the stream `inputs[i].iter().cloned().encode(&mut Inflater::new(), Action::Finish)` (or `ZlibEncoder` /
/// `GZipEncoder`) collects, bit for bit.  Inputs of at most 65 535 bytes are one block for certain and are encoded together,
/// however many there are.  Panics on a kind outside 0..=2.
pub fn deflate_encode_batch(kind: usize, inputs: &[&[u8]]) -> Result<Vec<Vec<u8>>, CompressionError> {
    deflate_encode_batch_dict(kind, inputs, &[])
}

/// The same with one preset dictionary for every input (`df_encode_batch_dict`): element `i` is the stream of
/// `Inflater::with_dict(dict)` / `ZlibEncoder::with_dict(dict)` over `inputs[i]`.  An empty dictionary is none.  Panics on
/// a kind outside 0..=2 and on gzip with a dictionary (`GZipEncoder` has no `with_dict`).
pub fn deflate_encode_batch_dict(kind: usize, inputs: &[&[u8]], dict: &[u8]) -> Result<Vec<Vec<u8>>, CompressionError> {
    assert!(kind <= 2, "invalid kind");
    assert!(kind != 2 || dict.is_empty(), "gzip takes no preset dictionary");
    let ptrs: Vec<*const u8> = inputs.iter().map(|x| x.as_ptr()).collect();
    let lens: Vec<usize> = inputs.iter().map(|x| x.len()).collect();
    let mut off: Vec<u64> = Vec::new();
    off.resize(inputs.len(), 0);
    let mut len = off.clone();
    let mut out: *mut u8 = core::ptr::null_mut();
    let rc = unsafe {
        ffi::df_encode_batch_dict(
            kind as i32, 0, ptrs.as_ptr(), lens.as_ptr(), inputs.len(), dict.as_ptr(), dict.len(), &mut out, off.as_mut_ptr(), len.as_mut_ptr(),
        )
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let streams = (0..inputs.len())
        .map(|i| unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec())
        .collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(streams)
}

/// One input as a BGZF file (`df_bgzf_encode_buffer`, device 0): gzip members of at most `block_bytes` (0: 65 280) input
/// bytes side by side, then the 28-byte EOF marker when `eof` is set.  The reference has no such writer; every member is
/// a stream that zlib, gzip(1) and htslib read.  Returns the file and the file offset of every block, the last entry
/// being where the marker starts (the file's length without one).  Panics on a `block_bytes` above 65 280.
pub fn bgzf_encode(input: &[u8], block_bytes: u32, eof: bool) -> Result<(Vec<u8>, Vec<u64>), CompressionError> {
    assert!(block_bytes <= 65280, "invalid block size");
    let count = unsafe { ffi::df_bgzf_block_count(input.len(), block_bytes) };
    let mut off: Vec<u64> = Vec::new();
    off.resize(count + 1, 0);
    let mut out: *mut u8 = core::ptr::null_mut();
    let mut len: usize = 0;
    let rc = unsafe {
        ffi::df_bgzf_encode_buffer(0, input.as_ptr(), input.len(), block_bytes, eof as i32, &mut out, &mut len, off.as_mut_ptr())
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let file = unsafe { core::slice::from_raw_parts(out, len) }.to_vec();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok((file, off))
}

/// The block index of a BGZF file (`df_bgzf_index_buffer`): `coff[k]` / `uoff[k]` are where block `k` starts in the file and
/// in the uncompressed bytes, `count + 1` entries each, the last pair being the end of the last complete block -- the
/// `.gzi` table.  `verdict` is the chain's (0, or the status of a `DataError` / `UnexpectedEof`): the blocks in front of a
/// fault are still indexed.
pub struct BgzfIndex {
    pub coff: Vec<u64>,
    pub uoff: Vec<u64>,
    pub verdict: i32,
}

/// The BSIZE chain of a BGZF file, walked on the host: parsing, not decoding -- no GPU is needed.
pub fn bgzf_index(input: &[u8]) -> Result<BgzfIndex, CompressionError> {
    let mut c: *mut u64 = core::ptr::null_mut();
    let mut u: *mut u64 = core::ptr::null_mut();
    let mut count: usize = 0;
    let mut verdict: i32 = 0;
    let rc = unsafe { ffi::df_bgzf_index_buffer(input.as_ptr(), input.len(), &mut c, &mut u, &mut count, &mut verdict) };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let coff = unsafe { core::slice::from_raw_parts(c, count + 1) }.to_vec();
    let uoff = unsafe { core::slice::from_raw_parts(u, count + 1) }.to_vec();
    unsafe {
        ffi::bz_free(c as *mut core::ffi::c_void);
        ffi::bz_free(u as *mut core::ffi::c_void);
    }
    Ok(BgzfIndex { coff, uoff, verdict })
}

/// The uncompressed bytes `[ustart, ustart + ulen)` of a BGZF file, clamped to its end (`df_bgzf_read_buffer`, device 0):
/// only the blocks the range touches are uploaded and decoded.  `Err` carries the bytes of the range in front of the
/// fault.  Range reads pay off for ranges of many blocks, not for one record.
pub fn bgzf_read(input: &[u8], ustart: u64, ulen: u64) -> Result<Vec<u8>, (CompressionError, Vec<u8>)> {
    let mut out: *mut u8 = core::ptr::null_mut();
    let mut len: usize = 0;
    let rc = unsafe { ffi::df_bgzf_read_buffer(0, input.as_ptr(), input.len(), ustart, ulen, &mut out, &mut len) };
    let bytes = if out.is_null() {
        Vec::new()
    } else {
        let b = unsafe { core::slice::from_raw_parts(out, len) }.to_vec();
        unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
        b
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err((CompressionError::from_status(rc), bytes));
    }
    Ok(bytes)
}

/// A whole BGZF file: `bgzf_read` over everything.
pub fn bgzf_decode(input: &[u8]) -> Result<Vec<u8>, (CompressionError, Vec<u8>)> {
    bgzf_read(input, 0, u64::MAX)
}

/// Many independent streams in one call (`bz_decode_batch`, device 0): element `i` of the result is what
/// `inputs[i].iter().cloned().decode(&mut BZip2Decoder::new())` yields -- `Ok(bytes)`, or the `BZip2Error` with the bytes
/// the iterator hands out in front of it.  An entry's verdict is its own: a bad one hides nothing behind it.  The outer
/// `Err` is an infrastructure failure (`last_status` says which).
#[cfg(feature = "bzip2")]
pub fn decode_batch(inputs: &[&[u8]]) -> Result<Vec<Result<Vec<u8>, (BZip2Error, Vec<u8>)>>, CompressionError> {
    let ptrs: Vec<*const u8> = inputs.iter().map(|x| x.as_ptr()).collect();
    let lens: Vec<usize> = inputs.iter().map(|x| x.len()).collect();
    let mut off: Vec<u64> = Vec::new();
    off.resize(inputs.len(), 0);
    let mut len = off.clone();
    let mut verdict: Vec<i32> = Vec::new();
    verdict.resize(inputs.len(), 0);
    let mut out: *mut u8 = core::ptr::null_mut();
    let rc = unsafe {
        ffi::bz_decode_batch(0, ptrs.as_ptr(), lens.as_ptr(), inputs.len(), &mut out, off.as_mut_ptr(), len.as_mut_ptr(), verdict.as_mut_ptr())
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let entries = (0..inputs.len())
        .map(|i| {
            let bytes = unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec();
            if verdict[i] == ffi::BZ_OK { Ok(bytes) } else { Err((BZip2Error::from_status(verdict[i]), bytes)) }
        })
        .collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(entries)
}

/// Many independent LZHUF streams in one call (`bz_lzh_decode_batch`, device 0, strict): element `i` of the result is what
/// `inputs[i].iter().cloned().decode(&mut LzhufDecoder::new(&method))` yields -- `Ok(bytes)`, or the error with the bytes in
/// front of it.  `orig_lens`: empty, or the original length of every stream (`u64::MAX`: not known).  The outer `Err` is an
/// infrastructure failure (`last_status` says which).
#[cfg(feature = "lzhuf")]
pub fn lzh_decode_batch(method: crate::lzhuf::LzhufMethod, inputs: &[&[u8]], orig_lens: &[u64]) -> Result<Vec<Result<Vec<u8>, (CompressionError, Vec<u8>)>>, CompressionError> {
    if !orig_lens.is_empty() && orig_lens.len() != inputs.len() {
        return Err(CompressionError::from_status(ffi::BZ_E_PARAM));
    }
    let ptrs: Vec<*const u8> = inputs.iter().map(|x| x.as_ptr()).collect();
    let lens: Vec<usize> = inputs.iter().map(|x| x.len()).collect();
    let mut off: Vec<u64> = Vec::new();
    off.resize(inputs.len(), 0);
    let mut len = off.clone();
    let mut verdict: Vec<i32> = Vec::new();
    verdict.resize(inputs.len(), 0);
    let mut out: *mut u8 = core::ptr::null_mut();
    let ol = if orig_lens.is_empty() { core::ptr::null() } else { orig_lens.as_ptr() };
    let rc = unsafe {
        ffi::bz_lzh_decode_batch(method.abi(), -1, 0, ptrs.as_ptr(), lens.as_ptr(), ol, inputs.len(), &mut out, off.as_mut_ptr(), len.as_mut_ptr(), verdict.as_mut_ptr())
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let entries = (0..inputs.len())
        .map(|i| {
            let bytes = unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec();
            if verdict[i] == ffi::BZ_OK { Ok(bytes) } else { Err((CompressionError::from_status(verdict[i]), bytes)) }
        })
        .collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(entries)
}

/// Many independent inputs as LZHUF streams in one call (`bz_lzh_encode_batch`, device 0): element `i` of the result is
/// `inputs[i].iter().cloned().encode(&mut LzhufEncoder::new(&method), Action::Finish)` collected, byte for byte.
#[cfg(feature = "lzhuf")]
pub fn lzh_encode_batch(method: crate::lzhuf::LzhufMethod, inputs: &[&[u8]]) -> Result<Vec<Vec<u8>>, CompressionError> {
    let ptrs: Vec<*const u8> = inputs.iter().map(|x| x.as_ptr()).collect();
    let lens: Vec<usize> = inputs.iter().map(|x| x.len()).collect();
    let mut off: Vec<u64> = Vec::new();
    off.resize(inputs.len(), 0);
    let mut len = off.clone();
    let mut out: *mut u8 = core::ptr::null_mut();
    let rc = unsafe { ffi::bz_lzh_encode_batch(method.abi(), 0, ptrs.as_ptr(), lens.as_ptr(), inputs.len(), &mut out, off.as_mut_ptr(), len.as_mut_ptr()) };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let streams = (0..inputs.len()).map(|i| unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec()).collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(streams)
}

/// The member table of an LHA archive (`bz_lha_index_buffer`; the host alone, no GPU): the members in front of the first
/// fault, and the fault as `Some((verdict, position of its header))` when the archive does not end cleanly.
#[cfg(feature = "lzhuf")]
pub fn lha_index(archive: &[u8]) -> Result<(Vec<ffi::LhaMember>, Option<(CompressionError, u64)>), CompressionError> {
    let (mut count, mut fault, mut pos) = (0usize, 0i32, 0u64);
    let rc = unsafe { ffi::bz_lha_index_buffer(archive.as_ptr(), archive.len(), core::ptr::null_mut(), 0, &mut count, &mut fault, &mut pos) };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let mut members: Vec<ffi::LhaMember> = Vec::new();
    members.resize(count, ffi::LhaMember::default());
    let rc = unsafe { ffi::bz_lha_index_buffer(archive.as_ptr(), archive.len(), members.as_mut_ptr(), count, &mut count, &mut fault, &mut pos) };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    Ok((members, if fault == ffi::BZ_OK { None } else { Some((CompressionError::from_status(fault), pos)) }))
}

/// Members of an LHA archive in one call (`bz_lha_read_buffer`, device 0, a window of spaces): `sel` holds ascending member
/// indices, `None` reads all.  Element `k` is `Ok(bytes)` only when the member's CRC-16 is its header's, else the error with
/// the bytes that exist.  The outer `Err` is an infrastructure failure (`last_status` says which).
#[cfg(feature = "lzhuf")]
pub fn lha_read(archive: &[u8], sel: Option<&[usize]>) -> Result<Vec<Result<Vec<u8>, (CompressionError, Vec<u8>)>>, CompressionError> {
    let count = match sel {
        Some(s) => s.len(),
        None => lha_index(archive)?.0.len(),
    };
    let mut off: Vec<u64> = Vec::new();
    off.resize(count, 0);
    let mut len = off.clone();
    let mut verdict: Vec<i32> = Vec::new();
    verdict.resize(count, 0);
    let mut out: *mut u8 = core::ptr::null_mut();
    let mut fault = 0i32;
    let sel_ptr = sel.map_or(core::ptr::null(), |s| s.as_ptr());
    let rc = unsafe {
        ffi::bz_lha_read_buffer(0, archive.as_ptr(), archive.len(), sel_ptr, count, 0x20, &mut out, off.as_mut_ptr(), len.as_mut_ptr(), verdict.as_mut_ptr(), &mut fault)
    };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let entries = (0..count)
        .map(|i| {
            let bytes = unsafe { core::slice::from_raw_parts(out.add(off[i] as usize), len[i] as usize) }.to_vec();
            if verdict[i] == ffi::BZ_OK { Ok(bytes) } else { Err((CompressionError::from_status(verdict[i]), bytes)) }
        })
        .collect();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(entries)
}

/// One member for `lha_write`: `name` and `dir` are raw bytes (a directory's components are separated by 0xFF), `mtime` the
/// header's raw time field, `is_dir` a `-lhd-` member without data.
#[cfg(feature = "lzhuf")]
#[derive(Clone, Debug, Default)]
pub struct LhaFile<'a> {
    pub name: &'a [u8],
    pub dir: &'a [u8],
    pub bytes: &'a [u8],
    pub mtime: u32,
    pub attr: u8,
    pub os_id: u8,
    pub is_dir: bool,
}

/// An LHA archive of many members in one call (`bz_lha_write_buffer`, device 0): `method` is 4 .. 7 (`-lh4-` .. `-lh7-`) or
/// 0 (stored), `level` the header level 0 .. 2.  A member whose stream would not be shorter than its bytes is stored.
#[cfg(feature = "lzhuf")]
pub fn lha_write(files: &[LhaFile], method: i32, level: i32) -> Result<Vec<u8>, CompressionError> {
    let entries: Vec<ffi::LhaEntry> = files
        .iter()
        .map(|f| ffi::LhaEntry { name: f.name.as_ptr(), name_len: f.name.len() as u32, dir: f.dir.as_ptr(), dir_len: f.dir.len() as u32, mtime: f.mtime, attr: f.attr, os_id: f.os_id, is_dir: f.is_dir as u8, pad: 0 })
        .collect();
    let ins: Vec<*const u8> = files.iter().map(|f| f.bytes.as_ptr()).collect();
    let lens: Vec<usize> = files.iter().map(|f| f.bytes.len()).collect();
    let mut out: *mut u8 = core::ptr::null_mut();
    let mut len = 0usize;
    let rc = unsafe { ffi::bz_lha_write_buffer(method, level, 0, ins.as_ptr(), lens.as_ptr(), entries.as_ptr(), files.len(), &mut out, &mut len) };
    if rc != ffi::BZ_OK {
        note_status(rc);
        return Err(CompressionError::from_status(rc));
    }
    let archive = unsafe { core::slice::from_raw_parts(out, len) }.to_vec();
    unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
    Ok(archive)
}

pub(crate) fn note_status(rc: i32) {
    if rc != 0 {
        LAST_STATUS.store(rc, Ordering::Relaxed);
    }
}
