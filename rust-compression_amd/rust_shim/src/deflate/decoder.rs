//! `Deflater` (the reference's `src/deflate/decoder.rs`) over section 5 of the C ABI: `df_decode_buffer_dict`.
//! The first `next` collects the input iterator and decodes it in one call; the bytes come out in order,
//! an error (if any) after the bytes in front of it.  The verdicts follow RFC 1951 / 1950 / 1952 (the
//! contract in `include/bz2_mi355x.h`), not the reference's decoder, which swallows the errors of its
//! block decoder (its `src/deflate/decoder.rs:376-383`).  `ZlibDecoder` and `GZipDecoder` are the same
//! type with another `kind`; `MultiGZipDecoder` is the gzip kind over section 6 (`df_decode_members_buffer`).
//! `Deflater::with_dict` and `ZlibDecoder::with_dict` (the reference's lines 358-404) hand the dictionary to
//! the call: its last 32 768 bytes are history in front of the output; an empty one is no dictionary.
#[cfg(not(feature = "std"))]
use alloc::vec::Vec;

use crate::error::CompressionError;
use crate::ffi;

#[derive(Debug)]
pub struct DeflateFamilyDecoder {
    kind: i32,
    members: bool,
    dict: Vec<u8>,
    ready: Option<Vec<u8>>,
    pos: usize,
    verdict: i32,
}

impl DeflateFamilyDecoder {
    pub(crate) fn with_kind(kind: i32) -> Self {
        Self { kind, members: false, dict: Vec::new(), ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    /// kinds DEFLATE and ZLIB (`GZipDecoder` has no `with_dict`)
    pub(crate) fn with_kind_and_dict(kind: i32, dict: &[u8]) -> Self {
        Self { kind, members: false, dict: dict.to_vec(), ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    /// every member of a gzip file (section 6 of the C ABI)
    pub(crate) fn with_members() -> Self {
        Self { kind: ffi::DF_KIND_GZIP, members: true, dict: Vec::new(), ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    fn run<I: Iterator<Item = u8>>(&mut self, iter: &mut I) {
        let input: Vec<u8> = iter.collect();
        let mut out: *mut u8 = core::ptr::null_mut();
        let mut n: usize = 0;
        let rc = if self.members {
            unsafe { ffi::df_decode_members_buffer(0, input.as_ptr(), input.len(), &mut out, &mut n) }
        } else {
            unsafe { ffi::df_decode_buffer_dict(self.kind, 0, input.as_ptr(), input.len(), self.dict.as_ptr(), self.dict.len(), &mut out, &mut n) }
        };
        let mut bytes = Vec::new();
        if !out.is_null() {
            bytes.extend_from_slice(unsafe { core::slice::from_raw_parts(out, n) });
            unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
        }
        self.ready = Some(bytes);
        self.verdict = rc;
    }

    pub(crate) fn next_item<I: Iterator<Item = u8>>(&mut self, iter: &mut I) -> Option<Result<u8, CompressionError>> {
        if self.ready.is_none() {
            self.run(iter);
        }
        let ready = self.ready.as_ref().unwrap();
        if self.pos < ready.len() {
            self.pos += 1;
            return Some(Ok(ready[self.pos - 1]));
        }
        if self.verdict != ffi::BZ_OK {
            let rc = core::mem::replace(&mut self.verdict, ffi::BZ_OK);
            return Some(Err(CompressionError::from_status(rc)));
        }
        None
    }
}

macro_rules! deflate_family_decoder {
    ($name:ident, $kind:expr) => {
        impl $name {
            pub fn new() -> Self {
                $name(crate::deflate::decoder::DeflateFamilyDecoder::with_kind($kind))
            }
        }
        impl Default for $name {
            fn default() -> Self {
                Self::new()
            }
        }
        impl crate::traits::decoder::Decoder for $name {
            type Input = u8;
            type Output = u8;
            type Error = crate::error::CompressionError;
            fn next<I: Iterator<Item = u8>>(&mut self, iter: &mut I) -> Option<Result<u8, crate::error::CompressionError>> {
                self.0.next_item(iter)
            }
        }
    };
}
pub(crate) use deflate_family_decoder;

pub struct Deflater(DeflateFamilyDecoder);

deflate_family_decoder!(Deflater, ffi::DF_KIND_DEFLATE);

impl Deflater {
    pub fn with_dict(dict: &[u8]) -> Self {
        Deflater(DeflateFamilyDecoder::with_kind_and_dict(ffi::DF_KIND_DEFLATE, dict))
    }
}
