//! `Deflater` (the reference's `src/deflate/decoder.rs`) over section 5 of the C ABI: `df_decode_buffer`.
//! The first `next` collects the input iterator and decodes it in one call; the bytes come out in order,
//! an error (if any) after the bytes in front of it.  The verdicts follow RFC 1951 / 1950 / 1952 (the
//! contract in `include/bz2_mi355x.h`), not the reference's decoder, which swallows the errors of its
//! block decoder (its `src/deflate/decoder.rs:376-383`).  `ZlibDecoder` and `GZipDecoder` are the same
//! type with another `kind`; `MultiGZipDecoder` is the gzip kind over section 6 (`df_decode_members_buffer`).
#[cfg(not(feature = "std"))]
use alloc::vec::Vec;

use crate::error::CompressionError;
use crate::ffi;

#[derive(Debug)]
pub struct DeflateFamilyDecoder {
    kind: i32,
    members: bool,
    ready: Option<Vec<u8>>,
    pos: usize,
    verdict: i32,
}

impl DeflateFamilyDecoder {
    pub(crate) fn with_kind(kind: i32) -> Self {
        Self { kind, members: false, ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    /// every member of a gzip file (section 6 of the C ABI)
    pub(crate) fn with_members() -> Self {
        Self { kind: ffi::DF_KIND_GZIP, members: true, ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    fn run<I: Iterator<Item = u8>>(&mut self, iter: &mut I) {
        let input: Vec<u8> = iter.collect();
        let mut out: *mut u8 = core::ptr::null_mut();
        let mut n: usize = 0;
        let rc = if self.members {
            unsafe { ffi::df_decode_members_buffer(0, input.as_ptr(), input.len(), &mut out, &mut n) }
        } else {
            unsafe { ffi::df_decode_buffer(self.kind, 0, input.as_ptr(), input.len(), &mut out, &mut n) }
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
