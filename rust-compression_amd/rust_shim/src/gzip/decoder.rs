//! `GZipDecoder` (the reference's `src/gzip/decoder.rs`): the header with its optional fields as the
//! reference checks them (its lines 92-108, 175-191), the Deflate stream of the first member, CRC-32 and
//! ISIZE little endian.
use crate::deflate::decoder::{deflate_family_decoder, DeflateFamilyDecoder};
use crate::ffi;

pub struct GZipDecoder(DeflateFamilyDecoder);

deflate_family_decoder!(GZipDecoder, ffi::DF_KIND_GZIP);

/// Every member of a gzip file, one after the other (flate2's `MultiGzDecoder`, gzip(1)): zero padding between and
/// behind members is skipped, anything else behind a member is a `DataError` after the bytes in front of it.
/// `GZipDecoder` stops behind the first member, as the reference's does.
#[derive(Debug)]
pub struct MultiGZipDecoder(DeflateFamilyDecoder);

impl MultiGZipDecoder {
    pub fn new() -> Self {
        MultiGZipDecoder(DeflateFamilyDecoder::with_members())
    }
}

impl Default for MultiGZipDecoder {
    fn default() -> Self {
        Self::new()
    }
}

impl crate::traits::decoder::Decoder for MultiGZipDecoder {
    type Input = u8;
    type Output = u8;
    type Error = crate::error::CompressionError;
    fn next<I: Iterator<Item = u8>>(&mut self, iter: &mut I) -> Option<Result<u8, crate::error::CompressionError>> {
        self.0.next_item(iter)
    }
}
