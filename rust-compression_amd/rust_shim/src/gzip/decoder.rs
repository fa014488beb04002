//! `GZipDecoder` (the reference's `src/gzip/decoder.rs`): the header with its optional fields as the
//! reference checks them (its lines 92-108, 175-191), the Deflate stream of the first member, CRC-32 and
//! ISIZE little endian.
use crate::deflate::decoder::{deflate_family_decoder, DeflateFamilyDecoder};
use crate::ffi;

pub struct GZipDecoder(DeflateFamilyDecoder);

deflate_family_decoder!(GZipDecoder, ffi::DF_KIND_GZIP);
