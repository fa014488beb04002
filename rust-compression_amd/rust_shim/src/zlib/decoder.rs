//! `ZlibDecoder` (the reference's `src/zlib/decoder.rs`), without a preset dictionary: CMF / FLG as the
//! reference checks them (its lines 78-90), FDICT refused, the Deflate stream, Adler-32 big endian.
use crate::deflate::decoder::{deflate_family_decoder, DeflateFamilyDecoder};
use crate::ffi;

pub struct ZlibDecoder(DeflateFamilyDecoder);

deflate_family_decoder!(ZlibDecoder, ffi::DF_KIND_ZLIB);
