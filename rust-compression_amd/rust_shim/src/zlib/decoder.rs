//! `ZlibDecoder` (the reference's `src/zlib/decoder.rs`): CMF / FLG as the reference checks them (its lines
//! 62-101), the Deflate stream, Adler-32 big endian.  `new`: FDICT is refused.  `with_dict`: FDICT must be set
//! and DICTID must be the Adler-32 of the whole dictionary (an empty dictionary is `new`); the dictionary's last
//! 32 768 bytes are history in front of the output, and the trailer's Adler-32 covers the output alone.
use crate::deflate::decoder::{deflate_family_decoder, DeflateFamilyDecoder};
use crate::ffi;

pub struct ZlibDecoder(DeflateFamilyDecoder);

deflate_family_decoder!(ZlibDecoder, ffi::DF_KIND_ZLIB);

impl ZlibDecoder {
    pub fn with_dict(dict: &[u8]) -> Self {
        ZlibDecoder(DeflateFamilyDecoder::with_kind_and_dict(ffi::DF_KIND_ZLIB, dict))
    }
}
