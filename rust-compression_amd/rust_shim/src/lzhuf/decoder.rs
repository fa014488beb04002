//! `LzhufDecoder` (the reference's `src/lzhuf/decoder.rs:323-349`) over section 9 of the C ABI: `bz_lzh_decode_buffer`.
//! The first `next` collects the input iterator and decodes it in one call; the bytes come out in order, an error (if
//! any) after the bytes in front of it.  The verdicts are those of the contract in `include/bz2_mi355x.h`: strict
//! (no distance reaches in front of the output: `prefill` -1), the end of the stream at a block boundary with fewer than
//! 16 bits left or a zero block length.  `with_len` hands over the original length an LHA member header carries;
//! `with_prefill` the byte that LHA's decoders fill their window with (0x20; the reference's ring reads 0).
#[cfg(not(feature = "std"))]
use alloc::vec::Vec;

use crate::error::CompressionError;
use crate::ffi;
use crate::lzhuf::LzhufMethod;
use crate::traits::decoder::Decoder;

#[derive(Debug)]
pub struct LzhufDecoder {
    method: i32,
    prefill: i32,
    orig_len: u64,
    ready: Option<Vec<u8>>,
    pos: usize,
    verdict: i32,
}

impl LzhufDecoder {
    pub fn new(method: &LzhufMethod) -> Self {
        Self { method: method.abi(), prefill: -1, orig_len: u64::MAX, ready: None, pos: 0, verdict: ffi::BZ_OK }
    }

    /// decoding ends with `Ok` as soon as `orig_len` bytes exist; a stream that ends sooner is `UnexpectedEof`
    pub fn with_len(method: &LzhufMethod, orig_len: u64) -> Self {
        Self { orig_len, ..Self::new(method) }
    }

    /// every byte in front of the output has the value `fill`: any distance up to the window is valid at any position
    pub fn with_prefill(mut self, fill: u8) -> Self {
        self.prefill = fill as i32;
        self
    }

    fn run<I: Iterator<Item = u8>>(&mut self, iter: &mut I) {
        let input: Vec<u8> = iter.collect();
        let mut out: *mut u8 = core::ptr::null_mut();
        let mut n: usize = 0;
        let rc = unsafe { ffi::bz_lzh_decode_buffer(self.method, self.prefill, 0, input.as_ptr(), input.len(), self.orig_len, &mut out, &mut n) };
        let mut bytes = Vec::new();
        if !out.is_null() {
            bytes.extend_from_slice(unsafe { core::slice::from_raw_parts(out, n) });
            unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
        }
        self.ready = Some(bytes);
        self.verdict = rc;
    }
}

impl Decoder for LzhufDecoder {
    type Input = u8;
    type Output = u8;
    type Error = CompressionError;

    fn next<I: Iterator<Item = u8>>(&mut self, iter: &mut I) -> Option<Result<u8, CompressionError>> {
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
