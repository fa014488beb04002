//! `LzhufEncoder` (the reference's `src/lzhuf/encoder.rs`) over section 10 of the C ABI: `bz_lzh_encode_buffer`.
//! `Action::Run` collects the iterator's bytes and yields nothing; `Action::Finish` collects the rest, encodes everything
//! in one call and yields the stream -- byte for byte what the reference's encoder writes.  `Action::Flush` is not
//! offered: the first `next` with it yields a parameter error.
#[cfg(not(feature = "std"))]
use alloc::vec::Vec;

use crate::action::Action;
use crate::error::CompressionError;
use crate::ffi;
use crate::lzhuf::LzhufMethod;
use crate::traits::encoder::Encoder;

#[derive(Debug)]
pub struct LzhufEncoder {
    method: i32,
    input: Vec<u8>,
    ready: Option<Vec<u8>>,
    pos: usize,
    error: Option<i32>,
}

impl LzhufEncoder {
    pub fn new(method: &LzhufMethod) -> Self {
        Self { method: method.abi(), input: Vec::new(), ready: None, pos: 0, error: None }
    }

    fn finish(&mut self) {
        let mut out: *mut u8 = core::ptr::null_mut();
        let mut n: usize = 0;
        let rc = unsafe { ffi::bz_lzh_encode_buffer(self.method, 0, self.input.as_ptr(), self.input.len(), &mut out, &mut n) };
        let mut bytes = Vec::new();
        if !out.is_null() {
            bytes.extend_from_slice(unsafe { core::slice::from_raw_parts(out, n) });
            unsafe { ffi::bz_free(out as *mut core::ffi::c_void) };
        }
        if rc != ffi::BZ_OK {
            crate::mi355x::note_status(rc);
            self.error = Some(rc);
        }
        self.input = Vec::new();
        self.ready = Some(bytes);
    }
}

impl Encoder for LzhufEncoder {
    type Error = CompressionError;
    type In = u8;
    type Out = u8;

    fn next<I: Iterator<Item = u8>>(&mut self, iter: &mut I, action: Action) -> Option<Result<u8, CompressionError>> {
        if self.ready.is_none() {
            match action {
                Action::Run => {
                    self.input.extend(iter);
                    return None;
                }
                Action::Flush => return Some(Err(CompressionError::from_status(ffi::BZ_E_PARAM))),
                Action::Finish => {
                    self.input.extend(iter);
                    self.finish();
                }
            }
        }
        if let Some(rc) = self.error.take() {
            return Some(Err(CompressionError::from_status(rc)));
        }
        let ready = self.ready.as_ref().unwrap();
        if self.pos < ready.len() {
            self.pos += 1;
            return Some(Ok(ready[self.pos - 1]));
        }
        None
    }
}
