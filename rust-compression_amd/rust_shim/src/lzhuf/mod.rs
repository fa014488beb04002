//! `lzhuf` (the reference's `src/lzhuf/mod.rs`): the LHA methods `-lh4-` .. `-lh7-`.  Decoder and encoder run on the
//! GPU (sections 9 and 10 of the C ABI).
pub mod decoder;
pub mod encoder;

#[derive(Clone, Copy, Debug)]
pub enum LzhufMethod {
    Lh4,
    Lh5,
    Lh6,
    Lh7,
}

impl LzhufMethod {
    /// the C ABI's `BZ_LZH_LH4` .. `BZ_LZH_LH7`
    pub(crate) fn abi(self) -> i32 {
        match self {
            LzhufMethod::Lh4 => 4,
            LzhufMethod::Lh5 => 5,
            LzhufMethod::Lh6 => 6,
            LzhufMethod::Lh7 => 7,
        }
    }
}
