// compression.hpp -- C++ mirror of the reference's encode interface for the BZip2 path, over the
// C ABI (include/bz2_mi355x.h).  Header-only; this is what a Rust shim does in Rust (see
// INTEGRATION.md and rust_shim/src/lib.rs).
//
//   reference (Rust)                                     here
//   ---------------------------------------------------  -----------------------------------------
//   enum Action { Run, Flush, Finish }  src/action.rs:8   compression::Action
//   enum CompressionError {..}          src/error.rs:10   compression::CompressionError
//   trait Encoder { fn next(..) }       src/traits/encoder.rs:81-93   compression::Encoder (concept)
//   struct BZip2Encoder                 src/bzip2/encoder.rs:40-159   compression::BZip2Encoder
//   EncodeExt::encode / EncodeIterator  src/traits/encoder.rs:12-79   compression::encode(), EncodeIterator
//   enum BZip2Error {..}                src/bzip2/error.rs:5-11       compression::BZip2Error (+ to_compression_error)
//   struct BZip2Decoder                 src/bzip2/decoder.rs:583-612  compression::BZip2Decoder
//   DecodeExt::decode / DecodeIterator  src/traits/decoder.rs:15-86   compression::decode(), DecodeIterator
//
// Semantics kept: BZip2Encoder(level) throws std::invalid_argument where the reference panics
// (level outside 1..=9); next() returns std::nullopt for None, a Result holding either the byte
// or the error; Default == level 9.
#pragma once
#include "../../include/bz2_mi355x.h"

#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace compression {

enum class Action { Run = BZ_ACTION_RUN, Flush = BZ_ACTION_FLUSH, Finish = BZ_ACTION_FINISH };

enum class CompressionError { DataError, UnexpectedEof, Unexpected };

inline const char *description(CompressionError e)
{ // src/error.rs:34-41
    switch (e) {
    case CompressionError::DataError: return "data integrity error in data";
    case CompressionError::UnexpectedEof: return "file ends unexpectedly";
    default: return "unexpected error";
    }
}

inline CompressionError from_status(int rc)
{
    if (rc == BZ_E_DATA) return CompressionError::DataError;
    if (rc == BZ_E_EOF) return CompressionError::UnexpectedEof;
    return CompressionError::Unexpected; // HIP failures, missing GPU, ... (the encoder's only error, encoder.rs:623)
}

template <class T, class E = CompressionError> struct Result {
    bool ok;
    T value;
    E error;
    static Result Ok(T v) { return Result{true, v, E::Unexpected}; }
    static Result Err(E e) { return Result{false, T(), e}; }
};

// src/bzip2/error.rs:5-11
enum class BZip2Error { DataError, DataErrorMagicFirst, DataErrorMagic, UnexpectedEof, Unexpected };

inline const char *description(BZip2Error e)
{ // src/bzip2/error.rs:31-42
    switch (e) {
    case BZip2Error::DataError: return "data integrity (CRC) error in data";
    case BZip2Error::DataErrorMagicFirst: return "bad magic number (file not created by bzip2)";
    case BZip2Error::DataErrorMagic: return "trailing garbage after EOF ignored";
    case BZip2Error::UnexpectedEof: return "file ends unexpectedly";
    default: return "unexpected error";
    }
}

// impl From<BZip2Error> for CompressionError, src/bzip2/error.rs:45-53
inline CompressionError to_compression_error(BZip2Error e)
{
    if (e == BZip2Error::UnexpectedEof) return CompressionError::UnexpectedEof;
    if (e == BZip2Error::Unexpected) return CompressionError::Unexpected;
    return CompressionError::DataError;
}

inline BZip2Error bzip2_error_from_status(int rc)
{
    switch (rc) {
    case BZ_E_DATA: return BZip2Error::DataError;
    case BZ_E_MAGIC_FIRST: return BZip2Error::DataErrorMagicFirst;
    case BZ_E_MAGIC: return BZip2Error::DataErrorMagic;
    case BZ_E_EOF: return BZip2Error::UnexpectedEof;
    default: return BZip2Error::Unexpected; // HIP failures, missing GPU, ...
    }
}

class BZip2Encoder {
  public:
    using In = uint8_t;
    using Out = uint8_t;
    using Error = CompressionError;

    explicit BZip2Encoder(int level = 9, int device = 0)
    {
        const int rc = bz_enc_create(&h_, level, device);
        if (rc == BZ_E_PARAM) throw std::invalid_argument("invalid level"); // the reference panics
        if (rc != BZ_OK) throw std::runtime_error(bz_strerror(rc));
        buf_.resize(1 << 16);
    }
    // BZip2Encoder::with_devices: the same encoder over several GPUs of this process (bz_enc_create_multi)
    BZip2Encoder(int level, const std::vector<int> &devices)
    {
        const int rc = bz_enc_create_multi(&h_, level, devices.data(), static_cast<int>(devices.size()));
        if (rc == BZ_E_PARAM) throw std::invalid_argument("invalid level or device list");
        if (rc != BZ_OK) throw std::runtime_error(bz_strerror(rc));
        buf_.resize(1 << 16);
    }
    BZip2Encoder(const BZip2Encoder &) = delete;
    BZip2Encoder &operator=(const BZip2Encoder &) = delete;
    ~BZip2Encoder() { bz_enc_destroy(h_); }

    // Self-check (bz_enc_set_verify): every job's blocks are decoded on the device and compared with their input
    // before their bytes are handed out.  stats: blocks checked, jobs redone, redone jobs that failed again, ns.
    BZip2Encoder &verified(bool on = true)
    {
        bz_enc_set_verify(h_, on ? 1 : 0);
        return *this;
    }
    void verify_stats(uint64_t out[4]) { bz_enc_verify_stats(h_, out); }

    // Many independent inputs in one call (bz_encode_batch): element i of the result is the stream a
    // BZip2Encoder(level) makes of inputs[i] with Action::Finish, bit for bit; inputs that are certain to be one block
    // are encoded together.  `inputs`: any range of byte ranges with data() and size() (a span of spans, a vector of
    // vectors).
    template <class Spans>
    static Result<std::vector<std::vector<uint8_t>>> encode_batch(int level, const Spans &inputs, int device = 0)
    {
        using R = Result<std::vector<std::vector<uint8_t>>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        uint8_t *out = nullptr;
        const int rc = bz_encode_batch(level, device, ptrs.data(), lens.data(), ptrs.size(), &out, off.data(), len.data());
        if (rc == BZ_E_PARAM) throw std::invalid_argument("invalid level"); // the reference panics
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<std::vector<uint8_t>> streams(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) streams[i].assign(out + off[i], out + off[i] + len[i]);
        bz_free(out);
        return R::Ok(std::move(streams));
    }

    // Encoder::next (src/traits/encoder.rs:87-92, src/bzip2/encoder.rs:120-158)
    template <class I, class S> std::optional<Result<uint8_t>> next(I &it, const S &end, Action action)
    {
        if (pos_ == len_) {
            int rc = refill();
            if (rc < 0) return Result<uint8_t>::Err(from_status(rc));
            if (len_ == 0) {
                // pull input in bulk (the reference pulls byte by byte; same bytes, fewer calls)
                for (;;) {
                    chunk_.clear();
                    while (it != end && chunk_.size() < kChunk) {
                        chunk_.push_back(static_cast<uint8_t>(*it));
                        ++it;
                    }
                    if (!chunk_.empty()) {
                        rc = bz_enc_write(h_, chunk_.data(), chunk_.size());
                        if (rc != BZ_OK) return Result<uint8_t>::Err(from_status(rc));
                        if (bz_enc_pending(h_)) break;
                    }
                    if (it == end) {
                        rc = bz_enc_end(h_, static_cast<int>(action));
                        if (rc != BZ_OK) return Result<uint8_t>::Err(from_status(rc));
                        break;
                    }
                }
                rc = refill();
                if (rc < 0) return Result<uint8_t>::Err(from_status(rc));
                if (len_ == 0) return std::nullopt;
            }
        }
        return Result<uint8_t>::Ok(buf_[pos_++]);
    }

  private:
    int refill()
    {
        const long k = bz_enc_read(h_, buf_.data(), buf_.size());
        if (k < 0) return static_cast<int>(k);
        len_ = static_cast<size_t>(k);
        pos_ = 0;
        return 0;
    }
    static constexpr size_t kChunk = 1 << 20;
    bz_enc *h_ = nullptr;
    std::vector<uint8_t> buf_, chunk_;
    size_t pos_ = 0, len_ = 0;
};

// Deflate / zlib / gzip encoders (include/bz2_mi355x.h section 4):
//   Inflater     src/deflate/encoder.rs:92-260   (the reference's name for its Deflate ENCODER)
//   ZlibEncoder  src/zlib/encoder.rs:55-157      GZipEncoder  src/gzip/encoder.rs:50-135
// Action::Run accumulates, Action::Finish produces the stream; Action::Flush writes the bytes so far as a
// byte-aligned segment (Inflater only: the zlib / gzip wrappers refuse it BEFORE pulling any input --
// CompressionError::Unexpected -- because the reference's wrappers end their container at the first None).
template <int Kind> class DeflateFamilyEncoder {
  public:
    using In = uint8_t;
    using Out = uint8_t;
    using Error = CompressionError;

    explicit DeflateFamilyEncoder(int device = 0)
    {
        const int rc = df_enc_create(&h_, Kind, device);
        if (rc != BZ_OK) throw std::runtime_error(bz_strerror(rc));
        buf_.resize(1 << 16);
    }
    // ::with_dict (src/deflate/encoder.rs:134-153, src/zlib/encoder.rs:74-93; GZipEncoder has none)
    static DeflateFamilyEncoder *with_dict(const uint8_t *dict, size_t dict_len, int device = 0)
    {
        auto *e = new DeflateFamilyEncoder(device);
        df_enc_destroy(e->h_);
        e->h_ = nullptr;
        const int rc = df_enc_create_dict(&e->h_, Kind, device, dict, dict_len);
        if (rc != BZ_OK) {
            delete e;
            throw std::runtime_error(bz_strerror(rc));
        }
        return e;
    }
    DeflateFamilyEncoder(const DeflateFamilyEncoder &) = delete;
    DeflateFamilyEncoder &operator=(const DeflateFamilyEncoder &) = delete;
    ~DeflateFamilyEncoder() { df_enc_destroy(h_); }

    template <class I, class S> std::optional<Result<uint8_t>> next(I &it, const S &end, Action action)
    {
        if (pos_ == len_) {
            int rc = refill();
            if (rc < 0) return Result<uint8_t>::Err(from_status(rc));
            if (len_ == 0) {
                // the wrappers do not touch the iterator once their trailer is out (src/zlib/encoder.rs:130-136)
                if (Kind != DF_KIND_DEFLATE && df_enc_finished(h_)) return std::nullopt;
                while (it != end) {
                    chunk_.clear();
                    while (it != end && chunk_.size() < kChunk) {
                        chunk_.push_back(static_cast<uint8_t>(*it));
                        ++it;
                    }
                    rc = df_enc_write(h_, chunk_.data(), chunk_.size());
                    if (rc != BZ_OK) return Result<uint8_t>::Err(from_status(rc));
                }
                rc = df_enc_end(h_, static_cast<int>(action));
                if (rc != BZ_OK) return Result<uint8_t>::Err(from_status(rc));
                rc = refill();
                if (rc < 0) return Result<uint8_t>::Err(from_status(rc));
                if (len_ == 0) return std::nullopt;
            }
        }
        return Result<uint8_t>::Ok(buf_[pos_++]);
    }

    // Many independent inputs in one call (df_encode_batch): element i of the result is the stream this encoder makes of
    // inputs[i] with Action::Finish, bit for bit; inputs of at most 65 535 bytes are encoded together.  `inputs`: any range
    // of byte ranges with data() and size().
    template <class Spans> static Result<std::vector<std::vector<uint8_t>>> encode_batch(const Spans &inputs, int device = 0)
    {
        return encode_batch(inputs, nullptr, 0, device);
    }
    // ... with one preset dictionary for every input (df_encode_batch_dict): the streams of ::with_dict encoders
    template <class Spans>
    static Result<std::vector<std::vector<uint8_t>>> encode_batch(const Spans &inputs, const uint8_t *dict, size_t dict_len, int device = 0)
    {
        using R = Result<std::vector<std::vector<uint8_t>>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        uint8_t *out = nullptr;
        const int rc = df_encode_batch_dict(Kind, device, ptrs.data(), lens.data(), ptrs.size(), dict, dict_len, &out, off.data(), len.data());
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<std::vector<uint8_t>> streams(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) streams[i].assign(out + off[i], out + off[i] + len[i]);
        bz_free(out);
        return R::Ok(std::move(streams));
    }

  private:
    int refill()
    {
        const long k = df_enc_read(h_, buf_.data(), buf_.size());
        if (k < 0) return static_cast<int>(k);
        len_ = static_cast<size_t>(k);
        pos_ = 0;
        return 0;
    }
    static constexpr size_t kChunk = 1 << 20;
    df_enc *h_ = nullptr;
    std::vector<uint8_t> buf_, chunk_;
    size_t pos_ = 0, len_ = 0;
};
using Inflater = DeflateFamilyEncoder<DF_KIND_DEFLATE>;
using ZlibEncoder = DeflateFamilyEncoder<DF_KIND_ZLIB>;
using GZipEncoder = DeflateFamilyEncoder<DF_KIND_GZIP>;

// EncodeIterator (src/traits/encoder.rs:41-79): a single-pass input range
template <class I, class S, class E> class EncodeIterator {
  public:
    EncodeIterator(I first, S last, E &enc, Action a) : it_(first), end_(last), enc_(enc), action_(a) {}
    std::optional<Result<typename E::Out>> next() { return enc_.next(it_, end_, action_); }

  private:
    I it_;
    S end_;
    E &enc_;
    Action action_;
};

// EncodeExt::encode (src/traits/encoder.rs:25-39)
template <class C, class E> auto encode(const C &container, E &encoder, Action action)
{
    return EncodeIterator<decltype(container.begin()), decltype(container.end()), E>(container.begin(),
                                                                                      container.end(), encoder, action);
}

class BZip2Decoder {
  public:
    using Input = uint8_t;
    using Output = uint8_t;
    using Error = BZip2Error;

    explicit BZip2Decoder(int device = 0) // BZip2Decoder::new, src/bzip2/decoder.rs:588-594
    {
        const int rc = bz_dec_create(&h_, device);
        if (rc != BZ_OK) throw std::runtime_error(bz_strerror(rc));
        buf_.resize(1 << 16);
    }
    BZip2Decoder(const BZip2Decoder &) = delete;
    BZip2Decoder &operator=(const BZip2Decoder &) = delete;
    ~BZip2Decoder() { bz_dec_destroy(h_); }

    // Decoder::next (src/traits/decoder.rs:95-98, src/bzip2/decoder.rs:604-612): the decoded bytes in
    // order, then the Err item if the stream is bad, then None
    template <class I, class S> std::optional<Result<uint8_t, BZip2Error>> next(I &it, const S &end)
    {
        while (pos_ == len_) {
            const long k = bz_dec_read(h_, buf_.data(), buf_.size());
            if (k < 0) {
                if (failed_) return std::nullopt;
                failed_ = true;
                return Result<uint8_t, BZip2Error>::Err(bzip2_error_from_status(static_cast<int>(k)));
            }
            if (k > 0) {
                len_ = static_cast<size_t>(k);
                pos_ = 0;
                break;
            }
            if (ended_) return std::nullopt; // 0 after the end: the clean end
            // nothing ready: hand over more input (the reference pulls bytes on demand; the bytes are the same)
            chunk_.clear();
            while (it != end && chunk_.size() < kChunk) {
                chunk_.push_back(static_cast<uint8_t>(*it));
                ++it;
            }
            if (!chunk_.empty()) {
                const int rc = bz_dec_write(h_, chunk_.data(), chunk_.size());
                if (rc != BZ_OK) return Result<uint8_t, BZip2Error>::Err(bzip2_error_from_status(rc));
            }
            if (it == end) {
                ended_ = true;
                (void)bz_dec_end(h_); // the verdict comes back from bz_dec_read behind the last byte
            }
        }
        return Result<uint8_t, BZip2Error>::Ok(buf_[pos_++]);
    }

    // Many independent streams in one call (bz_decode_batch): element i of the result is what
    // `inputs[i].decode(&mut BZip2Decoder::new())` yields -- the bytes in front of the verdict, and the Err item if the
    // entry is bad (an entry's verdict is its own: a bad one hides nothing behind it).  The outer Err is an
    // infrastructure failure.  `inputs`: any range of byte ranges with data() and size().
    struct Entry {
        std::vector<uint8_t> bytes;
        std::optional<BZip2Error> error;
    };
    template <class Spans> static Result<std::vector<Entry>> decode_batch(const Spans &inputs, int device = 0)
    {
        using R = Result<std::vector<Entry>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        std::vector<int32_t> verdict(ptrs.size());
        uint8_t *out = nullptr;
        const int rc = bz_decode_batch(device, ptrs.data(), lens.data(), ptrs.size(), &out, off.data(), len.data(), verdict.data());
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<Entry> entries(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) {
            entries[i].bytes.assign(out + off[i], out + off[i] + len[i]);
            if (verdict[i] != BZ_OK) entries[i].error = bzip2_error_from_status(verdict[i]);
        }
        bz_free(out);
        return R::Ok(std::move(entries));
    }

  private:
    static constexpr size_t kChunk = 1 << 20;
    bz_dec *h_ = nullptr;
    std::vector<uint8_t> buf_, chunk_;
    size_t pos_ = 0, len_ = 0;
    bool ended_ = false, failed_ = false;
};

// Deflate / zlib / gzip decoders (include/bz2_mi355x.h section 5):
//   Deflater     src/deflate/decoder.rs   (the reference's name for its Deflate DECODER)
//   ZlibDecoder  src/zlib/decoder.rs      GZipDecoder  src/gzip/decoder.rs
// The first next() collects the input range and decodes it in one df_decode_buffer_dict call; the bytes come out in order,
// then the Err item if the stream is bad (RFC 1951 / 1950 / 1952 decide, see the header), then None.
//   ::with_dict  Deflater and ZlibDecoder (src/deflate/decoder.rs:358-404, src/zlib/decoder.rs:152-158; GZipDecoder has none)
//   MultiGZipDecoder  every member of a gzip file (section 6, df_decode_members_buffer): what gzip(1) yields; GZipDecoder
//                     stops behind the first member, as the reference's does
template <int Kind, bool Members = false> class DeflateFamilyDecoder {
  public:
    using Input = uint8_t;
    using Output = uint8_t;
    using Error = CompressionError;

    explicit DeflateFamilyDecoder(int device = 0) : device_(device) {} // (does not touch the device)
    // the dictionary is copied; an empty one is no dictionary (section 5, clause (c))
    static DeflateFamilyDecoder with_dict(const uint8_t *dict, size_t dict_len, int device = 0)
    {
        static_assert(Kind != DF_KIND_GZIP, "GZipDecoder has no with_dict");
        DeflateFamilyDecoder d(device);
        d.dict_.assign(dict, dict + dict_len);
        return d;
    }

    template <class I, class S> std::optional<Result<uint8_t>> next(I &it, const S &end)
    {
        if (!ran_) {
            ran_ = true;
            std::vector<uint8_t> in;
            for (; it != end; ++it) in.push_back(static_cast<uint8_t>(*it));
            uint8_t *out = nullptr;
            size_t n = 0;
            verdict_ = Members ? df_decode_members_buffer(device_, in.data(), in.size(), &out, &n)
                               : df_decode_buffer_dict(Kind, device_, in.data(), in.size(), dict_.data(), dict_.size(), &out, &n);
            if (out) {
                buf_.assign(out, out + n);
                bz_free(out);
            }
        }
        if (pos_ < buf_.size()) return Result<uint8_t>::Ok(buf_[pos_++]);
        if (verdict_ != BZ_OK) {
            const int rc = verdict_;
            verdict_ = BZ_OK;
            return Result<uint8_t>::Err(from_status(rc));
        }
        return std::nullopt;
    }

    // Many independent streams in one call (df_decode_batch): element i is what `inputs[i].decode(..)` yields.
    struct Entry {
        std::vector<uint8_t> bytes;
        std::optional<CompressionError> error;
    };
    template <class Spans> static Result<std::vector<Entry>> decode_batch(const Spans &inputs, int device = 0)
    {
        return decode_batch(inputs, nullptr, 0, device);
    }
    // ... with one preset dictionary for every stream (df_decode_batch_dict)
    template <class Spans> static Result<std::vector<Entry>> decode_batch(const Spans &inputs, const uint8_t *dict, size_t dict_len, int device = 0)
    {
        using R = Result<std::vector<Entry>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        std::vector<int32_t> verdict(ptrs.size());
        uint8_t *out = nullptr;
        const int rc =
            df_decode_batch_dict(Kind, device, ptrs.data(), lens.data(), ptrs.size(), dict, dict_len, &out, off.data(), len.data(), verdict.data());
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<Entry> entries(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) {
            entries[i].bytes.assign(out + off[i], out + off[i] + len[i]);
            if (verdict[i] != BZ_OK) entries[i].error = from_status(verdict[i]);
        }
        bz_free(out);
        return R::Ok(std::move(entries));
    }

  private:
    int device_;
    bool ran_ = false;
    int verdict_ = BZ_OK;
    std::vector<uint8_t> buf_, dict_;
    size_t pos_ = 0;
};
using Deflater = DeflateFamilyDecoder<DF_KIND_DEFLATE>;
using ZlibDecoder = DeflateFamilyDecoder<DF_KIND_ZLIB>;
using GZipDecoder = DeflateFamilyDecoder<DF_KIND_GZIP>;
using MultiGZipDecoder = DeflateFamilyDecoder<DF_KIND_GZIP, true>;

// LZHUF decoder (include/bz2_mi355x.h section 9):
//   enum LzhufMethod    src/lzhuf/mod.rs:14-38        the LHA methods -lh4- .. -lh7-
//   LzhufDecoder        src/lzhuf/decoder.rs:323-349  LzhufDecoder::new(&method)
// The first next() collects the input range and decodes it in one bz_lzh_decode_buffer call; the bytes come out in order,
// then the Err item if the stream is bad under the contract of section 9, then None.  orig_len: the original length an LHA
// member header carries (none: the stream ends at a block boundary with fewer than 16 bits left or a zero block length);
// prefill: -1 strict (the default), 0 .. 255 the value of every byte in front of the output (LHA's decoders use 0x20).
enum class LzhufMethod { Lh4 = BZ_LZH_LH4, Lh5 = BZ_LZH_LH5, Lh6 = BZ_LZH_LH6, Lh7 = BZ_LZH_LH7 };

class LzhufDecoder {
  public:
    using Input = uint8_t;
    using Output = uint8_t;
    using Error = CompressionError;

    explicit LzhufDecoder(LzhufMethod method, int device = 0, std::optional<uint64_t> orig_len = std::nullopt, int prefill = -1)
        : method_(static_cast<int>(method)), device_(device), prefill_(prefill), orig_len_(orig_len ? *orig_len : UINT64_MAX)
    {
    } // (does not touch the device)

    template <class I, class S> std::optional<Result<uint8_t>> next(I &it, const S &end)
    {
        if (!ran_) {
            ran_ = true;
            std::vector<uint8_t> in;
            for (; it != end; ++it) in.push_back(static_cast<uint8_t>(*it));
            uint8_t *out = nullptr;
            size_t n = 0;
            verdict_ = bz_lzh_decode_buffer(method_, prefill_, device_, in.data(), in.size(), orig_len_, &out, &n);
            if (out) {
                buf_.assign(out, out + n);
                bz_free(out);
            }
        }
        if (pos_ < buf_.size()) return Result<uint8_t>::Ok(buf_[pos_++]);
        if (verdict_ != BZ_OK) {
            const int rc = verdict_;
            verdict_ = BZ_OK;
            return Result<uint8_t>::Err(from_status(rc));
        }
        return std::nullopt;
    }

    // Many independent streams in one call (bz_lzh_decode_batch): element i is what `inputs[i].decode(..)` yields.
    // orig_lens: empty, or one length per stream (UINT64_MAX: not known).
    struct Entry {
        std::vector<uint8_t> bytes;
        std::optional<CompressionError> error;
    };
    template <class Spans>
    static Result<std::vector<Entry>> decode_batch(const Spans &inputs, LzhufMethod method, const std::vector<uint64_t> &orig_lens = {},
                                                   int prefill = -1, int device = 0)
    {
        using R = Result<std::vector<Entry>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        if (!orig_lens.empty() && orig_lens.size() != ptrs.size()) return R::Err(from_status(BZ_E_PARAM));
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        std::vector<int32_t> verdict(ptrs.size());
        uint8_t *out = nullptr;
        const int rc = bz_lzh_decode_batch(static_cast<int>(method), prefill, device, ptrs.data(), lens.data(),
                                           orig_lens.empty() ? nullptr : orig_lens.data(), ptrs.size(), &out, off.data(), len.data(), verdict.data());
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<Entry> entries(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) {
            entries[i].bytes.assign(out + off[i], out + off[i] + len[i]);
            if (verdict[i] != BZ_OK) entries[i].error = from_status(verdict[i]);
        }
        bz_free(out);
        return R::Ok(std::move(entries));
    }

  private:
    int method_, device_, prefill_;
    uint64_t orig_len_;
    bool ran_ = false;
    int verdict_ = BZ_OK;
    std::vector<uint8_t> buf_;
    size_t pos_ = 0;
};

// LZHUF encoder (include/bz2_mi355x.h section 10):
//   LzhufEncoder        src/lzhuf/encoder.rs          LzhufEncoder::new(&method)
// Action::Run collects the input range and yields nothing; Action::Finish collects the rest, encodes everything in one
// bz_lzh_encode_buffer call and yields the stream, byte for byte the reference's.  Action::Flush is not offered: a
// parameter error.
class LzhufEncoder {
  public:
    using Input = uint8_t;
    using Output = uint8_t;
    using Error = CompressionError;

    explicit LzhufEncoder(LzhufMethod method, int device = 0) : method_(static_cast<int>(method)), device_(device) {} // (does not touch the device)

    template <class I, class S> std::optional<Result<uint8_t>> next(I &it, const S &end, Action action)
    {
        if (!done_) {
            if (action == Action::Flush) return Result<uint8_t>::Err(from_status(BZ_E_PARAM));
            for (; it != end; ++it) in_.push_back(static_cast<uint8_t>(*it));
            if (action == Action::Run) return std::nullopt;
            done_ = true;
            uint8_t *out = nullptr;
            size_t n = 0;
            status_ = bz_lzh_encode_buffer(method_, device_, in_.data(), in_.size(), &out, &n);
            if (out) {
                buf_.assign(out, out + n);
                bz_free(out);
            }
            in_.clear();
        }
        if (status_ != BZ_OK) {
            const int rc = status_;
            status_ = BZ_OK;
            return Result<uint8_t>::Err(from_status(rc));
        }
        if (pos_ < buf_.size()) return Result<uint8_t>::Ok(buf_[pos_++]);
        return std::nullopt;
    }

    // Many independent inputs in one call (bz_lzh_encode_batch): element i is the stream of inputs[i].
    template <class Spans>
    static Result<std::vector<std::vector<uint8_t>>> encode_batch(const Spans &inputs, LzhufMethod method, int device = 0)
    {
        using R = Result<std::vector<std::vector<uint8_t>>>;
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &x : inputs) {
            ptrs.push_back(reinterpret_cast<const uint8_t *>(x.data()));
            lens.push_back(x.size());
        }
        std::vector<uint64_t> off(ptrs.size()), len(ptrs.size());
        uint8_t *out = nullptr;
        const int rc = bz_lzh_encode_batch(static_cast<int>(method), device, ptrs.data(), lens.data(), ptrs.size(), &out, off.data(), len.data());
        if (rc != BZ_OK) return R::Err(from_status(rc));
        std::vector<std::vector<uint8_t>> streams(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) streams[i].assign(out + off[i], out + off[i] + len[i]);
        bz_free(out);
        return R::Ok(std::move(streams));
    }

  private:
    int method_, device_;
    bool done_ = false;
    int status_ = BZ_OK;
    std::vector<uint8_t> in_, buf_;
    size_t pos_ = 0;
};

// LHA archives (include/bz2_mi355x.h section 11): the member table on the host (bz_lha_index_buffer, no GPU), and the bytes
// of all members or of a chosen subset in one call (bz_lha_read_buffer), every member with its own verdict (clean only when
// its CRC-16 is its header's).
struct LhaIndex {
    std::vector<bz_lha_member> members;
    int fault = BZ_OK;      // BZ_OK: the archive ends cleanly; else the verdict that ended the walk
    uint64_t fault_pos = 0; // ... and the header it lies in
};
inline Result<LhaIndex> lha_index(const uint8_t *in, size_t n)
{
    using R = Result<LhaIndex>;
    LhaIndex idx;
    size_t count = 0;
    int32_t fault = BZ_OK;
    int rc = bz_lha_index_buffer(in, n, nullptr, 0, &count, &fault, &idx.fault_pos);
    if (rc != BZ_OK) return R::Err(from_status(rc));
    idx.members.resize(count);
    rc = bz_lha_index_buffer(in, n, idx.members.data(), count, &count, &fault, &idx.fault_pos);
    if (rc != BZ_OK) return R::Err(from_status(rc));
    idx.fault = fault;
    return R::Ok(std::move(idx));
}
// sel: ascending member indices; empty with `all`: every member of the table
inline Result<std::vector<LzhufDecoder::Entry>> lha_read(const uint8_t *in, size_t n, const std::vector<size_t> &sel = {}, bool all = true,
                                                        int prefill = 0x20, int device = 0)
{
    using R = Result<std::vector<LzhufDecoder::Entry>>;
    size_t count = sel.size();
    if (all && sel.empty()) {
        auto idx = lha_index(in, n);
        if (!idx.ok) return R::Err(idx.error);
        count = idx.value.members.size();
    }
    std::vector<uint64_t> off(count), len(count);
    std::vector<int32_t> verdict(count);
    uint8_t *out = nullptr;
    int32_t fault = BZ_OK;
    const int rc = bz_lha_read_buffer(device, in, n, sel.empty() && all ? nullptr : sel.data(), count, prefill, &out, off.data(), len.data(),
                                      verdict.data(), &fault);
    if (rc != BZ_OK) return R::Err(from_status(rc));
    std::vector<LzhufDecoder::Entry> entries(count);
    for (size_t i = 0; i < count; ++i) {
        entries[i].bytes.assign(out + off[i], out + off[i] + len[i]);
        if (verdict[i] != BZ_OK) entries[i].error = from_status(verdict[i]);
    }
    bz_free(out);
    return R::Ok(std::move(entries));
}

// An LHA archive of many members in one call (include/bz2_mi355x.h section 12, bz_lha_write_buffer): method BZ_LHA_LH4 ..
// BZ_LHA_LH7 or BZ_LHA_STORED, header level 0 .. 2; a member whose stream would not be shorter than its bytes is stored.
struct LhaFile {
    std::vector<uint8_t> name, dir; // raw bytes; a directory's components are separated by 0xFF
    std::vector<uint8_t> bytes;
    uint32_t mtime = 0;
    uint8_t attr = 0x20, os_id = 0x55;
    bool is_dir = false;
};
inline Result<std::vector<uint8_t>> lha_write(const std::vector<LhaFile> &files, int method = BZ_LHA_LH5, int level = 2, int device = 0)
{
    using R = Result<std::vector<uint8_t>>;
    std::vector<bz_lha_entry> entries(files.size());
    std::vector<const uint8_t *> ins(files.size());
    std::vector<size_t> lens(files.size());
    for (size_t i = 0; i < files.size(); ++i) {
        const LhaFile &f = files[i];
        entries[i] = bz_lha_entry{f.name.data(), (uint32_t)f.name.size(), f.dir.data(), (uint32_t)f.dir.size(), f.mtime, f.attr, f.os_id,
                                  (uint8_t)f.is_dir, 0};
        ins[i] = f.bytes.data();
        lens[i] = f.bytes.size();
    }
    uint8_t *out = nullptr;
    size_t len = 0;
    const int rc = bz_lha_write_buffer(method, level, device, ins.data(), lens.data(), entries.data(), files.size(), &out, &len);
    if (rc != BZ_OK) return R::Err(from_status(rc));
    std::vector<uint8_t> arc(out, out + len);
    bz_free(out);
    return R::Ok(std::move(arc));
}

// One input as a BGZF file (include/bz2_mi355x.h section 7, df_bgzf_encode_buffer): gzip members of at most block_bytes
// (0: 65 280) input bytes side by side, then the 28-byte EOF marker unless eof is false.  The reference has no such writer;
// every member is a stream that zlib, gzip(1) and htslib read.  block_off, when not null, receives the file offset of every
// block and, last, that of the marker (the file's length without one).
inline Result<std::vector<uint8_t>> bgzf_compress(const uint8_t *in, size_t n, uint32_t block_bytes = 0, bool eof = true, int device = 0,
                                                  std::vector<uint64_t> *block_off = nullptr)
{
    using R = Result<std::vector<uint8_t>>;
    if (block_bytes > DF_BGZF_BLOCK) return R::Err(from_status(BZ_E_PARAM));
    std::vector<uint64_t> off(df_bgzf_block_count(n, block_bytes) + 1);
    uint8_t *out = nullptr;
    size_t len = 0;
    const int rc = df_bgzf_encode_buffer(device, in, n, block_bytes, eof ? 1 : 0, &out, &len, off.data());
    if (rc != BZ_OK) return R::Err(from_status(rc));
    std::vector<uint8_t> file(out, out + len);
    bz_free(out);
    if (block_off) *block_off = std::move(off);
    return R::Ok(std::move(file));
}

// Reading BGZF (include/bz2_mi355x.h section 8).  The index of a file in host memory: the BSIZE chain, walked on the host
// (parsing, not decoding: no GPU is needed).  coff / uoff hold count + 1 entries -- the .gzi table, and the last pair the
// end of the last complete block; verdict is the chain's: the blocks in front of a fault are still indexed.
struct BgzfIndex {
    std::vector<uint64_t> coff, uoff;
    int verdict = BZ_OK;
    size_t blocks() const { return coff.empty() ? 0 : coff.size() - 1; }
    uint64_t total() const { return uoff.empty() ? 0 : uoff.back() - uoff.front(); }
};
inline Result<BgzfIndex> bgzf_index(const uint8_t *in, size_t n)
{
    using R = Result<BgzfIndex>;
    uint64_t *c = nullptr, *u = nullptr;
    size_t count = 0;
    int32_t v = BZ_OK;
    const int rc = df_bgzf_index_buffer(in, n, &c, &u, &count, &v);
    if (rc != BZ_OK) return R::Err(from_status(rc));
    BgzfIndex ix;
    ix.coff.assign(c, c + count + 1);
    ix.uoff.assign(u, u + count + 1);
    ix.verdict = v;
    bz_free(c);
    bz_free(u);
    return R::Ok(std::move(ix));
}
// The uncompressed bytes [ustart, ustart + ulen) of a BGZF file, clamped to its end (df_bgzf_read_buffer): only the blocks
// the range touches are uploaded and decoded.  A fault in front of or inside the range is the Err; `partial`, when not
// null, receives the range's bytes in front of it.  Range reads pay off for ranges of many blocks, not for one record.
inline Result<std::vector<uint8_t>> bgzf_read(const uint8_t *in, size_t n, uint64_t ustart, uint64_t ulen, int device = 0,
                                              std::vector<uint8_t> *partial = nullptr)
{
    using R = Result<std::vector<uint8_t>>;
    uint8_t *out = nullptr;
    size_t len = 0;
    const int rc = df_bgzf_read_buffer(device, in, n, ustart, ulen, &out, &len);
    std::vector<uint8_t> bytes;
    if (out) {
        bytes.assign(out, out + len);
        bz_free(out);
    }
    if (rc != BZ_OK) {
        if (partial) *partial = std::move(bytes);
        return R::Err(from_status(rc));
    }
    return R::Ok(std::move(bytes));
}
inline Result<std::vector<uint8_t>> bgzf_decompress(const uint8_t *in, size_t n, int device = 0, std::vector<uint8_t> *partial = nullptr)
{
    return bgzf_read(in, n, 0, UINT64_MAX, device, partial);
}

// DecodeIterator (src/traits/decoder.rs:45-86)
template <class I, class S, class D> class DecodeIterator {
  public:
    DecodeIterator(I first, S last, D &dec) : it_(first), end_(last), dec_(dec) {}
    std::optional<Result<typename D::Output, typename D::Error>> next() { return dec_.next(it_, end_); }

  private:
    I it_;
    S end_;
    D &dec_;
};

// DecodeExt::decode (src/traits/decoder.rs:27-43)
template <class C, class D> auto decode(const C &container, D &decoder)
{
    return DecodeIterator<decltype(container.begin()), decltype(container.end()), D>(container.begin(),
                                                                                      container.end(), decoder);
}

// `.collect::<Result<Vec<_>, _>>()`
template <class It> auto collect(It iter)
{
    using Item = typename decltype(iter.next())::value_type;
    using Err = decltype(Item::error);
    std::vector<uint8_t> out;
    for (;;) {
        auto r = iter.next();
        if (!r) break;
        if (!r->ok) return Result<std::vector<uint8_t>, Err>::Err(r->error);
        out.push_back(r->value);
    }
    return Result<std::vector<uint8_t>, Err>::Ok(std::move(out));
}

} // namespace compression
