// FLAC frame decoding (RFC 9639) for the ffmpeg-free read, on gfx950 and on the host from one source.
//
// iss_flac_index (host, context-free) finds every frame of a file: a memchr scan for sync codes, the header parse and its
// CRC-8, frame / sample-number continuity.  flac_decode_frame decodes one frame from those rows: subframe headers with wasted
// bits, CONSTANT / VERBATIM / FIXED 0-4 / LPC 1-32, Rice and Rice2 partitions with escapes, stereo decorrelation, the zero
// padding and the CRC-16 footer.  It is __host__ __device__: iss_flac_decode_host runs it on the CPU, flac_decode_kernel runs
// it with one lane per frame over the frames of every file of a call (one ragged 1-D grid).
//
// Samples are written in the stored format of the file's WAV twin: int16 (8-bit widened x << 8) or int32 (24-bit x << 8),
// interleaved.  The second subframe of a stereo pair is combined with the first on the way out: the first is stored (modulo
// the output width, which is exact for left/side and side/right and lossless for mid, which always fits) and read back.
// LPC / FIXED history and coefficients live in registers: the residual loop is a template on the order bucket (4, 8, 16, 32)
// and on the sum width, so no register array is indexed at run time.
//
// Windows (include/iss.h, iss_window): the decode is a template on the sink.  Sink<false> is the sink there always was;
// Sink<true> keeps only the samples lo <= i < hi of its frame, so a frame that straddles a window's edge is decoded whole
// (its predictor chain starts at the frame; header, padding and CRC-16 checks all run) and stored in part.  A skipped
// sample is neither stored nor read back: the second subframe of a stereo pair reads only what the first stored at the same i.
#include "decode_pass.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int FL_THREADS = 64;

enum FlacStatus {
    FL_OK = 0, FL_SUBFRAME_TYPE, FL_PAD_BIT, FL_WASTED, FL_RESIDUAL_METHOD, FL_PARTITION, FL_LPC_PRECISION, FL_LPC_SHIFT,
    FL_OVERRUN, FL_PADDING, FL_FOOTER, FL_CRC16,
};

__host__ __device__ inline uint16_t crc16_entry(uint32_t b) {
    uint32_t c = b << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) : (c << 1);
    return (uint16_t)c;
}

// 64-bit MSB-first bit reader over 32-bit big-endian words.  Words at or past `wend` (the frame's last byte) read as 0, and
// on the host so do bytes past the buffer: a reader never touches memory outside its frame's words.
struct Bits {
    const uint8_t* base;
    int64_t blen;          // host: bytes of the buffer (device: unused)
    int64_t wpos, wend;
    uint64_t c;
    int n;
    bool bad;

    __host__ __device__ inline uint32_t word(int64_t w) const {
#ifdef __HIP_DEVICE_COMPILE__
        return __builtin_bswap32(reinterpret_cast<const uint32_t*>(base)[w]);
#else
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) {
            const int64_t i = 4 * w + k;
            v = (v << 8) | (i < blen ? base[i] : 0u);
        }
        return v;
#endif
    }
    __host__ __device__ inline void init(const uint8_t* b, int64_t bl, int64_t byte0, int64_t byte_end) {
        base = b; blen = bl; wpos = byte0 >> 2; wend = (byte_end + 3) >> 2; c = 0; n = 0; bad = false;
        refill();
        get((int)(byte0 & 3) * 8);
    }
    __host__ __device__ inline void refill() {
        if (n <= 32) {
            const uint32_t w = wpos < wend ? word(wpos) : 0u;
            c |= (uint64_t)w << (32 - n);
            n += 32;
            ++wpos;
        }
    }
    __host__ __device__ inline int64_t pos() const { return wpos * 32 - n; }      // absolute bit index of the next bit
    __host__ __device__ inline uint32_t get(int k) {                            // 0 <= k <= 32
        refill();
        if (k == 0) return 0;
        const uint32_t v = (uint32_t)(c >> (64 - k));
        c <<= k;
        n -= k;
        return v;
    }
    __host__ __device__ inline int32_t sget(int k) {
        const uint32_t v = get(k);
        return k == 0 ? 0 : (int32_t)(v << (32 - k)) >> (32 - k);
    }
    // zeros ended by a one; `limit` = absolute bit past which the count stops (sets `bad`)
    __host__ __device__ inline uint32_t unary(int64_t limit) {
        uint32_t q = 0;
        for (;;) {
            refill();
            if (c) {
                const int z = __builtin_clzll(c);
                q += (uint32_t)z;
                c <<= z;
                c <<= 1;
                n -= z + 1;
                return q;
            }
            q += (uint32_t)n;
            c = 0;
            n = 0;
            if (pos() > limit) { bad = true; return q; }
        }
    }
};

// Where one subframe's samples go.  kind 0: stored as they are; 1..3: the second subframe of left/side, side/right and
// mid/side, combined with the first (already stored) into both channels.
template <bool WIN>
struct Sink {
    uint8_t* p;
    int stride, chan, sh, kind;
    bool wide;
    int lo, hi;            // WIN: the frame's samples inside the window

    __host__ __device__ inline int32_t ld(int64_t e) const {
        return wide ? reinterpret_cast<const int32_t*>(p)[e] : (int32_t)reinterpret_cast<const int16_t*>(p)[e];
    }
    __host__ __device__ inline void st(int64_t e, uint32_t v) const {
        if (wide) reinterpret_cast<int32_t*>(p)[e] = (int32_t)v;
        else      reinterpret_cast<int16_t*>(p)[e] = (int16_t)(uint16_t)v;
    }
    __host__ __device__ inline void put(int64_t i, int32_t v) const {
        if constexpr (WIN)
            if (i < lo || i >= hi) return;
        const int64_t e = i * stride;
        switch (kind) {
            case 0: st(e + chan, (uint32_t)v << sh); break;
            case 1: st(e + 1, (uint32_t)ld(e) - ((uint32_t)v << sh)); break;                     // right = left - side
            case 2: st(e, (uint32_t)ld(e) + ((uint32_t)v << sh)); st(e + 1, (uint32_t)v << sh); break;   // left = side + right
            default: {                                                                           // mid/side
                const int32_t mid = (int32_t)((uint32_t)(ld(e) >> sh) << 1) | (v & 1);
                st(e, (uint32_t)((mid + v) >> 1) << sh);
                st(e + 1, (uint32_t)((mid - v) >> 1) << sh);
            }
        }
    }
};

// Residual partitions + prediction of a FIXED or LPC subframe, history and coefficients in registers.  N: order bucket (>=
// order); WIDE: 64-bit sums.  The warm-up samples have been read into h (h[0] most recent) and emitted.
template <int N, bool WIDE, class S>
__host__ __device__ __forceinline__ int residual_predict(Bits& br, int64_t limit, const S& out, int bs, int order, const int32_t (&q)[N],
                                                int32_t (&h)[N], int shift, int wasted) {
    const uint32_t method = br.get(2);
    if (method > 1) return FL_RESIDUAL_METHOD;
    const int pbits = method ? 5 : 4, esc = (1 << pbits) - 1;
    const int porder = (int)br.get(4);
    const int psize = bs >> porder;
    if ((psize << porder) != bs || psize < order) return FL_PARTITION;
    int64_t i = order;
    for (int part = 0; part < (1 << porder); ++part) {
        const int k = (int)br.get(pbits);
        const int64_t iend = (int64_t)(part + 1) * psize;
        const int ew = k == esc ? (int)br.get(5) : 0;
        for (; i < iend; ++i) {
            int32_t r;
            if (k == esc) {
                r = br.sget(ew);
            } else {
                const uint32_t u = (br.unary(limit) << k) | br.get(k);
                r = (int32_t)((u >> 1) ^ (0u - (u & 1)));
            }
            int32_t pred;
            if (WIDE) {
                int64_t s = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) s += (int64_t)q[j] * h[j];
                pred = (int32_t)(s >> shift);
            } else {
                uint32_t s = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) s += (uint32_t)q[j] * (uint32_t)h[j];
                pred = (int32_t)s >> shift;
            }
            const int32_t x = (int32_t)((uint32_t)r + (uint32_t)pred);
#pragma unroll
            for (int j = N - 1; j > 0; --j) h[j] = h[j - 1];
            h[0] = x;
            out.put(i, (int32_t)((uint32_t)x << wasted));
        }
        if (br.bad || br.pos() > limit) return FL_OVERRUN;
    }
    return FL_OK;
}

// warm-up, coefficients, then the residual loop of bucket N
template <int N, class S>
__host__ __device__ __forceinline__ int predicted(Bits& br, int64_t limit, const S& out, int bs, int sbps, int wasted, int order,
                                         int fixed) {
    int32_t q[N], h[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { q[j] = 0; h[j] = 0; }
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j < order) {
            const int32_t v = br.sget(sbps);
#pragma unroll
            for (int m = N - 1; m > 0; --m) h[m] = h[m - 1];
            h[0] = v;
            out.put(j, (int32_t)((uint32_t)v << wasted));
        }
    int shift = 0, qbits = 0;
    if (fixed) {
        if (N >= 4) {                                    // RFC 9639 11.28: the fixed predictors of order 1..4
            const int32_t t[4][4] = {{1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
#pragma unroll
            for (int o = 1; o <= 4; ++o)
                if (order == o) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j < N ? j : 0] = t[o - 1][j];
                }
        }
        qbits = 4;
    } else {
        const int prec = (int)br.get(4) + 1;
        if (prec == 16) return FL_LPC_PRECISION;
        shift = br.sget(5);
        if (shift < 0) return FL_LPC_SHIFT;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < order) q[j] = br.sget(prec);
        qbits = prec + (order > 1 ? 32 - __builtin_clz((uint32_t)(order - 1)) : 0);
    }
    if (br.bad || br.pos() > limit) return FL_OVERRUN;
    if (sbps + qbits > 32) return residual_predict<N, true>(br, limit, out, bs, order, q, h, shift, wasted);
    return residual_predict<N, false>(br, limit, out, bs, order, q, h, shift, wasted);
}

// One frame: subframes after its `hdr`-byte header, samples [0, bs) of every channel into dst (element 0 = channel 0 of
// the frame's first sample), then padding and CRC-16.  Returns a FlacStatus.
// WIN: only samples [lo, hi) of the frame are stored (dst is still where sample 0 would go)
template <bool WIN>
__host__ __device__ __forceinline__ int flac_decode_frame(const uint8_t* base, int64_t blen, int64_t off, int64_t len, int hdr, int bs, int mode,
                                          int bps, uint8_t* dst, bool wide, const uint16_t* crc_tab, int lo = 0, int hi = 0) {
    const int nch = mode < 8 ? mode + 1 : 2;
    const int64_t end_bit = (off + len - 2) * 8;
    Bits br;
    br.init(base, blen, off + hdr, off + len);
    Sink<WIN> out{dst, nch, 0, (wide ? 32 : 16) - bps, 0, wide, lo, hi};
    for (int ch = 0; ch < nch; ++ch) {
        const bool side = (mode == 8 && ch == 1) || (mode == 9 && ch == 0) || (mode == 10 && ch == 1);
        int sbps = bps + (side ? 1 : 0);
        out.chan = ch;
        out.kind = (mode >= 8 && ch == 1) ? mode - 7 : 0;
        if (br.get(1)) return FL_PAD_BIT;
        const int type = (int)br.get(6);
        int wasted = 0;
        if (br.get(1)) wasted = (int)br.unary(end_bit) + 1;
        if (wasted >= sbps) return FL_WASTED;
        sbps -= wasted;
        int rc = FL_OK;
        if (type == 0) {
            const int32_t v = (int32_t)((uint32_t)br.sget(sbps) << wasted);
            for (int i = 0; i < bs; ++i) out.put(i, v);
        } else if (type == 1) {
            if (br.pos() + (int64_t)bs * sbps > end_bit) return FL_OVERRUN;
            for (int i = 0; i < bs; ++i) out.put(i, (int32_t)((uint32_t)br.sget(sbps) << wasted));
        } else if (type >= 8 && type <= 12) {
            const int order = type - 8;
            if (order > bs) return FL_PARTITION;
            rc = predicted<4>(br, end_bit, out, bs, sbps, wasted, order, 1);
        } else if (type >= 32) {
            const int order = type - 31;
            if (order > bs) return FL_PARTITION;
            if (order <= 4)       rc = predicted<4>(br, end_bit, out, bs, sbps, wasted, order, 0);
            else if (order <= 8)  rc = predicted<8>(br, end_bit, out, bs, sbps, wasted, order, 0);
            else if (order <= 16) rc = predicted<16>(br, end_bit, out, bs, sbps, wasted, order, 0);
            else                  rc = predicted<32>(br, end_bit, out, bs, sbps, wasted, order, 0);
        } else {
            return FL_SUBFRAME_TYPE;
        }
        if (rc) return rc;
        if (br.bad || br.pos() > end_bit) return FL_OVERRUN;
    }
    if (br.get((int)((8 - (br.pos() & 7)) & 7))) return FL_PADDING;
    if (br.pos() != end_bit) return FL_FOOTER;
    // CRC-16 of everything in front of the footer, four bytes per table pass where the reader allows
    Bits cr;
    cr.init(base, blen, off, off + len);
    uint32_t crc = 0;
    int64_t nb = len - 2;
    for (; nb >= 4; nb -= 4) {
        const uint32_t w = cr.get(32);
#pragma unroll
        for (int s = 24; s >= 0; s -= 8) crc = ((crc << 8) ^ crc_tab[((crc >> 8) ^ (w >> s)) & 0xFF]) & 0xFFFF;
    }
    for (; nb > 0; --nb) crc = ((crc << 8) ^ crc_tab[((crc >> 8) ^ cr.get(8)) & 0xFF]) & 0xFFFF;
    if (crc != cr.get(16)) return FL_CRC16;
    return FL_OK;
}

struct FlacFrameDev {
    int64_t src_off;      // absolute byte offset of the frame in the source buffer
    int64_t dst_byte;     // byte offset of its first output element (signal or staging buffer)
    int32_t len, hdr, bs;
    int16_t mode, bps;
    int8_t wide, to_sig, pad0, pad1;
    int32_t pad2;
};

struct FlacWinDev { int32_t lo, hi; };      // beside FlacFrameDev k of a windowed call: the frame's samples inside its job's window

// WIN = false is the kernel every call without windows launches; WIN = true reads the window table that follows the rows
template <bool WIN>
__global__ __launch_bounds__(FL_THREADS) void flac_decode_kernel(const uint8_t* __restrict__ src, const FlacFrameDev* __restrict__ fr,
                                                                 int64_t nfr, int16_t* sig, uint8_t* stage, int32_t* __restrict__ status) {
    __shared__ uint16_t tab[256];
    for (int k = threadIdx.x; k < 256; k += FL_THREADS) tab[k] = crc16_entry((uint32_t)k);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    if (i >= nfr) return;
    const FlacFrameDev F = fr[i];
    uint8_t* dst = (F.to_sig ? reinterpret_cast<uint8_t*>(sig) : stage) + F.dst_byte;
    if constexpr (WIN) {
        const FlacWinDev W = reinterpret_cast<const FlacWinDev*>(fr + nfr)[i];
        status[i] = flac_decode_frame<true>(src, 0, F.src_off, F.len, F.hdr, F.bs, F.mode, F.bps, dst, F.wide != 0, tab, W.lo, W.hi);
    } else {
        status[i] = flac_decode_frame<false>(src, 0, F.src_off, F.len, F.hdr, F.bs, F.mode, F.bps, dst, F.wide != 0, tab);
    }
}

const uint16_t* host_crc16_table() {
    static uint16_t t[256];
    static bool done = false;
    if (!done) {
        for (int k = 0; k < 256; ++k) t[k] = crc16_entry((uint32_t)k);
        done = true;
    }
    return t;
}

uint8_t crc8(const uint8_t* p, int64_t n) {
    uint32_t c = 0;
    for (int64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    return (uint8_t)c;
}

const int kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
const int kBps[8] = {0, 8, 12, -1, 16, 20, 24, 32};

// Frame header at buf[pos]: -> nullptr and the row + coded number, or the reason it is not a valid header.
const char* parse_header(const uint8_t* buf, int64_t len, int64_t pos, const iss_flac_info& si, iss_flac_frame& row,
                         uint64_t& number, int& variable) {
    if (len - pos < 6) return "truncated frame header";
    if (buf[pos] != 0xFF || (buf[pos + 1] & 0xFE) != 0xF8) return "no frame sync code";
    variable = buf[pos + 1] & 1;
    const int bs_code = buf[pos + 2] >> 4, sr_code = buf[pos + 2] & 15;
    const int ch_code = buf[pos + 3] >> 4, ss_code = (buf[pos + 3] >> 1) & 7;
    if (bs_code == 0) return "reserved block size code";
    if (sr_code == 15) return "invalid sample rate code";
    if (ch_code > 10) return "reserved channel assignment";
    if (ss_code == 3) return "reserved sample size code";
    if (buf[pos + 3] & 1) return "reserved header bit set";
    int64_t p = pos + 4;
    const uint8_t b0 = buf[p];
    int nb = 0;
    while (nb < 8 && (b0 & (0x80 >> nb))) ++nb;
    if (nb == 1 || nb == 8 || nb > (variable ? 7 : 6)) return "invalid coded number";
    const int extra = nb ? nb - 1 : 0;
    if (p + 1 + extra > len) return "truncated frame header";
    uint64_t v = nb ? (uint64_t)(b0 & (0x7F >> nb)) : b0;
    for (int k = 1; k <= extra; ++k) {
        if ((buf[p + k] & 0xC0) != 0x80) return "invalid coded number";
        v = (v << 6) | (buf[p + k] & 0x3F);
    }
    number = v;
    p += 1 + extra;
    int bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code <= 7) {
        const int nbb = bs_code == 6 ? 1 : 2;
        if (p + nbb > len) return "truncated frame header";
        bs = (nbb == 1 ? buf[p] : (buf[p] << 8) | buf[p + 1]) + 1;
        p += nbb;
    } else bs = 256 << (bs_code - 8);
    int rate = sr_code ? kRates[sr_code < 12 ? sr_code : 0] : si.sample_rate;
    if (sr_code >= 12) {
        const int nbr = sr_code == 12 ? 1 : 2;
        if (p + nbr > len) return "truncated frame header";
        const int r = nbr == 1 ? buf[p] : (buf[p] << 8) | buf[p + 1];
        rate = sr_code == 12 ? r * 1000 : sr_code == 13 ? r : r * 10;
        p += nbr;
    }
    if (p + 1 > len) return "truncated frame header";
    if (crc8(buf + pos, p - pos) != buf[p]) return "header CRC-8 mismatch";
    const int bps = ss_code ? kBps[ss_code] : si.bps;
    const int nch = ch_code < 8 ? ch_code + 1 : 2;
    if (rate != si.sample_rate) return "sample rate differs from STREAMINFO";
    if (bps != si.bps) return "sample size differs from STREAMINFO";
    if (nch != si.channels) return "channel count differs from STREAMINFO";
    if (si.max_block > 0 && bs > si.max_block) return "block size above the STREAMINFO maximum";
    row.offset = pos;
    row.length = 0;
    row.first_sample = 0;
    row.block_size = bs;
    row.channel_mode = ch_code;
    row.bps = bps;
    row.header_bytes = (int32_t)(p + 1 - pos);
    return nullptr;
}

int index_fail(int64_t* err_offset, char* err, int32_t err_len, int64_t off, const char* fmt, ...) {
    if (err_offset) *err_offset = off;
    if (err && err_len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)err_len, fmt, ap);
        va_end(ap);
    }
    return ISS_EINVAL;
}

}  // namespace

extern "C" int iss_flac_crc(const uint8_t* buf, int64_t n, int32_t* crc8_out, int32_t* crc16_out) {
    if ((!buf && n > 0) || n < 0) return ISS_EINVAL;
    if (crc8_out) *crc8_out = crc8(buf, n);
    if (crc16_out) {
        const uint16_t* t = host_crc16_table();
        uint32_t c = 0;
        for (int64_t i = 0; i < n; ++i) c = ((c << 8) ^ t[((c >> 8) ^ buf[i]) & 0xFF]) & 0xFFFF;
        *crc16_out = (int32_t)c;
    }
    return ISS_OK;
}

extern "C" int iss_flac_index(const uint8_t* buf, int64_t len, int64_t first_frame, const iss_flac_info* si, iss_flac_frame* frames,
                              int64_t cap, int64_t* nframes, int64_t* err_offset, char* err, int32_t err_len) {
    if (err && err_len > 0) err[0] = 0;
    if (err_offset) *err_offset = -1;
    if (!buf || !si || !nframes || (!frames && cap > 0) || len < 0 || first_frame < 0 || first_frame > len || cap < 0)
        return index_fail(err_offset, err, err_len, 0, "bad argument");
    *nframes = 0;
    if (si->channels < 1 || si->channels > 8 || si->sample_rate < 1)
        return index_fail(err_offset, err, err_len, first_frame, "bad STREAMINFO");
    int64_t pos = first_frame, k = 0, total = 0;
    int strategy = -1, first_bs = 0, prev_bs = 0;
    while (pos < len) {
        iss_flac_frame row;
        uint64_t num;
        int var;
        const char* why = parse_header(buf, len, pos, *si, row, num, var);
        if (why) return index_fail(err_offset, err, err_len, pos, "%s", why);
        if (strategy < 0) { strategy = var; first_bs = row.block_size; }
        if (var != strategy) return index_fail(err_offset, err, err_len, pos, "blocking strategy changes within the stream");
        if (var ? num != (uint64_t)total : num != (uint64_t)k)
            return index_fail(err_offset, err, err_len, pos, "frame-sequence break (%s %llu, expected %lld)",
                              var ? "sample number" : "frame number", (unsigned long long)num, (long long)(var ? total : k));
        if (!var && k > 0 && prev_bs != first_bs)
            return index_fail(err_offset, err, err_len, pos, "frame-sequence break (a short block before the last frame)");
        // the next frame: a sync code whose header parses, passes its CRC-8 and continues the sequence
        const uint64_t want = var ? (uint64_t)(total + row.block_size) : (uint64_t)(k + 1);
        int64_t next = len, bad_at = -1;
        const char* bad_why = nullptr;
        for (int64_t s = pos + row.header_bytes; s + 1 < len;) {
            const void* hit = memchr(buf + s, 0xFF, (size_t)(len - 1 - s));
            if (!hit) break;
            const int64_t q = (const uint8_t*)hit - buf;
            if (buf[q + 1] == (0xF8 | var)) {
                iss_flac_frame r2;
                uint64_t n2;
                int v2;
                const char* w2 = parse_header(buf, len, q, *si, r2, n2, v2);
                if (!w2 && n2 == want) { next = q; break; }
                if (bad_at < 0) { bad_at = q; bad_why = w2 ? w2 : "frame-sequence break"; }
            }
            s = q + 1;
        }
        // no successor although STREAMINFO says more samples follow: name the first sync code that did not make a frame
        if (next == len && si->total_samples > 0 && total + row.block_size < si->total_samples)
            return index_fail(err_offset, err, err_len, bad_at >= 0 ? bad_at : pos, "%s",
                              bad_at >= 0 ? bad_why : "stream ends before the STREAMINFO total");
        row.length = next - pos;
        row.first_sample = total;
        if (row.length < row.header_bytes + 3) return index_fail(err_offset, err, err_len, pos, "truncated frame");
        if (k >= cap) { *nframes = k; return ISS_ENOMEM; }
        frames[k] = row;
        total += row.block_size;
        prev_bs = row.block_size;
        ++k;
        pos = next;
    }
    if (k == 0) return index_fail(err_offset, err, err_len, first_frame, "no audio frames");
    if (si->total_samples > 0 && si->total_samples != total)
        return index_fail(err_offset, err, err_len, frames[k - 1].offset, "STREAMINFO total of %lld samples differs from the "
                          "frames' %lld", (long long)si->total_samples, (long long)total);
    *nframes = k;
    return ISS_OK;
}

// The rows tile [0, total) in order; with a window `w` they are a contiguous run of the file's frames (the file's numbering)
// that lies inside [0, total) and covers [w->s_begin, w->s_end).
static bool frame_rows_ok(const iss_flac_frame* fr, int64_t nfr, int64_t bytes, int32_t channels, int32_t bps, int64_t total,
                          const iss_window* w = nullptr) {
    int64_t t = w ? fr[0].first_sample : 0;
    if (w && (t < 0 || t > w->s_begin)) return false;
    for (int64_t k = 0; k < nfr; ++k) {
        const iss_flac_frame& f = fr[k];
        const int nch = f.channel_mode < 8 ? f.channel_mode + 1 : 2;
        if (f.offset < 0 || f.header_bytes < 6 || f.length < f.header_bytes + 3 || f.offset > bytes - f.length ||
            f.length > (int64_t)1 << 30 || f.first_sample != t || f.block_size < 1 || f.block_size > 65536 ||
            f.channel_mode < 0 || f.channel_mode > 10 || nch != channels || f.bps != bps)
            return false;
        t += f.block_size;
    }
    return w ? t >= w->s_end && t <= total : t == total;
}

extern "C" int iss_flac_decode_host(const uint8_t* buf, int64_t len, const iss_flac_frame* frames, int64_t nframes, int32_t channels,
                                    int32_t bps, int64_t frames_total, void* out, int32_t* status_out) {
    if (!buf || !frames || !out || !status_out || nframes < 1 || (bps != 8 && bps != 16 && bps != 24) ||
        !frame_rows_ok(frames, nframes, len, channels, bps, frames_total))
        return ISS_EINVAL;
    const bool wide = bps > 16;
    const uint16_t* tab = host_crc16_table();
    for (int64_t k = 0; k < nframes; ++k) {
        const iss_flac_frame& f = frames[k];
        uint8_t* dst = (uint8_t*)out + f.first_sample * channels * (wide ? 4 : 2);
        status_out[k] = flac_decode_frame<false>(buf, len, f.offset, f.length, f.header_bytes, f.block_size, f.channel_mode, f.bps, dst,
                                          wide, tab);
    }
    return ISS_OK;
}

// the five entry points: windows beside the jobs, splits (with their selection table) beside the jobs, both, or neither; or
// the mix tables `mix` (with or without windows)
static int flac_decode(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                       const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal, int32_t* status_out,
                       const iss_split* splits, const int32_t* channel_sel, int64_t nsel, const IssMixTables* mix = nullptr) {
    if (!c || njobs < 0 || (njobs > 0 && (!jobs || !frames || !status_out)) || src_bytes < 0 || (!src && src_bytes > 0) ||
        nframes < 0 || (mix && njobs > 0 && !mix->sets))
        return iss_fail(c, ISS_EINVAL, "iss_flac_decode: bad argument");
    IssDecodePass pass;
    int rc = pass.begin(c, "iss_flac_decode", n_signal, njobs);
    if (rc) return rc;
    pass.jsplits = splits; pass.sel = channel_sel; pass.nsel = nsel; pass.jmix = mix;
    // one table: the frame rows, then (windowed) their FlacWinDev
    std::vector<uint8_t> table((size_t)nframes * (sizeof(FlacFrameDev) + (windows ? sizeof(FlacWinDev) : 0)));
    FlacFrameDev* dev = reinterpret_cast<FlacFrameDev*>(table.data());
    FlacWinDev* dwin = reinterpret_cast<FlacWinDev*>(dev + nframes);
    std::vector<char> used((size_t)nframes, 0);
    for (int32_t j = 0; j < njobs; ++j) {
        const iss_flac_job& J = jobs[j];
        if (J.channels < 1 || J.channels > 8 || (J.bps != 8 && J.bps != 16 && J.bps != 24))
            return iss_fail(c, ISS_EINVAL, "iss_flac_decode: job %d: %d channels of %d bits", j, J.channels, J.bps);
        if (J.frame_begin < 0 || J.nframes < 1 || J.frame_begin > nframes - J.nframes)
            return iss_fail(c, ISS_EINVAL, "iss_flac_decode: job %d: rows [%lld, +%lld) outside the %lld frames", j,
                            (long long)J.frame_begin, (long long)J.nframes, (long long)nframes);
        if (J.frames_total < 1 || J.frames_total > ((int64_t)1 << 40) / (4 * J.channels))
            return iss_fail(c, ISS_EINVAL, "iss_flac_decode: job %d: %lld samples", j, (long long)J.frames_total);
        if (J.src_offset < 0 || J.src_offset > src_bytes ||
            !frame_rows_ok(frames + J.frame_begin, J.nframes, src_bytes - J.src_offset, J.channels, J.bps, J.frames_total,
                           windows ? windows + j : nullptr))
            return iss_fail(c, ISS_EINVAL, "iss_flac_decode: job %d: frame rows outside the source bytes, not consecutive from "
                            "sample 0 to frames_total%s, or not of the job's channels / bits", j,
                            windows ? " (windowed: not a run of the file's frames that covers the window)" : "");
        for (int64_t k = J.frame_begin; k < J.frame_begin + J.nframes; ++k) {
            if (used[(size_t)k]) return iss_fail(c, ISS_EINVAL, "iss_flac_decode: frame row %lld belongs to two jobs", (long long)k);
            used[(size_t)k] = 1;
        }
        const bool wide = J.bps > 16;
        const int esz = wide ? 4 : 2;
        bool to_sig;
        int64_t base;
        if ((rc = pass.place(j, {J.output, J.filter, J.dst_offset, J.frames_out}, J.frames_total, J.channels, esz,
                             J.channels == 1 && !wide, "mono 8/16-bit", to_sig, base, windows ? windows + j : nullptr)))
            return rc;
        const int64_t s_begin = windows ? windows[j].s_begin : 0;      // `base` is where this sample goes
        for (int64_t k = J.frame_begin; k < J.frame_begin + J.nframes; ++k) {
            const iss_flac_frame& f = frames[k];
            FlacFrameDev& d = dev[(size_t)k];
            d.src_off = J.src_offset + f.offset;
            d.dst_byte = base + (f.first_sample - s_begin) * J.channels * esz;
            if (windows) {
                const int64_t lo = s_begin - f.first_sample, hi = windows[j].s_end - f.first_sample;
                dwin[k].lo = (int32_t)std::max<int64_t>(lo, 0);
                dwin[k].hi = (int32_t)std::min<int64_t>(std::max<int64_t>(hi, 0), f.block_size);
            }
            d.len = (int32_t)f.length; d.hdr = f.header_bytes; d.bs = f.block_size;
            d.mode = (int16_t)f.channel_mode; d.bps = (int16_t)f.bps;
            d.wide = wide ? 1 : 0; d.to_sig = to_sig ? 1 : 0; d.pad0 = d.pad1 = 0; d.pad2 = 0;
        }
    }
    for (int64_t k = 0; k < nframes; ++k)
        if (!used[(size_t)k]) return iss_fail(c, ISS_EINVAL, "iss_flac_decode: frame row %lld belongs to no job", (long long)k);
    if ((rc = pass.commit(&c->flac))) return rc;
    if (nframes == 0) return ISS_OK;
    if ((rc = pass.upload(c->flac, src, src_bytes, (size_t)(src_bytes + 16) / 4 * 4 + 16, table.data(), table.size(), nframes)))
        return rc;
    iss_prof_begin(c, ISS_PROF_FRONTEND, 0.0);
    iss_prof_inst(c, "flac_decode_kernel");
    hipLaunchKernelGGL(windows ? flac_decode_kernel<true> : flac_decode_kernel<false>, dim3((unsigned)((nframes + FL_THREADS - 1) / FL_THREADS)), dim3(FL_THREADS), 0, c->stream,
                       (const uint8_t*)c->flac.src.p, (const FlacFrameDev*)c->flac.rows.p, nframes, (int16_t*)c->sig.p,
                       (uint8_t*)c->flac.stage.p, (int32_t*)c->flac.status.p);
    ISS_HIP(c, hipGetLastError());
    iss_prof_end(c);
    return pass.finish(c->flac, status_out, nframes);
}

extern "C" int iss_flac_decode_windows(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                                       const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal,
                                       int32_t* status_out) {
    return flac_decode(c, src, src_bytes, frames, nframes, jobs, windows, njobs, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_flac_decode(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                               const iss_flac_job* jobs, int32_t njobs, int64_t n_signal, int32_t* status_out) {
    return flac_decode(c, src, src_bytes, frames, nframes, jobs, nullptr, njobs, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_flac_decode_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                                     const iss_flac_job* jobs, int32_t njobs, int64_t n_signal, int32_t* status_out,
                                     const iss_split* splits, const int32_t* channel_sel, int64_t nsel) {
    return flac_decode(c, src, src_bytes, frames, nframes, jobs, nullptr, njobs, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_flac_decode_windows_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames,
                                             int64_t nframes, const iss_flac_job* jobs, const iss_window* windows, int32_t njobs,
                                             int64_t n_signal, int32_t* status_out, const iss_split* splits,
                                             const int32_t* channel_sel, int64_t nsel) {
    return flac_decode(c, src, src_bytes, frames, nframes, jobs, windows, njobs, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_flac_decode_mix(iss_ctx* c, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                                   const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal,
                                   int32_t* status_out, const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes,
                                   const iss_mix_term* terms, int64_t nterms) {
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return flac_decode(c, src, src_bytes, frames, nframes, jobs, windows, njobs, n_signal, status_out, nullptr, nullptr, 0, &mix);
}

extern "C" int iss_flac_get_stage(iss_ctx* c, int32_t job, void* out, int64_t bytes) {
    return c ? iss_codec_get_stage(c, c->flac, job, out, bytes) : iss_fail(c, ISS_EINVAL, "iss_flac_get_stage: bad argument");
}

extern "C" int iss_flac_stats(iss_ctx* c, int64_t* launches, int64_t* frames) {
    return iss_get_counters(c ? &c->flac.count : nullptr, launches, frames);
}
