// How a stored sample becomes float64, and how a workgroup stages channels of interleaved frames in LDS: written once for
// resample.hip (every resample_kernel instantiation) and survey.hip (survey_kernel).  Device code only; not part of the ABI.
#pragma once
#include "iss_internal.h"
#include "survey_plan.h"     // SetChanDev: a row of the per-channel table of a survey job over a set

namespace {

constexpr int RS_THREADS = 256;

__device__ __forceinline__ double to_f64(uint8_t x) { return __ddiv_rn(__dsub_rn((double)x, 128.0), 128.0); }
__device__ __forceinline__ double to_f64(int8_t x) { return __ddiv_rn((double)x, 128.0); }     // = the u8 twin x + 128
__device__ __forceinline__ double to_f64(int16_t x) { return __ddiv_rn((double)x, 32768.0); }
__device__ __forceinline__ double to_f64(int32_t x) { return __ddiv_rn((double)x, 2147483648.0); }
__device__ __forceinline__ double to_f64(float x) { return (double)x; }
__device__ __forceinline__ double to_f64(double x) { return x; }

// G.711 expansion (include/iss.h states both): the decoded 16-bit value of a stored byte
__device__ __forceinline__ int ulaw_value(uint32_t b) {
    const uint32_t u = ~b & 0xFFu;
    const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int alaw_value(uint32_t b) {
    const uint32_t a = (b ^ 0x55u) & 0xFFu;
    int t = (int)((a & 15u) << 4);
    const int s = (int)((a >> 4) & 7u);
    if (s == 0) t += 8;
    else if (s == 1) t += 0x108;
    else t = (t + 0x108) << (s - 1);
    return (a & 0x80u) ? t : -t;
}

// one stored sample -> float64 with libsndfile's scaling: as stored, G.711, or byte-swapped (big-endian sources)
template <typename T> struct LdPlain {
    using type = T;
    static __device__ __forceinline__ double get(const T* q) { return to_f64(*q); }
};
struct LdUlaw {
    using type = uint8_t;
    static __device__ __forceinline__ double get(const uint8_t* q) { return to_f64((int16_t)ulaw_value(*q)); }
};
struct LdAlaw {
    using type = uint8_t;
    static __device__ __forceinline__ double get(const uint8_t* q) { return to_f64((int16_t)alaw_value(*q)); }
};
struct LdSwapI16 {
    using type = uint16_t;
    static __device__ __forceinline__ double get(const uint16_t* q) { return to_f64((int16_t)__builtin_bswap16(*q)); }
};
struct LdSwapI32 {
    using type = uint32_t;
    static __device__ __forceinline__ double get(const uint32_t* q) { return to_f64((int32_t)__builtin_bswap32(*q)); }
};
struct LdSwapF32 {
    using type = uint32_t;
    static __device__ __forceinline__ double get(const uint32_t* q) { return (double)__uint_as_float(__builtin_bswap32(*q)); }
};
struct LdSwapF64 {
    using type = uint64_t;
    static __device__ __forceinline__ double get(const uint64_t* q) { return __longlong_as_double((long long)__builtin_bswap64(*q)); }
};

// frames s0 .. s0+len-1 of `gc` selected channels, each on its own: span[k * stride + .] = channel sel[k] (sel == NULL: channel
// c0 + k).  Thread e takes (frame e / gc, channel e % gc): neighbouring lanes read neighbouring samples of a frame
// (WIN: stage_span's rule -- s0 + k is the file's own frame, 0 outside [0, W.frames_total), read at W.in_begin less)
template <typename L, bool WIN>
__device__ __forceinline__ void stage_channels(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                               double* __restrict__ span, int stride, int c0, int gc,
                                               const int32_t* __restrict__ sel, const RsWinDev& W) {
    using T = typename L::type;
    const T* p = reinterpret_cast<const T*>(src);
    const int total = len * gc;
    for (int e = threadIdx.x; e < total; e += RS_THREADS) {
        const int k = e / gc, kk = e - k * gc;
        int64_t j = s0 + k;
        double v = 0.0;
        bool in = j >= 0 && j < n_in;
        if constexpr (WIN) {
            in = j >= 0 && j < W.frames_total;
            j -= W.in_begin;
            in = in && j >= 0 && j < n_in;                 // (the planner saw to it that a window reaches no unstaged frame)
        }
        if (in) v = L::get(p + j * ch + (sel ? sel[kk] : c0 + kk));
        span[(int64_t)kk * stride + k] = v;
    }
}

// File sets (include/iss.h): a channel of a job is channel c_local of one MEMBER, which the host resolved once per job to where
// its first sample lies (`off`, a byte offset into the source), the member's frames and its channels (`step`).  Sample j of the
// channel is the stored one while the member lasts and 0.0 after it: the zero the interleaved twin stores there.
// (the planner saw to it that every member's bytes lie inside the source and are aligned to the sample)
template <typename L>
__device__ __forceinline__ double set_sample(const uint8_t* __restrict__ src, int64_t off, int64_t frames, int step, int64_t j) {
    using T = typename L::type;
    return j < frames ? L::get(reinterpret_cast<const T*>(src + off) + j * step) : 0.0;
}

// stage_channels for a set (survey.hip), channels `chans[0, gc)`, frames s0 .. s0+len-1 (all inside the job: the survey's chunks
// are), the same rows at the same places.  Channel-major: row after row, the threads striding over the frames of one -- a wave
// reads consecutive frames of one member instead of one frame of 64 members, and the row of the channel table is the same for
// the whole workgroup (scalar loads, no division per sample)
template <typename L>
__device__ __forceinline__ void stage_set_channels(const uint8_t* __restrict__ src, const SetChanDev* __restrict__ chans, int64_t s0,
                                                   int len, double* __restrict__ span, int stride, int gc) {
    for (int kk = 0; kk < gc; ++kk) {
        const SetChanDev C = chans[kk];
        double* row = span + (int64_t)kk * stride;
        for (int k = threadIdx.x; k < len; k += RS_THREADS) row[k] = set_sample<L>(src, C.off, C.frames, C.step, s0 + k);
    }
}

// stage_mixes for a set (resample.hip; whole sources only): frames s0 .. s0+len-1 of `gm` mixes, span[q * stride + .] = mix q of
// `mixes`, its terms the RsSetTermDev rows of `rows`.  The arithmetic is stage_mixes', term for term: a frame outside the job is
// 0, a frame past the end of a term's member is w * 0.0 in the sum.  Channel-major, as stage_set_channels: mix after mix
template <typename L>
__device__ __forceinline__ void stage_set_mixes(const uint8_t* __restrict__ src, int64_t n_in, int64_t s0, int len,
                                                double* __restrict__ span, int stride, int gm, const RsMixRow* __restrict__ mixes,
                                                const RsTermDev* __restrict__ rows) {
    for (int q = 0; q < gm; ++q) {
        const RsMixRow M = mixes[q];
        const RsSetTermDev* t = reinterpret_cast<const RsSetTermDev*>(rows + M.term_begin);
        double* row = span + (int64_t)q * stride;
        for (int k = threadIdx.x; k < len; k += RS_THREADS) {
            const int64_t j = s0 + k;
            double v = 0.0;
            if (j >= 0 && j < n_in) {
                v = __dmul_rn(t[0].weight, set_sample<L>(src, t[0].off, t[0].frames, t[0].step, j));
                for (int n = 1; n < M.term_count; ++n)
                    v = __dadd_rn(v, __dmul_rn(t[n].weight, set_sample<L>(src, t[n].off, t[n].frames, t[n].step, j)));
                v = __ddiv_rn(v, M.divisor);
            }
            row[k] = v;
        }
    }
}

}  // namespace
