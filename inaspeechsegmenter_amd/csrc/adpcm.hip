// IMA ADPCM (WAV format tag 0x11) and Microsoft ADPCM (tag 2) decoding for the ffmpeg-free read, on gfx950 and on the host
// from one source.
//
// ima_decode_block walks ONE channel of ONE block: the 4-byte channel header (predictor = first sample, step index), then
// that channel's 4-byte words, 8 nibbles each, low nibble first (include/iss.h states the step).  It is __host__ __device__:
// iss_adpcm_decode_host runs it on the CPU, adpcm_decode_kernel on the device.
//
// Grid: ragged over (job, block), one 64-lane workgroup (a wave) per block; job k owns blocks [block_base_k, +nblocks_k), a
// prefix sum built on the host, found by binary search as the resample kernel finds its tile's job.  The predictor chain of
// a channel is serial, so lane c walks channel c (c, c + 64, ... for wide files) and writes its samples interleaved into
// LDS; after a barrier the whole wave copies the block's samples to global memory, consecutive lanes to consecutive 16-bit
// samples (a lane per block would store 16-bit samples a block apart: one cache line per store).  All offsets are 64-bit.
//
// Coders: the kernel is a template over the coder (CODER_IMA, CODER_MS).  The two differ in the block walk (ima_decode_block /
// ms_decode_block), in samples_per_block and in the one status code a malformed header gives; grid, search, LDS, barrier, store,
// windows and offsets are written once.  ms_decode_block walks ONE channel of ONE Microsoft block: predictor index, delta and two
// seed samples from the 7-byte-per-channel header, then that channel's 4-bit codes, high nibble first, cycling through the
// channels.  Its header fields sit at odd offsets and a block need not start on a 4-byte boundary, so it reads bytes only.
//
// Windows (include/iss.h, iss_window): WIN = true is a second instantiation for calls that carry a window beside every job.
// The job's blocks are the file's blocks from block0 on; a block is walked into LDS as always (the walk starts at its header),
// and the coalesced store keeps the samples inside [s_begin, s_end), at their position counted from s_begin.
#include "decode_pass.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int AD_THREADS = 64;
constexpr int AD_MAX_ALIGN = 32768;               // bytes per block at most: its samples (< 4 bytes each stored byte) fit LDS

constexpr int16_t kStep[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
    1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132,
    7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__host__ __device__ inline int ima_step(int idx) { return kStep[idx]; }

__host__ __device__ inline uint32_t load_le32(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const uint32_t*>(p);                     // blocks start on 4-byte boundaries (checked on the host)
#else
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

// Channel `c` of the block at `blk` (`ch` channels): samples 0 .. n-1 to out[s * stride].  -> ISS_ADPCM_* of the header.
__host__ __device__ inline int ima_decode_block(const uint8_t* blk, int ch, int c, int n, int16_t* out, int64_t stride) {
    const uint32_t hdr = load_le32(blk + 4 * c);
    int pred = (int16_t)(hdr & 0xFFFFu);
    int idx = (int)((hdr >> 16) & 0xFFu);
    int status = ISS_ADPCM_OK;
    if (idx > 88) { idx = 88; status = ISS_ADPCM_STEP_INDEX; }
    if (n > 0) out[0] = (int16_t)pred;
    const uint8_t* words = blk + 4 * (int64_t)ch + 4 * c;
    for (int s = 1; s < n; s += 8, words += 4 * (int64_t)ch) {
        uint32_t w = load_le32(words);
        const int m = n - s < 8 ? n - s : 8;
        for (int k = 0; k < m; ++k, w >>= 4) {
            const int nib = (int)(w & 15u);
            const int step = ima_step(idx);
            int d = step >> 3;
            if (nib & 1) d += step >> 2;
            if (nib & 2) d += step >> 1;
            if (nib & 4) d += step;
            pred = (nib & 8) ? pred - d : pred + d;
            pred = pred < -32768 ? -32768 : (pred > 32767 ? 32767 : pred);
            idx += (nib & 4) ? 2 * (nib & 3) + 2 : -1;                 // {-1,-1,-1,-1,2,4,6,8}[nib & 7]
            idx = idx < 0 ? 0 : (idx > 88 ? 88 : idx);
            out[(int64_t)(s + k) * stride] = (int16_t)pred;
        }
    }
    return status;
}

constexpr int16_t kMsC1[7] = {256, 512, 0, 192, 240, 460, 392};
constexpr int16_t kMsC2[7] = {0, -256, 0, 64, 0, -208, -232};
constexpr int16_t kMsAdapt[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
constexpr int MS_DELTA_MIN = 16, MS_DELTA_MAX = 1 << 21;     // the cap: 768 * 2^21, and 8 * 2^21 beside a prediction below 2^17, stay inside 32 bits

__host__ __device__ inline int ms_c1(int p) { return kMsC1[p]; }
__host__ __device__ inline int ms_c2(int p) { return kMsC2[p]; }
__host__ __device__ inline int ms_adapt(int n) { return kMsAdapt[n]; }
__host__ __device__ inline int load_le16s(const uint8_t* p) { return (int16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8)); }

// Channel `c` of the Microsoft ADPCM block at `blk` (`ch` channels): samples 0 .. n-1 to out[s * stride].  -> ISS_ADPCM_* of the
// header.  Bytes only: nothing here needs the block aligned.
__host__ __device__ inline int ms_decode_block(const uint8_t* blk, int ch, int c, int n, int16_t* out, int64_t stride) {
    int p = blk[c];
    int status = ISS_ADPCM_OK;
    if (p >= 7) { p = 0; status = ISS_ADPCM_PREDICTOR; }
    const int c1 = ms_c1(p), c2 = ms_c2(p);
    int delta = load_le16s(blk + ch + 2 * c);
    if (delta < MS_DELTA_MIN) delta = MS_DELTA_MIN;
    int s1 = load_le16s(blk + 3 * ch + 2 * c), s2 = load_le16s(blk + 5 * ch + 2 * c);
    if (n > 0) out[0] = (int16_t)s2;
    if (n > 1) out[stride] = (int16_t)s1;
    const uint8_t* body = blk + 7 * ch;
    int k = c;                                                            // the code's number in the block: (s - 2) * ch + c
    for (int s = 2; s < n; ++s, k += ch) {
        const int byte = body[k >> 1];
        const int nib = (k & 1) ? (byte & 15) : (byte >> 4);
        const int sn = nib >= 8 ? nib - 16 : nib;
        int v = ((s1 * c1 + s2 * c2) >> 8) + sn * delta;                  // (arithmetic shift: floor)
        v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
        s2 = s1; s1 = v;
        delta = (ms_adapt(nib) * delta) >> 8;
        delta = delta < MS_DELTA_MIN ? MS_DELTA_MIN : (delta > MS_DELTA_MAX ? MS_DELTA_MAX : delta);
        out[(int64_t)s * stride] = (int16_t)v;
    }
    return status;
}

enum { CODER_IMA = 0, CODER_MS = 1 };

struct AdJobDev {
    int64_t src_off, block_base, nblocks, frames_total, dst_byte;   // dst_byte: into the signal (to_sig) or the staging buffer
    int32_t ch, block_align, spb, to_sig;
};

struct AdWinDev { int64_t block0, s_begin, s_end; };      // beside AdJobDev k of a windowed call (dst_byte: where sample s_begin goes)

template <int CODER, bool WIN>
__global__ __launch_bounds__(AD_THREADS) void adpcm_decode_kernel(const uint8_t* __restrict__ src, const AdJobDev* __restrict__ jobs,
                                                                  int njobs, int16_t* __restrict__ sig, uint8_t* __restrict__ stage,
                                                                  int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) int16_t ad_smem[];
    const int64_t b = blockIdx.x;
    int lo = 0, hi = njobs - 1;                                          // last job whose block_base <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block_base <= b) lo = mid; else hi = mid - 1;
    }
    const AdJobDev J = jobs[lo];
    const int64_t kb = b - J.block_base;
    if (kb >= J.nblocks) return;                                         // (never: the grid is the sum of the jobs' blocks)
    AdWinDev W{};
    if constexpr (WIN) W = reinterpret_cast<const AdWinDev*>(jobs + njobs)[lo];     // the window table follows the job table
    const int64_t first = (W.block0 + kb) * J.spb;                       // the block's first sample, in the file's numbering
    const int n = (int)min((int64_t)J.spb, J.frames_total - first);      // a `fact` count may cut the last block
    const uint8_t* blk = src + J.src_off + kb * (int64_t)J.block_align;
    int st = ISS_ADPCM_OK;
    for (int c = threadIdx.x; c < J.ch; c += AD_THREADS) {
        if constexpr (CODER == CODER_IMA) st |= ima_decode_block(blk, J.ch, c, n, ad_smem + c, J.ch);
        else st |= ms_decode_block(blk, J.ch, c, n, ad_smem + c, J.ch);
    }
    // (the barrier tells zero from non-zero only: the one code a coder has; a second code of one coder needs the value itself reduced)
    st = __syncthreads_or(st) ? (CODER == CODER_IMA ? ISS_ADPCM_STEP_INDEX : ISS_ADPCM_PREDICTOR) : ISS_ADPCM_OK;
    if (threadIdx.x == 0) status[b] = st;
    int16_t* dst = reinterpret_cast<int16_t*>((J.to_sig ? reinterpret_cast<uint8_t*>(sig) : stage) + J.dst_byte) +
                   (first - W.s_begin) * J.ch;
    const int total = n * J.ch;
    if constexpr (WIN) {
        const int i_lo = (int)max(W.s_begin - first, (int64_t)0) * J.ch, i_hi = (int)min(W.s_end - first, (int64_t)n) * J.ch;
        for (int i = i_lo + threadIdx.x; i < i_hi; i += AD_THREADS) dst[i] = ad_smem[i];
    } else {
        for (int i = threadIdx.x; i < total; i += AD_THREADS) dst[i] = ad_smem[i];
    }
}

int samples_per_block(int coder, int32_t block_align, int32_t ch) {
    return coder == CODER_IMA ? (block_align / ch - 4) * 2 + 1 : (block_align - 7 * ch) * 2 / ch + 2;
}

bool geometry_ok(int coder, int64_t nblocks, int32_t ch, int32_t block_align, int64_t frames_total) {
    if (ch < 1 || ch > 64 || block_align > AD_MAX_ALIGN) return false;
    if (coder == CODER_IMA ? block_align <= 4 * ch || block_align % (4 * ch) != 0
                           : block_align <= 7 * ch || (block_align - 7 * ch) * 2 % ch != 0)
        return false;
    if (nblocks < 1 || nblocks > ((int64_t)1 << 40) / block_align) return false;
    const int64_t spb = samples_per_block(coder, block_align, ch);
    return frames_total > (nblocks - 1) * spb && frames_total <= nblocks * spb;
}

}  // namespace

static int decode_host(int coder, const uint8_t* buf, int64_t len, int64_t nblocks, int32_t channels, int32_t block_align,
                       int64_t frames_total, int16_t* out, int32_t* status_out) {
    if (!buf || !out || !status_out || len < 0 || !geometry_ok(coder, nblocks, channels, block_align, frames_total) ||
        nblocks * (int64_t)block_align > len)
        return ISS_EINVAL;
    const int64_t spb = samples_per_block(coder, block_align, channels);
    for (int64_t k = 0; k < nblocks; ++k) {
        const int n = (int)std::min<int64_t>(spb, frames_total - k * spb);
        int st = ISS_ADPCM_OK;
        for (int c = 0; c < channels; ++c)
            st |= (coder == CODER_IMA ? ima_decode_block : ms_decode_block)(buf + k * block_align, channels, c, n,
                                                                            out + k * spb * channels + c, channels);
        status_out[k] = st;
    }
    return ISS_OK;
}

extern "C" int iss_adpcm_decode_host(const uint8_t* buf, int64_t len, int64_t nblocks, int32_t channels, int32_t block_align,
                                     int64_t frames_total, int16_t* out, int32_t* status_out) {
    return decode_host(CODER_IMA, buf, len, nblocks, channels, block_align, frames_total, out, status_out);
}

extern "C" int iss_msadpcm_decode_host(const uint8_t* buf, int64_t len, int64_t nblocks, int32_t channels, int32_t block_align,
                                       int64_t frames_total, int16_t* out, int32_t* status_out) {
    return decode_host(CODER_MS, buf, len, nblocks, channels, block_align, frames_total, out, status_out);
}

// the five entry points of a coder: windows beside the jobs, splits (with their selection table) beside the jobs, both, or
// neither; or the mix tables `mix` (with or without windows).  Each coder has its own IssCodec: a pass that holds files of both makes two calls, and the second must not take the
// status and staging buffers the first has not been read from yet.
static int adpcm_decode(iss_ctx* c, int coder, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, const iss_window* windows,
                        int32_t njobs, int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_split* splits,
                        const int32_t* channel_sel, int64_t nsel, const IssMixTables* mix = nullptr) {
    const char* who = coder == CODER_IMA ? "iss_adpcm_decode" : "iss_msadpcm_decode";
    if (!c || njobs < 0 || (njobs > 0 && (!jobs || !status_out)) || src_bytes < 0 || (!src && src_bytes > 0) || nblocks_total < 0 ||
        (mix && njobs > 0 && !mix->sets))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument", who);
    IssCodec& dec = coder == CODER_IMA ? c->adpcm : c->msadpcm;
    IssDecodePass pass;
    int rc = pass.begin(c, who, n_signal, njobs);
    if (rc) return rc;
    pass.jsplits = splits; pass.sel = channel_sel; pass.nsel = nsel; pass.jmix = mix;
    // one table: the job rows, then (windowed) their AdWinDev
    std::vector<uint8_t> table((size_t)njobs * (sizeof(AdJobDev) + (windows ? sizeof(AdWinDev) : 0)));
    AdJobDev* dev = reinterpret_cast<AdJobDev*>(table.data());
    AdWinDev* dwin = reinterpret_cast<AdWinDev*>(dev + njobs);
    int64_t blocks = 0, lds = 0;
    for (int32_t j = 0; j < njobs; ++j) {
        const iss_adpcm_job& J = jobs[j];
        // windowed: the geometry of the file up to the window's last block, and exactly the blocks the window touches
        int64_t block0 = 0;
        bool geo;
        if (windows) {
            const iss_window& w = windows[j];
            geo = geometry_ok(coder, 1, J.channels, J.block_align, 1) && w.s_begin >= 0 && w.s_begin < w.s_end && w.s_end <= J.frames_total;
            if (geo) {
                const int64_t spb = samples_per_block(coder, J.block_align, J.channels);
                block0 = w.s_begin / spb;
                geo = J.nblocks == (w.s_end - 1) / spb - block0 + 1 && J.frames_total <= ((int64_t)1 << 40) / J.block_align * spb;
            }
        } else {
            geo = geometry_ok(coder, J.nblocks, J.channels, J.block_align, J.frames_total);
        }
        if (!geo)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: %lld blocks of %d bytes, %d channels, %lld samples%s", who, j,
                            (long long)J.nblocks, J.block_align, J.channels, (long long)J.frames_total,
                            windows ? " (windowed: not the blocks of the window)" : "");
        if (J.block_begin != blocks)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: status rows start at %lld, expected %lld", who, j,
                            (long long)J.block_begin, (long long)blocks);
        const int64_t nbytes = J.nblocks * J.block_align;
        if (J.src_offset < 0 || J.src_offset % 4 != 0 || J.src_offset > src_bytes - nbytes)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: source bytes [%lld, %lld) outside the %lld-byte buffer or "
                            "not aligned to 4", who, j, (long long)J.src_offset, (long long)(J.src_offset + nbytes), (long long)src_bytes);
        AdJobDev& d = dev[(size_t)j];
        d.src_off = J.src_offset; d.block_base = blocks; d.nblocks = J.nblocks; d.frames_total = J.frames_total;
        d.ch = J.channels; d.block_align = J.block_align; d.spb = samples_per_block(coder, J.block_align, J.channels);
        bool to_sig;
        if ((rc = pass.place(j, {J.output, J.filter, J.dst_offset, J.frames_out}, J.frames_total, J.channels, 2, J.channels == 1,
                             "mono", to_sig, d.dst_byte, windows ? windows + j : nullptr)))
            return rc;
        if (windows) dwin[j] = AdWinDev{block0, windows[j].s_begin, windows[j].s_end};
        d.to_sig = to_sig ? 1 : 0;
        lds = std::max<int64_t>(lds, (int64_t)d.spb * d.ch * 2);
        blocks += J.nblocks;
    }
    if (blocks != nblocks_total)
        return iss_fail(c, ISS_EINVAL, "%s: the jobs hold %lld blocks, not %lld", who, (long long)blocks,
                        (long long)nblocks_total);
    if (blocks > 0x7fffffffLL) return iss_fail(c, ISS_EINVAL, "%s: %lld blocks in one call", who, (long long)blocks);
    if ((rc = pass.commit(&dec))) return rc;
    if (blocks == 0) return ISS_OK;
    if ((rc = pass.upload(dec, src, src_bytes, (size_t)std::max<int64_t>(src_bytes, 16), table.data(), table.size(), blocks)))
        return rc;
    auto kernel = coder == CODER_IMA ? (windows ? adpcm_decode_kernel<CODER_IMA, true> : adpcm_decode_kernel<CODER_IMA, false>)
                                     : (windows ? adpcm_decode_kernel<CODER_MS, true> : adpcm_decode_kernel<CODER_MS, false>);
    if (lds + 1024 > 64 * 1024)                        // (the kernel's static LDS, 256 bytes, counts towards the 64 KiB default)
        ISS_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    iss_prof_begin(c, ISS_PROF_FRONTEND, 0.0);
    iss_prof_inst(c, coder == CODER_IMA ? "adpcm_decode_kernel" : "msadpcm_decode_kernel");
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AD_THREADS), (size_t)lds, c->stream,
                       (const uint8_t*)dec.src.p, (const AdJobDev*)dec.rows.p, (int)njobs, (int16_t*)c->sig.p,
                       (uint8_t*)dec.stage.p, (int32_t*)dec.status.p);
    ISS_HIP(c, hipGetLastError());
    iss_prof_end(c);
    return pass.finish(dec, status_out, blocks);
}

extern "C" int iss_adpcm_decode_windows(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                        const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                        int32_t* status_out) {
    return adpcm_decode(c, CODER_IMA, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_adpcm_decode(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                                int64_t nblocks_total, int64_t n_signal, int32_t* status_out) {
    return adpcm_decode(c, CODER_IMA, src, src_bytes, jobs, nullptr, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_adpcm_decode_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                                      int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_split* splits,
                                      const int32_t* channel_sel, int64_t nsel) {
    return adpcm_decode(c, CODER_IMA, src, src_bytes, jobs, nullptr, njobs, nblocks_total, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_adpcm_decode_windows_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                              const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                              int32_t* status_out, const iss_split* splits, const int32_t* channel_sel,
                                              int64_t nsel) {
    return adpcm_decode(c, CODER_IMA, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_adpcm_decode_mix(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, const iss_window* windows,
                                    int32_t njobs, int64_t nblocks_total, int64_t n_signal, int32_t* status_out,
                                    const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                                    int64_t nterms) {
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return adpcm_decode(c, CODER_IMA, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0, &mix);
}

extern "C" int iss_adpcm_get_stage(iss_ctx* c, int32_t job, void* out, int64_t bytes) {
    return c ? iss_codec_get_stage(c, c->adpcm, job, out, bytes) : iss_fail(c, ISS_EINVAL, "iss_adpcm_get_stage: bad argument");
}

extern "C" int iss_adpcm_stats(iss_ctx* c, int64_t* launches, int64_t* blocks) {
    return iss_get_counters(c ? &c->adpcm.count : nullptr, launches, blocks);
}

// the same eight for Microsoft ADPCM: its own codec state, the same rows
extern "C" int iss_msadpcm_decode_windows(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                        const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                        int32_t* status_out) {
    return adpcm_decode(c, CODER_MS, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_msadpcm_decode(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                                int64_t nblocks_total, int64_t n_signal, int32_t* status_out) {
    return adpcm_decode(c, CODER_MS, src, src_bytes, jobs, nullptr, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0);
}

extern "C" int iss_msadpcm_decode_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                                      int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_split* splits,
                                      const int32_t* channel_sel, int64_t nsel) {
    return adpcm_decode(c, CODER_MS, src, src_bytes, jobs, nullptr, njobs, nblocks_total, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_msadpcm_decode_windows_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                              const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                              int32_t* status_out, const iss_split* splits, const int32_t* channel_sel,
                                              int64_t nsel) {
    return adpcm_decode(c, CODER_MS, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, splits, channel_sel, nsel);
}

extern "C" int iss_msadpcm_decode_mix(iss_ctx* c, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, const iss_window* windows,
                                      int32_t njobs, int64_t nblocks_total, int64_t n_signal, int32_t* status_out,
                                      const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                                      int64_t nterms) {
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return adpcm_decode(c, CODER_MS, src, src_bytes, jobs, windows, njobs, nblocks_total, n_signal, status_out, nullptr, nullptr, 0, &mix);
}

extern "C" int iss_msadpcm_get_stage(iss_ctx* c, int32_t job, void* out, int64_t bytes) {
    return c ? iss_codec_get_stage(c, c->msadpcm, job, out, bytes) : iss_fail(c, ISS_EINVAL, "iss_msadpcm_get_stage: bad argument");
}

extern "C" int iss_msadpcm_stats(iss_ctx* c, int64_t* launches, int64_t* blocks) {
    return iss_get_counters(c ? &c->msadpcm.count : nullptr, launches, blocks);
}
