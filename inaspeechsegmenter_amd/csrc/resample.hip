// Downmix + polyphase low-pass resampling + PCM16 quantisation of stored samples at any rate, for gfx950 (float64).
// Stored: WAV's little-endian PCM / float, signed 8-bit, G.711 mu-law / A-law bytes, big-endian 16/32/64-bit (ISS_RS_SWAP).
//
// Replaces the 16 kHz-only assertion of the ffmpeg-free read (io.py:53-55): iss_resample_pcm16 turns the stored samples of
// many files (one H2D copy) into 16 kHz mono PCM16 in the resident signal, in ONE launch of resample_kernel.  The
// arithmetic is inaspeechsegmenter_amd/resample.py's `resample_ref` to the bit (include/iss.h states it).
//
// Grid: ragged over (job, output tile).  Job k owns tiles [tile_base_k, tile_base_k + ceil(frames_out / tile_k)), a prefix
// sum built on the host; a workgroup finds its job by binary search.  A tile is 256 * R consecutive outputs (R = 4, 2 or 1:
// the largest whose input span fits 64 KiB).  Per workgroup:
//   1. the filter table (2*hl+1 float64) goes into LDS when it fits next to the span (160 KiB per workgroup on gfx950);
//      larger tables (e.g. 44 056 Hz: 110 141 taps) are read through L1/L2
//   2. the input span s0 = floor((i0*down - hl)/up) .. floor((i_last*down + hl)/up) is staged in LDS, each frame's channels
//      converted and averaged to float64 on the way; frames outside [0, frames_in) are 0 (a job never reads another's bytes)
//   3. thread t computes outputs i0 + t + 256*r: first input j0 = ceil((i*down - hl)/up), its tap i*down + hl - j0*up, then
//      every `up`-th tap down to 0, summed in ascending j with separate multiply and add, then rint * 32768 and saturation
// All index arithmetic is 64-bit: i*down passes 2^31 after ~5 minutes of 44.1 kHz output.
//
// Windows (include/iss.h, iss_window): WIN = true is a second pair of instantiations for calls that carry a window beside every
// job.  The tiles are laid over the outputs [out_begin, out_end) of the window, the staged bytes hold the file's frames from
// in_begin on, and frames outside [0, frames_total) are 0: steps 2 and 3 are otherwise the code above, on the file's own indices.
//
// Splits (include/iss.h, iss_split): SPLIT = true is a third pair of instantiations for calls that carry a split row beside every
// job.  A job with a selection of channels writes each selected channel apart instead of averaging them: its grid is ragged over
// (channel group, tile), a group being the selected channels whose spans fit RS_SPAN_MAX side by side.  The workgroup stages
// span[k][.] for the channels of its group in one pass over the interleaved frames ((frame, channel) flattened over the threads:
// contiguous reads when the selection is the channels in order) and runs step 3 once per channel, on m[j] = the channel's own
// sample.  A job without a selection (sel_count 0) is the downmix above, in the same launch.
//
// Windows with splits (include/iss.h, "Windows and splits together"): WIN = SPLIT = true is the fourth pair, for calls that carry
// both rows beside every job.  The workgroup takes (channel group, tile) from its block index as a split does, lays the tile
// over [out_begin, out_end) as a window does, and stages its group's channels by the window's rule: the file's own frame
// indices, read at in_begin less, 0 outside [0, frames_total).  Table: job rows, window rows, split rows, channel selections.
//
// Mixes (include/iss.h, iss_mixset): MIX = true is two more pairs, plain and windowed, for calls that carry a mix-set row beside
// every job.  A staged row is a linear combination of channels instead of one channel: the workgroup takes (mix group, tile)
// from its block index as a split takes (channel group, tile), stages span[q][.] = (w_0 x[., c_0] + w_1 x[., c_1] + ...) / d for
// the mixes q of its group ((frame, mix) flattened over the threads, the terms in order, every product, sum and the one
// division rounded on its own) and runs step 3 once per mix.  Geometry is split_geometry's for mix_count rows; a job without
// mixes (mix_count 0) is the downmix above, in the same launch.  Table: job rows, (window rows,) mix-set rows, mix rows, terms.
//
// File sets (include/iss.h, iss_set): SET = true is one more pair, MIX without windows, for calls whose jobs read the members of a
// file set -- one file per channel or per group of channels -- as the interleaved file they stand for.  The planner resolves every
// term of every mix to the member its channel lies in (RsSetTermDev: byte offset, frames, channels of the member) and writes a
// job without mixes as the mix of all its channels (w = 1, d = their count: the downmix above, to the bit), so the workgroup
// only stages differently: stage_set_mixes, (mix, frame) flattened over the threads with the frame running fastest -- a wave
// reads consecutive frames of one member --, a sample past the end of a member 0.0.  Step 3 is the code above.
//
// Schedules (include/iss.h, iss_sched): SCHED = true is one more pair, MIX without windows, for calls that carry a schedule beside
// every job: ONE output row per job, whose staged frame j is mixed by the mix of the run that governs j.  The workgroup finds the
// runs of the first and the last frame of its span once -- block-uniform values, kept in scalar registers -- and where they are one
// run stages exactly as stage_mixes stages one mix; else every frame searches its run between those two (stage_sched).  The
// planner writes a run without a mix as the mix of all the job's channels (w = 1, d = their count), as the set planner does.
// Table: job rows, mix-set rows (mix_begin: the job's RsSchedDev), then 16-byte rows: mix rows, term rows, RsSchedDev, RsRunDev.
//
// Fades (include/iss.h, "Fades"): FADE = true is one more pair, SCHED with a half-width in every run row, for scheduled calls in
// which a run cross-fades in over [begin - half, begin + half).  A workgroup whose span lies in one run and touches neither that
// run's zone nor the head of the next run's stages as SCHED does; any other blends per frame (stage_sched_fade).  A call whose
// half-widths are all 0 launches the SCHED pair.
#include "decode_pass.h"
#include "rs_readers.h"      // to_f64, the Ld* readers, stage_channels: shared with survey.hip
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int64_t RS_LDS_MAX = 160 * 1024;         // bytes of LDS one workgroup may use on gfx950
constexpr int64_t RS_SPAN_MAX = 64 * 1024;         // a tile's input span (float64) is kept under this when R > 1

// frames s0 .. s0+len-1 of one source, downmixed to float64 (channels summed in order, divided by their count)
// (WIN: the source's bytes start at frame W.in_begin of a file of W.frames_total frames, n_in of them staged)
template <typename L, bool WIN>
__device__ __forceinline__ void stage_span(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                           double* __restrict__ span, const RsWinDev& W) {
    using T = typename L::type;
    const T* p = reinterpret_cast<const T*>(src);
    for (int k = threadIdx.x; k < len; k += RS_THREADS) {
        int64_t j = s0 + k;
        double v = 0.0;
        bool in = j >= 0 && j < n_in;
        if constexpr (WIN) {
            in = j >= 0 && j < W.frames_total;
            j -= W.in_begin;
            in = in && j >= 0 && j < n_in;                 // (the planner saw to it that a window reaches no unstaged frame)
        }
        if (in) {
            const T* q = p + j * ch;
            v = L::get(q);
            for (int c = 1; c < ch; ++c) v = __dadd_rn(v, L::get(q + c));
            if (ch > 1) v = __ddiv_rn(v, (double)ch);
        }
        span[k] = v;
    }
}

// frames s0 .. s0+len-1 of `gm` mixes: span[q * stride + .] = mix q of `mixes`, its terms rows of `rows` (include/iss.h states
// the arithmetic).  Thread e takes (frame e / gm, mix e % gm); WIN: stage_span's rule.  A frame outside the file is 0, not 0 / d
template <typename L, bool WIN>
__device__ __forceinline__ void stage_mixes(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                            double* __restrict__ span, int stride, int gm, const RsMixRow* __restrict__ mixes,
                                            const RsTermDev* __restrict__ rows, const RsWinDev& W) {
    using T = typename L::type;
    const T* p = reinterpret_cast<const T*>(src);
    const int total = len * gm;
    for (int e = threadIdx.x; e < total; e += RS_THREADS) {
        const int k = e / gm, q = e - k * gm;
        int64_t j = s0 + k;
        double v = 0.0;
        bool in = j >= 0 && j < n_in;
        if constexpr (WIN) {
            in = j >= 0 && j < W.frames_total;
            j -= W.in_begin;
            in = in && j >= 0 && j < n_in;                 // (the planner saw to it that a window reaches no unstaged frame)
        }
        if (in) {
            const T* f = p + j * ch;
            const RsMixRow M = mixes[q];
            const RsTermDev* t = rows + M.term_begin;
            v = __dmul_rn(t[0].weight, L::get(f + t[0].channel));
            for (int n = 1; n < M.term_count; ++n) v = __dadd_rn(v, __dmul_rn(t[n].weight, L::get(f + t[n].channel)));
            v = __ddiv_rn(v, M.divisor);
        }
        span[(int64_t)q * stride + k] = v;
    }
}

// the last of the run rows runs[lo .. hi] that begins at or before frame j (runs[lo] does)
__device__ __forceinline__ int run_of(const RsRunDev* __restrict__ runs, int lo, int hi, int64_t j) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (runs[mid].begin <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// frames s0 .. s0+len-1 of a scheduled job (include/iss.h, "Schedules"): span[.] = the frame mixed by the mix of its run.  `rows`:
// the call's 16-byte rows, `sched` the job's row among them.  ra, rb: the runs of the first and the last frame of the file in the
// span, the same for every lane.  One run: stage_mixes for that mix.  Else each frame finds its run in [ra, rb]
template <typename L>
__device__ __forceinline__ void stage_sched(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                            double* __restrict__ span, const RsSchedDev* __restrict__ sched,
                                            const RsTermDev* __restrict__ rows) {
    using T = typename L::type;
    const RsSchedDev S = *sched;
    const RsRunDev* runs = reinterpret_cast<const RsRunDev*>(rows) + S.run_begin;
    const RsMixRow* mixes = reinterpret_cast<const RsMixRow*>(rows);
    const int64_t ja = max(s0, (int64_t)0), jb = min(s0 + len, n_in) - 1;
    int ra = 0, rb = 0;
    if (ja <= jb) {
        ra = run_of(runs, 0, S.run_count - 1, ja);
        rb = run_of(runs, ra, S.run_count - 1, jb);
    }
    ra = __builtin_amdgcn_readfirstlane(ra);
    rb = __builtin_amdgcn_readfirstlane(rb);
    if (ra == rb) {
        stage_mixes<L, false>(src, n_in, ch, s0, len, span, 0, 1, mixes + runs[ra].mix, rows, RsWinDev{});
        return;
    }
    const T* p = reinterpret_cast<const T*>(src);
    for (int k = threadIdx.x; k < len; k += RS_THREADS) {
        const int64_t j = s0 + k;
        double v = 0.0;
        if (j >= 0 && j < n_in) {
            const T* f = p + j * ch;
            const RsMixRow M = mixes[runs[run_of(runs, ra, rb, j)].mix];
            const RsTermDev* t = rows + M.term_begin;
            v = __dmul_rn(t[0].weight, L::get(f + t[0].channel));
            for (int n = 1; n < M.term_count; ++n) v = __dadd_rn(v, __dmul_rn(t[n].weight, L::get(f + t[n].channel)));
            v = __ddiv_rn(v, M.divisor);
        }
        span[k] = v;
    }
}

// frame `f` of a source mixed by row M: the terms in order, every product, sum and the one division rounded on its own
template <typename L>
__device__ __forceinline__ double mix_frame(const typename L::type* __restrict__ f, const RsMixRow M, const RsTermDev* __restrict__ rows) {
    const RsTermDev* t = rows + M.term_begin;
    double v = __dmul_rn(t[0].weight, L::get(f + t[0].channel));
    for (int n = 1; n < M.term_count; ++n) v = __dadd_rn(v, __dmul_rn(t[n].weight, L::get(f + t[n].channel)));
    return __ddiv_rn(v, M.divisor);
}

// stage_sched for a job whose runs fade in (include/iss.h, "Fades"): run r's zone is [begin_r - half_r, begin_r + half_r), the
// zones disjoint and in order (the planner saw to both), so a frame of run r lies in r's own zone, in the head of run r + 1's, or
// in neither.  One run over the whole span and no zone touched: stage_mixes for that mix, as stage_sched.  Else each frame finds
// its run and stages p + a * (q - p) inside a zone -- p by the earlier run's mix, q by the later one's, a = (2k + 1) / (4 half)
// for the zone's k-th frame --, the plain mix outside
template <typename L>
__device__ __forceinline__ void stage_sched_fade(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                                 double* __restrict__ span, const RsSchedDev* __restrict__ sched,
                                                 const RsTermDev* __restrict__ rows) {
    using T = typename L::type;
    const RsSchedDev S = *sched;
    const RsRunDev* runs = reinterpret_cast<const RsRunDev*>(rows) + S.run_begin;
    const RsMixRow* mixes = reinterpret_cast<const RsMixRow*>(rows);
    const int64_t ja = max(s0, (int64_t)0), jb = min(s0 + len, n_in) - 1;
    int ra = 0, rb = 0;
    if (ja <= jb) {
        ra = run_of(runs, 0, S.run_count - 1, ja);
        rb = run_of(runs, ra, S.run_count - 1, jb);
    }
    ra = __builtin_amdgcn_readfirstlane(ra);
    rb = __builtin_amdgcn_readfirstlane(rb);
    if (ra == rb) {
        const RsRunDev A = runs[ra];
        bool clear = ja >= A.begin + A.half;               // past the run's own zone ...
        if (ra + 1 < S.run_count) {                        // ... and before the next run's
            const RsRunDev B = runs[ra + 1];
            clear = clear && jb < B.begin - B.half;
        }
        if (clear) {
            stage_mixes<L, false>(src, n_in, ch, s0, len, span, 0, 1, mixes + A.mix, rows, RsWinDev{});
            return;
        }
    }
    const T* p = reinterpret_cast<const T*>(src);
    for (int k = threadIdx.x; k < len; k += RS_THREADS) {
        const int64_t j = s0 + k;
        double v = 0.0;
        if (j >= 0 && j < n_in) {
            const T* f = p + j * ch;
            const int r = run_of(runs, ra, rb, j);
            RsRunDev A = runs[r], B = A;                   // A: the earlier run of a blend, B: the later one, whose zone it is
            bool blend = j < A.begin + A.half;             // (half > 0 only from run 1 on)
            if (blend) A = runs[r - 1];
            else if (r + 1 < S.run_count) {
                B = runs[r + 1];
                blend = j >= B.begin - B.half;
            }
            v = mix_frame<L>(f, mixes[A.mix], rows);
            if (blend) {
                const double q = mix_frame<L>(f, mixes[B.mix], rows);
                const double a = __ddiv_rn((double)(2 * (j - (B.begin - B.half)) + 1), (double)(4 * (int64_t)B.half));
                v = __dadd_rn(v, __dmul_rn(a, __dsub_rn(q, v)));
            }
        }
        span[k] = v;
    }
}

// what a workgroup of a SPLIT launch stages: the downmix (gc == 0), or channels [c0, c0 + gc) of its job's selection;
// of a MIX launch: the downmix, or the gc mixes from `mix` on (rows of the 16-byte table `rows`, which holds their terms too)
// of a SCHED launch: one row by the job's schedule, the RsSchedDev `mix` points at (a 16-byte row of `rows`, as the mixes its
// runs name are)
struct RsGroup { int64_t dst_stride; int stride, c0, gc; const int32_t* sel; const RsMixRow* mix; const RsTermDev* rows; };

template <typename L, bool WIN, bool SPLIT, bool MIX, bool SET, bool SCHED = false, bool FADE = false>
__device__ __forceinline__ void stage(const uint8_t* __restrict__ src, int64_t n_in, int ch, int64_t s0, int len,
                                      double* __restrict__ span, const RsWinDev& W, const RsGroup& G) {
    if constexpr (FADE) {                                  // a scheduled call, a run of which fades in
        stage_sched_fade<L>(src, n_in, ch, s0, len, span, reinterpret_cast<const RsSchedDev*>(G.mix), G.rows);
        return;
    }
    if constexpr (SCHED) {                                 // every job of a scheduled call has a schedule
        stage_sched<L>(src, n_in, ch, s0, len, span, reinterpret_cast<const RsSchedDev*>(G.mix), G.rows);
        return;
    }
    if constexpr (SET) {                                   // every job of a set call has mixes: the planner wrote its downmix as one
        stage_set_mixes<L>(src, n_in, s0, len, span, G.stride, G.gc, G.mix, G.rows);
        return;
    }
    if constexpr (SPLIT) {
        if (G.gc > 0) { stage_channels<L, WIN>(src, n_in, ch, s0, len, span, G.stride, G.c0, G.gc, G.sel, W); return; }
    }
    if constexpr (MIX) {
        if (G.gc > 0) { stage_mixes<L, WIN>(src, n_in, ch, s0, len, span, G.stride, G.gc, G.mix, G.rows, W); return; }
    }
    stage_span<L, WIN>(src, n_in, ch, s0, len, span, W);
}

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {      // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

__device__ __forceinline__ void compute_tile(const RsJobDev& J, const double* __restrict__ tab, const double* __restrict__ span,
                                             int64_t s0, int64_t i0, int64_t i_end, int16_t* __restrict__ dst) {
    const int64_t up = J.up, down = J.down, hl = J.hl;
    for (int64_t i = i0 + threadIdx.x; i < i_end; i += RS_THREADS) {
        const int64_t j0 = -floor_div(hl - i * down, up);                  // ceil((i*down - hl) / up)
        int t = (int)(i * down + hl - j0 * up);                             // in (2*hl - up, 2*hl]
        const double* sp = span + (j0 - s0);
        double acc = 0.0;
        for (; t >= 0; t -= (int)up, ++sp) acc = __dadd_rn(acc, __dmul_rn(tab[t], *sp));
        const double q = fmin(fmax(rint(__dmul_rn(acc, 32768.0)), -32768.0), 32767.0);
        dst[J.dst_off + i] = (int16_t)q;
    }
}

// EXT = false: the five little-endian WAV formats only, the instantiation every call without a newer format launches (its
// switch, and so its code, is what it was before the newer formats existed); EXT = true adds them behind the default case.
// SPLIT = false is the kernel every call without splits launches; SPLIT = true reads the split table and the channel selections
// that follow the rows.  MIX = true (never with SPLIT) reads the mix-set table and the mix and term rows that follow it.
// SET = true (only with MIX, never with WIN; include/iss.h, "File sets") is the pair for calls whose jobs read the members of a
// file set: the tables are a mix call's, the term rows RsSetTermDev in the place of RsTermDev, and stage_set_mixes reads them.
// SCHED = true (only with MIX, never with WIN or SET; include/iss.h, "Schedules") is the pair for calls whose jobs carry a
// schedule: the tables are a mix call's with the schedule and run rows behind the term rows, and stage_sched reads them.
// FADE = true (only with SCHED; include/iss.h, "Fades") is the pair for scheduled calls in which a run has a fade zone: the same
// tables, the run rows' half-widths read as well, and stage_sched_fade stages.
#define RS_STAGE(L) stage<L, WIN, SPLIT, MIX, SET, SCHED, FADE>(s, J.n_in, J.ch, s0, len, span, W, G)
template <bool EXT, bool WIN, bool SPLIT, bool MIX = false, bool SET = false, bool SCHED = false, bool FADE = false>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const uint8_t* __restrict__ src, const RsJobDev* __restrict__ jobs,
                                                              int njobs, int16_t* __restrict__ dst) {
    static_assert(!(SPLIT && MIX), "a call carries split rows or mix-set rows");
    static_assert(!SET || (MIX && !WIN), "a set call is a mix call over whole sources");
    static_assert(!SCHED || (MIX && !WIN && !SET), "a scheduled call is a mix call over whole interleaved sources");
    static_assert(!FADE || SCHED, "fades belong to the runs of a schedule");
    extern __shared__ __attribute__((aligned(16))) double rs_smem[];
    const int64_t b = blockIdx.x;
    int lo = 0, hi = njobs - 1;                                             // last job whose tile_base <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile_base <= b) lo = mid; else hi = mid - 1;
    }
    const RsJobDev J = jobs[lo];
    RsWinDev W{};
    if constexpr (WIN) W = reinterpret_cast<const RsWinDev*>(jobs + njobs)[lo];      // the window table follows the job table
    int64_t t = b - J.tile_base;                                            // SPLIT: (channel group, tile), else the tile
    RsGroup G{};
    if constexpr (SPLIT) {
        const void* after = jobs + njobs;                                            // the split table follows the job table
        if constexpr (WIN) after = reinterpret_cast<const RsWinDev*>(after) + njobs;      // (WIN: ... follows the window table),
        const RsSplitDev* splits = reinterpret_cast<const RsSplitDev*>(after);
        const int32_t* sels = reinterpret_cast<const int32_t*>(splits + njobs);          // the channel selections follow that
        const RsSplitDev S = splits[lo];
        if (S.sel_count > 0) {
            const int g = (int)(t / S.ntiles);
            t -= g * S.ntiles;
            G.dst_stride = S.dst_stride; G.stride = S.stride; G.c0 = g * S.group; G.gc = min(S.group, S.sel_count - G.c0);
            G.sel = S.ident ? nullptr : sels + S.sel_begin + G.c0;
            dst += (int64_t)G.c0 * S.dst_stride;
        }
    }
    if constexpr (MIX) {
        const void* after = jobs + njobs;                                            // the mix-set table follows the job table
        if constexpr (WIN) after = reinterpret_cast<const RsWinDev*>(after) + njobs;      // (WIN: ... follows the window table),
        const RsMixDev* sets = reinterpret_cast<const RsMixDev*>(after);
        const RsMixRow* rows = reinterpret_cast<const RsMixRow*>(sets + njobs);          // the mix rows and the term rows follow that
        const RsMixDev S = sets[lo];
        if constexpr (SCHED) {                                                       // one row: mix_begin names the job's schedule row
            G.dst_stride = S.dst_stride; G.stride = S.stride; G.gc = 1;
            G.rows = reinterpret_cast<const RsTermDev*>(rows);
            G.mix = rows + S.mix_begin;
        } else if (S.mix_count > 0) {
            const int g = (int)(t / S.ntiles);
            t -= g * S.ntiles;
            G.dst_stride = S.dst_stride; G.stride = S.stride; G.c0 = g * S.group; G.gc = min(S.group, S.mix_count - G.c0);
            G.mix = rows + S.mix_begin + G.c0; G.rows = reinterpret_cast<const RsTermDev*>(rows);
            dst += (int64_t)G.c0 * S.dst_stride;
        }
    }
    const int64_t i0 = (WIN ? W.out_begin : 0) + t * J.tile;
    const int64_t i_end = min(i0 + (int64_t)J.tile, WIN ? W.out_end : J.n_out);
    const int64_t s0 = floor_div(i0 * J.down - J.hl, J.up);
    const int64_t s1 = floor_div((i_end - 1) * J.down + J.hl, J.up);
    const int len = (int)(s1 - s0 + 1);
    const int ntaps = 2 * J.hl + 1;
    double* span = rs_smem + (J.lds_tab ? ((ntaps + 1) & ~1) : 0);        // 16-byte aligned carve
    if (J.lds_tab)
        for (int k = threadIdx.x; k < ntaps; k += RS_THREADS) rs_smem[k] = J.taps[k];
    const uint8_t* s = src + J.src_off;
    switch (J.fmt) {
        case ISS_RS_U8:  RS_STAGE(LdPlain<uint8_t>); break;
        case ISS_RS_I16: RS_STAGE(LdPlain<int16_t>); break;
        case ISS_RS_I32: RS_STAGE(LdPlain<int32_t>); break;
        case ISS_RS_F32: RS_STAGE(LdPlain<float>); break;
        default:
            if constexpr (!EXT) {
                RS_STAGE(LdPlain<double>);
            } else {
                switch (J.fmt) {
                    case ISS_RS_F64:  RS_STAGE(LdPlain<double>); break;
                    case ISS_RS_I8:   RS_STAGE(LdPlain<int8_t>); break;
                    case ISS_RS_ULAW: RS_STAGE(LdUlaw); break;
                    case ISS_RS_ALAW: RS_STAGE(LdAlaw); break;
                    case ISS_RS_I16 | ISS_RS_SWAP: RS_STAGE(LdSwapI16); break;
                    case ISS_RS_I32 | ISS_RS_SWAP: RS_STAGE(LdSwapI32); break;
                    case ISS_RS_F32 | ISS_RS_SWAP: RS_STAGE(LdSwapF32); break;
                    default:          RS_STAGE(LdSwapF64); break;      // ISS_RS_F64 | ISS_RS_SWAP
                }
            }
            break;
    }
    __syncthreads();
    if constexpr (SPLIT || MIX) {
        if (G.gc > 0) {                                                     // one pass of step 3 per channel (mix) of the group
            for (int k = 0; k < G.gc; ++k, span += G.stride, dst += G.dst_stride) {
                if (J.lds_tab) compute_tile(J, rs_smem, span, s0, i0, i_end, dst);
                else           compute_tile(J, J.taps, span, s0, i0, i_end, dst);
            }
            return;
        }
    }
    if (J.lds_tab) compute_tile(J, rs_smem, span, s0, i0, i_end, dst);
    else           compute_tile(J, J.taps, span, s0, i0, i_end, dst);
}
#undef RS_STAGE

const int kFmtBytes[11] = {1, 2, 4, 4, 8, 0, 0, 0, 1, 1, 1};      // bytes per stored sample of ISS_RS_* (0: not a format)

// longest input span of a tile of `tile` outputs: floor(((tile-1)*down + 2*hl) / up) + 2 frames
int64_t span_frames(const iss_ctx::RsFilter& f, int64_t tile) {
    return ((tile - 1) * f.down + 2 * (int64_t)f.hl) / f.up + 2;
}

// (tile, group, stride) of a job of `nsel` channels written apart: the largest tile at which the spans of two channels (of
// one, for a single channel) fit RS_SPAN_MAX side by side, then as many channels per group as fit at that tile.  `stride`,
// float64 between the spans of a group: the span rounded up to 16, plus 16 / group -- the 16 lanes of one LDS store group
// hold 16 / group frames of each channel, which then fall on different banks
void split_geometry(const iss_ctx::RsFilter& f, int64_t nsel, int64_t& tile, int64_t& group, int64_t& stride) {
    const int64_t keep = std::min<int64_t>(nsel, 2);
    tile = RS_THREADS * 4;
    while (tile > RS_THREADS && keep * span_frames(f, tile) * 8 > RS_SPAN_MAX) tile /= 2;
    const int64_t span = span_frames(f, tile);
    group = std::max<int64_t>(1, std::min(nsel, RS_SPAN_MAX / (span * 8)));
    stride = group == 1 ? span : (span + 15) / 16 * 16 + std::max<int64_t>(1, 16 / group);
}

}  // namespace

extern "C" int iss_resample_filter(iss_ctx* c, int32_t up, int32_t down, const double* taps, int64_t ntaps, int32_t* id_out) {
    if (!c || !taps || !id_out) return iss_fail(c, ISS_EINVAL, "iss_resample_filter: NULL argument");
    if (up < 1 || down < 1 || up > 384000 || down > 384000)
        return iss_fail(c, ISS_EINVAL, "iss_resample_filter: up %d / down %d out of range", up, down);
    const int64_t want = up == 1 && down == 1 ? 1 : 20 * (int64_t)std::max(up, down) + 1;
    if (ntaps != want)
        return iss_fail(c, ISS_EINVAL, "iss_resample_filter: %lld taps for %d/%d, expected %lld", (long long)ntaps, up, down,
                        (long long)want);
    auto it = c->rs_filter_id.find({up, down});
    if (it != c->rs_filter_id.end()) { *id_out = it->second; return ISS_OK; }
    ISS_HIP(c, hipSetDevice(c->device));
    iss_ctx::RsFilter f;
    f.up = up; f.down = down; f.hl = (int32_t)((ntaps - 1) / 2); f.ntaps = ntaps;
    ISS_HIP(c, hipMalloc((void**)&f.d_taps, (size_t)ntaps * sizeof(double)));
    hipError_t e = hipMemcpy(f.d_taps, taps, (size_t)ntaps * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(f.d_taps);
        return iss_fail(c, ISS_EHIP, "iss_resample_filter: hipMemcpy: %s", hipGetErrorString(e));
    }
    const int32_t id = (int32_t)c->rs_filters.size();
    c->rs_filters.push_back(f);
    c->rs_filter_id[{up, down}] = id;
    *id_out = id;
    return ISS_OK;
}

static int64_t floor_div_host(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }      // b > 0

// mix q of job k (row `m` of the call's mixes) against the call's term rows and the job's channels: ISS_OK, or the refusal
static int check_mix(iss_ctx* c, const char* who, int32_t k, int32_t q, const iss_mix& m, const IssMixTables& mix, int32_t channels) {
    if (m.term_count < 1 || m.term_begin < 0 || m.term_begin > mix.nterms - m.term_count)
        return iss_fail(c, ISS_EINVAL, "%s: job %d: mix %d: term rows [%d, +%d) outside the %lld of the call, or no "
                        "term", who, k, q, m.term_begin, m.term_count, (long long)mix.nterms);
    if (!std::isfinite(m.divisor) || m.divisor == 0.0)
        return iss_fail(c, ISS_EINVAL, "%s: job %d: mix %d: divisor %g", who, k, q, m.divisor);
    for (int32_t n = 0; n < m.term_count; ++n) {
        const iss_mix_term& t = mix.terms[m.term_begin + n];
        if (t.channel < 0 || t.channel >= channels)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: mix %d: term %d: channel %d of %d", who, k, q, n, t.channel, channels);
        if (!std::isfinite(t.weight))
            return iss_fail(c, ISS_EINVAL, "%s: job %d: mix %d: term %d: weight %g", who, k, q, n, t.weight);
    }
    return ISS_OK;
}

int iss_resample_plan(iss_ctx* c, const iss_resample_job* jobs, const iss_window* wins, int32_t njobs, int64_t src_bytes,
                      int64_t nsig, std::vector<std::pair<int64_t, int64_t>> ranges, const char* who, IssRsPlan& plan,
                      const iss_split* splits, const int32_t* sel, int64_t nsel, const IssMixTables* mix, const IssSetTables* set,
                      const IssSchedTables* sched) {
    // validate every job, build the device descriptors and the tile prefix sum
    std::vector<RsJobDev>& dj = plan.dj;
    dj.assign((size_t)njobs, RsJobDev{});
    plan.dw.assign(wins ? (size_t)njobs : 0, RsWinDev{});
    plan.ds.assign(splits ? (size_t)njobs : 0, RsSplitDev{});
    plan.sel.clear();
    plan.dm.assign(mix ? (size_t)njobs : 0, RsMixDev{});
    plan.mixes.clear();
    plan.terms.clear();
    if (mix && (splits || (njobs > 0 && !mix->sets) || mix->nmixes < 0 || mix->nmixes > 0x3fffffffLL || (mix->nmixes > 0 && !mix->mixes) ||
                mix->nterms < 0 || mix->nterms > 0x3fffffffLL || (mix->nterms > 0 && !mix->terms)))
        return iss_fail(c, ISS_EINVAL, "%s: bad mix tables", who);
    plan.sterms.clear();
    plan.set = set != nullptr;
    if (set && (!mix || wins || (njobs > 0 && !set->sets) || set->nmembers < 0 || (set->nmembers > 0 && !set->members)))
        return iss_fail(c, ISS_EINVAL, "%s: bad set tables", who);
    // a set call: the device's rows are written job by job below -- a job's mixes (its downmix: one mix of all its channels), their
    // terms resolved to the job's members --, the mix rows first: as many as the jobs' mix counts add up to, 1 for a downmix
    int64_t set_mixes = 0;
    for (int32_t k = 0; set && k < njobs; ++k) set_mixes += std::max(mix->sets[k].mix_count, 1);
    if (set_mixes > 0x3fffffffLL) return iss_fail(c, ISS_EINVAL, "%s: %lld mixes in one call", who, (long long)set_mixes);
    std::vector<SetChanDev> chans;                         // the channels of the job at hand
    plan.scheds.clear();
    plan.runs.clear();
    plan.sched = sched != nullptr;
    plan.fade = false;
    if (sched && (!mix || wins || splits || set || (njobs > 0 && !sched->scheds) || sched->nruns < 0 || sched->nruns > 0x3fffffffLL ||
                  (sched->nruns > 0 && !sched->runs)))      // (a *_sched_fade entry point saw to its `fades` itself)
        return iss_fail(c, ISS_EINVAL, "%s: bad schedule tables", who);
    std::vector<int32_t> mix_seen;                         // a scheduled call: the last job whose channels mix q was checked against
    std::vector<char> has_none;                            // ... and the jobs with a run that names no mix
    if (sched) { mix_seen.assign((size_t)mix->nmixes, -1); has_none.assign((size_t)njobs, 0); }
    if (mix && !set && !sched) {                                     // the device's rows: the mixes, then the terms they count from there
        plan.mixes.resize((size_t)mix->nmixes);
        plan.terms.resize((size_t)mix->nterms);
        for (int64_t q = 0; q < mix->nmixes; ++q)
            plan.mixes[(size_t)q] = RsMixRow{(int32_t)((int64_t)mix->mixes[q].term_begin + mix->nmixes), mix->mixes[q].term_count,
                                             mix->mixes[q].divisor};      // (a row of no job is never read, nor checked)
        for (int64_t q = 0; q < mix->nterms; ++q) plan.terms[(size_t)q] = RsTermDev{mix->terms[q].channel, 0, mix->terms[q].weight};
    }
    if (splits && (nsel < 0 || nsel > 0x7fffffffLL || (nsel > 0 && !sel)))
        return iss_fail(c, ISS_EINVAL, "%s: a bad channel selection table", who);
    if (splits) plan.sel.assign(sel, sel + nsel);
    int64_t tiles = 0, lds = 0;
    for (int32_t k = 0; k < njobs; ++k) {
        const iss_resample_job& J = jobs[k];
        const int32_t code = J.format & ~ISS_RS_SWAP;
        if (J.format < 0 || code > ISS_RS_ALAW || kFmtBytes[code] == 0 || ((J.format & ISS_RS_SWAP) && kFmtBytes[code] < 2))
            return iss_fail(c, ISS_EINVAL, "%s: job %d: bad format %d", who, k, J.format);
        if (J.channels < 1 || J.channels > 1024)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: %d channels", who, k, J.channels);
        if (J.filter < 0 || J.filter >= (int32_t)c->rs_filters.size())
            return iss_fail(c, ISS_EINVAL, "%s: job %d: unknown filter %d", who, k, J.filter);
        const iss_ctx::RsFilter& f = c->rs_filters[(size_t)J.filter];
        const int64_t esz = kFmtBytes[code];
        if (J.frames_in < 1 || J.frames_in > (int64_t(1) << 40) / (esz * J.channels))
            return iss_fail(c, ISS_EINVAL, "%s: job %d: %lld frames", who, k, (long long)J.frames_in);
        const int64_t nbytes = J.frames_in * J.channels * esz;
        if (set) {                                         // its members' bytes instead: chans = where each of its channels lies
            std::string why;
            chans.clear();
            if (!set_channels(set->sets[k], set->members, set->nmembers, J.frames_in, J.channels, J.src_offset, esz, src_bytes, chans, why))
                return iss_fail(c, ISS_EINVAL, "%s: job %d: %s", who, k, why.c_str());
        } else if (J.src_offset < 0 || J.src_offset % esz != 0 || J.src_offset > src_bytes - nbytes)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: source bytes [%lld, %lld) outside the %lld-byte buffer or "
                            "not aligned to %lld", who, k, (long long)J.src_offset, (long long)(J.src_offset + nbytes),
                            (long long)src_bytes, (long long)esz);
        int64_t nout = (J.frames_in * f.up + f.down - 1) / f.down, out_begin = 0;
        if (wins) {
            // the window's outputs lie inside the file's, and their reach [j_lo, j_hi] inside the staged frames
            const iss_window& w = wins[k];
            if (w.frames_total < 1 || w.frames_total > (int64_t(1) << 40) / (esz * J.channels) || w.s_begin < 0 ||
                w.s_begin >= w.s_end || w.s_end > w.frames_total || w.s_end - w.s_begin != J.frames_in)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: window frames [%lld, %lld) of %lld, %lld staged", who, k,
                                (long long)w.s_begin, (long long)w.s_end, (long long)w.frames_total, (long long)J.frames_in);
            const int64_t file_out = (w.frames_total * f.up + f.down - 1) / f.down;
            if (w.out_begin < 0 || w.out_count < 1 || w.out_begin > file_out - w.out_count)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: window outputs [%lld, +%lld) outside the file's %lld", who, k,
                                (long long)w.out_begin, (long long)w.out_count, (long long)file_out);
            const int64_t j_lo = std::max<int64_t>(0, -floor_div_host(f.hl - w.out_begin * f.down, f.up));    // ceil: the first tap
            const int64_t j_hi = std::min(w.frames_total - 1, floor_div_host((w.out_begin + w.out_count - 1) * f.down + f.hl, f.up));
            if (j_lo < w.s_begin || j_hi >= w.s_end)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: window outputs [%lld, +%lld) reach frames [%lld, %lld], staged are "
                                "[%lld, %lld)", who, k, (long long)w.out_begin, (long long)w.out_count, (long long)j_lo,
                                (long long)j_hi, (long long)w.s_begin, (long long)w.s_end);
            nout = w.out_count;
            out_begin = w.out_begin;
            plan.dw[(size_t)k] = RsWinDev{w.s_begin, w.frames_total, w.out_begin, w.out_begin + w.out_count};
        }
        if (J.frames_out != nout && wins)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: frames_out %lld, the window's out_count is %lld", who, k,
                            (long long)J.frames_out, (long long)nout);
        if (J.frames_out != nout)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: frames_out %lld, ceil(%lld * %d / %d) = %lld", who, k,
                            (long long)J.frames_out, (long long)J.frames_in, f.up, f.down, (long long)nout);
        if (J.dst_offset < 0 || J.dst_offset > nsig - nout)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: output [%lld, %lld) outside the %lld-sample signal", who, k,
                            (long long)J.dst_offset, (long long)(J.dst_offset + nout), (long long)nsig);
        ranges.push_back({J.dst_offset, J.dst_offset + nout});
        int64_t tile = RS_THREADS * 4, span_b, groups = 1;
        if (splits && splits[k].sel_count != 0) {
            // a selection: its rows, its channels, and one destination range per selected channel
            const iss_split& sp = splits[k];
            if (sp.sel_count < 0 || sp.sel_begin < 0 || sp.sel_begin > nsel - sp.sel_count)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: selection rows [%d, +%d) outside the %lld of channel_sel", who, k,
                                sp.sel_begin, sp.sel_count, (long long)nsel);
            bool ident = true;
            for (int32_t q = 0; q < sp.sel_count; ++q) {
                const int32_t ch = sel[sp.sel_begin + q];
                if (ch < 0 || ch >= J.channels)
                    return iss_fail(c, ISS_EINVAL, "%s: job %d: selected channel %d of %d", who, k, ch, J.channels);
                ident = ident && ch == q;
            }
            if (sp.dst_stride < nout || sp.dst_stride > (int64_t(1) << 40))
                return iss_fail(c, ISS_EINVAL, "%s: job %d: dst_stride %lld below the %lld outputs of a channel", who, k,
                                (long long)sp.dst_stride, (long long)nout);
            const int64_t last = J.dst_offset + (sp.sel_count - 1) * sp.dst_stride;
            if (last > nsig - nout)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: output [%lld, %lld) of selected channel %d outside the %lld-sample "
                                "signal", who, k, (long long)last, (long long)(last + nout), sp.sel_count - 1, (long long)nsig);
            for (int32_t q = 1; q < sp.sel_count; ++q)
                ranges.push_back({J.dst_offset + q * sp.dst_stride, J.dst_offset + q * sp.dst_stride + nout});
            int64_t group, stride;
            split_geometry(f, sp.sel_count, tile, group, stride);
            span_b = group * stride * 8;
            groups = (sp.sel_count + group - 1) / group;
            plan.ds[(size_t)k] = RsSplitDev{sp.dst_stride, (nout + tile - 1) / tile, sp.sel_begin, sp.sel_count, (int32_t)group,
                                            (int32_t)stride, ident ? 1 : 0, 0};
        } else if (sched) {
            // a schedule: its run rows, every mix a run names against this job's channels; one output row
            const iss_sched& sc = sched->scheds[k];
            if (sc.run_count < 1 || sc.run_count > (1 << 20) || sc.run_begin < 0 || sc.run_begin > sched->nruns - sc.run_count)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: run rows [%d, +%d) outside the %lld of the call, or not 1 .. 2^20 of "
                                "them", who, k, sc.run_begin, sc.run_count, (long long)sched->nruns);
            for (int32_t q = 0; q < sc.run_count; ++q) {
                const iss_sched_run& r = sched->runs[sc.run_begin + q];
                if (q == 0 && r.begin_frame != 0)
                    return iss_fail(c, ISS_EINVAL, "%s: job %d: run 0 begins at frame %lld, not 0", who, k, (long long)r.begin_frame);
                if (q > 0 && r.begin_frame <= sched->runs[sc.run_begin + q - 1].begin_frame)
                    return iss_fail(c, ISS_EINVAL, "%s: job %d: run %d begins at frame %lld, run %d at %lld: begins ascend strictly",
                                    who, k, q, (long long)r.begin_frame, q - 1, (long long)sched->runs[sc.run_begin + q - 1].begin_frame);
                if (r.mix < -1 || r.mix >= mix->nmixes)
                    return iss_fail(c, ISS_EINVAL, "%s: job %d: run %d: mix %d outside [-1, %lld)", who, k, q, r.mix,
                                    (long long)mix->nmixes);
                if (sched->fades) {                        // zones [begin - half, begin + half): none for run 0, disjoint and in order
                    const int32_t h = sched->fades[sc.run_begin + q];
                    if (h < 0)
                        return iss_fail(c, ISS_EINVAL, "%s: job %d: run %d: fade half-width %d is negative", who, k, q, h);
                    if (q == 0 && h != 0)
                        return iss_fail(c, ISS_EINVAL, "%s: job %d: run 0: fade half-width %d: the first run has nothing to fade from",
                                        who, k, h);
                    const int64_t pb = q > 0 ? sched->runs[sc.run_begin + q - 1].begin_frame : 0;      // (no sum that could pass 2^63)
                    const int32_t ph = q > 0 ? sched->fades[sc.run_begin + q - 1] : 0;
                    if (q > 0 && pb > r.begin_frame - h - ph)
                        return iss_fail(c, ISS_EINVAL, "%s: job %d: run %d: its fade zone, %d frames either side of frame %lld, overlaps "
                                        "that of run %d, %d frames either side of frame %lld", who, k, q, h, (long long)r.begin_frame,
                                        q - 1, ph, (long long)pb);
                    plan.fade = plan.fade || h != 0;
                }
                if (r.mix < 0) has_none[(size_t)k] = 1;
                else if (mix_seen[(size_t)r.mix] != k) {
                    if (int rc = check_mix(c, who, k, r.mix, mix->mixes[r.mix], *mix, J.channels)) return rc;
                    mix_seen[(size_t)r.mix] = k;
                }
            }
            int64_t group, stride;
            split_geometry(f, 1, tile, group, stride);
            span_b = group * stride * 8;
            plan.dm[(size_t)k] = RsMixDev{nout, (nout + tile - 1) / tile, 0, 1, (int32_t)group, (int32_t)stride};      // (mix_begin: below)
        } else if (mix && mix->sets[k].mix_count != 0) {
            // mixes: their rows, every term of every one of them, and one destination range per mix
            const iss_mixset& ms = mix->sets[k];
            if (ms.mix_count < 0 || ms.mix_begin < 0 || ms.mix_begin > mix->nmixes - ms.mix_count)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: mix rows [%d, +%d) outside the %lld of the call", who, k, ms.mix_begin,
                                ms.mix_count, (long long)mix->nmixes);
            for (int32_t q = 0; q < ms.mix_count; ++q)
                if (int rc = check_mix(c, who, k, q, mix->mixes[ms.mix_begin + q], *mix, J.channels)) return rc;
            if (ms.dst_stride < nout || ms.dst_stride > (int64_t(1) << 40))
                return iss_fail(c, ISS_EINVAL, "%s: job %d: dst_stride %lld below the %lld outputs of a mix", who, k,
                                (long long)ms.dst_stride, (long long)nout);
            if ((nsig - nout - J.dst_offset) / ms.dst_stride < ms.mix_count - 1)      // (no product that could pass 2^63)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: output of mix %d, %d strides of %lld behind %lld, outside the "
                                "%lld-sample signal", who, k, ms.mix_count - 1, ms.mix_count - 1, (long long)ms.dst_stride,
                                (long long)J.dst_offset, (long long)nsig);
            for (int32_t q = 1; q < ms.mix_count; ++q)
                ranges.push_back({J.dst_offset + q * ms.dst_stride, J.dst_offset + q * ms.dst_stride + nout});
            int64_t group, stride;
            split_geometry(f, ms.mix_count, tile, group, stride);
            span_b = group * stride * 8;
            groups = (ms.mix_count + group - 1) / group;
            int32_t mix_begin = ms.mix_begin;
            if (set) {                                     // the job's own rows: every term resolved to the member it reads
                mix_begin = (int32_t)plan.mixes.size();
                for (int32_t q = 0; q < ms.mix_count; ++q) {
                    const iss_mix& m = mix->mixes[ms.mix_begin + q];
                    const int64_t at = set_mixes + 2 * (int64_t)plan.sterms.size();
                    if (at + 2 * (int64_t)m.term_count > 0x7fffffffLL)
                        return iss_fail(c, ISS_EINVAL, "%s: job %d: too many term rows in one call", who, k);
                    plan.mixes.push_back(RsMixRow{(int32_t)at, m.term_count, m.divisor});
                    for (int32_t n = 0; n < m.term_count; ++n) {
                        const iss_mix_term& t = mix->terms[m.term_begin + n];
                        const SetChanDev& C = chans[(size_t)t.channel];
                        plan.sterms.push_back(RsSetTermDev{C.off, C.frames, t.weight, C.step, 0});
                    }
                }
            }
            plan.dm[(size_t)k] = RsMixDev{ms.dst_stride, (nout + tile - 1) / tile, mix_begin, ms.mix_count, (int32_t)group,
                                          (int32_t)stride};
        } else if (set) {
            // the plain downmix of a set: the mix of all its channels in order, every weight 1, divisor = their count -- the
            // plain call's sums and its one division (one channel: x * 1 / 1), in one output at dst_offset
            const int64_t at = set_mixes + 2 * (int64_t)plan.sterms.size();
            if (at + 2 * (int64_t)J.channels > 0x7fffffffLL)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: too many term rows in one call", who, k);
            const int32_t mix_begin = (int32_t)plan.mixes.size();
            plan.mixes.push_back(RsMixRow{(int32_t)at, J.channels, (double)J.channels});
            for (const SetChanDev& C : chans) plan.sterms.push_back(RsSetTermDev{C.off, C.frames, 1.0, C.step, 0});
            int64_t group, stride;
            split_geometry(f, 1, tile, group, stride);
            span_b = group * stride * 8;
            plan.dm[(size_t)k] = RsMixDev{nout, (nout + tile - 1) / tile, mix_begin, 1, (int32_t)group, (int32_t)stride};
        } else {
            while (tile > RS_THREADS && span_frames(f, tile) * 8 > RS_SPAN_MAX) tile /= 2;
            span_b = span_frames(f, tile) * 8;
        }
        const int64_t tab_b = ((f.ntaps + 1) & ~int64_t(1)) * 8;
        const bool lds_tab = span_b + tab_b <= RS_LDS_MAX;
        lds = std::max(lds, span_b + (lds_tab ? tab_b : 0));
        RsJobDev& d = dj[(size_t)k];
        d.src_off = J.src_offset; d.n_in = J.frames_in; d.dst_off = J.dst_offset - out_begin; d.n_out = nout; d.tile_base = tiles;
        d.taps = f.d_taps; d.ch = J.channels; d.fmt = J.format; d.up = f.up; d.down = f.down; d.hl = f.hl;
        d.tile = (int32_t)tile; d.lds_tab = lds_tab ? 1 : 0; d.pad = 0;
        tiles += groups * ((nout + tile - 1) / tile);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].first < ranges[k - 1].second)
            return iss_fail(c, ISS_EINVAL, "%s: output ranges [%lld, %lld) and [%lld, %lld) overlap", who,
                            (long long)ranges[k - 1].first, (long long)ranges[k - 1].second, (long long)ranges[k].first,
                            (long long)ranges[k].second);
    if (tiles > 0x7fffffffLL) return iss_fail(c, ISS_EINVAL, "%s: %lld tiles in one call", who, (long long)tiles);
    if (sched) {
        // the 16-byte rows: the call's mixes and one all-channel mix per job with a run that names none (w = 1, d = its channels:
        // the plain downmix, to the bit), their terms, one RsSchedDev per job, every job's runs -- indices from the first mix row
        int64_t nmix = mix->nmixes, nterm = mix->nterms, nrun = 0;
        for (int32_t k = 0; k < njobs; ++k) {
            if (has_none[(size_t)k]) { nmix += 1; nterm += jobs[k].channels; }
            nrun += sched->scheds[k].run_count;
        }
        if (nmix + nterm + njobs + nrun > 0x7fffffffLL)
            return iss_fail(c, ISS_EINVAL, "%s: %lld rows of mixes, terms and runs in one call", who, (long long)(nmix + nterm + njobs + nrun));
        plan.mixes.reserve((size_t)nmix); plan.terms.reserve((size_t)nterm); plan.runs.reserve((size_t)nrun);
        for (int64_t q = 0; q < mix->nmixes; ++q)
            plan.mixes.push_back(RsMixRow{(int32_t)((int64_t)mix->mixes[q].term_begin + nmix), mix->mixes[q].term_count,
                                          mix->mixes[q].divisor});        // (a row no run names is never read, nor checked)
        for (int64_t q = 0; q < mix->nterms; ++q) plan.terms.push_back(RsTermDev{mix->terms[q].channel, 0, mix->terms[q].weight});
        for (int32_t k = 0; k < njobs; ++k) {
            const iss_sched& sc = sched->scheds[k];
            int32_t none = -1;
            if (has_none[(size_t)k]) {
                none = (int32_t)plan.mixes.size();
                plan.mixes.push_back(RsMixRow{(int32_t)(nmix + (int64_t)plan.terms.size()), jobs[k].channels, (double)jobs[k].channels});
                for (int32_t ch = 0; ch < jobs[k].channels; ++ch) plan.terms.push_back(RsTermDev{ch, 0, 1.0});
            }
            plan.scheds.push_back(RsSchedDev{(int32_t)(nmix + nterm + njobs + (int64_t)plan.runs.size()), sc.run_count, 0});
            for (int32_t q = 0; q < sc.run_count; ++q) {
                const iss_sched_run& r = sched->runs[sc.run_begin + q];
                // (a zone wholly past the file blends no frame: written as none, so that begin + half stays far from 2^63)
                const int32_t h = sched->fades ? sched->fades[sc.run_begin + q] : 0;
                plan.runs.push_back(RsRunDev{r.begin_frame, r.mix < 0 ? none : r.mix, r.begin_frame - h >= jobs[k].frames_in ? 0 : h});
            }
            plan.dm[(size_t)k].mix_begin = (int32_t)(nmix + nterm + k);
        }
    }
    plan.tiles = tiles;
    plan.lds = lds;
    return ISS_OK;
}

int iss_resample_launch(iss_ctx* c, const uint8_t* dev_src, const IssRsPlan& plan) {
    const std::vector<RsJobDev>& dj = plan.dj;
    if (dj.empty()) return ISS_OK;
    const bool win = !plan.dw.empty(), split = !plan.ds.empty(), mix = !plan.dm.empty();
    int rc;
    if (mix) {                                         // one table: the jobs, (their windows,) their mix sets, the mix rows, the terms
        const size_t nj = dj.size() * sizeof(RsJobDev), nw = win ? dj.size() * sizeof(RsWinDev) : 0, nm = dj.size() * sizeof(RsMixDev);
        const size_t nr = plan.mixes.size() * sizeof(RsMixRow);         // (a set call: its own term rows in the place of `terms`)
        const size_t nt = plan.set ? plan.sterms.size() * sizeof(RsSetTermDev) : plan.terms.size() * sizeof(RsTermDev);
        const size_t nc = plan.scheds.size() * sizeof(RsSchedDev), nu = plan.runs.size() * sizeof(RsRunDev);      // (a scheduled call)
        std::vector<uint8_t> rows(nj + nw + nm + std::max<size_t>(nr + nt, 16) + nc + nu);
        memcpy(rows.data(), dj.data(), nj);
        if (win) memcpy(rows.data() + nj, plan.dw.data(), nw);
        memcpy(rows.data() + nj + nw, plan.dm.data(), nm);
        if (nr) memcpy(rows.data() + nj + nw + nm, plan.mixes.data(), nr);
        if (nt) memcpy(rows.data() + nj + nw + nm + nr, plan.set ? (const void*)plan.sterms.data() : (const void*)plan.terms.data(), nt);
        if (nc) memcpy(rows.data() + nj + nw + nm + nr + nt, plan.scheds.data(), nc);
        if (nu) memcpy(rows.data() + nj + nw + nm + nr + nt + nc, plan.runs.data(), nu);
        rc = iss_upload_rows(c, c->rs_jobs, rows.data(), rows.size());
    } else if (split) {                                       // one table: the jobs, (their windows,) their splits, the channel selections
        const size_t nj = dj.size() * sizeof(RsJobDev), nw = win ? dj.size() * sizeof(RsWinDev) : 0, ns = dj.size() * sizeof(RsSplitDev);
        std::vector<uint8_t> rows(nj + nw + ns + std::max<size_t>(plan.sel.size(), 1) * sizeof(int32_t));
        memcpy(rows.data(), dj.data(), nj);
        if (win) memcpy(rows.data() + nj, plan.dw.data(), nw);
        memcpy(rows.data() + nj + nw, plan.ds.data(), ns);
        if (!plan.sel.empty()) memcpy(rows.data() + nj + nw + ns, plan.sel.data(), plan.sel.size() * sizeof(int32_t));
        rc = iss_upload_rows(c, c->rs_jobs, rows.data(), rows.size());
    } else if (win) {                                         // one table: the jobs, then their windows
        std::vector<uint8_t> rows(dj.size() * (sizeof(RsJobDev) + sizeof(RsWinDev)));
        memcpy(rows.data(), dj.data(), dj.size() * sizeof(RsJobDev));
        memcpy(rows.data() + dj.size() * sizeof(RsJobDev), plan.dw.data(), dj.size() * sizeof(RsWinDev));
        rc = iss_upload_rows(c, c->rs_jobs, rows.data(), rows.size());
    } else {
        rc = iss_upload_rows(c, c->rs_jobs, dj.data(), dj.size() * sizeof(RsJobDev));
    }
    if (rc) return rc;
    bool ext = false;                                  // a format newer than the WAV five: the instantiation that reads them all
    for (const RsJobDev& d : dj) ext = ext || d.fmt > ISS_RS_F64;
    auto kernel = plan.fade ? (ext ? resample_kernel<true, false, false, true, false, true, true> : resample_kernel<false, false, false, true, false, true, true>)
                  : plan.sched ? (ext ? resample_kernel<true, false, false, true, false, true> : resample_kernel<false, false, false, true, false, true>)
                  : plan.set ? (ext ? resample_kernel<true, false, false, true, true> : resample_kernel<false, false, false, true, true>)
                  : mix ? (win ? (ext ? resample_kernel<true, true, false, true> : resample_kernel<false, true, false, true>)
                             : (ext ? resample_kernel<true, false, false, true> : resample_kernel<false, false, false, true>))
                  : split && win ? (ext ? resample_kernel<true, true, true> : resample_kernel<false, true, true>)
                  : split ? (ext ? resample_kernel<true, false, true> : resample_kernel<false, false, true>)
                  : win ? (ext ? resample_kernel<true, true, false> : resample_kernel<false, true, false>)
                        : (ext ? resample_kernel<true, false, false> : resample_kernel<false, false, false>);
    if (plan.lds > 64 * 1024)
        ISS_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    double flops = 0;
    for (size_t k = 0; k < dj.size(); ++k)
        flops += 2.0 * (double)dj[k].n_out * (2.0 * dj[k].hl + 1) / dj[k].up * (split ? std::max(plan.ds[k].sel_count, 1) : mix ? std::max(plan.dm[k].mix_count, 1) : 1);
    iss_prof_begin(c, ISS_PROF_FRONTEND, flops);
    iss_prof_inst(c, "resample_kernel");
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.tiles), dim3(RS_THREADS), (size_t)plan.lds, c->stream,
                       dev_src, (const RsJobDev*)c->rs_jobs.p, (int)dj.size(), (int16_t*)c->sig.p);
    ISS_HIP(c, hipGetLastError());
    iss_prof_end(c);
    c->rs_count.launches += 1;
    c->rs_count.units += (int64_t)dj.size();
    return ISS_OK;
}

// the one body of the five entry points: `windows`, `splits`, both or neither beside the jobs (a null pointer is "neither"), or
// the tables `mix` of iss_resample_pcm16_mix (with or without windows)
static int resample_pcm16(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                          int64_t n_signal, const iss_window* windows, const iss_split* splits, const int32_t* channel_sel,
                          int64_t nsel, const IssMixTables* mix = nullptr, const IssSchedTables* sched = nullptr) {
    const char* who = sched && sched->fades ? "iss_resample_pcm16_sched_fade" : sched ? "iss_resample_pcm16_sched" : mix ? "iss_resample_pcm16_mix" : splits && windows ? "iss_resample_pcm16_windows_split" : splits ? "iss_resample_pcm16_split"
                      : windows ? "iss_resample_pcm16_windows" : "iss_resample_pcm16";
    if (!c || njobs < 0 || (njobs > 0 && !jobs) || src_bytes < 0 || (!src && src_bytes > 0) || (mix && !sched && njobs > 0 && !mix->sets) ||
        (sched && njobs > 0 && !sched->scheds))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument", who);
    if (sched && windows) return iss_fail(c, ISS_EINVAL, "%s: windows passed with a schedule, which governs whole sources", who);
    IssDecodePass pass;
    int rc = pass.begin(c, who, n_signal, 0);
    if (sched) { pass.jmix = mix; pass.jsched = sched; pass.rmixsets.assign((size_t)njobs, iss_mixset{0, 0, 0}); }      // (no job has a mix set)
    else if (mix) { pass.jmix = mix; pass.rmixsets.assign(mix->sets, mix->sets + njobs); }
    pass.rjobs.assign(jobs, jobs + njobs); pass.stage = src_bytes;      // no placement: the caller's rows over the caller's bytes
    if (windows) { pass.rwins.assign(windows, windows + njobs); pass.windowed = true; }
    if (splits) { pass.rsplits.assign(splits, splits + njobs); pass.split = true; pass.sel = channel_sel; pass.nsel = nsel; }
    if (rc || (rc = pass.commit(nullptr))) return rc;
    if (njobs == 0) return ISS_OK;
    if ((rc = iss_upload_payload(c, c->rs_src, "resample", src, src_bytes, (size_t)std::max<int64_t>(src_bytes, 16)))) return rc;
    return iss_resample_launch(c, (const uint8_t*)c->rs_src.p, pass.plan);
}

extern "C" int iss_resample_pcm16_windows(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                          const iss_window* windows, int32_t njobs, int64_t n_signal) {
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, windows, nullptr, nullptr, 0);
}

extern "C" int iss_resample_pcm16_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                                        int64_t n_signal, const iss_split* splits, const int32_t* channel_sel, int64_t nsel) {
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, nullptr, splits, channel_sel, nsel);
}

extern "C" int iss_resample_pcm16_windows_split(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                                const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_split* splits,
                                                const int32_t* channel_sel, int64_t nsel) {
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, windows, splits, channel_sel, nsel);
}

extern "C" int iss_resample_pcm16_mix(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                      const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_mixset* mixsets,
                                      const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms) {
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, windows, nullptr, nullptr, 0, &mix);
}

extern "C" int iss_resample_pcm16_sched(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                        const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                        const iss_sched_run* runs, int64_t nruns, const iss_mix* mixes, int64_t nmixes,
                                        const iss_mix_term* terms, int64_t nterms) {
    const IssMixTables mix{nullptr, mixes, nmixes, terms, nterms};
    const IssSchedTables sched{scheds, runs, nruns};
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, windows, nullptr, nullptr, 0, &mix, &sched);
}

extern "C" int iss_resample_pcm16_sched_fade(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                             const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                             const iss_sched_run* runs, int64_t nruns, const int32_t* fades, const iss_mix* mixes,
                                             int64_t nmixes, const iss_mix_term* terms, int64_t nterms) {
    if (!fades && nruns > 0) return iss_fail(c, ISS_EINVAL, "iss_resample_pcm16_sched_fade: bad argument");
    const IssMixTables mix{nullptr, mixes, nmixes, terms, nterms};
    const IssSchedTables sched{scheds, runs, nruns, fades};
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, windows, nullptr, nullptr, 0, &mix, &sched);
}

// what `origin` holds for iss_resample_staged_mix: its id (0: nothing), and for a codec the codec
static int64_t staged_held(iss_ctx* c, int32_t origin, IssCodec*& dec) {
    dec = origin == ISS_STAGED_FLAC ? &c->flac : origin == ISS_STAGED_ADPCM ? &c->adpcm : origin == ISS_STAGED_MSADPCM ? &c->msadpcm
                                                                                                                           : nullptr;
    return dec ? dec->held : c->sv_held.id;
}

static const char* const kStagedOrigin[4] = {"survey", "flac", "adpcm", "msadpcm"};

extern "C" int iss_staged_payload(iss_ctx* c, int32_t origin, int64_t* payload_out) {
    if (!c || !payload_out || origin < ISS_STAGED_SURVEY || origin > ISS_STAGED_MSADPCM)
        return iss_fail(c, ISS_EINVAL, "iss_staged_payload: bad argument");
    IssCodec* dec;
    const int64_t id = staged_held(c, origin, dec);
    if (id == 0) return iss_fail(c, ISS_ESTATE, "iss_staged_payload: origin %s holds no payload", kStagedOrigin[origin]);
    *payload_out = id;
    return ISS_OK;
}

// The rows of a *_mix call over bytes a survey call (origin survey) or a decode call (a codec) left on the device: every row is
// matched against what was uploaded / staged and rewritten to the byte offset it lies at, then planned and launched as
// resample_pcm16 does -- without its upload.  Everything up to commit() is host work on vectors of this call
// `sched` (iss_resample_staged_sched; `mixsets` is then NULL): a schedule beside every job in the place of a mix set, no windows
static int resample_staged(iss_ctx* c, const char* who, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                           const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_mixset* mixsets,
                           const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms,
                           const IssSchedTables* sched) {
    if (!c || origin < ISS_STAGED_SURVEY || origin > ISS_STAGED_MSADPCM || njobs < 0 ||
        (njobs > 0 && (!jobs || (sched ? !sched->scheds : !mixsets))))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument", who);
    if (sched && windows) return iss_fail(c, ISS_EINVAL, "%s: windows passed with a schedule, which governs whole sources", who);
    IssCodec* dec;
    const int64_t id = staged_held(c, origin, dec);
    if (id == 0)
        return iss_fail(c, ISS_ESTATE, "%s: origin %s holds no payload (no %s call went before)", who, kStagedOrigin[origin],
                        dec ? "decode" : "iss_survey");
    if (id != payload)
        return iss_fail(c, ISS_ESTATE, "%s: origin %s: payload %lld has been replaced by a later call (it holds payload %lld)", who,
                        kStagedOrigin[origin], (long long)payload, (long long)id);
    std::vector<iss_resample_job> rows(jobs, jobs + njobs);
    int64_t held_bytes = dec ? 0 : c->sv_held.bytes;
    if (dec)
        for (size_t q = 0; q < dec->stage_off.size(); ++q)
            if (dec->stage_off[q] >= 0) held_bytes = std::max(held_bytes, dec->stage_off[q] + dec->stage_bytes[q]);
    for (int32_t k = 0; k < njobs; ++k) {
        iss_resample_job& J = rows[(size_t)k];
        if (J.channels < 1 || J.channels > 1024 || J.frames_in < 1 || J.frames_in > (int64_t(1) << 40))
            return iss_fail(c, ISS_EINVAL, "%s: job %d: %lld frames of %d channels", who, k, (long long)J.frames_in, J.channels);
        if (dec) {
            const int64_t q = J.src_offset;
            if (q < 0 || q >= (int64_t)dec->stage_off.size() || dec->stage_off[(size_t)q] < 0)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: job %lld of the last iss_%s_decode did not go to the staging buffer", who,
                                k, (long long)q, dec->name);
            const int32_t esz = dec->stage_esz[(size_t)q];
            if (J.format != (esz == 4 ? ISS_RS_I32 : ISS_RS_I16))
                return iss_fail(c, ISS_EINVAL, "%s: job %d: format %d: staged job %lld holds %s samples", who, k, J.format,
                                (long long)q, esz == 4 ? "ISS_RS_I32" : "ISS_RS_I16");
            const int64_t nbytes = J.frames_in * J.channels * esz;
            if (dec->stage_bytes[(size_t)q] != nbytes)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: staged job %lld holds %lld bytes, the row states %lld frames of %d "
                                "channels: %lld", who, k, (long long)q, (long long)dec->stage_bytes[(size_t)q], (long long)J.frames_in,
                                J.channels, (long long)nbytes);
            J.src_offset = dec->stage_off[(size_t)q];
        } else {
            bool found = false;
            for (const iss_survey_job& S : c->sv_held.jobs) {
                if (!c->sv_held.sets.empty()) break;       // (jobs of iss_survey_set: their rows describe no interleaved bytes)
                found = found || (S.src_offset == J.src_offset && S.frames_in == J.frames_in && S.channels == J.channels &&
                                  S.format == J.format);
            }
            if (!found)
                return iss_fail(c, ISS_EINVAL, "%s: job %d: no job of the last iss_survey held %lld frames of %d channels in format "
                                "%d at byte %lld", who, k, (long long)J.frames_in, J.channels, J.format, (long long)J.src_offset);
        }
    }
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    IssDecodePass pass;
    int rc = pass.begin(c, who, n_signal, 0);
    pass.jmix = &mix;
    if (sched) { pass.jsched = sched; pass.rmixsets.assign((size_t)njobs, iss_mixset{0, 0, 0}); }
    else if (njobs > 0) pass.rmixsets.assign(mixsets, mixsets + njobs);
    pass.rjobs = rows; pass.stage = held_bytes;
    if (windows) { pass.rwins.assign(windows, windows + njobs); pass.windowed = true; }
    if (rc || (rc = pass.commit(nullptr))) return rc;
    if (njobs == 0) return ISS_OK;
    return iss_resample_launch(c, (const uint8_t*)(dec ? dec->stage.p : c->sv_src.p), pass.plan);
}

extern "C" int iss_resample_staged_mix(iss_ctx* c, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                                       const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_mixset* mixsets,
                                       const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms) {
    return resample_staged(c, "iss_resample_staged_mix", origin, payload, jobs, windows, njobs, n_signal, mixsets, mixes, nmixes, terms,
                           nterms, nullptr);
}

extern "C" int iss_resample_staged_sched(iss_ctx* c, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                                         const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                         const iss_sched_run* runs, int64_t nruns, const iss_mix* mixes, int64_t nmixes,
                                         const iss_mix_term* terms, int64_t nterms) {
    const IssSchedTables sched{scheds, runs, nruns};
    return resample_staged(c, "iss_resample_staged_sched", origin, payload, jobs, windows, njobs, n_signal, nullptr, mixes, nmixes,
                           terms, nterms, &sched);
}

extern "C" int iss_resample_staged_sched_fade(iss_ctx* c, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                                              const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                              const iss_sched_run* runs, int64_t nruns, const int32_t* fades, const iss_mix* mixes,
                                              int64_t nmixes, const iss_mix_term* terms, int64_t nterms) {
    if (!fades && nruns > 0) return iss_fail(c, ISS_EINVAL, "iss_resample_staged_sched_fade: bad argument");
    const IssSchedTables sched{scheds, runs, nruns, fades};
    return resample_staged(c, "iss_resample_staged_sched_fade", origin, payload, jobs, windows, njobs, n_signal, nullptr, mixes, nmixes,
                           terms, nterms, &sched);
}

// The body of the two set entry points (include/iss.h, "File sets"): the jobs planned over their members' bytes in `src_bytes` of
// source, then the upload (src != NULL) and the launch over dev_src (NULL: the resampler's own source buffer, uploaded here)
static int resample_set(iss_ctx* c, const char* who, const uint8_t* dev_src, const void* src, int64_t src_bytes,
                        const iss_resample_job* jobs, int32_t njobs, int64_t n_signal, const IssSetTables& set, const IssMixTables& mix) {
    IssDecodePass pass;
    int rc = pass.begin(c, who, n_signal, 0);
    pass.jmix = &mix; pass.jset = &set;
    if (njobs > 0) pass.rmixsets.assign(mix.sets, mix.sets + njobs);
    pass.rjobs.assign(jobs, jobs + njobs); pass.stage = src_bytes;
    if (rc || (rc = pass.commit(nullptr))) return rc;
    if (njobs == 0) return ISS_OK;
    if (!dev_src) {
        if ((rc = iss_upload_payload(c, c->rs_src, "resample", src, src_bytes, (size_t)std::max<int64_t>(src_bytes, 16)))) return rc;
        dev_src = (const uint8_t*)c->rs_src.p;
    }
    return iss_resample_launch(c, dev_src, pass.plan);
}

extern "C" int iss_resample_pcm16_set(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                                      int64_t n_signal, const iss_set* sets, const iss_set_member* members, int64_t nmembers,
                                      const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                                      int64_t nterms) {
    const char* who = "iss_resample_pcm16_set";
    if (!c || njobs < 0 || (njobs > 0 && (!jobs || !sets || !mixsets)) || src_bytes < 0 || (!src && src_bytes > 0))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument", who);
    const IssSetTables set{sets, members, nmembers};
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return resample_set(c, who, nullptr, src, src_bytes, jobs, njobs, n_signal, set, mix);
}

// iss_resample_staged_mix for sets: every job is matched against a job of the iss_survey_set whose payload the survey's source
// buffer holds -- frames, channels, format, and member row for member row --, then planned and launched over those bytes
extern "C" int iss_resample_staged_set(iss_ctx* c, int32_t origin, int64_t payload, const iss_resample_job* jobs, int32_t njobs,
                                       int64_t n_signal, const iss_set* sets, const iss_set_member* members, int64_t nmembers,
                                       const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                                       int64_t nterms) {
    const char* who = "iss_resample_staged_set";
    if (!c || origin != ISS_STAGED_SURVEY || njobs < 0 || (njobs > 0 && (!jobs || !sets || !mixsets)) || nmembers < 0 ||
        (nmembers > 0 && !members))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument (the origin of a set is ISS_STAGED_SURVEY)", who);
    const iss_ctx::Held& H = c->sv_held;
    if (H.id == 0)
        return iss_fail(c, ISS_ESTATE, "%s: origin survey holds no payload (no iss_survey_set went before)", who);
    if (H.id != payload)
        return iss_fail(c, ISS_ESTATE, "%s: origin survey: payload %lld has been replaced by a later call (it holds payload %lld)", who,
                        (long long)payload, (long long)H.id);
    for (int32_t k = 0; k < njobs; ++k) {
        const iss_resample_job& J = jobs[k];
        const iss_set& S = sets[k];
        bool found = false;
        if (S.member_count >= 1 && S.member_begin >= 0 && S.member_begin <= nmembers - S.member_count)
            for (size_t q = 0; q < H.sets.size() && !found; ++q) {
                const iss_survey_job& V = H.jobs[q];
                const iss_set& T = H.sets[q];
                if (V.frames_in != J.frames_in || V.channels != J.channels || V.format != J.format || T.member_count != S.member_count)
                    continue;
                found = true;
                for (int32_t m = 0; m < S.member_count && found; ++m) {
                    const iss_set_member& A = members[S.member_begin + m];
                    const iss_set_member& B = H.members[(size_t)(T.member_begin + m)];
                    found = A.src_offset == B.src_offset && A.frames == B.frames && A.channels == B.channels;
                }
            }
        if (!found)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: no job of the last iss_survey_set held these members: %lld frames of %d "
                            "channels in format %d, %d member rows from %d on", who, k, (long long)J.frames_in, J.channels, J.format,
                            S.member_count, S.member_begin);
    }
    const IssSetTables set{sets, members, nmembers};
    const IssMixTables mix{mixsets, mixes, nmixes, terms, nterms};
    return resample_set(c, who, (const uint8_t*)c->sv_src.p, nullptr, H.bytes, jobs, njobs, n_signal, set, mix);
}

// (tile, channels per group) the planner gives a job of `nsel` selected channels (or mixes) through filter `filter`
extern "C" int iss_resample_split_geometry(iss_ctx* c, int32_t filter, int32_t nsel, int32_t* tile_out, int32_t* group_out) {
    if (!c || !tile_out || !group_out || nsel < 1 || filter < 0 || filter >= (int32_t)c->rs_filters.size())
        return iss_fail(c, ISS_EINVAL, "iss_resample_split_geometry: bad argument");
    int64_t tile, group, stride;
    split_geometry(c->rs_filters[(size_t)filter], nsel, tile, group, stride);
    *tile_out = (int32_t)tile; *group_out = (int32_t)group;
    return ISS_OK;
}

extern "C" int iss_resample_pcm16(iss_ctx* c, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                                  int64_t n_signal) {
    return resample_pcm16(c, src, src_bytes, jobs, njobs, n_signal, nullptr, nullptr, nullptr, 0);
}

extern "C" int iss_resample_stats(iss_ctx* c, int64_t* launches, int64_t* jobs) {
    return iss_get_counters(c ? &c->rs_count : nullptr, launches, jobs);
}
