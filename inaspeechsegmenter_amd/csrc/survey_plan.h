// The host side of a channel survey (include/iss.h, "Channel survey"): the chunk geometry and the device's job table, built and
// validated from the caller's rows.  Plain C++ with no HIP in it: survey.hip includes it, and tools/survey_plan_check.cpp builds
// it for the host alone, under the sanitizers.  Not part of the ABI.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/iss.h"

constexpr int SV_THREADS = 256;                        // lanes of a chunk: four waves
constexpr int SV_CHUNK = ISS_SURVEY_CHUNK;             // frames of a chunk: four terms per lane
constexpr int SV_GROUP = ISS_SURVEY_PAIR_CHANNELS;     // channels staged in LDS side by side; pairs are computed up to here
constexpr int SV_PART = 6 * SV_GROUP + SV_GROUP * (SV_GROUP - 1) / 2;      // figures of one group: 8-byte words per wave in LDS
static_assert(SV_CHUNK % SV_THREADS == 0, "every lane holds the same number of terms of a full chunk");

// one job of the device's table: n frames of ch channels from byte src_off of the source, its chunks numbered from chunk_base,
// their partial rows from word ws_off of the workspace, its result row from word res_off of the results
struct SvJobDev {
    int64_t src_off, n, chunk_base, ws_off, res_off;
    double full;
    int32_t ch, fmt;
};
static_assert(sizeof(SvJobDev) == 56, "rows are copied to the device as they stand");

// one channel of a job over a file set (include/iss.h, "File sets"): sample (j, this channel) lies at byte off + j * step * sample
// bytes of the source while j < frames, and is 0.0 from there on.  The rows follow the job rows on the device, a set job's
// src_off being the index of its first one
struct SetChanDev { int64_t off, frames; int32_t step, pad; };
static_assert(sizeof(SetChanDev) == 24 && sizeof(SvJobDev) % 8 == 0, "8-byte aligned behind the job rows");

// beside SvJobDev k of a blocked call (include/iss.h, "Survey blocks"): the job's blocks hold K chunks each (the last fewer), a
// block's row is cut into `wgroups` groups of SV_THREADS words, the job's (block, word group) units are numbered from unit_base
// and its block rows start at word out_off of the block results.  The rows follow the job rows on the device
struct SvBlkDev { int64_t unit_base, out_off; int32_t K, wgroups; };
static_assert(sizeof(SvBlkDev) == 24, "8-byte aligned behind the job rows");

struct SvPlan {
    std::vector<SvJobDev> dj;
    std::vector<SvBlkDev> blk;                         // a blocked call: one per job
    int64_t blk_units = 0, blk_words = 0;              // ... the grid of survey_reduce_blocks_kernel and the words it writes
    std::vector<SetChanDev> chans;                     // a set call: every job's channels, in job order
    int64_t chunks = 0, ws_words = 0, res_words = 0;
    int64_t lds = 0;                                   // bytes of dynamic LDS survey_kernel needs for these jobs
    int32_t max_row = 0;                               // the widest result row, in words
};

inline int sv_fmt_bytes(int32_t format) {              // bytes per stored sample of an ISS_RS_* format, 0: not a format
    static const int kBytes[11] = {1, 2, 4, 4, 8, 0, 0, 0, 1, 1, 1};
    const int32_t code = format & ~ISS_RS_SWAP;
    if (format < 0 || code > ISS_RS_ALAW || kBytes[code] == 0 || ((format & ISS_RS_SWAP) && kBytes[code] < 2)) return 0;
    return kBytes[code];
}

inline int64_t sv_pairs(int ch) { return ch <= SV_GROUP ? (int64_t)ch * (ch - 1) / 2 : 0; }
inline int64_t sv_row_words(int ch) { return 6 * (int64_t)ch + sv_pairs(ch); }
// float64 between the staged channels of a group of gc: the chunk, and for gc > 1 the 16 / gc frames of each channel that the
// 16 lanes of one LDS store group hold, so that those fall on different banks (resample.hip, split_geometry)
inline int sv_stride(int gc) { return gc == 1 ? SV_CHUNK : SV_CHUNK + (16 / gc > 1 ? 16 / gc : 1); }
inline int64_t sv_lds_bytes(int ch) {
    const int gc = ch < SV_GROUP ? ch : SV_GROUP;
    return ((int64_t)4 * SV_PART + (int64_t)gc * sv_stride(gc)) * 8;
}

// The members of one job of a set call (its set row S, the call's member rows; the job states frames_in frames of `channels`
// channels of esz-byte samples at src_offset 0 of a buffer of src_bytes) -> one SetChanDev per channel of the job appended to
// `chans`, or false with `why` (the resample planner and sv_plan put the job in front of it) and `chans` as it was
inline bool set_channels(const iss_set& S, const iss_set_member* members, int64_t nmembers, int64_t frames_in, int32_t channels,
                         int64_t src_offset, int64_t esz, int64_t src_bytes, std::vector<SetChanDev>& chans, std::string& why) {
    char text[224];
    auto fail = [&](const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
        snprintf(text, sizeof text, fmt, a, b, c, d);
        why = text;
        return false;
    };
    if (S.member_count < 1 || S.member_count > 1024 || S.member_begin < 0 || !members || S.member_begin > nmembers - S.member_count)
        return fail("member rows [%lld, +%lld) empty, above 1024 or outside the %lld of the call", S.member_begin, S.member_count,
                    nmembers);
    if (src_offset != 0) return fail("src_offset %lld: a set job states 0, its members say where the bytes lie", src_offset);
    int64_t nch = 0, longest = 0;
    for (int32_t m = 0; m < S.member_count; ++m) {
        const iss_set_member& M = members[S.member_begin + m];
        if (M.channels < 1 || M.channels > 1024 || M.frames < 1 || M.frames > (int64_t(1) << 40) / (esz * M.channels))
            return fail("member %lld: %lld frames of %lld channels", m, M.frames, M.channels);
        const int64_t nbytes = M.frames * M.channels * esz;
        if (M.src_offset < 0 || M.src_offset % esz != 0 || M.src_offset > src_bytes - nbytes)
            return fail("member %lld: source bytes from %lld on (%lld of them) outside the %lld-byte buffer or misaligned", m,
                        M.src_offset, nbytes, src_bytes);
        nch += M.channels;
        if (M.frames > longest) longest = M.frames;
    }
    if (nch != channels) return fail("the members hold %lld channels, the job row states %lld", nch, channels);
    if (longest != frames_in) return fail("the longest member holds %lld frames, the job row states %lld", longest, frames_in);
    for (int32_t m = 0; m < S.member_count; ++m) {
        const iss_set_member& M = members[S.member_begin + m];
        for (int32_t c = 0; c < M.channels; ++c) chans.push_back(SetChanDev{M.src_offset + c * esz, M.frames, M.channels, 0});
    }
    return true;
}

// `sets` (with `members`, nmembers; NULL: not a set call): a set row beside every job, whose channels are those of its members
// (include/iss.h, "File sets"; never with `wins` or the codec vectors): plan.chans gets a row per channel of every job.
// `stage_off` / `stage_bytes` NULL: the rows' src_offset are byte offsets into a buffer of src_bytes.  Else (the codec entries):
// src_offset is an index into the two vectors, what a decode call staged per job (offset -1: not staged).
// `block_chunks` (NULL: not a blocked call; never with `wins` or `sets`): K of every job, plan.blk gets a row per job.
// -> true, or false with `err` saying which job and why (plan is then not to be used)
inline bool sv_plan(const iss_survey_job* jobs, const iss_window* wins, int32_t njobs, int64_t src_bytes,
                    const std::vector<int64_t>* stage_off, const std::vector<int64_t>* stage_bytes, SvPlan& plan,
                    std::string& err, const iss_set* sets = nullptr, const iss_set_member* members = nullptr,
                    int64_t nmembers = 0, const int32_t* block_chunks = nullptr) {
    char text[256];
    auto fail = [&](int k, const char* why, long long a = 0, long long b = 0, long long c = 0) {
        char body[192];
        snprintf(body, sizeof body, why, a, b, c);
        snprintf(text, sizeof text, "job %d: %s", k, body);
        err = text;
        return false;
    };
    plan = SvPlan{};
    plan.dj.assign((size_t)(njobs > 0 ? njobs : 0), SvJobDev{});
    for (int32_t k = 0; k < njobs; ++k) {
        const iss_survey_job& J = jobs[k];
        const int64_t esz = sv_fmt_bytes(J.format);
        if (esz == 0) return fail(k, "bad format %lld", J.format);
        if (stage_off && J.format != ISS_RS_I16 && J.format != ISS_RS_I32)
            return fail(k, "format %lld: a decoder stages ISS_RS_I16 or ISS_RS_I32", J.format);
        if (J.channels < 1 || J.channels > 1024) return fail(k, "%lld channels", J.channels);
        if (!(J.full > 0.0) || !std::isfinite(J.full)) return fail(k, "full must be a finite value above 0");
        if (J.frames_in < 1 || J.frames_in > (int64_t(1) << 40) / (esz * J.channels)) return fail(k, "%lld frames", J.frames_in);
        const int64_t nbytes = J.frames_in * J.channels * esz;
        int64_t off = J.src_offset;
        if (sets) {
            std::string why;
            if (wins || stage_off) return fail(k, "a set call takes no windows and no decoder's staging");
            off = (int64_t)plan.chans.size();              // the job's rows of the channel table
            if (!set_channels(sets[k], members, nmembers, J.frames_in, J.channels, J.src_offset, esz, src_bytes, plan.chans, why)) {
                snprintf(text, sizeof text, "job %d: %s", k, why.c_str());
                err = text;
                return false;
            }
        } else if (stage_off) {
            if (off < 0 || off >= (int64_t)stage_off->size() || (*stage_off)[(size_t)off] < 0)
                return fail(k, "job %lld of the last decode call did not go to the staging buffer", off);
            if ((*stage_bytes)[(size_t)off] != nbytes)
                return fail(k, "staged job %lld holds %lld bytes, the row states %lld", off, (*stage_bytes)[(size_t)off], nbytes);
            off = (*stage_off)[(size_t)off];
        } else if (off < 0 || off % esz != 0 || off > src_bytes - nbytes) {
            return fail(k, "source bytes from %lld on (%lld of them) outside the %lld-byte buffer or misaligned", off, nbytes, src_bytes);
        }
        int64_t n = J.frames_in;
        if (wins) {
            const iss_window& w = wins[k];
            if (w.s_begin < 0 || w.s_begin >= w.s_end || w.s_end > w.frames_total || w.s_end - w.s_begin != J.frames_in)
                return fail(k, "window frames [%lld, %lld) of %lld do not match the frames staged", w.s_begin, w.s_end, w.frames_total);
            if (w.out_count < 1 || w.out_begin < w.s_begin || w.out_begin > w.s_end - w.out_count)
                return fail(k, "surveyed frames [%lld, +%lld) outside the staged frames", w.out_begin, w.out_count);
            off += (w.out_begin - w.s_begin) * J.channels * esz;
            n = w.out_count;
        }
        SvJobDev& d = plan.dj[(size_t)k];
        d.src_off = off; d.n = n; d.chunk_base = plan.chunks; d.ws_off = plan.ws_words; d.res_off = plan.res_words;
        d.full = J.full; d.ch = J.channels; d.fmt = J.format;
        const int64_t chunks = (n + SV_CHUNK - 1) / SV_CHUNK, row = sv_row_words(J.channels);
        plan.chunks += chunks;
        plan.ws_words += chunks * row;
        plan.res_words += row;
        if (row > plan.max_row) plan.max_row = (int32_t)row;
        if (sv_lds_bytes(J.channels) > plan.lds) plan.lds = sv_lds_bytes(J.channels);
        if (plan.chunks > 0x7fffffffLL) return fail(k, "%lld chunks in one call", plan.chunks);
        if (block_chunks) {
            if (wins || sets) return fail(k, "a blocked call takes no windows and no sets");
            const int64_t K = block_chunks[k];
            if (K < 1) return fail(k, "block_chunks %lld: a block holds at least one chunk", K);
            const int64_t nblocks = (chunks + K - 1) / K, wgroups = (row + SV_THREADS - 1) / SV_THREADS;
            plan.blk.push_back(SvBlkDev{plan.blk_units, plan.blk_words, (int32_t)K, (int32_t)wgroups});
            plan.blk_units += nblocks * wgroups;
            plan.blk_words += nblocks * row;
            if (plan.blk_units > 0x7fffffffLL) return fail(k, "%lld block units in one call", plan.blk_units);
        }
    }
    return true;
}
