// Channel survey for gfx950: per-channel peak, counts, sum and sum of squares of stored samples, and the cross-products between
// the channels of a file of up to 16, in one pass over the stored bytes (float64, no FMA, no floating-point atomic).
//
// include/iss.h ("Channel survey") states the figures and the survey order; inaspeechsegmenter_amd/resample.py `survey_ref` is
// that order in numpy, and the device equals it to the bit.  survey_plan.h builds the job table on the host.
//
// survey_kernel.  Grid: ragged over (job, chunk); job k owns blocks [chunk_base_k, chunk_base_k + ceil(n_k / 1024)), a prefix
// sum built on the host, and a workgroup finds its job by binary search (as resample_kernel does).  Per workgroup, per group of
// up to 16 channels (a file of up to 16 channels is one group):
//   1. the chunk's frames of the group's channels go to LDS as float64, one row per channel -- (frame, channel) flattened over
//      the threads, the readers of rs_readers.h: the stored bytes are read once, coalesced
//   2. per channel, lane t walks its frames t, t + 256, ... of the row: a non-finite value is counted and replaced by 0.0 in
//      the row; sum, sum of squares, peak and the counts are reduced over the wave by shuffles (the tree of the survey order),
//      and lane 0 of each wave leaves the wave's figures in LDS
//   3. (up to 16 channels) per pair c < d the same walk over the products of two rows: every pair reads LDS, not memory
//   4. one thread per figure combines the four waves in order and writes it to the chunk's row of the workspace (plain stores;
//      every word of the row is written, so nothing of an earlier call is ever read)
// survey_reduce_kernel.  One thread per (job, word of its row) walks the job's chunk rows in ascending order -- sums added from
// +0.0, peaks by max, counts as int64 -- and writes the result row.  Only the result rows come back to the host.
// Offsets into the source, the workspace and the results are 64-bit.  LDS: 4 * 216 words of wave figures, then 16 rows of
// 1025 float64 (138 112 bytes for 16 channels; 15 104 for one).
#include "decode_pass.h"
#include "rs_readers.h"
#include "survey_plan.h"
#include <algorithm>
#include <cstring>

namespace {

static_assert(SV_THREADS == RS_THREADS, "stage_channels strides by RS_THREADS");

__device__ __forceinline__ double wave_sum(double v) {                     // lane l += lane l + s, s = 32 .. 1: lane 0 holds the tree's sum
    for (int s = 32; s > 0; s >>= 1) v = __dadd_rn(v, __shfl_down(v, s));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int s = 32; s > 0; s >>= 1) v = fmax(v, __shfl_down(v, s));
    return v;
}
__device__ __forceinline__ int wave_count(int v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    return v;
}

// SET = false is the kernel every survey of interleaved frames launches.  SET = true (include/iss.h, "File sets") stages the same
// rows through the per-channel table that follows the job rows, J.src_off being the job's first row of it: steps 2 to 4, and so
// every figure, are the code below on the same LDS
#define SV_STAGE(L)                                                                                             \
    do {                                                                                                        \
        if constexpr (SET) stage_set_channels<L>(src, chans + c0, k0, len, span, stride, gc);                   \
        else stage_channels<L, false>(s, J.n, ch, k0, len, span, stride, c0, gc, nullptr, W);                   \
    } while (0)
template <bool SET>
__global__ __launch_bounds__(SV_THREADS) void survey_kernel(const uint8_t* __restrict__ src, const SvJobDev* __restrict__ jobs,
                                                            int njobs, unsigned long long* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) double sv_smem[];
    const int64_t b = blockIdx.x;
    int lo = 0, hi = njobs - 1;                                             // last job whose chunk_base <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].chunk_base <= b) lo = mid; else hi = mid - 1;
    }
    const SvJobDev J = jobs[lo];
    const int64_t q = b - J.chunk_base, k0 = q * SV_CHUNK;
    const int len = (int)min((int64_t)SV_CHUNK, J.n - k0);
    const int ch = J.ch, npairs = ch <= SV_GROUP ? ch * (ch - 1) / 2 : 0;
    unsigned long long* row = ws + J.ws_off + q * (6 * (int64_t)ch + npairs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* part = sv_smem;                                                 // [wave][SV_PART]: what each wave found for the group
    double* span = sv_smem + 4 * SV_PART;
    const uint8_t* s = src + J.src_off;
    const SetChanDev* chans = nullptr;                                      // SET: the job's rows of the channel table
    if constexpr (SET) chans = reinterpret_cast<const SetChanDev*>(jobs + njobs) + J.src_off;
    const RsWinDev W{};
    for (int c0 = 0; c0 < ch; c0 += SV_GROUP) {
        const int gc = min(SV_GROUP, ch - c0);
        const int stride = gc == 1 ? SV_CHUNK : SV_CHUNK + max(16 / gc, 1);
        switch (J.fmt) {
            case ISS_RS_U8:   SV_STAGE(LdPlain<uint8_t>); break;
            case ISS_RS_I16:  SV_STAGE(LdPlain<int16_t>); break;
            case ISS_RS_I32:  SV_STAGE(LdPlain<int32_t>); break;
            case ISS_RS_F32:  SV_STAGE(LdPlain<float>); break;
            case ISS_RS_F64:  SV_STAGE(LdPlain<double>); break;
            case ISS_RS_I8:   SV_STAGE(LdPlain<int8_t>); break;
            case ISS_RS_ULAW: SV_STAGE(LdUlaw); break;
            case ISS_RS_ALAW: SV_STAGE(LdAlaw); break;
            case ISS_RS_I16 | ISS_RS_SWAP: SV_STAGE(LdSwapI16); break;
            case ISS_RS_I32 | ISS_RS_SWAP: SV_STAGE(LdSwapI32); break;
            case ISS_RS_F32 | ISS_RS_SWAP: SV_STAGE(LdSwapF32); break;
            default:          SV_STAGE(LdSwapF64); break;                   // ISS_RS_F64 | ISS_RS_SWAP
        }
        __syncthreads();
        for (int kk = 0; kk < gc; ++kk) {                                   // step 2: one channel's row
            double* sp = span + kk * stride;
            double a1 = 0.0, a2 = 0.0, pk = 0.0;
            int nz = 0, nf = 0, nn = 0;
            for (int k = threadIdx.x; k < len; k += SV_THREADS) {
                double v = sp[k];
                if (!(fabs(v) <= 1.7976931348623157e308)) { v = 0.0; sp[k] = 0.0; ++nn; }      // NaN, +-Inf
                const double av = fabs(v);
                a1 = __dadd_rn(a1, v);
                a2 = __dadd_rn(a2, __dmul_rn(v, v));
                pk = fmax(pk, av);
                nz += v == 0.0;
                nf += av >= J.full;
            }
            a1 = wave_sum(a1); a2 = wave_sum(a2); pk = wave_max(pk);
            nz = wave_count(nz); nf = wave_count(nf); nn = wave_count(nn);
            if (lane == 0) {
                double* p = part + wave * SV_PART;
                p[kk] = a1; p[gc + kk] = a2; p[2 * gc + kk] = pk;
                p[3 * gc + kk] = __longlong_as_double(nz); p[4 * gc + kk] = __longlong_as_double(nf);
                p[5 * gc + kk] = __longlong_as_double(nn);
            }
        }
        __syncthreads();                                                    // (the rows hold no non-finite value from here on)
        if (npairs > 0) {                                                   // step 3
            int idx = 6 * gc;
            for (int c = 0; c < gc; ++c)
                for (int d = c + 1; d < gc; ++d, ++idx) {
                    const double* pc = span + c * stride;
                    const double* pd = span + d * stride;
                    double a = 0.0;
                    for (int k = threadIdx.x; k < len; k += SV_THREADS) a = __dadd_rn(a, __dmul_rn(pc[k], pd[k]));
                    a = wave_sum(a);
                    if (lane == 0) part[wave * SV_PART + idx] = a;
                }
            __syncthreads();
        }
        const int t = threadIdx.x;                                          // step 4: figure t of the group
        if (t < 6 * gc + npairs) {
            const double p0 = part[t], p1 = part[SV_PART + t], p2 = part[2 * SV_PART + t], p3 = part[3 * SV_PART + t];
            const int kind = t < 6 * gc ? t / gc : 6;
            const int64_t dest = kind < 6 ? (int64_t)kind * ch + c0 + (t - kind * gc) : 6 * (int64_t)ch + (t - 6 * gc);
            unsigned long long out;
            if (kind == 2) out = (unsigned long long)__double_as_longlong(fmax(fmax(p0, p1), fmax(p2, p3)));
            else if (kind >= 3 && kind < 6)
                out = (unsigned long long)(__double_as_longlong(p0) + __double_as_longlong(p1) + __double_as_longlong(p2) +
                                           __double_as_longlong(p3));
            else out = (unsigned long long)__double_as_longlong(__dadd_rn(__dadd_rn(__dadd_rn(p0, p1), p2), p3));
            row[dest] = out;
        }
        __syncthreads();                                                    // the next group stages over these rows
    }
}
#undef SV_STAGE

// word w of job blockIdx.x's result row: its chunk rows in ascending order
__global__ __launch_bounds__(SV_THREADS) void survey_reduce_kernel(const SvJobDev* __restrict__ jobs,
                                                                   const unsigned long long* __restrict__ ws,
                                                                   unsigned long long* __restrict__ res) {
    const SvJobDev J = jobs[blockIdx.x];
    const int ch = J.ch;
    const int64_t width = 6 * (int64_t)ch + (ch <= SV_GROUP ? ch * (ch - 1) / 2 : 0);
    const int64_t w = (int64_t)blockIdx.y * SV_THREADS + threadIdx.x;
    if (w >= width) return;
    const int64_t chunks = (J.n + SV_CHUNK - 1) / SV_CHUNK;
    const unsigned long long* p = ws + J.ws_off + w;
    const bool is_max = w >= 2 * (int64_t)ch && w < 3 * (int64_t)ch, is_count = w >= 3 * (int64_t)ch && w < 6 * (int64_t)ch;
    double acc = 0.0;
    long long cnt = 0;
    for (int64_t q0 = 0; q0 < chunks; q0 += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = q0 + u < chunks ? p[(q0 + u) * width] : 0ull;      // (+0.0, or a count of 0)
        const int m = (int)min((int64_t)8, chunks - q0);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < m) {
                if (is_count) cnt += (long long)v[u];
                else if (is_max) acc = fmax(acc, __longlong_as_double((long long)v[u]));
                else acc = __dadd_rn(acc, __longlong_as_double((long long)v[u]));
            }
        }
    }
    res[J.res_off + w] = is_count ? (unsigned long long)cnt : (unsigned long long)__double_as_longlong(acc);
}

// Survey blocks (include/iss.h).  Grid: ragged over (job, block, group of SV_THREADS words); job k owns units [unit_base_k,
// unit_base_k + nblocks_k * wgroups_k) of the SvBlkDev rows that follow the job rows, a prefix sum built on the host, and a
// workgroup finds its job by binary search.  Thread t adds word w = group * SV_THREADS + t of the block's chunk rows [block * K,
// min((block + 1) * K, chunks)) in ascending order, exactly as survey_reduce_kernel adds a job's, and stores it: plain stores,
// every word of every block row written once
__global__ __launch_bounds__(SV_THREADS) void survey_reduce_blocks_kernel(const SvJobDev* __restrict__ jobs, int njobs,
                                                                          const unsigned long long* __restrict__ ws,
                                                                          unsigned long long* __restrict__ res) {
    const SvBlkDev* blks = reinterpret_cast<const SvBlkDev*>(jobs + njobs);
    const int64_t b = blockIdx.x;
    int lo = 0, hi = njobs - 1;                                             // last job whose unit_base <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blks[mid].unit_base <= b) lo = mid; else hi = mid - 1;
    }
    const SvJobDev J = jobs[lo];
    const SvBlkDev B = blks[lo];
    const int ch = J.ch;
    const int64_t width = 6 * (int64_t)ch + (ch <= SV_GROUP ? ch * (ch - 1) / 2 : 0);
    const int u = (int)(b - B.unit_base), blk = u / B.wgroups;
    const int64_t w = (int64_t)(u - blk * B.wgroups) * SV_THREADS + threadIdx.x;
    if (w >= width) return;
    const int64_t chunks = (J.n + SV_CHUNK - 1) / SV_CHUNK;
    const int64_t q_begin = (int64_t)blk * B.K, q_end = min(q_begin + B.K, chunks);
    const unsigned long long* p = ws + J.ws_off + w;
    const bool is_max = w >= 2 * (int64_t)ch && w < 3 * (int64_t)ch, is_count = w >= 3 * (int64_t)ch && w < 6 * (int64_t)ch;
    double acc = 0.0;
    long long cnt = 0;
    for (int64_t q0 = q_begin; q0 < q_end; q0 += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = q0 + k < q_end ? p[(q0 + k) * width] : 0ull;        // (+0.0, or a count of 0)
        const int m = (int)min((int64_t)8, q_end - q0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < m) {
                if (is_count) cnt += (long long)v[k];
                else if (is_max) acc = fmax(acc, __longlong_as_double((long long)v[k]));
                else acc = __dadd_rn(acc, __longlong_as_double((long long)v[k]));
            }
        }
    }
    res[B.out_off + (int64_t)blk * width + w] = is_count ? (unsigned long long)cnt : (unsigned long long)__double_as_longlong(acc);
}

// the body of the five entry points: the rows planned against `src_bytes` of uploaded bytes (dec == NULL) or against what `dec`
// staged last; both launches; the result rows copied back before it returns.  `set`: the tables of iss_survey_set (else NULL).
// `blocked`: a *_blocks entry point (include/iss.h, "Survey blocks") with K per job and the block rows' destination: the third
// launch, and a second copy back
int survey_call(iss_ctx* c, const char* who, IssCodec* dec, const void* src, int64_t src_bytes, const iss_survey_job* jobs,
                const iss_window* windows, int32_t njobs, void* results, const IssSetTables* set = nullptr, bool blocked = false,
                const int32_t* block_chunks = nullptr, void* block_results = nullptr) {
    if (!c || njobs < 0 || (njobs > 0 && (!jobs || !results)) || src_bytes < 0 || (!dec && !src && src_bytes > 0) ||
        (set && njobs > 0 && !set->sets) || (set && (set->nmembers < 0 || (set->nmembers > 0 && !set->members))) ||
        (blocked && njobs > 0 && (!block_chunks || !block_results)))
        return iss_fail(c, ISS_EINVAL, "%s: bad argument", who);
    SvPlan plan;
    std::string err;
    if (!sv_plan(jobs, windows, njobs, src_bytes, dec ? &dec->stage_off : nullptr, dec ? &dec->stage_bytes : nullptr, plan, err,
                 set ? set->sets : nullptr, set ? set->members : nullptr, set ? set->nmembers : 0, blocked ? block_chunks : nullptr))
        return iss_fail(c, ISS_EINVAL, "%s: %s", who, err.c_str());
    if (njobs == 0) return ISS_OK;
    ISS_HIP(c, hipSetDevice(c->device));
    int rc;
    const uint8_t* dev_src = dec ? (const uint8_t*)dec->stage.p : nullptr;
    if (!dec) {
        if ((rc = iss_upload_payload(c, c->sv_src, "survey", src, src_bytes, (size_t)std::max<int64_t>(src_bytes, 16)))) return rc;
        dev_src = (const uint8_t*)c->sv_src.p;
    }
    if ((rc = iss_reserve(c, c->sv_ws, (size_t)plan.ws_words * 8))) return rc;
    if ((rc = iss_reserve(c, c->sv_res, (size_t)plan.res_words * 8))) return rc;
    if (blocked) {                                         // one table: the jobs, then the block geometry of every one of them
        if ((rc = iss_reserve(c, c->sv_blk, (size_t)plan.blk_words * 8))) return rc;
        const size_t nj = plan.dj.size() * sizeof(SvJobDev), nb = plan.blk.size() * sizeof(SvBlkDev);
        std::vector<uint8_t> rows(nj + nb);
        memcpy(rows.data(), plan.dj.data(), nj);
        memcpy(rows.data() + nj, plan.blk.data(), nb);
        rc = iss_upload_rows(c, c->sv_jobs, rows.data(), rows.size());
    } else if (set) {                                      // one table: the jobs, then the channels of every one of them
        const size_t nj = plan.dj.size() * sizeof(SvJobDev), nc = plan.chans.size() * sizeof(SetChanDev);
        std::vector<uint8_t> rows(nj + nc);
        memcpy(rows.data(), plan.dj.data(), nj);
        memcpy(rows.data() + nj, plan.chans.data(), nc);
        rc = iss_upload_rows(c, c->sv_jobs, rows.data(), rows.size());
    } else {
        rc = iss_upload_rows(c, c->sv_jobs, plan.dj.data(), plan.dj.size() * sizeof(SvJobDev));
    }
    if (rc) return rc;
    auto kernel = set ? survey_kernel<true> : survey_kernel<false>;
    if (plan.lds > 64 * 1024)
        ISS_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    iss_prof_begin(c, ISS_PROF_FRONTEND, 0.0);
    iss_prof_inst(c, "survey_kernel");
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.chunks), dim3(SV_THREADS), (size_t)plan.lds, c->stream, dev_src,
                       (const SvJobDev*)c->sv_jobs.p, (int)njobs, (unsigned long long*)c->sv_ws.p);
    ISS_HIP(c, hipGetLastError());
    iss_prof_end(c);
    iss_prof_begin(c, ISS_PROF_FRONTEND, 0.0);
    iss_prof_inst(c, "survey_reduce_kernel");
    hipLaunchKernelGGL(survey_reduce_kernel, dim3((unsigned)njobs, (unsigned)((plan.max_row + SV_THREADS - 1) / SV_THREADS)),
                       dim3(SV_THREADS), 0, c->stream, (const SvJobDev*)c->sv_jobs.p, (const unsigned long long*)c->sv_ws.p,
                       (unsigned long long*)c->sv_res.p);
    ISS_HIP(c, hipGetLastError());
    iss_prof_end(c);
    if (blocked) {
        iss_prof_begin(c, ISS_PROF_FRONTEND, 0.0);
        iss_prof_inst(c, "survey_reduce_blocks_kernel");
        hipLaunchKernelGGL(survey_reduce_blocks_kernel, dim3((unsigned)plan.blk_units), dim3(SV_THREADS), 0, c->stream,
                           (const SvJobDev*)c->sv_jobs.p, (int)njobs, (const unsigned long long*)c->sv_ws.p,
                           (unsigned long long*)c->sv_blk.p);
        ISS_HIP(c, hipGetLastError());
        iss_prof_end(c);
        ISS_HIP(c, hipMemcpyAsync(block_results, c->sv_blk.p, (size_t)plan.blk_words * 8, hipMemcpyDeviceToHost, c->stream));
    }
    ISS_HIP(c, hipMemcpyAsync(results, c->sv_res.p, (size_t)plan.res_words * 8, hipMemcpyDeviceToHost, c->stream));
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    c->sv_count.launches += 1;
    c->sv_count.units += njobs;
    if (!dec) {                                            // sv_src holds these jobs' bytes until the next upload into it
        c->sv_held.id = ++c->held_seq;
        c->sv_held.bytes = src_bytes;
        c->sv_held.jobs.assign(jobs, jobs + njobs);
        c->sv_held.sets.clear();
        c->sv_held.members.clear();
        if (set) {
            c->sv_held.sets.assign(set->sets, set->sets + njobs);
            c->sv_held.members.assign(set->members, set->members + set->nmembers);
        }
    }
    return ISS_OK;
}

}  // namespace

extern "C" int iss_survey(iss_ctx* c, const void* src, int64_t src_bytes, const iss_survey_job* jobs, const iss_window* windows,
                          int32_t njobs, void* results) {
    return survey_call(c, "iss_survey", nullptr, src, src_bytes, jobs, windows, njobs, results);
}

extern "C" int iss_survey_set(iss_ctx* c, const void* src, int64_t src_bytes, const iss_survey_job* jobs, int32_t njobs,
                              const iss_set* sets, const iss_set_member* members, int64_t nmembers, void* results) {
    const IssSetTables set{sets, members, nmembers};
    return survey_call(c, "iss_survey_set", nullptr, src, src_bytes, jobs, nullptr, njobs, results, &set);
}

extern "C" int iss_flac_survey(iss_ctx* c, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results) {
    return survey_call(c, "iss_flac_survey", c ? &c->flac : nullptr, nullptr, 0, jobs, windows, njobs, results);
}

extern "C" int iss_adpcm_survey(iss_ctx* c, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results) {
    return survey_call(c, "iss_adpcm_survey", c ? &c->adpcm : nullptr, nullptr, 0, jobs, windows, njobs, results);
}

extern "C" int iss_msadpcm_survey(iss_ctx* c, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results) {
    return survey_call(c, "iss_msadpcm_survey", c ? &c->msadpcm : nullptr, nullptr, 0, jobs, windows, njobs, results);
}

extern "C" int iss_survey_blocks(iss_ctx* c, const void* src, int64_t src_bytes, const iss_survey_job* jobs, int32_t njobs,
                                 const int32_t* block_chunks, void* results, void* block_results) {
    return survey_call(c, "iss_survey_blocks", nullptr, src, src_bytes, jobs, nullptr, njobs, results, nullptr, true, block_chunks,
                       block_results);
}

extern "C" int iss_flac_survey_blocks(iss_ctx* c, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks,
                                      void* results, void* block_results) {
    return survey_call(c, "iss_flac_survey_blocks", c ? &c->flac : nullptr, nullptr, 0, jobs, nullptr, njobs, results, nullptr, true,
                       block_chunks, block_results);
}

extern "C" int iss_adpcm_survey_blocks(iss_ctx* c, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks,
                                       void* results, void* block_results) {
    return survey_call(c, "iss_adpcm_survey_blocks", c ? &c->adpcm : nullptr, nullptr, 0, jobs, nullptr, njobs, results, nullptr,
                       true, block_chunks, block_results);
}

extern "C" int iss_msadpcm_survey_blocks(iss_ctx* c, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks,
                                         void* results, void* block_results) {
    return survey_call(c, "iss_msadpcm_survey_blocks", c ? &c->msadpcm : nullptr, nullptr, 0, jobs, nullptr, njobs, results, nullptr,
                       true, block_chunks, block_results);
}

extern "C" int iss_survey_geometry(int32_t* chunk_out, int32_t* lanes_out, int32_t* pair_channels_out) {
    if (!chunk_out || !lanes_out || !pair_channels_out) return ISS_EINVAL;
    *chunk_out = SV_CHUNK; *lanes_out = SV_THREADS; *pair_channels_out = SV_GROUP;
    return ISS_OK;
}

extern "C" int iss_survey_stats(iss_ctx* c, int64_t* launches, int64_t* jobs) {
    return iss_get_counters(c ? &c->sv_count : nullptr, launches, jobs);
}
