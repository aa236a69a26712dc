// Internal state of libiss_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <string>
#include <vector>
#include <unordered_map>
#include <map>
#include <memory>
#include "../../include/iss.h"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct ConvOp;   // cnn.hip

struct IssCounters { int64_t launches = 0, units = 0; };   // what the *_stats entry points report (iss_get_counters)
// A coded decoder's device buffers and what its last call left (decode_pass.h).  A new format adds one member to iss_ctx
struct IssCodec {
    const char* name;                                  // "flac": iss_<name>_decode, <name>_h2d
    DevBuf src, rows, status, stage;                   // payload, row table, per-unit status, staging buffer of the last call
    std::vector<int64_t> stage_off, stage_bytes;       // per job of the last call (-1: not staged)
    std::vector<int32_t> stage_esz;                    // ... and the bytes of a staged sample (2: ISS_RS_I16, 4: ISS_RS_I32)
    IssCounters count;                                 // launches, units (frames / blocks) decoded
    int64_t held = 0;                                  // id of what `stage` holds for iss_resample_staged_mix (0: nothing whole)
};

// A network's device parameter arrays once another net shares them (iss_cnn_load_shared): freed with their last user.
struct IssParamArrays {
    float* blob = nullptr;
    uint16_t *wh = nullptr, *wl = nullptr, *wh16 = nullptr, *wl16 = nullptr;
    ~IssParamArrays();                    // cnn.hip
};

struct IssNet {
    bool loaded = false;
    std::vector<int32_t> prog;            // nrows * ISS_PROG_COLS
    int nrows = 0;
    float* d_blob = nullptr;              // parameters (conv weights [Cout][Kpad])
    uint16_t* d_wh = nullptr;             // bf16 hi part of every blob element (same offsets)
    uint16_t* d_wl = nullptr;             // bf16 lo part
    uint16_t* d_wh16 = nullptr;           // fp16 hi / lo parts (ISS_PREC_F16X3)
    uint16_t* d_wl16 = nullptr;
    bool f16_ok = false;                  // every parameter is inside fp16's range
    std::shared_ptr<IssParamArrays> shared_params;   // set once the five arrays above are shared with another net: freed with the last holder
    std::map<std::pair<int, int>, uint16_t*> dhl_wp;   // (row, fp16?) -> the dense layer's weights packed for conv_dhl_kernel (built at first use)
    float* d_wsum = nullptr;              // patch-mode first layers: sum_k w[c][k] per output channel (shared first layer)
    std::vector<int64_t> wsum_off;        // per row: offset into d_wsum, -1 = none
    std::vector<int64_t> wsumx_off;       // per row: offset of S[W][Cout] (zero-padded first layers: per-column weight sums), -1 = none
    int64_t blob_floats = 0;
    std::vector<int64_t> w_dev_off;       // per row: offset of the padded weight matrix in d_blob
    std::vector<int32_t> kpad;            // per row: K padded to the GEMM k-tile
    int32_t* d_ktab = nullptr;            // per-conv im2col tables
    std::vector<int64_t> ktab_off;        // per row
    int nbuf = 0;
    std::vector<int64_t> buf_elems;
    int in_h = 0, in_w = 0, in_c = 0, out_dim = 0;
    double flops_per_sample = 0;
    // footprint cache (conv_select.h tile_span / tile_rows): (row, TM, 0, 0) -> largest pixel span of a TM-row tile of that row;
    // (row, hi, lo, cap) -> the tallest tile in [lo, hi] spanning at most cap pixels.  Keyed on what the value depends on, so every
    // kernel family that asks the same question shares the entry
    std::map<std::array<int, 4>, int> fp_pix;
    // precision guard (iss_set_precision_guard / iss_cnn_precision_info)
    int prec_override = -1;               // -1: the context's mode; else ISS_PREC_* for this network only
    bool prec_by_caller = false;          // prec_override came from iss_cnn_set_net_precision (else from the guard: iss_set_precision re-arms)
    int guard_state = 0;                  // ISS_GUARD_*
    float guard_dlogp = -1.f;             // max |log p(mode asked for) - log p(exact f32)| of the probe, -1 = never probed
    float guard_dlogp_chosen = -1.f;      // the same figure for the mode the network runs in after the probe
    int guard_slots = 0;                  // windows the probe compared
};

struct iss_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;

    // sidekit tables
    bool sk_tables = false;
    double* d_window = nullptr;           // 400
    float* d_melw = nullptr;              // packed non-zero weights per filter
    int32_t* d_mellim = nullptr;          // 24 x {first_bin, n_bins, weight_offset}
    double* d_tw = nullptr;               // W256 (256 complex) then W512 (256 complex)

    // resident signal
    DevBuf sig;                           // owned copy
    const void* sig_ptr = nullptr;        // points into sig.p or to caller's device memory
    int sig_kind = 0;                     // 0 none, 1 pcm16, 2 f32
    int64_t sig_n = 0;

    // resampler (resample.hip): filters per (up, down), the raw-source and job buffers of the last call
    struct RsFilter { int32_t up = 1, down = 1, hl = 0; int64_t ntaps = 1; double* d_taps = nullptr; };
    std::vector<RsFilter> rs_filters;
    std::map<std::pair<int32_t, int32_t>, int32_t> rs_filter_id;
    DevBuf rs_src, rs_jobs;
    IssCounters rs_count;                 // launches, jobs

    // the coded decoders: FLAC (flac.hip: rows = frames), IMA ADPCM and Microsoft ADPCM (adpcm.hip: rows = jobs, status per block).
    // The two ADPCM coders share a kernel template and nothing of their state: a pass with files of both makes two calls
    IssCodec flac{"flac"}, adpcm{"adpcm"}, msadpcm{"msadpcm"};

    // channel survey (survey.hip): uploaded bytes, job rows, per-chunk partial rows, result rows of the last call
    DevBuf sv_src, sv_jobs, sv_ws, sv_res, sv_blk;   // sv_blk: the block rows of a *_survey_blocks call
    IssCounters sv_count;                 // survey_kernel launches, jobs
    // what a later call may resample without uploading it again (iss_resample_staged_mix): the payload of the last iss_survey in
    // sv_src, with the rows that describe it; a codec's is its IssCodec::held.  Ids count up over all origins of the context
    // (a payload of iss_survey_set: the set row of every job and the call's member rows too; else both empty)
    struct Held { int64_t id = 0, bytes = 0; std::vector<iss_survey_job> jobs; std::vector<iss_set> sets; std::vector<iss_set_member> members; } sv_held;
    int64_t held_seq = 0;
    IssCounters up_count;                 // iss_upload_payload: copies, bytes (iss_upload_stats)

    // resident features
    DevBuf mspec, loge;
    int32_t T = 0;
    bool have_feats = false;
    uint64_t feat_epoch = 1;              // bumped wherever have_feats, sig_* (iss_set_signal) or T is set: what was derived from the features is stale

    // dead windows (cnn.hip, cnn_probs_impl): per resident log-mel row the lowest column holding a non-finite value (24: none),
    // read back once per feature set, and per network width w the prefix count of rows whose flag is < w
    uint64_t flags_epoch = 0;             // feat_epoch the row flags belong to
    uint64_t flags_queued = 0;            // feat_epoch whose flags iss_sidekit has put on the stream (kernel + read-back): they are on the host after the next wait
    DevBuf d_rowflag;
    uint8_t* h_rowflag = nullptr;         // page-locked, grow-only
    size_t h_rowflag_cap = 0;
    std::map<int, std::vector<int32_t>> bad_prefix;
    DevBuf d_lfinite;                     // finite flags of the compacted (live) window list; d_finite holds the caller's slots
    int64_t win_total = 0, win_dead = 0;  // iss_cnn_dead_stats

    // CNN engine
    IssNet nets[ISS_MAX_NETS];
    uint64_t ws_limit = 24ull << 30;                // of 288 GB: the x-vector net then runs the 1 816 windows per pass its 2^31-element buffers allow (12 GiB: 1 072, -2 %)
    int precision = ISS_PREC_F16X3;
    float guard_threshold = 5e-4f;        // precision guard: escalate a patch network to exact f32 above this max |d log p| (<= 0: guard off)
    bool in_guard = false;
    uint32_t diag = 0;                    // ISS_DIAG_* kernel-selection switches (iss_set_diag; 0 in production)
    std::vector<DevBuf> act;              // activation buffers (grown on demand)
    DevBuf d_winrow, d_stats, d_finite, d_out, d_in;
    DevBuf raw1;                          // shared first layer: raw conv over the log-mel rows of the current chunk

    // vbx
    bool vbx_tables = false;
    double* d_vbx_window = nullptr;
    double* d_vbx_melw = nullptr;
    int32_t* d_vbx_mellim = nullptr;
    DevBuf vbx_sig, vbx_dither, vbx_fb, vbx_out;
    DevBuf vbx_meta;                       // batch front end: per-file sample offsets (int64; resident parts: begins, then lengths) then frame offsets (int32)
    int32_t vbx_T = 0;
    int64_t vbx_dither_n = 0;              // length of the dither stream cached in vbx_dither (0 = none)
    IssCounters vbx_res_count;             // iss_vbx_features_resident: calls (one fbank launch each), parts

    // pinned staging buffers of the asynchronous entry points (window lists): reused once their copy has completed
    struct Staging { void* p = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool busy = false; };
    std::vector<Staging> staging;
    // tickets of iss_cnn_probs_async: ticket t <-> tickets[t - ticket_base].  A call's result lands in the caller's arrays front
    // to back, one landing per pass (page-locked outputs) or one in all: slots [0, slot_end) are there once `ev` has completed.
    // slot_end ascends and the last one is the call's slot count; the last event is what iss_wait waits for
    struct Landing { int32_t slot_end; hipEvent_t ev; };
    struct Ticket { std::vector<Landing> land; size_t done = 0; };   // done: landings iss_wait_slots has seen complete
    std::vector<Ticket> tickets;
    int64_t ticket_base = 1;
    hipEvent_t order_ev = nullptr;        // iss_signal_pcm16_device*: producer stream -> library stream

    // multi-GPU (RCCL, dlopen'ed)
    void* comm = nullptr;                 // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    DevBuf comm_send, comm_recv;

    // profiling
    bool prof = false;
    double prof_ms[ISS_PROF_KINDS] = {};
    int64_t prof_launch[ISS_PROF_KINDS] = {};
    double prof_flops[ISS_PROF_KINDS] = {};
    double prof_row_ms[ISS_PROF_ROWS] = {};
    int64_t prof_row_launch[ISS_PROF_ROWS] = {};
    struct Pending { hipEvent_t a, b; int kind; int sub; int row; double flops; std::string inst; };
    std::vector<Pending> pending;
    // per kernel INSTANTIATION (template arguments spelled out by the launcher): what bench.py's roofline.dominant reports
    struct Inst { std::string name; double ms = 0; int64_t launches = 0; double flops = 0; };
    std::vector<Inst> prof_inst;
    std::vector<hipEvent_t> ev_pool;
};

int iss_fail(iss_ctx* c, int code, const char* fmt, ...);
int iss_reserve(iss_ctx* c, DevBuf& b, size_t bytes);
void iss_set_signal(iss_ctx* c, const void* ptr, int kind, int64_t n);   // the resident signal is now this; features are stale
int iss_stage_host(iss_ctx* c, const void* src, size_t bytes, void** pinned_out, int* slot_out);   // copy into a pinned staging buffer
void iss_stage_mark(iss_ctx* c, int slot);                                                       // record 'consumed' on the stream
int iss_rowflag_host(iss_ctx* c, size_t rows);                                                   // page-locked h_rowflag of >= rows bytes

// the lowest column of one 24-column log-mel row that holds a non-finite value, 24 if none (host and device)
__host__ __device__ inline int iss_row_flag(const float* row) {
    for (int k = 0; k < 24; ++k) {
        const float v = row[k];
        if (!(v - v == 0.f)) return k;            // inf - inf and nan - nan are NaN
    }
    return 24;
}

#define ISS_HIP(c, call)                                                                  \
    do {                                                                                  \
        hipError_t e__ = (call);                                                          \
        if (e__ != hipSuccess)                                                            \
            return iss_fail((c), ISS_EHIP, "%s failed: %s (%s:%d)", #call,                \
                            hipGetErrorString(e__), __FILE__, __LINE__);                  \
    } while (0)

// profiling brackets: record events around a kernel class when enabled
void iss_prof_begin(iss_ctx* c, int kind, double flops);
void iss_prof_tag(iss_ctx* c, int sub);      // kernel class (ISS_PROF_* >= 3) of the launch bracketed last: counted there too
void iss_prof_row(iss_ctx* c, int row);      // op-program row of the launch bracketed last
void iss_prof_inst(iss_ctx* c, const char* fmt, ...);   // kernel instantiation of the launch bracketed last (printf-style name)
void iss_prof_end(iss_ctx* c);
void iss_prof_collect(iss_ctx* c);

// resample.hip: a validated set of resample jobs (device descriptors, tiles, LDS), launched from any device source
struct RsJobDev {
    int64_t src_off, n_in, dst_off, n_out, tile_base;
    const double* taps;
    int32_t ch, fmt, up, down, hl, tile, lds_tab, pad;
};
struct RsWinDev { int64_t in_begin, frames_total, out_begin, out_end; };   // beside RsJobDev k of a windowed call (n_in: staged frames)
// beside RsJobDev k of a split call: sel_count selected channels (rows [sel_begin, +sel_count) of the selection table; 0: downmix),
// `group` of them per workgroup at `stride` float64 apart in LDS, each over `ntiles` tiles; ident: the selection is 0, 1, 2, ...
struct RsSplitDev { int64_t dst_stride, ntiles; int32_t sel_begin, sel_count, group, stride, ident, pad; };
// beside RsJobDev k of a mix call: mix_count mixes (0: downmix), `group` of them per workgroup at `stride` float64 apart in LDS,
// each over `ntiles` tiles; the job's mixes are rows [mix_begin, +mix_count) of the 16-byte rows that follow the mix-set table:
// first the call's RsMixRow, then its RsTermDev, a mix's term_begin counted from the first of those rows
struct RsMixDev { int64_t dst_stride, ntiles; int32_t mix_begin, mix_count, group, stride; };
struct RsMixRow { int32_t term_begin, term_count; double divisor; };
struct RsTermDev { int32_t channel, pad; double weight; };
// a term row of a set call (include/iss.h, "File sets") in the place of RsTermDev, two 16-byte rows: the term's channel resolved
// on the host to where it lies -- sample (j, that channel) of its member at byte off + j * step * sample bytes, 0.0 from frame
// `frames` on
struct RsSetTermDev { int64_t off, frames; double weight; int32_t step, pad; };
static_assert(sizeof(RsMixRow) == 16 && sizeof(RsTermDev) == 16 && sizeof(RsSetTermDev) == 32, "one array of 16-byte rows");
// a scheduled call (include/iss.h, "Schedules"): a mix call whose every job writes one row; RsMixDev.mix_begin of job k names its
// RsSchedDev among the 16-byte rows -- mix rows, term rows, one RsSchedDev per job, then the RsRunDev rows --, every index counted
// from the first mix row.  run_begin: the job's first RsRunDev; RsRunDev.mix: the RsMixRow the run's frames are mixed by;
// RsRunDev.half: the half-width of the run's fade zone (include/iss.h, "Fades"; 0 in every call without fades)
struct RsSchedDev { int32_t run_begin, run_count; int64_t pad; };
struct RsRunDev { int64_t begin; int32_t mix, half; };
static_assert(sizeof(RsSchedDev) == 16 && sizeof(RsRunDev) == 16, "one array of 16-byte rows");
// the two tables of a *_sched entry point; `scheds` one per job.  `fades`: the half-widths of a *_sched_fade entry point, one per
// row of `runs` (NULL: a *_sched entry point, every half-width 0)
struct IssSchedTables { const iss_sched* scheds; const iss_sched_run* runs; int64_t nruns; const int32_t* fades = nullptr; };
// the three tables of a *_mix entry point (include/iss.h); `sets` one per job
struct IssMixTables { const iss_mixset* sets; const iss_mix* mixes; int64_t nmixes; const iss_mix_term* terms; int64_t nterms; };
// the two tables of a *_set entry point; `sets` one per job
struct IssSetTables { const iss_set* sets; const iss_set_member* members; int64_t nmembers; };
struct IssRsPlan {
    std::vector<RsJobDev> dj;
    std::vector<RsWinDev> dw;             // empty: no windows, the launch every call made before there were any
    std::vector<RsSplitDev> ds;           // empty: no splits, likewise
    std::vector<int32_t> sel;             // the channel selections the rows of ds point into
    std::vector<RsMixDev> dm;             // empty: no mixes, likewise
    std::vector<RsMixRow> mixes;          // the mix rows the rows of dm point into ...
    std::vector<RsTermDev> terms;         // ... and the term rows those point into
    std::vector<RsSetTermDev> sterms;     // a set call: its term rows in the place of `terms`, and `set` says so
    bool set = false;
    std::vector<RsSchedDev> scheds;       // a scheduled call: one per job, and `sched` says so ...
    std::vector<RsRunDev> runs;           // ... and every job's runs, their mixes resolved to rows of `mixes`
    bool sched = false;
    bool fade = false;                    // ... a run of which has a fade zone: the FADE instantiation
    int64_t tiles = 0, lds = 0;
};
// `ranges`: destination ranges of other writers of the same call, checked for overlap with the jobs' (error texts start with `who`)
// `wins`: NULL, or a window beside every job (include/iss.h);  `splits`: NULL, or a split beside every job, into sel[0, nsel);
// `mix`: NULL, or the tables of a mix call with a mix set beside every job (never together with `splits`)
// `set`: NULL, or the tables of a set call with a set beside every job (with `mix`, without `wins`): the jobs read their members
// `sched`: NULL, or the tables of a scheduled call with a schedule beside every job (with `mix`, whose sets are not read; without
// `wins`, `splits`, `set`)
int iss_resample_plan(iss_ctx* c, const iss_resample_job* jobs, const iss_window* wins, int32_t njobs, int64_t src_bytes, int64_t nsig,
                      std::vector<std::pair<int64_t, int64_t>> ranges, const char* who, IssRsPlan& plan,
                      const iss_split* splits = nullptr, const int32_t* sel = nullptr, int64_t nsel = 0,
                      const IssMixTables* mix = nullptr, const IssSetTables* set = nullptr, const IssSchedTables* sched = nullptr);
int iss_resample_launch(iss_ctx* c, const uint8_t* dev_src, const IssRsPlan& plan);

// implemented in the .hip files
int iss_launch_sidekit(iss_ctx* c);
int iss_cnn_free(iss_ctx* c, int net_id);
int iss_enqueue_row_flags(iss_ctx* c);       // cnn.hip: row_flags_kernel over the resident features and its read-back, no wait
