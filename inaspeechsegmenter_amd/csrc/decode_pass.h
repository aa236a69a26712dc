// The host side of one decode pass, shared by iss_flac_decode, iss_adpcm_decode and iss_resample_pcm16 (not part of the ABI).
//
// An entry point reads: begin, validate my rows (place each job), commit, upload, MY LAUNCH, finish.  Everything before
// commit() returns ISS_OK is host work on the pass's own vectors: a refused call leaves the context and the device as they were.
#pragma once
#include "iss_internal.h"

static_assert(ISS_FLAC_TO_SIGNAL == ISS_ADPCM_TO_SIGNAL && ISS_FLAC_TO_STAGE == ISS_ADPCM_TO_STAGE, "one placement for both");

struct IssJobDst { int32_t output, filter; int64_t dst_offset, frames_out; };   // the tail iss_flac_job and iss_adpcm_job share

struct IssDecodePass {
    iss_ctx* c = nullptr;
    const char* who = "";                  // the entry point's name: every error text starts with it
    int64_t n_signal = -1, nsig = 0;       // as given, and the length of the signal the jobs write into
    std::vector<std::pair<int64_t, int64_t>> ranges;          // signal ranges of the TO_SIGNAL jobs
    std::vector<iss_resample_job> rjobs;                      // one per TO_STAGE job with a filter: reads the staging buffer
    std::vector<iss_window> rwins;                            // beside rjobs (a whole-file window for a job without one) ...
    bool windowed = false;                                    // ... and handed to the planner only when the call has windows
    const iss_split* jsplits = nullptr;                       // a split entry point's rows, one per JOB (NULL: the plain call) ...
    std::vector<iss_split> rsplits;                           // ... handed on beside rjobs (no selection for a job without one) ...
    bool split = false;                                       // ... and to the planner only when the call has splits,
    const int32_t* sel = nullptr;                             // with the caller's channel selection table
    int64_t nsel = 0;
    const IssMixTables* jmix = nullptr;                       // a mix entry point's tables, `sets` one per JOB (NULL: not one) ...
    std::vector<iss_mixset> rmixsets;                         // ... the sets handed on beside rjobs (no mixes for a job without any)
    const IssSetTables* jset = nullptr;                       // a set entry point's tables, `sets` one per job = per row of rjobs (NULL: not one)
    const IssSchedTables* jsched = nullptr;                   // a scheduled entry point's tables, `scheds` one per row of rjobs (NULL: not one)
    std::vector<int64_t> stage_off, stage_bytes;              // per job (-1: not staged)
    std::vector<int32_t> stage_esz;                           // per job: bytes of a staged sample
    int64_t stage = 0;                                        // bytes those rows read from: the staging buffer so far
    IssRsPlan plan;

    // hipSetDevice and the signal rule: n_signal < 0 needs the context's own PCM16 upload (else ISS_ESTATE)
    int begin(iss_ctx* ctx, const char* name, int64_t n_sig, int32_t njobs);
    // Job j: frames_total x channels samples of esz (2 or 4) bytes.  TO_SIGNAL, where signal_ok (`only` names who may, for the
    // error text): range checked and recorded.  TO_STAGE: the next 16-byte aligned staging offset, and with a filter the
    // resample row reading it.  -> to_sig, and dst_byte into the signal / the staging buffer
    // `w` (NULL: the whole file): the job produces samples [s_begin, s_end) only, and that many are placed; dst_byte is where
    // sample s_begin goes.  Checked here: the window lies inside the file and states the job's frames_total.
    // A job's split (jsplits) goes to its resample row; a selection on a job without one (TO_SIGNAL, or no filter) is refused.
    // Likewise a job's mix set (jmix).
    int place(int32_t j, const IssJobDst& d, int64_t frames_total, int32_t channels, int esz, bool signal_ok, const char* only,
              bool& to_sig, int64_t& dst_byte, const iss_window* w = nullptr);
    // Plans rjobs against the recorded ranges, then changes the context: a zeroed signal of its own for n_signal >= 0, features
    // stale, and the stage tables of `dec` (NULL: the raw resampler, whose rjobs are the caller's rows and `stage` its source bytes)
    int commit(IssCodec* dec);
    // payload (bytes of it, into a buffer of cap bytes: the kernel's reads past the end are the decoder's to size), row table,
    // `units` status entries, staging buffer;  then, after the decoder's launch: status back, counters, the resample launch
    int upload(IssCodec& dec, const void* payload, int64_t bytes, size_t cap, const void* rows, size_t row_bytes, int64_t units);
    int finish(IssCodec& dec, int32_t* status_out, int64_t units);
};

int iss_upload_payload(iss_ctx* c, DevBuf& b, const char* name, const void* src, int64_t bytes, size_t cap);   // bracketed "<name>_h2d(n B)"
int iss_upload_rows(iss_ctx* c, DevBuf& b, const void* rows, size_t bytes);        // through a pinned staging buffer
int iss_codec_get_stage(iss_ctx* c, IssCodec& dec, int32_t job, void* out, int64_t bytes);      // texts: iss_<dec.name>_get_stage
int iss_get_counters(const IssCounters* k, int64_t* launches, int64_t* units);     // k == NULL: ISS_EINVAL
