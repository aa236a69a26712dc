// decode_pass.h: the host sequence the coded decoders and the raw resampler share.  No kernels here.
#include "decode_pass.h"
#include <algorithm>

int IssDecodePass::begin(iss_ctx* ctx, const char* name, int64_t n_sig, int32_t njobs) {
    c = ctx; who = name; n_signal = nsig = n_sig;
    ISS_HIP(c, hipSetDevice(c->device));
    if (n_signal < 0) {
        if (c->sig_kind != 1 || c->sig_ptr != c->sig.p)
            return iss_fail(c, ISS_ESTATE, "%s: n_signal < 0 needs a PCM16 signal uploaded by iss_signal_pcm16", who);
        nsig = c->sig_n;
    }
    stage_off.assign((size_t)njobs, -1);
    stage_bytes.assign((size_t)njobs, 0);
    stage_esz.assign((size_t)njobs, 0);
    return ISS_OK;
}

int IssDecodePass::place(int32_t j, const IssJobDst& d, int64_t frames_total, int32_t channels, int esz, bool signal_ok,
                         const char* only, bool& to_sig, int64_t& dst_byte, const iss_window* w) {
    iss_window full{0, frames_total, frames_total, 0, d.frames_out};
    if (w) {
        windowed = true;
        if (w->frames_total != frames_total || w->s_begin < 0 || w->s_begin >= w->s_end || w->s_end > frames_total)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: window [%lld, %lld) of %lld samples, the job has %lld", who, j,
                            (long long)w->s_begin, (long long)w->s_end, (long long)w->frames_total, (long long)frames_total);
        full = *w;
        frames_total = w->s_end - w->s_begin;              // what is placed from here on
    }
    const iss_split none{0, 0, 0};
    const iss_split& sp = jsplits ? jsplits[j] : none;
    if (jsplits) split = true;
    if (sp.sel_count != 0 && !(d.output == ISS_FLAC_TO_STAGE && d.filter >= 0))
        return iss_fail(c, ISS_EINVAL, "%s: job %d: a channel selection needs a TO_STAGE job with a filter", who, j);
    const iss_mixset nomix{0, 0, 0};
    const iss_mixset& ms = jmix ? jmix->sets[j] : nomix;
    if (ms.mix_count != 0 && !(d.output == ISS_FLAC_TO_STAGE && d.filter >= 0))
        return iss_fail(c, ISS_EINVAL, "%s: job %d: mixes need a TO_STAGE job with a filter", who, j);
    if (d.output == ISS_FLAC_TO_SIGNAL) {
        if (!signal_ok) return iss_fail(c, ISS_EINVAL, "%s: job %d: only %s sources go to the signal", who, j, only);
        if (d.dst_offset < 0 || d.dst_offset > nsig - frames_total)
            return iss_fail(c, ISS_EINVAL, "%s: job %d: output [%lld, %lld) outside the %lld-sample signal", who, j,
                            (long long)d.dst_offset, (long long)(d.dst_offset + frames_total), (long long)nsig);
        ranges.push_back({d.dst_offset, d.dst_offset + frames_total});
        to_sig = true;
        dst_byte = d.dst_offset * 2;
    } else if (d.output == ISS_FLAC_TO_STAGE) {
        to_sig = false;
        dst_byte = stage_off[(size_t)j] = stage;
        stage_bytes[(size_t)j] = frames_total * channels * esz;
        stage_esz[(size_t)j] = esz;
        stage += (stage_bytes[(size_t)j] + 15) / 16 * 16;
        if (d.filter >= 0) {
            iss_resample_job r{};
            r.src_offset = dst_byte; r.frames_in = frames_total; r.channels = channels;
            r.format = esz == 4 ? ISS_RS_I32 : ISS_RS_I16; r.filter = d.filter; r.dst_offset = d.dst_offset;
            r.frames_out = d.frames_out;
            rjobs.push_back(r);
            rwins.push_back(full);
            rsplits.push_back(sp);
            rmixsets.push_back(ms);
        }
    } else {
        return iss_fail(c, ISS_EINVAL, "%s: job %d: bad output %d", who, j, d.output);
    }
    return ISS_OK;
}

int IssDecodePass::commit(IssCodec* dec) {
    IssMixTables rmix{};                                   // the caller's mix and term rows, the sets beside rjobs
    if (jmix) { rmix = *jmix; rmix.sets = rmixsets.data(); }
    int rc = iss_resample_plan(c, rjobs.data(), windowed ? rwins.data() : nullptr, (int32_t)rjobs.size(), stage, nsig, ranges,
                               who, plan, split ? rsplits.data() : nullptr, sel, nsel, jmix ? &rmix : nullptr, jset, jsched);
    if (rc) return rc;
    if (n_signal >= 0) {                                   // a signal of its own, zero wherever no job writes
        if ((rc = iss_reserve(c, c->sig, (size_t)nsig * 2 + 16))) return rc;
        if (nsig > 0) ISS_HIP(c, hipMemsetAsync(c->sig.p, 0, (size_t)nsig * 2, c->stream));
    }
    iss_set_signal(c, c->sig.p, 1, nsig);                  // (n_signal < 0: what begin() found, written to from here on)
    if (dec) { dec->stage_off = stage_off; dec->stage_bytes = stage_bytes; dec->stage_esz = stage_esz; dec->held = 0; }      // (held again once finish() is through)
    return ISS_OK;
}

int iss_upload_payload(iss_ctx* c, DevBuf& b, const char* name, const void* src, int64_t bytes, size_t cap) {
    if (&b == &c->sv_src) c->sv_held.id = 0;               // whatever it held is being replaced
    if (int rc = iss_reserve(c, b, cap)) return rc;
    iss_prof_begin(c, ISS_PROF_OTHER, 0.0);
    iss_prof_inst(c, "%s_h2d(%lld B)", name, (long long)bytes);
    if (bytes > 0) ISS_HIP(c, hipMemcpyAsync(b.p, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    iss_prof_end(c);
    if (bytes > 0) { c->up_count.launches += 1; c->up_count.units += bytes; }
    return ISS_OK;
}

extern "C" int iss_upload_stats(iss_ctx* c, int64_t* copies, int64_t* bytes) {
    return iss_get_counters(c ? &c->up_count : nullptr, copies, bytes);
}

int iss_upload_rows(iss_ctx* c, DevBuf& b, const void* rows, size_t bytes) {
    if (int rc = iss_reserve(c, b, bytes)) return rc;
    void* pinned = nullptr;
    int slot = -1;
    if (int rc = iss_stage_host(c, rows, bytes, &pinned, &slot)) return rc;
    ISS_HIP(c, hipMemcpyAsync(b.p, pinned, bytes, hipMemcpyHostToDevice, c->stream));
    iss_stage_mark(c, slot);
    return ISS_OK;
}

int IssDecodePass::upload(IssCodec& dec, const void* payload, int64_t bytes, size_t cap, const void* rows, size_t row_bytes,
                          int64_t units) {
    int rc;
    if ((rc = iss_reserve(c, dec.src, cap))) return rc;
    if ((rc = iss_reserve(c, dec.rows, row_bytes))) return rc;
    if ((rc = iss_reserve(c, dec.status, (size_t)units * 4))) return rc;
    if ((rc = iss_reserve(c, dec.stage, (size_t)std::max<int64_t>(stage, 16)))) return rc;
    if ((rc = iss_upload_payload(c, dec.src, dec.name, payload, bytes, cap))) return rc;
    return iss_upload_rows(c, dec.rows, rows, row_bytes);
}

int IssDecodePass::finish(IssCodec& dec, int32_t* status_out, int64_t units) {
    ISS_HIP(c, hipMemcpyAsync(status_out, dec.status.p, (size_t)units * 4, hipMemcpyDeviceToHost, c->stream));
    dec.count.launches += 1;
    dec.count.units += units;
    dec.held = ++c->held_seq;
    return iss_resample_launch(c, (const uint8_t*)dec.stage.p, plan);     // (no rows: nothing launched)
}

int iss_codec_get_stage(iss_ctx* c, IssCodec& dec, int32_t job, void* out, int64_t bytes) {
    if (!out && bytes > 0) return iss_fail(c, ISS_EINVAL, "iss_%s_get_stage: bad argument", dec.name);
    if (job < 0 || job >= (int32_t)dec.stage_off.size() || dec.stage_off[(size_t)job] < 0)
        return iss_fail(c, ISS_EINVAL, "iss_%s_get_stage: job %d of the last iss_%s_decode did not go to the staging buffer",
                        dec.name, job, dec.name);
    if (bytes != dec.stage_bytes[(size_t)job])
        return iss_fail(c, ISS_EINVAL, "iss_%s_get_stage: job %d holds %lld bytes, not %lld", dec.name, job,
                        (long long)dec.stage_bytes[(size_t)job], (long long)bytes);
    ISS_HIP(c, hipSetDevice(c->device));
    if (bytes > 0)
        ISS_HIP(c, hipMemcpyAsync(out, (const uint8_t*)dec.stage.p + dec.stage_off[(size_t)job], (size_t)bytes,
                                  hipMemcpyDeviceToHost, c->stream));
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    return ISS_OK;
}

int iss_get_counters(const IssCounters* k, int64_t* launches, int64_t* units) {
    if (!k) return ISS_EINVAL;
    if (launches) *launches = k->launches;
    if (units) *units = k->units;
    return ISS_OK;
}
