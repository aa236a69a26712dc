// Stand-alone check of the host side of the channel survey (inaspeechsegmenter_amd/csrc/survey_plan.h): the chunk geometry and
// the job table the device reads, built for the host alone so that it can run under the sanitizers.  No GPU, no HIP.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/survey_plan_check.cpp -o survey_plan_check
//   ./survey_plan_check        -> "survey_plan_check: N checks passed", exit status 0
#include "../inaspeechsegmenter_amd/csrc/survey_plan.h"
#include <cstdlib>

static int checks = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        ++checks;                                                                           \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static iss_survey_job job(int64_t off, int64_t frames, int32_t ch, int32_t fmt, double full = 0.5) {
    iss_survey_job j{};
    j.src_offset = off; j.frames_in = frames; j.channels = ch; j.format = fmt; j.full = full;
    return j;
}

int main() {
    SvPlan plan;
    std::string err;

    // geometry: what every row of the workspace and of the results holds, and what the kernel's LDS carve needs
    CHECK(sv_row_words(1) == 6 && sv_row_words(2) == 13 && sv_row_words(16) == 96 + 120 && sv_row_words(17) == 102);
    CHECK(sv_pairs(16) == 120 && sv_pairs(17) == 0 && sv_pairs(1) == 0);
    CHECK(sv_stride(1) == SV_CHUNK && sv_stride(2) == SV_CHUNK + 8 && sv_stride(16) == SV_CHUNK + 1 && sv_stride(3) == SV_CHUNK + 5);
    CHECK(sv_lds_bytes(16) == sv_lds_bytes(1024) && sv_lds_bytes(16) <= 160 * 1024 && sv_lds_bytes(1) < sv_lds_bytes(2));
    CHECK(6 * SV_GROUP + sv_pairs(SV_GROUP) <= SV_THREADS);              // one thread per figure of a group
    CHECK(sv_fmt_bytes(ISS_RS_I16) == 2 && sv_fmt_bytes(ISS_RS_F64 | ISS_RS_SWAP) == 8 && sv_fmt_bytes(ISS_RS_ULAW) == 1);
    CHECK(sv_fmt_bytes(ISS_RS_U8 | ISS_RS_SWAP) == 0 && sv_fmt_bytes(5) == 0 && sv_fmt_bytes(-1) == 0 && sv_fmt_bytes(11) == 0);

    // a ragged call: prefix sums of chunks, workspace rows and result rows; every chunk edge
    const int64_t frames[] = {1, SV_CHUNK - 1, SV_CHUNK, SV_CHUNK + 1, 3 * SV_CHUNK + 17};
    const int32_t chans[] = {1, 2, 16, 17, 3};
    std::vector<iss_survey_job> jobs;
    int64_t bytes = 0;
    for (int k = 0; k < 5; ++k) {
        jobs.push_back(job(bytes, frames[k], chans[k], ISS_RS_I16));
        bytes += (frames[k] * chans[k] * 2 + 15) / 16 * 16;
    }
    CHECK(sv_plan(jobs.data(), nullptr, 5, bytes, nullptr, nullptr, plan, err));
    int64_t chunks = 0, ws = 0, res = 0;
    for (int k = 0; k < 5; ++k) {
        const SvJobDev& d = plan.dj[(size_t)k];
        CHECK(d.chunk_base == chunks && d.ws_off == ws && d.res_off == res && d.n == frames[k] && d.ch == chans[k]);
        CHECK(d.src_off == jobs[(size_t)k].src_offset && d.src_off + d.n * d.ch * 2 <= bytes);
        const int64_t c = (frames[k] + SV_CHUNK - 1) / SV_CHUNK;
        chunks += c; ws += c * sv_row_words(chans[k]); res += sv_row_words(chans[k]);
    }
    CHECK(plan.chunks == chunks && chunks == 1 + 1 + 1 + 2 + 4 && plan.ws_words == ws && plan.res_words == res);
    CHECK(plan.max_row == 216 && plan.lds == sv_lds_bytes(16));

    // windows: the surveyed frames inside the staged ones, the offset in bytes
    iss_window w{100, 100 + 3000, 5000, 1100, 1500};
    iss_survey_job one = job(64, 3000, 3, ISS_RS_I32);
    CHECK(sv_plan(&one, &w, 1, 64 + 3000 * 3 * 4, nullptr, nullptr, plan, err));
    CHECK(plan.dj[0].src_off == 64 + 1000 * 3 * 4 && plan.dj[0].n == 1500 && plan.chunks == 2);
    w.out_count = 2001;                                                  // one frame past the staged ones
    CHECK(!sv_plan(&one, &w, 1, 64 + 3000 * 3 * 4, nullptr, nullptr, plan, err) && err.find("job 0") == 0);
    w = iss_window{100, 3100, 5000, 99, 10};
    CHECK(!sv_plan(&one, &w, 1, 64 + 3000 * 3 * 4, nullptr, nullptr, plan, err));
    w = iss_window{100, 3101, 5000, 100, 10};                            // states one frame more than the job holds
    CHECK(!sv_plan(&one, &w, 1, 64 + 3000 * 3 * 4, nullptr, nullptr, plan, err));
    w = iss_window{2100, 5100, 5000, 2100, 10};                          // past the end of the file
    CHECK(!sv_plan(&one, &w, 1, 64 + 3000 * 3 * 4, nullptr, nullptr, plan, err));

    // refusals of a row
    iss_survey_job bad = job(0, 10, 2, ISS_RS_I16);
    CHECK(sv_plan(&bad, nullptr, 1, 40, nullptr, nullptr, plan, err));
    CHECK(!sv_plan(&bad, nullptr, 1, 39, nullptr, nullptr, plan, err));    // one byte short
    bad.src_offset = 1;
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));    // misaligned
    bad = job(0, 0, 2, ISS_RS_I16);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));
    bad = job(0, 10, 0, ISS_RS_I16);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));
    bad = job(0, 10, 1025, ISS_RS_U8);
    CHECK(!sv_plan(&bad, nullptr, 1, 1 << 20, nullptr, nullptr, plan, err));
    bad = job(0, 10, 2, 7);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));
    bad = job(0, 10, 2, ISS_RS_I16, 0.0);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));
    bad = job(0, 10, 2, ISS_RS_I16, NAN);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));
    bad = job(0, (int64_t(1) << 40), 2, ISS_RS_I16);
    CHECK(!sv_plan(&bad, nullptr, 1, INT64_MAX, nullptr, nullptr, plan, err));
    bad = job(-2, 10, 2, ISS_RS_I16);
    CHECK(!sv_plan(&bad, nullptr, 1, 64, nullptr, nullptr, plan, err));

    // the codec entries: src_offset is the index of a staged job
    const std::vector<int64_t> off{0, -1, 4096}, sz{4000, 0, 2 * 500 * 4};
    iss_survey_job st = job(2, 500, 2, ISS_RS_I32);
    CHECK(sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err) && plan.dj[0].src_off == 4096);
    st.src_offset = 1;
    CHECK(!sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err));            // not staged
    st.src_offset = 3;
    CHECK(!sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err));            // no such job
    st = job(0, 500, 2, ISS_RS_I32);
    CHECK(sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err) && plan.dj[0].src_off == 0);      // exactly the 4 000 bytes staged
    st = job(0, 501, 2, ISS_RS_I32);
    CHECK(!sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err));
    st = job(2, 1000, 2, ISS_RS_F32);
    CHECK(!sv_plan(&st, nullptr, 1, 0, &off, &sz, plan, err));            // a decoder stages integers

    // file sets: a job's channels resolved to its members; every refusal names the job and leaves no row behind
    {
        const iss_set_member mem[] = {{0, 3000, 1, 0}, {6000, 2000, 2, 0}, {14000, 1, 1, 0}};
        const iss_set two{0, 2}, three{0, 3};
        iss_survey_job sj = job(0, 3000, 3, ISS_RS_I16);
        CHECK(sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, mem, 3));
        CHECK(plan.chans.size() == 3 && plan.dj[0].src_off == 0 && plan.dj[0].n == 3000 && plan.chunks == 3);
        CHECK(plan.chans[0].off == 0 && plan.chans[0].frames == 3000 && plan.chans[0].step == 1);
        CHECK(plan.chans[1].off == 6000 && plan.chans[2].off == 6002 && plan.chans[2].frames == 2000 && plan.chans[2].step == 2);
        iss_survey_job both[2] = {sj, job(0, 3000, 4, ISS_RS_I16)};
        const iss_set rows[2] = {two, three};
        CHECK(sv_plan(both, nullptr, 2, 14002, nullptr, nullptr, plan, err, rows, mem, 3));
        CHECK(plan.chans.size() == 7 && plan.dj[1].src_off == 3 && plan.chans[6].off == 14000 && plan.chans[6].frames == 1);
        CHECK(!sv_plan(both, nullptr, 2, 14001, nullptr, nullptr, plan, err, rows, mem, 3) && err.find("job 1: member 2") == 0);
        CHECK(!sv_plan(&sj, nullptr, 1, 13999, nullptr, nullptr, plan, err, &two, mem, 3) && err.find("job 0: member 1") == 0);
        const iss_set none{0, 0}, past{2, 2}, before{-1, 2};
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &none, mem, 3) && err.find("job 0: member rows") == 0);
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &past, mem, 3));
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &before, mem, 3));
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, nullptr, 0));
        iss_survey_job off1 = job(2, 3000, 3, ISS_RS_I16), fewer = job(0, 2999, 3, ISS_RS_I16), wider = job(0, 3000, 4, ISS_RS_I16);
        CHECK(!sv_plan(&off1, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, mem, 3));
        CHECK(!sv_plan(&fewer, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, mem, 3));
        CHECK(!sv_plan(&wider, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, mem, 3));
        const iss_set_member odd[] = {{1, 3000, 1, 0}, {6000, 2000, 2, 0}}, empty[] = {{0, 3000, 1, 0}, {6000, 0, 2, 0}};
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, odd, 2));      // misaligned
        CHECK(!sv_plan(&sj, nullptr, 1, 14000, nullptr, nullptr, plan, err, &two, empty, 2));
        iss_window w0{0, 3000, 3000, 0, 3000};
        CHECK(!sv_plan(&sj, &w0, 1, 14000, nullptr, nullptr, plan, err, &two, mem, 3));           // whole sets only
    }

    // no jobs; many chunks
    CHECK(sv_plan(nullptr, nullptr, 0, 0, nullptr, nullptr, plan, err) && plan.dj.empty() && plan.chunks == 0);
    iss_survey_job big = job(0, (int64_t(1) << 40) / 2, 1, ISS_RS_I16);
    CHECK(sv_plan(&big, nullptr, 1, int64_t(1) << 40, nullptr, nullptr, plan, err) && plan.chunks == (int64_t(1) << 29));
    iss_survey_job bigs[5] = {big, big, big, big, big};
    bigs[0].frames_in = (int64_t(1) << 40);
    bigs[0].format = ISS_RS_U8;
    CHECK(sv_plan(bigs, nullptr, 1, int64_t(1) << 40, nullptr, nullptr, plan, err) && plan.chunks == (int64_t(1) << 30));
    for (auto& b : bigs) { b.frames_in = int64_t(1) << 39; b.format = ISS_RS_U8; b.src_offset = 0; }
    CHECK(!sv_plan(bigs, nullptr, 5, int64_t(1) << 40, nullptr, nullptr, plan, err));      // past 2^31 - 1 blocks in one grid

    // survey blocks (include/iss.h): K chunks a block, the last shorter; units = blocks x groups of SV_THREADS words; rows per job
    {
        const iss_survey_job jb[3] = {job(0, 5 * SV_CHUNK + 1, 2, ISS_RS_I16), job(40000, 1, 17, ISS_RS_I16), job(50000, 4 * SV_CHUNK, 1024, ISS_RS_U8)};
        const int32_t ks[3] = {2, 3, 4}, zero[3] = {2, 0, 4}, neg[3] = {-1, 3, 4};
        const int64_t nbytes = 50000 + 4 * SV_CHUNK * 1024;
        CHECK(sv_plan(jb, nullptr, 3, nbytes, nullptr, nullptr, plan, err, nullptr, nullptr, 0, ks) && plan.blk.size() == 3);
        CHECK(plan.blk[0].K == 2 && plan.blk[0].wgroups == 1 && plan.blk[0].unit_base == 0 && plan.blk[0].out_off == 0);      // 6 chunks: 3 blocks
        CHECK(plan.blk[1].unit_base == 3 && plan.blk[1].out_off == 3 * 13 && plan.blk[1].wgroups == 1);                          // 1 chunk: 1 block
        CHECK(plan.blk[2].unit_base == 4 && plan.blk[2].out_off == 3 * 13 + 102 && plan.blk[2].wgroups == 6 * 1024 / SV_THREADS);  // 1 block
        CHECK(plan.blk_units == 4 + 24 && plan.blk_words == 3 * 13 + 102 + 6 * 1024 && plan.res_words == 13 + 102 + 6 * 1024);
        CHECK(!sv_plan(jb, nullptr, 3, nbytes, nullptr, nullptr, plan, err, nullptr, nullptr, 0, zero) && err.find("job 1: block_chunks 0") == 0);
        CHECK(!sv_plan(jb, nullptr, 3, nbytes, nullptr, nullptr, plan, err, nullptr, nullptr, 0, neg) && err.find("job 0: block_chunks -1") == 0);
        const iss_window w[3] = {{0, 5 * SV_CHUNK + 1, 5 * SV_CHUNK + 1, 0, 10}, {0, 1, 1, 0, 1}, {0, 4 * SV_CHUNK, 4 * SV_CHUNK, 0, 5}};
        CHECK(!sv_plan(jb, w, 3, nbytes, nullptr, nullptr, plan, err, nullptr, nullptr, 0, ks));      // no windows with blocks
        CHECK(sv_plan(jb, nullptr, 3, nbytes, nullptr, nullptr, plan, err) && plan.blk.empty() && plan.blk_units == 0);
    }

    printf("survey_plan_check: %d checks passed\n", checks);
    return 0;
}
