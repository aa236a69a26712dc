/* iss.h -- C ABI of the MI355X-native inaSpeechSegmenter hot path (libiss_hip.so).
 *
 * The reference (ina-foss/inaSpeechSegmenter) has NO native/FFI boundary: its hot
 * path is numpy + TensorFlow/Keras + onnxruntime called from Python.  The entry
 * points below are what a ctypes binding inside the reference's own modules would
 * call instead; each one cites the reference interface it replaces (paths are
 * relative to the reference repo root, inaSpeechSegmenter/<file>:<line>).
 * INTEGRATION.md shows the reference-side ctypes stub.
 *
 * Conventions
 *   - plain C types only; no torch / numpy types cross this boundary.
 *   - every function returns 0 on success, a negative ISS_E* code on failure;
 *     iss_last_error(ctx) (ctx may be NULL for creation errors) gives the text.
 *   - the caller owns every host buffer; the library owns all device memory,
 *     streams and events and frees them in iss_destroy().
 *   - one context per (device, host thread); a context is not thread-safe.
 *   - there is NO CPU fallback: device entry points fail with ISS_ENODEV when no
 *     gfx950 device is usable.  The host-only helpers (iss_viterbi_*) need no GPU.
 */
#ifndef ISS_H
#define ISS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISS_OK        0
#define ISS_EINVAL   -1   /* bad argument / bad program                         */
#define ISS_ENODEV   -2   /* no usable HIP device                               */
#define ISS_EHIP     -3   /* a HIP runtime call failed (text in last_error)     */
#define ISS_ESTATE   -4   /* call order violated (e.g. features before signal)  */
#define ISS_ENOMEM   -5
#define ISS_ETIMEOUT -6   /* a collective did not complete (peer rank gone): communicator aborted */

typedef struct iss_ctx iss_ctx;

/* ------------------------------------------------------------------ context */
int         iss_create(int device_id, iss_ctx** out);
void        iss_destroy(iss_ctx* ctx);
const char* iss_last_error(const iss_ctx* ctx);
const char* iss_version(void);
/* Cap (bytes) on the activation workspace of the CNN engine; decides how many
 * 20 ms slots are pushed through the layer stack per pass.  Default 24 GiB.    */
int         iss_set_workspace_limit(iss_ctx* ctx, uint64_t bytes);
int         iss_synchronize(iss_ctx* ctx);

/* ---------------------------------------------------- SIDEKIT log-mel front end
 * replaces sidekit_mfcc.py:278-352 `mfcc(sig, get_mspec=True)` as called from
 * segmenter.py:58 (framing 400/160, per-frame pre-emphasis, log-energy, Hann,
 * rfft-512 in float64, 24-band mel, log).                                      */

/* Constant tables (built by the host mirror with the reference's formulas):
 * window  = numpy.hanning(400) float64         (sidekit_mfcc.py:223)
 * melbank = trfbank(16000,512,100,8000,0,24)[0], (24,257) float32 row-major
 *           (sidekit_mfcc.py:118-197,332).                                     */
int iss_sidekit_tables(iss_ctx* ctx, const double* window400, const float* melbank_24x257);

/* Hand a decoded 16 kHz mono signal to the device (host -> HBM copy).
 * pcm16: what `ffmpeg -acodec pcm_s16le` produces (io.py:61-68); converted on the
 * device as x/32768 exactly like libsndfile's float read (io.py:77).
 * f32  : what soundfile hands back for float WAVs (io.py:52).                  */
int iss_signal_pcm16(iss_ctx* ctx, const int16_t* pcm, int64_t n);
int iss_signal_f32(iss_ctx* ctx, const float* sig, int64_t n);
/* Same, but the samples are ALREADY in device memory (hipMalloc'ed pointer, e.g. a
 * torch tensor's data_ptr); no copy, the buffer must outlive the feature call.
 * ORDERING CONTRACT: the library works on its own non-blocking stream.  The call makes that
 * stream wait (hipStreamWaitEvent) for everything submitted so far to `producer_stream`
 * (a hipStream_t; NULL = the legacy default stream, which is what torch uses unless the
 * caller switched streams), so a tensor produced there -- async H2D copy, kernel output --
 * is complete before the front end reads it.  Work the caller submits to OTHER streams is
 * the caller's to synchronise.  The pointer must belong to the context's device
 * (checked with hipPointerGetAttributes; ISS_EINVAL otherwise).                         */
int iss_signal_pcm16_device(iss_ctx* ctx, const void* dev_pcm, int64_t n);
int iss_signal_pcm16_device_stream(iss_ctx* ctx, const void* dev_pcm, int64_t n, void* producer_stream);

/* WAV sources at other rates / channel counts without ffmpeg: replaces the 16 kHz-only assertion of the ffmpeg-free
 * read (io.py:53-55) with what `ffmpeg -ac 1 -ar 16000 -acodec pcm_s16le` is asked for, on the device:
 *   m[j] = mean over channels of the stored sample scaled like libsndfile (u8 (x-128)/128, i16 x/2^15, i32 x/2^31,
 *          f32 / f64 as stored), float64, channels summed in order then divided by their count;
 *   y[i] = sum over ascending j of taps[i*down + hl - j*up] * m[j]   (taps in [0, 2*hl], j in [0, frames_in), float64,
 *          no fused multiply-add), i < frames_out = ceil(frames_in*up/down): scipy.signal.resample_poly(m, up, down);
 *   pcm  = clip(rint(y * 32768), -32768, 32767)   (round half to even, saturate: ffmpeg's pcm_s16le).
 * The filter of a (up, down) pair is registered once per context: `taps` = 2*hl+1 float64, hl = (ntaps-1)/2
 * (inaspeechsegmenter_amd/resample.py designs it); a second registration of the same pair returns the same id and
 * copies nothing.  ntaps 1 with up = down = 1 is the identity (16 kHz sources with several channels).               */
#define ISS_RS_U8   0
#define ISS_RS_I16  1
#define ISS_RS_I32  2     /* 32-bit PCM, and 24-bit PCM widened to x << 8 */
#define ISS_RS_F32  3
#define ISS_RS_F64  4
/* (5 .. 7 are not formats: refused)                                                                                  */
#define ISS_RS_I8   8     /* signed 8-bit (AIFF, AU, CAF): reads like the unsigned 8-bit WAV holding x + 128               */
#define ISS_RS_ULAW 9     /* G.711 mu-law byte b: u = ~b & 0xFF, t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7),
                             value 0x84 - t if u & 0x80 else t - 0x84; reads like the PCM16 WAV holding the value         */
#define ISS_RS_ALAW 10    /* G.711 A-law byte b: a = b ^ 0x55, t = (a & 15) << 4, s = (a >> 4) & 7; s == 0: t += 8,
                             s == 1: t += 0x108, s > 1: t = (t + 0x108) << (s - 1); value t if a & 0x80 else -t           */
#define ISS_RS_SWAP 0x100 /* or-ed onto a 2-, 4- or 8-byte format: the samples are stored big-endian (AIFF, AU, CAF)      */
typedef struct {
    int64_t src_offset;   /* byte offset of the job's first stored sample in `src` (a multiple of the sample size)   */
    int64_t frames_in;    /* frames (samples per channel) of the source, >= 1                                        */
    int32_t channels;     /* interleaved channels, 1 .. 1024                                                         */
    int32_t format;       /* ISS_RS_*, | ISS_RS_SWAP for big-endian samples                                          */
    int32_t filter;       /* id returned by iss_resample_filter                                                      */
    int32_t reserved;     /* 0                                                                                       */
    int64_t dst_offset;   /* first output sample in the resident signal                                              */
    int64_t frames_out;   /* must be ceil(frames_in * up / down)                                                     */
} iss_resample_job;
int iss_resample_filter(iss_ctx* ctx, int32_t up, int32_t down, const double* taps, int64_t ntaps, int32_t* id_out);
/* One H2D copy of `src` (src_bytes bytes: the stored samples of every job) and ONE kernel launch for all jobs, the
 * PCM16 output written into the resident signal at each job's dst_offset.
 *   n_signal >= 0: the resident signal becomes a new zero-filled PCM16 signal of n_signal samples first (a call on its own);
 *   n_signal <  0: the jobs write into the PCM16 signal uploaded by the last iss_signal_pcm16 (a packed batch with room
 *                  left for the resampled files); every sample outside the jobs' ranges stays as uploaded.
 * Then iss_sidekit runs as on any uploaded signal.  `src` is read asynchronously: from page-locked memory
 * (iss_host_alloc) it must stay unchanged until the next synchronising call (iss_get_loge, iss_synchronize, ...).
 * ISS_EINVAL: bad format (ISS_RS_SWAP on a one-byte format included) or channel count, unknown filter, frames_out not ceil(frames_in*up/down), a source range outside
 * `src` or misaligned, a destination range outside the signal, or two destination ranges that overlap.
 * ISS_ESTATE: n_signal < 0 without a resident PCM16 signal of the context's own (iss_signal_pcm16).                  */
int iss_resample_pcm16(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                       int64_t n_signal);
/* Samples [offset, offset + n) of the resident PCM16 signal back to the host (e.g. the output of iss_resample_pcm16).  */
int iss_get_signal_pcm16(iss_ctx* ctx, int16_t* out, int64_t offset, int64_t n);
/* Resample kernel launches and jobs since the context was created.                                                   */
int iss_resample_stats(iss_ctx* ctx, int64_t* launches, int64_t* jobs);

/* FLAC sources without ffmpeg (the reference reads them with soundfile.read, io.py:36-55).  The decode contract: every
 * sample of a frame is what RFC 9639 defines (subframes CONSTANT / VERBATIM / FIXED 0-4 / LPC 1-32 with wasted bits, Rice /
 * Rice2 residuals with escapes, left/side, side/right and mid/side decorrelation), written in the stored format of the
 * file's WAV twin: int16 for 8- and 16-bit streams (8-bit widened x << 8), int32 x << 8 for 24-bit streams, channels
 * interleaved.  12/20/32-bit streams are not decoded.
 * iss_flac_index (host, no context): the frames of one stream.  buf[first_frame] is the first frame's sync code (after the
 * metadata blocks, which the caller parses into `info`); a frame is a sync code whose header parses, passes its CRC-8, matches
 * STREAMINFO (rate, channels, sample size, block size <= max_block) and continues the frame / sample numbering; it runs to
 * the next such frame or to the end of `buf`.  A sync pattern inside frame data is rejected by the numbering; the CRC-16 of
 * the decode is the final word.  -> ISS_OK with *nframes rows; ISS_EINVAL with the frame's byte offset in *err_offset and
 * the reason in err (bad header, CRC-8, frame-sequence break, truncated frame, a nonzero STREAMINFO total that differs from
 * the frames' sum); ISS_ENOMEM when more than `cap` frames were found (*nframes = cap: call again with more room).       */
typedef struct {
    int32_t sample_rate, channels, bps;   /* STREAMINFO                                                                 */
    int32_t min_block, max_block;         /* STREAMINFO block sizes (max_block 0: not checked)                          */
    int32_t reserved;                     /* 0                                                                          */
    int64_t total_samples;                /* samples per channel, 0 = unknown                                           */
} iss_flac_info;
typedef struct {
    int64_t offset;        /* byte offset of the frame's sync code                                                      */
    int64_t length;        /* bytes, CRC-16 footer included                                                            */
    int64_t first_sample;  /* per channel: the frames of a stream tile [0, total) in order                             */
    int32_t block_size;    /* samples per channel                                                                       */
    int32_t channel_mode;  /* 0..7: channel_mode + 1 independent channels; 8 left/side, 9 side/right, 10 mid/side      */
    int32_t bps;           /* 8, 16 or 24 (12, 20, 32 are indexed but not decoded)                                     */
    int32_t header_bytes;  /* frame header, CRC-8 included: the first subframe starts after it                         */
} iss_flac_frame;
int iss_flac_index(const uint8_t* buf, int64_t len, int64_t first_frame, const iss_flac_info* info, iss_flac_frame* frames,
                   int64_t cap, int64_t* nframes, int64_t* err_offset, char* err, int32_t err_len);
/* CRC-8 (poly 0x07) and CRC-16 (poly 0x8005), both init 0, unreflected, of buf[0, n) (host, no context).              */
int iss_flac_crc(const uint8_t* buf, int64_t n, int32_t* crc8_out, int32_t* crc16_out);
/* Frame status codes (status_out of the decoders): 0 = decoded and CRC-16 verified, else the first violation met.     */
#define ISS_FLAC_OK               0
#define ISS_FLAC_SUBFRAME_TYPE    1   /* reserved subframe type (or FIXED order > 4)                                   */
#define ISS_FLAC_PAD_BIT          2   /* subframe header's zero bit set                                                */
#define ISS_FLAC_WASTED           3   /* wasted bits >= the subframe's sample size                                     */
#define ISS_FLAC_RESIDUAL_METHOD  4   /* reserved residual coding method                                               */
#define ISS_FLAC_PARTITION        5   /* partition order does not divide the block, or predictor order > partition 0  */
#define ISS_FLAC_LPC_PRECISION    6   /* LPC coefficient precision code 1111                                           */
#define ISS_FLAC_LPC_SHIFT        7   /* negative LPC shift                                                            */
#define ISS_FLAC_OVERRUN          8   /* subframes run past the CRC-16 footer                                          */
#define ISS_FLAC_PADDING          9   /* nonzero byte-alignment padding                                                */
#define ISS_FLAC_FOOTER          10   /* subframes end before the CRC-16 footer                                        */
#define ISS_FLAC_CRC16           11   /* CRC-16 mismatch                                                               */
/* The host build of the decoder: every row of one stream (rows of iss_flac_index, offsets into buf) into `out`
 * (frames_total * channels samples of the stored format above), status_out[k] = ISS_FLAC_* of row k.  ISS_EINVAL (nothing
 * decoded) when a row lies outside buf, the rows do not tile [0, frames_total), or their channels / bps differ.          */
int iss_flac_decode_host(const uint8_t* buf, int64_t len, const iss_flac_frame* frames, int64_t nframes, int32_t channels,
                         int32_t bps, int64_t frames_total, void* out, int32_t* status_out);
#define ISS_FLAC_TO_SIGNAL  0   /* mono 8/16-bit at 16 kHz: PCM16 straight into the resident signal at dst_offset        */
#define ISS_FLAC_TO_STAGE   1   /* stored-format samples into the context's staging buffer (iss_flac_get_stage), and with
                                   filter >= 0 resampled from there into the resident signal like an iss_resample_job    */
typedef struct {
    int64_t src_offset;    /* byte offset in `src` that the job's frame offsets are relative to                        */
    int64_t frame_begin;   /* the job's rows of `frames`: [frame_begin, frame_begin + nframes)                         */
    int64_t nframes;
    int64_t frames_total;  /* samples per channel                                                                       */
    int32_t channels;      /* 1 .. 8                                                                                     */
    int32_t bps;           /* 8, 16 or 24                                                                                */
    int32_t output;        /* ISS_FLAC_TO_SIGNAL / ISS_FLAC_TO_STAGE                                                     */
    int32_t filter;        /* TO_STAGE: iss_resample_filter id, or -1 (decode only)                                     */
    int64_t dst_offset;    /* TO_SIGNAL, or TO_STAGE with a filter: first output sample in the resident signal          */
    int64_t frames_out;    /* TO_STAGE with a filter: ceil(frames_total * up / down)                                    */
} iss_flac_job;
/* One H2D copy of `src` (the compressed frames of every job), ONE launch of flac_decode_kernel (one lane per frame, every
 * frame of every job), and when some TO_STAGE job has a filter ONE launch of the resample kernel reading the staging
 * buffer.  n_signal as for iss_resample_pcm16 (>= 0: a new zero-filled signal; < 0: into the last iss_signal_pcm16 upload,
 * every sample outside the jobs' ranges stays as uploaded).  The staging buffer holds the TO_STAGE jobs in job order, each
 * at a multiple of 16 bytes.  status_out[k] (nframes int32, page-locked memory recommended) receives the ISS_FLAC_* code
 * of row k asynchronously: it is valid after the next synchronising call (iss_get_loge, iss_flac_get_stage,
 * iss_synchronize, ...), so a pass reads it with its log-energy.  A frame with a nonzero status leaves garbage in its own
 * output range only.  ISS_EINVAL (nothing launched): rows outside `src` or not tiling [0, frames_total) in order, a row in
 * no job or in two, bad channels / bps / output, a TO_SIGNAL job that is not mono 8/16-bit, destination ranges outside the
 * signal or overlapping, a resample job that iss_resample_pcm16 would refuse.  ISS_ESTATE: as iss_resample_pcm16.     */
int iss_flac_decode(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                    const iss_flac_job* jobs, int32_t njobs, int64_t n_signal, int32_t* status_out);
/* The stored-format samples of TO_STAGE job `job` of the last iss_flac_decode (bytes = frames_total * channels * 2 or 4)
 * back to the host; synchronises.                                                                                       */
int iss_flac_get_stage(iss_ctx* ctx, int32_t job, void* out, int64_t bytes);
/* FLAC decode launches and frames since the context was created.                                                     */
int iss_flac_stats(iss_ctx* ctx, int64_t* launches, int64_t* frames);

/* IMA ADPCM in WAV (format tag 0x11) without ffmpeg.  A block of `block_align` bytes holds, per channel, a 4-byte header
 * (int16 predictor = the block's first sample, uint8 step index <= 88, one reserved byte) and then 4-byte words interleaved
 * by channel, 8 nibbles each, low nibble first: samples_per_block = (block_align / channels - 4) * 2 + 1.  A nibble n moves
 * the state by the standard 89-entry step table:  step = table[idx]; d = step >> 3; n&1: d += step >> 2; n&2: d += step >> 1;
 * n&4: d += step; pred = clamp16(n&8 ? pred - d : pred + d); idx = clamp(idx + {-1,-1,-1,-1,2,4,6,8}[n&7], 0, 88).  The
 * decoded samples are PCM16, channels interleaved: the file reads like the PCM16 WAV holding them.                       */
#define ISS_ADPCM_OK          0
#define ISS_ADPCM_STEP_INDEX  1   /* a channel header's step index is above 88 (decoded from 88: garbage in that block only) */
#define ISS_ADPCM_TO_SIGNAL   0   /* mono at 16 kHz: PCM16 straight into the resident signal at dst_offset                  */
#define ISS_ADPCM_TO_STAGE    1   /* interleaved PCM16 into the context's staging buffer (iss_adpcm_get_stage), and with
                                     filter >= 0 resampled from there into the resident signal like an iss_resample_job    */
typedef struct {
    int64_t src_offset;    /* byte offset of the job's first block in `src`, a multiple of 4                             */
    int64_t block_begin;   /* the job's rows of the status array: [block_begin, block_begin + nblocks)                   */
    int64_t nblocks;       /* whole blocks, >= 1                                                                          */
    int64_t frames_total;  /* samples per channel, in ((nblocks - 1) * samples_per_block, nblocks * samples_per_block]     */
    int32_t channels;      /* 1 .. 64                                                                                     */
    int32_t block_align;   /* bytes per block: a multiple of 4 * channels, > 4 * channels, at most 32768 (iss_msadpcm_*:
                              the Microsoft geometry stated with those entry points)                                      */
    int32_t output;        /* ISS_ADPCM_TO_SIGNAL / ISS_ADPCM_TO_STAGE                                                    */
    int32_t filter;        /* TO_STAGE: iss_resample_filter id, or -1 (decode only)                                      */
    int64_t dst_offset;    /* TO_SIGNAL, or TO_STAGE with a filter: first output sample in the resident signal           */
    int64_t frames_out;    /* TO_STAGE with a filter: ceil(frames_total * up / down)                                     */
} iss_adpcm_job;
/* The host build of the decoder (no context): the blocks of one stream into out (frames_total * channels int16),
 * status_out[k] = ISS_ADPCM_* of block k.  ISS_EINVAL (nothing decoded): blocks outside buf or a bad geometry.           */
int iss_adpcm_decode_host(const uint8_t* buf, int64_t len, int64_t nblocks, int32_t channels, int32_t block_align,
                          int64_t frames_total, int16_t* out, int32_t* status_out);
/* One H2D copy of `src` (the blocks of every job), ONE launch of adpcm_decode_kernel over the blocks of every job (a wave
 * per block: lane c walks channel c's predictor chain into LDS, the wave then stores the block's interleaved samples
 * coalesced), and when some TO_STAGE job has a filter ONE launch of the resample kernel reading the staging buffer.
 * n_signal as for iss_resample_pcm16.  The staging buffer holds the TO_STAGE jobs in job order, each at a multiple of 16
 * bytes.  The jobs' status rows must tile [0, nblocks_total) in job order.  status_out (nblocks_total int32, page-locked
 * memory recommended) is written asynchronously: valid after the next synchronising call (iss_get_loge,
 * iss_adpcm_get_stage, iss_synchronize, ...).  ISS_EINVAL (nothing launched): a bad geometry, blocks outside `src`,
 * status rows that do not tile, a TO_SIGNAL job that is not mono, destination ranges outside the signal or overlapping, a
 * resample job that iss_resample_pcm16 would refuse.  ISS_ESTATE: as iss_resample_pcm16.                               */
int iss_adpcm_decode(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                     int64_t nblocks_total, int64_t n_signal, int32_t* status_out);
/* The PCM16 samples of TO_STAGE job `job` of the last iss_adpcm_decode (bytes = frames_total * channels * 2); synchronises. */
int iss_adpcm_get_stage(iss_ctx* ctx, int32_t job, void* out, int64_t bytes);
/* ADPCM decode launches and blocks since the context was created.                                                    */
int iss_adpcm_stats(iss_ctx* ctx, int64_t* launches, int64_t* blocks);

/* Microsoft ADPCM in WAV (format tag 2) without ffmpeg.  A block of `block_align` bytes, `ch` channels:
 *   header  bPredictor[ch] (uint8 each), iDelta[ch] (int16 LE each), iSamp1[ch] (int16 LE each), iSamp2[ch] (int16 LE each)
 *           = 7 * ch bytes
 *   body    4-bit codes, HIGH nibble first, cycling through the channels: code k (k = 0, 1, ...) belongs to sample 2 + k / ch of
 *           channel k % ch and sits in byte 7 * ch + (k >> 1), the high nibble when k is even
 *   samples_per_block = (block_align - 7 * ch) * 2 / ch + 2
 *   output  sample 0 = iSamp2, sample 1 = iSamp1, then per code n (0 .. 15), s = n >= 8 ? n - 16 : n:
 *             pred  = (samp1 * C1[bPredictor] + samp2 * C2[bPredictor]) >> 8     (arithmetic shift: floor, NOT C division)
 *             v     = clamp16(pred + s * delta);  samp2 = samp1;  samp1 = v;  emit v
 *             delta = min(2^21, max(16, (ADAPT[n] * delta) >> 8))
 *   C1 = {256, 512, 0, 192, 240, 460, 392}   C2 = {0, -256, 0, 64, 0, -208, -232}
 *   ADAPT = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230}
 * Channels are interleaved in the output: the file reads like the PCM16 WAV holding these samples.  Definitions:
 *   - the `>> 8` is floor, libsndfile's rule (the reference reads through it); the Microsoft text truncates towards zero, which
 *     differs on negative sums.  No libsndfile was at hand to pin the rule: it round-trips a noisy sine through a nearest-code
 *     encoder at 36 - 38 dB, which shows that the formulas hang together and nothing more.
 *   - the header's iDelta is read as a signed int16; a value below 16 (a negative one too) is raised to 16 before the first code.
 *   - delta can triple per code and the format gives it no ceiling; it is capped at 2^21, so that 768 * delta, 8 * delta and the
 *     prediction sum stay inside 32 bits and the host build has no signed overflow.  A code moves the output by up to 8 * delta, so a
 *     delta above 2^13 already spans the whole 16-bit range; an encoder that codes the nearest value never grows it further,
 *     and no encoder's stream reaches the cap (only crafted blocks do).  Host and device builds are one function.
 *   - bPredictor >= 7 is a malformed block: status ISS_ADPCM_PREDICTOR, the block decoded with predictor 0 (garbage in that
 *     block only), as a step index above 88 is treated in an IMA block.
 * Limits as for IMA: 1 .. 64 channels, block_align <= 32768; block_align > 7 * ch with (block_align - 7 * ch) * 2 a multiple of
 * ch.  A block need not be a multiple of 4 bytes (3 channels x 70 bytes) and header fields sit at odd offsets: the decoder
 * reads bytes.  The entry points take the rows of the IMA ones (iss_adpcm_job, iss_window, iss_split) and follow their
 * contracts word for word with this geometry; they keep device state of their own (source, rows, status, staging), so an
 * iss_msadpcm_decode after an iss_adpcm_decode overwrites nothing the first call's status or iss_adpcm_get_stage still reads. */
#define ISS_ADPCM_PREDICTOR   2   /* a Microsoft ADPCM channel header's bPredictor is above 6 (decoded with predictor 0)          */
int iss_msadpcm_decode_host(const uint8_t* buf, int64_t len, int64_t nblocks, int32_t channels, int32_t block_align,
                            int64_t frames_total, int16_t* out, int32_t* status_out);
int iss_msadpcm_decode(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                       int64_t nblocks_total, int64_t n_signal, int32_t* status_out);
int iss_msadpcm_get_stage(iss_ctx* ctx, int32_t job, void* out, int64_t bytes);
int iss_msadpcm_stats(iss_ctx* ctx, int64_t* launches, int64_t* blocks);

/* Windows: a time range of a file through the three kernels above, touching only what the range needs.  A window row stands
 * beside a job row (windows[k] belongs to jobs[k]); windows == NULL is the unwindowed call, to the bit and to the launch.
 *   resample rows   `src` holds frames [s_begin, s_end) of a file of frames_total frames (the job's frames_in = s_end -
 *                   s_begin); outputs i in [out_begin, out_begin + out_count) are computed exactly as the whole-file call
 *                   computes them (same tap walk, ascending-j sum, separate multiply and add, same rounding) and written to
 *                   dst_offset + i - out_begin (the job's frames_out = out_count).  Frames outside [0, frames_total) are
 *                   zero: the edge of the staged slice is not the edge of the file.  Tiles are laid over the window.  The reach
 *                   j_lo = max(0, ceil((out_begin*down - hl)/up)) .. j_hi = min(frames_total - 1, floor(((out_begin +
 *                   out_count - 1)*down + hl)/up)) -- the frames that carry a tap -- must lie inside [s_begin, s_end): else
 *                   ISS_EINVAL, nothing launched.  A tile's staging that starts one frame lower reads that frame as zero.
 *   decoder rows    the job's frames_total stays the FILE's samples per channel (the window's frames_total must equal it) and
 *                   the samples [s_begin, s_end) are produced: TO_SIGNAL at dst_offset + s - s_begin; TO_STAGE at the staging
 *                   position of s - s_begin (s_end - s_begin samples staged), and with a filter resampled from there as a
 *                   resample row with the same window (the job's frames_out = out_count).  out_begin / out_count are read
 *                   only with a filter.
 *     FLAC          the job's frame rows are a contiguous run of the file's frames, first_sample in the file's numbering,
 *                   covering [s_begin, s_end); frame offsets are relative to src_offset as always (the caller stages only the
 *                   run's bytes).  Every row is decoded whole (its predictor chain starts at the frame) and fully checked,
 *                   CRC-16 included; only samples inside the window are stored.  Frames that are not among the rows are not
 *                   decoded and so not checked.
 *     IMA ADPCM     the job's blocks are exactly the file's blocks s_begin / samples_per_block .. (s_end - 1) /
 *                   samples_per_block, src_offset pointing at the first of them; status rows as always, one per staged block.
 * Everything else (signal rule, status, staging, counters, errors) is as for the unwindowed entry point.                   */
typedef struct {
    int64_t s_begin, s_end;        /* stored-rate frames of the file, 0 <= s_begin < s_end <= frames_total                  */
    int64_t frames_total;          /* the file's frames (samples per channel)                                                */
    int64_t out_begin, out_count;  /* 16 kHz outputs: out_begin >= 0, out_count >= 1, inside ceil(frames_total * up / down)  */
} iss_window;
int iss_resample_pcm16_windows(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                               const iss_window* windows, int32_t njobs, int64_t n_signal);
int iss_flac_decode_windows(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                            const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal,
                            int32_t* status_out);
int iss_adpcm_decode_windows(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                             const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                             int32_t* status_out);
int iss_msadpcm_decode_windows(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                               const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                               int32_t* status_out);          /* as iss_adpcm_decode_windows, Microsoft ADPCM blocks */

/* Splits: the channels of a file written apart instead of averaged, through the same three entry points' kernels.  A split row
 * stands beside a job row (splits[k] belongs to jobs[k]); splits == NULL is the plain call, to the bit and to the launch.
 * channel_sel[0, nsel) is one table of 0-based channel indices for the whole call; a job's selection is its rows
 * sel[q] = channel_sel[sel_begin + q], q in [0, sel_count).
 *   resample rows   sel_count > 0: the job writes sel_count mono outputs of frames_out samples each, output q at dst_offset +
 *                   q * dst_stride.  Output q is channel c = sel[q] of the source alone: m[j] is the stored sample of channel c
 *                   scaled as above, with no sum and no division by the channel count; tap walk, ascending-j sum with separate
 *                   multiply and add, rounding and saturation are those of the plain call (inaspeechsegmenter_amd/resample.py's
 *                   resample_ref on the channel's column, to the bit; with up = down = 1 the stored PCM16 value itself).
 *                   Entries of a selection lie in [0, channels); they may repeat and come in any order.  dst_stride >=
 *                   frames_out.  Samples between the end of an output and the next stride are not written.
 *                   sel_count == 0: the job downmixes all its channels exactly as the plain call does, in the same launch;
 *                   dst_stride and sel_begin are not read.
 *   decoder rows    only a TO_STAGE job with a filter may carry sel_count > 0: the decode kernel stages the interleaved samples
 *                   as always, and the split row is handed to the resample row that reads them.  Any other job must have
 *                   sel_count == 0.
 * The grid of the resample launch is ragged over (job, channel group, tile): a group holds as many selected channels as fit
 * 64 KiB of float64 spans side by side at the job's tile (two channels are kept in one group before the tile grows); a
 * workgroup stages its group once and computes its channels one after the other.  iss_resample_split_geometry reports the
 * (tile, channels per group) of a selection of nsel channels through a registered filter.
 * ISS_EINVAL (checked before anything is launched or the context changes, the text names the job): sel_count < 0, selection
 * rows outside [0, nsel), a selected channel outside [0, channels), dst_stride < frames_out, one of the sel_count destination
 * ranges outside the signal, any two destination ranges of the call overlapping (those of other jobs and of TO_SIGNAL jobs
 * included), a decoder job with a selection that is not TO_STAGE with a filter.
 * iss_resample_stats counts a split job as ONE job whatever its sel_count; launches, status, staging, the signal rule and all
 * other errors are as for the plain entry point.                                                                              */
typedef struct {
    int64_t dst_stride;   /* samples between the outputs of consecutive selected channels, >= frames_out */
    int32_t sel_begin;    /* the job's rows of channel_sel: [sel_begin, sel_begin + sel_count)            */
    int32_t sel_count;    /* 0: downmix all channels, exactly as the plain call does                      */
} iss_split;
int iss_resample_pcm16_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                             int64_t n_signal, const iss_split* splits, const int32_t* channel_sel, int64_t nsel);
int iss_flac_decode_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                          const iss_flac_job* jobs, int32_t njobs, int64_t n_signal, int32_t* status_out,
                          const iss_split* splits, const int32_t* channel_sel, int64_t nsel);
int iss_adpcm_decode_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                           int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_split* splits,
                           const int32_t* channel_sel, int64_t nsel);
int iss_msadpcm_decode_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, int32_t njobs,
                             int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_split* splits,
                             const int32_t* channel_sel, int64_t nsel);
int iss_resample_split_geometry(iss_ctx* ctx, int32_t filter, int32_t nsel, int32_t* tile_out, int32_t* group_out);

/* Windows and splits together: a time range of single channels.  The *_windows_split entry points take a window row AND a split
 * row beside every job row (windows[k] and splits[k] belong to jobs[k]) and the channel_sel table of the call; each of the two
 * contracts above holds as written, with frames_out = out_count.
 *   resample rows   sel_count > 0: `src` holds frames [s_begin, s_end) of the file, all channels interleaved; output q is the
 *                   outputs i in [out_begin, out_begin + out_count) of channel sel[q] alone, computed exactly as the split
 *                   call computes them on the whole file (resample_ref(x[s_begin:s_end, c], rate, out_begin, out_count,
 *                   s_begin, frames_total), to the bit), written to dst_offset + q * dst_stride + i - out_begin.  dst_stride >=
 *                   out_count.  Frames outside [0, frames_total) are zero, the reach must lie inside [s_begin, s_end), and
 *                   samples between the end of an output and the next stride are not written.
 *                   sel_count == 0: the windowed downmix of iss_resample_pcm16_windows, in the same launch.
 *   decoder rows    only a TO_STAGE job with a filter may carry sel_count > 0: the decode kernel stages the interleaved samples
 *                   [s_begin, s_end) of the window as a windowed call does, and the resample row reads them with the same
 *                   window and the split row.  FLAC frame rows and IMA ADPCM blocks are those of the windowed call.
 * The grid of the resample launch is ragged over (job, channel group, tile) with the tiles laid over the window; groups and
 * tile are those iss_resample_split_geometry reports.  Device table: job rows, window rows, split rows, channel selections.
 * ISS_EINVAL: everything either contract refuses, with the same text.  iss_resample_stats counts a windowed split job as ONE
 * job.  A call with windows only or splits only takes the entry point it always took.                                         */
int iss_resample_pcm16_windows_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                     const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_split* splits,
                                     const int32_t* channel_sel, int64_t nsel);
int iss_flac_decode_windows_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                                  const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal,
                                  int32_t* status_out, const iss_split* splits, const int32_t* channel_sel, int64_t nsel);
int iss_adpcm_decode_windows_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                   const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                   int32_t* status_out, const iss_split* splits, const int32_t* channel_sel, int64_t nsel);
int iss_msadpcm_decode_windows_split(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs,
                                     const iss_window* windows, int32_t njobs, int64_t nblocks_total, int64_t n_signal,
                                     int32_t* status_out, const iss_split* splits, const int32_t* channel_sel, int64_t nsel);

/* Mixes: weighted sums of a file's channels, mixed and resampled in the same launch.  A MIX is K >= 1 terms (c_k, w_k) and a
 * divisor d: c_k a 0-based channel (channels may repeat and come in any order), w_k a finite float64, d finite and not zero.
 * For stored frame j, x[j, c] the stored sample scaled as for the plain call (libsndfile's rule):
 *     m[j] = ( (w_0 * x[j, c_0]) + w_1 * x[j, c_1] + ... + w_{K-1} * x[j, c_{K-1}] ) / d
 * in float64, every product and every sum rounded on its own (no FMA), terms in ascending k, the division always performed,
 * once, at the end (d = 1 is exact).  Tap walk, ascending-j sum with separate multiply and add, rint(y * 32768) and saturation
 * to [-32768, 32767] are those of the plain call, through the identity filter at 16 kHz too: a mix whose sum leaves [-1, 1)
 * saturates, and the output is PCM16 whatever the stored format (inaspeechsegmenter_amd/resample.py's mix_ref, to the bit).
 * Two identities: K = 1, w = 1, d = 1 is the split's output for that channel; all C channels in order, every w = 1, d = C is the
 * plain call's downmix.
 * Three tables go with a call: a mix-set row beside every job row (mixsets[k] belongs to jobs[k]), the call's mix rows
 * mixes[0, nmixes) and the call's term rows terms[0, nterms).  A job's mixes are rows [mix_begin, mix_begin + mix_count) of
 * `mixes`; a mix's terms are rows [term_begin, term_begin + term_count) of `terms`.
 *   resample rows   mix_count > 0: the job writes mix_count mono outputs of frames_out samples each, output q at dst_offset +
 *                   q * dst_stride (with a window: outputs i in [out_begin, out_begin + out_count) at dst_offset + q *
 *                   dst_stride + i - out_begin, frames outside [0, frames_total) zero, as for a windowed split).  Samples between
 *                   the end of an output and the next stride are not written.
 *                   mix_count == 0: the job downmixes all its channels exactly as the plain call does, in the same launch.
 *   decoder rows    only a TO_STAGE job with a filter may carry mix_count > 0: the decode kernel stages the interleaved samples
 *                   as always and the mix-set row is handed to the resample row that reads them.
 * `windows` is optional in every *_mix entry point: NULL is the unwindowed call, else a window row beside every job row, with
 * the contract of the *_windows entry points.  The grid of the resample launch is ragged over (job, mix group, tile); groups and
 * tile are what iss_resample_split_geometry reports for mix_count rows.  Device table: job rows, (window rows,) mix-set rows,
 * mix rows, term rows.
 * ISS_EINVAL (checked before anything is launched or the context changes, the text names the job): mix_count < 0, mix rows
 * outside [0, nmixes), term_count < 1, term rows outside [0, nterms), a term's channel outside [0, channels), a weight that is
 * not finite, a divisor that is zero or not finite, dst_stride < frames_out, one of the mix_count destination ranges outside the
 * signal, any two destination ranges of the call overlapping, a decoder job with mixes that is not TO_STAGE with a filter.
 * iss_resample_stats counts a mixed job as ONE job whatever its mix_count; launches, status, staging, the signal rule and all
 * other errors are as for the plain entry point.  The entry points above are unchanged, to the bit and to the launch.          */
typedef struct {
    int64_t dst_stride;   /* samples between the outputs of consecutive mixes, >= frames_out                 */
    int32_t mix_begin;    /* the job's rows of `mixes`: [mix_begin, mix_begin + mix_count)                    */
    int32_t mix_count;    /* 0: downmix all channels, exactly as the plain call does                         */
} iss_mixset;
typedef struct {
    int32_t term_begin;   /* the mix's rows of `terms`: [term_begin, term_begin + term_count)                 */
    int32_t term_count;   /* >= 1                                                                            */
    double divisor;       /* finite, not zero                                                                */
} iss_mix;
typedef struct {
    int32_t channel;      /* 0-based, below the job's channels                                               */
    int32_t reserved;     /* 0                                                                               */
    double weight;        /* finite                                                                          */
} iss_mix_term;
int iss_resample_pcm16_mix(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                           const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_mixset* mixsets,
                           const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms);
int iss_flac_decode_mix(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_flac_frame* frames, int64_t nframes,
                        const iss_flac_job* jobs, const iss_window* windows, int32_t njobs, int64_t n_signal, int32_t* status_out,
                        const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms);
int iss_adpcm_decode_mix(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, const iss_window* windows,
                         int32_t njobs, int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_mixset* mixsets,
                         const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms);
int iss_msadpcm_decode_mix(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_adpcm_job* jobs, const iss_window* windows,
                           int32_t njobs, int64_t nblocks_total, int64_t n_signal, int32_t* status_out, const iss_mixset* mixsets,
                           const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms, int64_t nterms);

/* Channel survey: per-channel level figures and the cross-products between channels of stored frames [a, b) of a source, in
 * one pass over the stored samples (survey.hip; inaspeechsegmenter_amd/resample.py `survey_ref` is the same arithmetic in
 * numpy, to the bit).  Nothing of the resident signal or the features is touched.
 *
 * Frames.  The whole file is a = 0, b = frames.  A time range (start_sec, stop_sec) of a file at rate sr is a = floor(start_sec
 * * sr + 0.5), b = min(frames, floor(stop_sec * sr + 0.5)) (the excerpt calls' rounding, on stored frames); the caller computes
 * it and refuses an empty range.  n = b - a >= 1 here.
 * Samples.  x[j, c] is the float64 value the resample kernel gives stored sample (j, c): the ISS_RS_* formats above with
 * libsndfile's scaling (24-bit PCM widened to x << 8, G.711 expanded, big-endian swapped, decoder output PCM16 or int32).  A
 * NaN or +-Inf sample of a float format is counted in `nonfinite` and is 0.0 in every other figure (zeros included).
 * Figures, per channel c:   peak = max_j |x|,  zeros = #{x == 0.0},  fullscale = #{|x| >= full} (`full` from the job row: the
 * largest positive value the stored format holds),  nonfinite,  s1 = sum_j x,  s2 = sum_j x*x;  and for channels <=
 * ISS_SURVEY_PAIR_CHANNELS, per pair c < d:  s12 = sum_j x[j,c] * x[j,d].  peak and the counts are exact.
 * The survey order of the three sums.  Every product and every addition is rounded on its own (no FMA).  The terms of a sum
 * are numbered k = j - a.  Chunk q holds terms [q * C, min(n, (q+1) * C)), C = ISS_SURVEY_CHUNK = 1024.  Within a chunk, lane
 * t of 256 starts from +0.0 and adds its terms t, t + 256, t + 512, t + 768 in that order (a missing term adds nothing); the 64
 * lanes of each of the four waves (lanes 64w .. 64w + 63) are combined by the tree  lane l += lane l + s  for s = 32, 16, 8, 4,
 * 2, 1; the chunk's sum is ((wave 0 + wave 1) + wave 2) + wave 3.  The job's sum starts from +0.0 and adds its chunk sums in
 * ascending q.  The order depends on (a, b) alone: not on the grid, on the other jobs of the call, or on where the bytes lie;
 * no floating-point atomic is used.
 *
 * Result row of job k, 8-byte words from results[result_offset_k] on, W = 6 * ch + (ch <= 16 ? ch * (ch - 1) / 2 : 0) of them,
 * result_offset_k = the sum of W over the jobs before it:   s1[ch], s2[ch], peak[ch] as float64;  zeros[ch], fullscale[ch],
 * nonfinite[ch] as int64;  then s12 as float64 in the order (0,1), (0,2), ..., (0,ch-1), (1,2), ...
 *
 * iss_survey: `src` = the stored bytes of every job (one H2D copy), one launch of survey_kernel over (job, chunk) and one of the
 * second stage; `results` (the sum of W words) is valid when the call returns.  windows == NULL: job k surveys its frames_in
 * frames at src_offset.  With windows (one beside every job): the job's bytes hold frames [s_begin, s_end) of the file, and
 * frames [out_begin, out_begin + out_count) are surveyed (counted in stored frames here, inside [s_begin, s_end): else
 * ISS_EINVAL) -- the same figures, to the bit, as a job holding those frames alone.
 * iss_flac_survey / iss_adpcm_survey / iss_msadpcm_survey: the same over what the codec's last decode call staged (TO_STAGE
 * jobs, with or without a filter): src_offset of a row is the INDEX of the staged job of that call, format ISS_RS_I16 or
 * ISS_RS_I32 as staged, frames_in * channels samples exactly what the job staged.  Nothing is uploaded but the rows.
 * Errors: ISS_EINVAL, nothing launched.  channels 1 .. 1024.                                                                 */
#define ISS_SURVEY_CHUNK          1024
#define ISS_SURVEY_PAIR_CHANNELS  16
typedef struct {
    int64_t src_offset;            /* byte offset of the job's first staged frame (codec entries: index of the staged job)   */
    int64_t frames_in;             /* frames the job's bytes hold                                                            */
    int32_t channels, format;      /* ISS_RS_*                                                                               */
    double  full;                  /* fullscale threshold, > 0                                                               */
} iss_survey_job;
int iss_survey(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_survey_job* jobs, const iss_window* windows,
               int32_t njobs, void* results);
int iss_flac_survey(iss_ctx* ctx, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results);
int iss_adpcm_survey(iss_ctx* ctx, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results);
int iss_msadpcm_survey(iss_ctx* ctx, const iss_survey_job* jobs, const iss_window* windows, int32_t njobs, void* results);
/* the chunk geometry: frames per chunk, lanes per chunk, and the channel count up to which pairs are computed */
int iss_survey_geometry(int32_t* chunk_out, int32_t* lanes_out, int32_t* pair_channels_out);
int iss_survey_stats(iss_ctx* ctx, int64_t* launches, int64_t* jobs);     /* survey_kernel launches, jobs surveyed */

/* Resampling what an earlier call left on the device: the rows of a *_mix call over bytes that are already there, so that a survey
 * of a file and its downmix -- any mix the survey suggests, or the plain one -- cost one upload and one decode.  Nothing is uploaded
 * but rows and tables; the kernels are the resample_kernel instantiations of iss_resample_pcm16_mix, and so is the arithmetic.
 * An ORIGIN is one of four device buffers and what its last writer left in it:
 *   ISS_STAGED_SURVEY    the payload of the context's last iss_survey (`src`, src_bytes of it).  A row must be one of that call's
 *                        jobs: the same src_offset (a byte offset), frames_in, channels and format.
 *   ISS_STAGED_FLAC / ISS_STAGED_ADPCM / ISS_STAGED_MSADPCM
 *                        what the codec's last decode call staged (TO_STAGE jobs, with or without a filter).  src_offset of a row
 *                        is the INDEX of the staged job of that call, as in iss_survey_job; format is ISS_RS_I16 or ISS_RS_I32 as
 *                        staged; frames_in * channels samples are exactly what the job staged (a windowed decode job: its
 *                        s_end - s_begin frames).
 * A PAYLOAD is what an origin holds, named by an id that counts up over the context's life: every iss_survey that uploads, and
 * every decode call of a codec that launches, leaves a new one in its origin.  iss_staged_payload gives the id of the payload an
 * origin holds now (ISS_ESTATE: none -- no such call went before, or the last one failed on its way).  The caller takes it right
 * after the call that made the payload and hands it to iss_resample_staged_mix, which refuses any other.
 * iss_resample_staged_mix: filter, dst_offset, frames_out, the optional window rows, mix-set, mix and term rows, mix_count == 0
 * (the plain downmix, to the bit what iss_resample_pcm16 writes), n_signal, counters and every error of iss_resample_pcm16_mix hold
 * as written there, with the origin's bytes in the place of `src`.  One launch for all jobs.
 * ISS_ESTATE (nothing launched, the context unchanged; the text names the entry point and the origin): the origin holds no
 * payload, or `payload` is not the one it holds -- a later call of that origin (any upload into the survey's source buffer, any
 * decode call of that codec) has replaced it.  n_signal < 0 without a signal: as iss_resample_pcm16.
 * ISS_EINVAL (found before anything changes): a row that does not match what was uploaded or staged in frames, channels or
 * format; a bad origin; everything iss_resample_pcm16_mix refuses.                                                              */
#define ISS_STAGED_SURVEY   0
#define ISS_STAGED_FLAC     1
#define ISS_STAGED_ADPCM    2
#define ISS_STAGED_MSADPCM  3
int iss_staged_payload(iss_ctx* ctx, int32_t origin, int64_t* payload_out);
int iss_resample_staged_mix(iss_ctx* ctx, int32_t origin, int64_t payload, const iss_resample_job* jobs, const iss_window* windows,
                            int32_t njobs, int64_t n_signal, const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes,
                            const iss_mix_term* terms, int64_t nterms);
/* Payload H2D copies (stored bytes for the resampler and the survey, compressed bytes for the decoders: not row tables, not
 * signals) and their bytes since the context was created: what "one upload per file" is counted with.                           */
int iss_upload_stats(iss_ctx* ctx, int64_t* copies, int64_t* bytes);

/* File sets: several files read as ONE multichannel source -- a call logger's one mono file per direction, a production
 * system's one mono file per track -- without interleaving anything on the host.  A SET is an ordered list of 1 .. 1024 MEMBERS,
 * each `frames` >= 1 frames of `channels` >= 1 interleaved channels of the job's format at byte `src_offset` of `src`.  It reads
 * exactly like its INTERLEAVED TWIN, the one source that holds the members' channels side by side (member 0's first, each
 * member's in order), as many frames as the longest member, a shorter member continued with samples whose value is 0.0:
 *     x[j, c] = j < frames_m ? (stored sample j * channels_m + c_local of member m, scaled as for the plain call) : 0.0
 * for channel c = (channels of the members before m) + c_local.  Such a sample is a digital zero to the survey, never fullscale
 * and never non-finite: what stored zeros of the twin give.  Everything else is the twin's, to the bit: the mix arithmetic of
 * "Mixes" above, the tap walk and the quantisation of the plain call, the figures and the survey order of "Channel survey".
 * Two tables go with a call beside those of the entry point it extends: a set row beside every job row (sets[k] belongs to
 * jobs[k]) and the call's member rows members[0, nmembers); a job's members are rows [member_begin, member_begin +
 * member_count).  In the job row `channels` is the sum of the members' channels, `frames_in` the largest of their `frames`, and
 * src_offset is 0: the members say where the bytes lie.  Members of several jobs may share bytes.
 *   iss_resample_pcm16_set    iss_resample_pcm16_mix without windows, for sets: whole sources only.  mix_count > 0 writes the
 *                             job's mixes apart (a split is one-term mixes: K = 1, w = 1, d = 1); mix_count == 0 is the plain
 *                             downmix of the twin, to the bit -- the planner writes it as the mix of all C channels in order,
 *                             every w = 1, d = C, the second identity of "Mixes".  Geometry: iss_resample_split_geometry for
 *                             mix_count rows (one row for the downmix).  The kernel is resample_kernel's SET instantiation: a
 *                             workgroup stages its mixes channel-major (a lane walks consecutive frames of one mix, so a wave
 *                             reads consecutive frames of one member); the order in which LDS is filled touches no arithmetic.
 *                             Device table: job rows, mix-set rows, mix rows, then the term rows, each resolved on the host to
 *                             (byte offset of the member's first sample of that channel, the member's frames and channels).
 *   iss_survey_set            iss_survey without windows, for sets: the same chunk geometry, partial rows, second stage and
 *                             result rows; survey_kernel's SET instantiation stages a chunk's rows through a per-channel table
 *                             (byte offset, frames, channels of the member) that follows the job rows.
 *   iss_resample_staged_set   iss_resample_pcm16_set over the payload the context's last iss_survey_set left in the survey's
 *                             source buffer (origin ISS_STAGED_SURVEY, the payload-id rule of iss_resample_staged_mix): a job
 *                             must be one of that call's, the same frames_in, channels, format and member rows.  Nothing is
 *                             uploaded but rows.  A payload left by iss_survey is not one of sets, and the other way round.
 * ISS_EINVAL (checked before anything is launched or the context changes, the text names the job): member_count < 1 or above
 * 1024, member rows outside [0, nmembers), a member with frames < 1 or channels < 1, the members' channels not adding up to the
 * job's `channels` or their longest not being its `frames_in`, a job's src_offset not 0, a member's bytes [src_offset, src_offset
 * + frames * channels * sample bytes) outside `src` or not aligned to the sample, and everything iss_resample_pcm16_mix (without
 * windows) / iss_survey refuse.  ISS_ESTATE for iss_resample_staged_set as for iss_resample_staged_mix.
 * Counters: a set job is ONE job of iss_resample_stats / iss_survey_stats whatever its members, and a call's payload one copy of
 * iss_upload_stats, its bytes `src_bytes`.  Every other entry point is unchanged, to the bit and to the launch.                 */
typedef struct {
    int32_t member_begin;  /* the job's rows of `members`: [member_begin, member_begin + member_count)         */
    int32_t member_count;  /* 1 .. 1024                                                                       */
} iss_set;
typedef struct {
    int64_t src_offset;    /* byte offset of the member's first frame in `src`, aligned to the sample          */
    int64_t frames;        /* >= 1                                                                            */
    int32_t channels;      /* >= 1: the member's own interleaved channels                                     */
    int32_t reserved;      /* 0                                                                               */
} iss_set_member;
int iss_resample_pcm16_set(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs, int32_t njobs,
                           int64_t n_signal, const iss_set* sets, const iss_set_member* members, int64_t nmembers,
                           const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                           int64_t nterms);
int iss_survey_set(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_survey_job* jobs, int32_t njobs, const iss_set* sets,
                   const iss_set_member* members, int64_t nmembers, void* results);
int iss_resample_staged_set(iss_ctx* ctx, int32_t origin, int64_t payload, const iss_resample_job* jobs, int32_t njobs,
                            int64_t n_signal, const iss_set* sets, const iss_set_member* members, int64_t nmembers,
                            const iss_mixset* mixsets, const iss_mix* mixes, int64_t nmixes, const iss_mix_term* terms,
                            int64_t nterms);

/* Schedules: a downmix that differs from one stretch of a file to the next.  A SCHEDULE of a file with n stored frames and C
 * channels is R >= 1 RUNS (begin_r, mix_r): begin_0 = 0 and the begins strictly ascending, in stored frames at the file's own
 * rate; mix_r a mix of "Mixes" or NONE.  Run r governs the frames [begin_r, begin_{r+1}), the last run to the end; a run that
 * begins at or past n governs nothing and is allowed.  The scheduled mono signal is m[j] = mixdown(x[j, :], mix_{r(j)}), in
 * float64 with the arithmetic of "Mixes": terms in order, every product, sum and the one division rounded on its own.  NONE
 * stands for the mix of all C channels in order with w = 1, d = C: by the second identity of "Mixes" the plain downmix, to the
 * bit.  Frames outside [0, n) are 0.0.  m is then resampled and quantised exactly as ever, so the FIR taps of outputs near a
 * boundary see samples of both runs: that is the definition, not an artefact (inaspeechsegmenter_amd/resample.py's
 * schedule_ref, to the bit).  Two identities: the schedule [(0, NONE)] gives the plain call's output, and [(0, mix)] what a
 * mix call gives for that one mix.
 * Tables of a call: a schedule row beside every job row (scheds[k] belongs to jobs[k]), the call's run rows runs[0, nruns) --
 * a job's runs are rows [run_begin, run_begin + run_count), run_count 1 .. 2^20 -- and the mix and term rows of a mix call; a
 * run's `mix` is a row of `mixes`, or -1 for NONE.  Every job writes ONE output of frames_out samples at dst_offset.
 * The kernel is resample_kernel's SCHED instantiation (a pair: the WAV five, and all formats).  Geometry:
 * iss_resample_split_geometry for one row.  A workgroup finds the runs of the first and the last frame of its span once (the
 * same for all its lanes); where they are one run -- nearly every tile of a real file -- it stages as a mix call stages one mix,
 * else each frame finds its run between those two.  Device table, 16-byte rows behind the job rows and the mix-set rows (one per
 * job, whose mix_begin names the job's schedule row): the call's mix rows and one all-channel mix per job with a NONE run, their
 * term rows, one {run_begin, run_count} row per job, then run rows {int64 begin_frame; int32 mix; int32 reserved}, every index
 * counted in 16-byte rows from the first mix row.
 *   iss_resample_pcm16_sched   the plain call's arguments, `windows` (which must be NULL: a schedule governs whole sources)
 *                              and the tables above.  One upload, one launch.
 *   iss_resample_staged_sched  the same over the bytes an origin holds: origins, payload ids and row matching exactly as
 *                              iss_resample_staged_mix, so FLAC, IMA and Microsoft ADPCM files ride on what their decode call
 *                              staged and a surveyed file on the survey's upload.
 * ISS_EINVAL (checked before anything is launched or the context changes, the text names the job): run_count < 1 or above 2^20,
 * run rows outside [0, nruns), a first begin that is not 0, begins not strictly ascending or negative, a mix index outside
 * [-1, nmixes), windows passed with a schedule, and for every mix a run names everything iss_resample_pcm16_mix refuses of a
 * mix (term rows, channels, weights, divisor), as well as everything it refuses of a job.  ISS_ESTATE as for
 * iss_resample_staged_mix.  iss_resample_stats counts one launch per call and one job per job row.  Every other entry point is
 * unchanged, to the bit and to the launch.                                                                                      */
typedef struct {
    int32_t run_begin;     /* the job's rows of `runs`: [run_begin, run_begin + run_count)                     */
    int32_t run_count;     /* 1 .. 2^20                                                                       */
} iss_sched;
typedef struct {
    int64_t begin_frame;   /* first stored frame the run governs; 0 for a job's first run, strictly ascending  */
    int32_t mix;           /* a row of `mixes`, or -1: the plain downmix of all channels                       */
    int32_t reserved;      /* 0                                                                               */
} iss_sched_run;
int iss_resample_pcm16_sched(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                             const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                             const iss_sched_run* runs, int64_t nruns, const iss_mix* mixes, int64_t nmixes,
                             const iss_mix_term* terms, int64_t nterms);
int iss_resample_staged_sched(iss_ctx* ctx, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                              const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                              const iss_sched_run* runs, int64_t nruns, const iss_mix* mixes, int64_t nmixes,
                              const iss_mix_term* terms, int64_t nterms);

/* Fades: a schedule whose runs cross-fade in instead of cutting in.  A schedule of "Schedules" gains one half-width h_r >= 0 per
 * run, counted in stored frames, h_0 = 0.  Run r >= 1 fades in over the ZONE Z_r = [begin_r - h_r, begin_r + h_r).  Zones are
 * disjoint and in order: begin_{r-1} + h_{r-1} <= begin_r - h_r for every r >= 1.  The first zone may start at frame 0; a zone
 * may reach past the file's end or lie past it.
 * Outside every zone m[j] is what "Schedules" says.  For j in Z_r: k = j - (begin_r - h_r), a = (2k + 1) / (4 h_r) -- both
 * integers exact in float64, one division --, p = mixdown(x[j, :], mix_{r-1}), q = mixdown(x[j, :], mix_r), each by the
 * arithmetic of "Mixes", and m[j] = p + a * (q - p): the subtraction, the product and the sum each rounded on its own.  The ramp
 * is linear and sampled at the centres of the zone's 2 h_r frames, so it never reaches 0 or 1: a passes 1/2 between the two
 * frames either side of begin_r.  NONE is the all-channel mix, as ever; frames outside [0, n) are 0.0; a run that begins at or
 * past n still fades in over the part of its zone that lies inside the file.  m is resampled and quantised as ever
 * (inaspeechsegmenter_amd/resample.py's schedule_ref, to the bit).
 * Two identities, to the bit: all h_r = 0 is the schedule without fades, and a boundary whose two mixes have equal terms and
 * divisor leaves m as if there were no boundary (q - p = 0, and p + a * 0 = p).
 * The kernel is resample_kernel's FADE instantiation (a pair, as SCHED's; FADE only with SCHED).  The half-width rides in the
 * reserved 32 bits of the device's run row.  A workgroup finds the runs of its span's first and last frame once, as SCHED does,
 * and stages as a mix call stages one mix only where those are one run AND the span touches neither that run's own zone nor the
 * head of the next run's; any other workgroup finds each frame's run, tests the run's own zone (blend with the run before) and
 * the next run's (blend with the run after), and stages the blend or the plain mix.  No LDS beyond SCHED's, no scratch.
 *   iss_resample_pcm16_sched_fade, iss_resample_staged_sched_fade
 *       their *_sched twin's arguments and `fades`, one half-width per row of `runs` (fades[i] belongs to runs[i]).  A call
 *       whose half-widths are all 0 launches the SCHED instantiation: the twin's launch, to the bit.
 * ISS_EINVAL (before anything is launched or the context changes, the text names job and run): a negative half-width, a
 * non-zero half-width on a job's first run, overlapping zones, and everything the twin refuses.  ISS_ESTATE as the twin.
 * iss_resample_stats counts as for the twin.  Every other entry point is unchanged, to the bit and to the launch.               */
int iss_resample_pcm16_sched_fade(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_resample_job* jobs,
                                  const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                  const iss_sched_run* runs, int64_t nruns, const int32_t* fades, const iss_mix* mixes,
                                  int64_t nmixes, const iss_mix_term* terms, int64_t nterms);
int iss_resample_staged_sched_fade(iss_ctx* ctx, int32_t origin, int64_t payload, const iss_resample_job* jobs,
                                   const iss_window* windows, int32_t njobs, int64_t n_signal, const iss_sched* scheds,
                                   const iss_sched_run* runs, int64_t nruns, const int32_t* fades, const iss_mix* mixes,
                                   int64_t nmixes, const iss_mix_term* terms, int64_t nterms);

/* Survey blocks: a survey resolved in time.  A TIMELINE cuts a file's stored frames into BLOCKS of B = K * 1024 frames counted
 * from frame 0: 1024 is ISS_SURVEY_CHUNK, K = max(1, floor(block_sec * sr / 1024 + 0.5)), the default block_sec = 10.0 a
 * definition.  The last block is shorter.  Block b's survey is the survey of frames [b * B, min((b + 1) * B, n)) by "Channel
 * survey", to the bit in every field.  This needs no new first stage: survey_kernel writes one partial row per 1024-frame
 * chunk and a block is a run of whole chunks, so a block's sums are its chunk rows added in ascending order from +0.0, its peak
 * their max and its counts their sums -- what the second stage does per job.  survey_reduce_blocks_kernel: grid ragged over
 * (job, block, group of 256 words), one thread per word of one block's row, plain stores only.  The whole-file survey comes
 * out of the same launch of survey_kernel and is reduced over ALL chunk rows, not over the block results (the association
 * differs): `results` is byte for byte what the twin without blocks writes.
 *   iss_survey_blocks, iss_flac_survey_blocks, iss_adpcm_survey_blocks, iss_msadpcm_survey_blocks
 *       the arguments of their iss_*survey twins without windows, block_chunks[njobs] (K of each job, >= 1) and
 *       `block_results`: one row per block with the layout of a result row, the jobs in order, a job's ceil(ceil(n / 1024) / K)
 *       blocks ascending.  Payload rules are the twin's: iss_survey_blocks uploads, and leaves a payload in origin
 *       ISS_STAGED_SURVEY; the codec entries read what the codec's last decode call staged.  A call counts as ONE launch of
 *       iss_survey_stats, its jobs as jobs.
 * ISS_EINVAL, nothing launched: a block_chunks entry below 1, a NULL table, everything the twin refuses.                        */
int iss_survey_blocks(iss_ctx* ctx, const void* src, int64_t src_bytes, const iss_survey_job* jobs, int32_t njobs,
                      const int32_t* block_chunks, void* results, void* block_results);
int iss_flac_survey_blocks(iss_ctx* ctx, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks, void* results,
                           void* block_results);
int iss_adpcm_survey_blocks(iss_ctx* ctx, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks, void* results,
                            void* block_results);
int iss_msadpcm_survey_blocks(iss_ctx* ctx, const iss_survey_job* jobs, int32_t njobs, const int32_t* block_chunks, void* results,
                              void* block_results);

/* Page-locked host memory (hipHostMalloc) for decode buffers and result arrays: copies
 * from / to it are truly asynchronous (pageable memory is staged by the runtime).        */
int iss_host_alloc(iss_ctx* ctx, size_t bytes, void** out);
int iss_host_free(iss_ctx* ctx, void* p);

/* Run the front end on the resident signal.  Results stay in HBM (mspec (T,24),
 * loge (T,)); *T_out = int((n-400)/160)+1 (sidekit_mfcc.py:254), 0 if n < 400.
 * Every call also queues one small kernel over the log-mel rows and a T-byte read-back behind the feature kernel (the row
 * flags by which iss_cnn_probs* finds dead windows), whether or not a network runs later: iss_get_loge's wait brings them to
 * the host; after any other wait the first iss_cnn_probs* call waits once more for the stream, without a second launch. */
int iss_sidekit(iss_ctx* ctx, int32_t* T_out);
int iss_get_loge(iss_ctx* ctx, float* loge_out /* T */);
int iss_get_mspec(iss_ctx* ctx, float* mspec_out /* T*24 */);
/* Replace the resident mel spectrogram (segment_feats(mspec, ...) entry,
 * segmenter.py:250, and the <68-frame padding of segmenter.py:61-65).          */
int iss_set_mspec(iss_ctx* ctx, const float* mspec, int32_t T);

/* ------------------------------------------------------------ small-CNN engine
 * replaces segmenter.py:76-88 `_get_patches` + :156-163 gather + `nn.predict`.
 *
 * A network is a flat op program (ISS_OP_* rows of ISS_PROG_COLS int32) plus one
 * float32 parameter blob; inaspeechsegmenter_amd/keras_model.py compiles a Keras
 * `model_config` into it.  net_id in [0, ISS_MAX_NETS).                        */
#define ISS_MAX_NETS   8
#define ISS_PROG_COLS  32

enum {
    ISS_OP_CONV     = 1,  /* conv2d / dense as implicit GEMM (MFMA) + fused epilogue (+ fused pool) */
    ISS_OP_POOL     = 2,  /* max / average pooling, NHWC; a padded (PT / PL, 'same') average leaves the padding out of the mean */
    ISS_OP_SOFTMAX  = 3,  /* softmax over the channel axis                               */
    ISS_OP_STATPOOL = 4,  /* mean || std over the time axis (resnet.py:123-127)          */
    ISS_OP_ACT      = 5,  /* elementwise activation beyond the fused ones: ISS_C_ACT 4 elu(alpha), 5 leaky relu(alpha),
                             6 selu, 7 softplus, 8 relu clipped at alpha (ReLU(max_value)); alpha = the float whose bits are in
                             ISS_C_ACTPARAM; 9 keras.layers.ReLU in full: x > threshold ? min(x, max_value) : negative_slope *
                             (x - threshold), (negative_slope, max_value (+inf: none), threshold) in ISS_C_ACTPARAM, ..2, ..3;
                             IN may equal OUT, and is never ISS_BUF_INPUT */
    ISS_OP_ELT      = 6,  /* merge / data-movement rows of graph-shaped models (keras.layers.Add, Concatenate, Permute ...; what
                             `keras.models.load_model`, segmenter.py:129-131, accepts beyond a chain).  Plain one-thread-per-element
                             kernels: correct, not fast.  ISS_C_ACT = kind (ISS_ELT_*); IN is never ISS_BUF_INPUT.
                             kinds ADD .. AVG: OUT[i] = IN[i] (op) RES[i] over H * W * CIN floats per sample (HO, WO, COUT = H, W, CIN;
                                               OUT may be IN or RES); ISS_C_ORDER = 1: followed by relu (Add + ReLU of a residual block);
                             COPY:    OUT[p][PL + c] = IN[p][PT + c] for c < KH, p over the H * W pixels; IN holds CIN and OUT COUT
                                      channels per pixel (HO, WO = H, W); OUT != IN.  Concatenate = one COPY per input;
                             ZERO:    OUT[p][PL + c] = 0 for c < KH (channel padding behind a COPY);
                             PERMUTE: OUT = IN with its (H, W, CIN) axes permuted, output axis i = input axis perm[i],
                                      perm = (KH, KW, SH); (HO, WO, COUT) = the permuted shape; OUT != IN */
};
enum { ISS_ELT_COPY = 0, ISS_ELT_ADD = 1, ISS_ELT_SUB = 2, ISS_ELT_MUL = 3, ISS_ELT_MAX = 4, ISS_ELT_MIN = 5, ISS_ELT_AVG = 6,
       ISS_ELT_ZERO = 7, ISS_ELT_PERMUTE = 8 };
/* column meaning of a program row (unused columns = 0, absent offsets = -1) */
enum {
    ISS_C_OP = 0, ISS_C_IN, ISS_C_OUT, ISS_C_RES,      /* buffer ids; RES = residual add   */
    ISS_C_H, ISS_C_W, ISS_C_CIN, ISS_C_HO, ISS_C_WO, ISS_C_COUT,
    ISS_C_KH, ISS_C_KW, ISS_C_SH, ISS_C_SW, ISS_C_PT, ISS_C_PL,
    ISS_C_ACT,                                          /* CONV: 0 none 1 relu 2 sigmoid 3 tanh (fused); ISS_OP_ACT rows: 4..9 */
    ISS_C_WOFF, ISS_C_BOFF,                             /* blob offsets: W [Cout][roundup32(kh*kw*Cin)] (WOFF % 8 == 0), bias */
    ISS_C_PSOFF, ISS_C_PTOFF,                           /* post-activation scale / shift   */
    ISS_C_INMODE,                                       /* 0 NHWC buffer, 1 z-normed mspec patch,
                                                           2 window of the resident vbx features (iss_vbx_embed) */
    ISS_C_POOLKIND,                                     /* POOL: 0 max 1 avg               */
    ISS_C_ORDER,                                        /* STATPOOL out order: 0 = (c,h) torch flatten */
    ISS_C_FPOOLH, ISS_C_FPOOLW,                         /* CONV: fused non-overlapping pool window applied after
                                                           the epilogue (0/1 = none; FPOOLH*FPOOLW in {2,4};
                                                           kind in ISS_C_POOLKIND).  HO/WO stay the conv's own
                                                           output size; OUT holds (HO/FPOOLH, WO/FPOOLW, COUT) */
    ISS_C_DUALW, ISS_C_DUALB,                           /* CONV, optional (0 = absent, else 1 + blob offset): row r is a 1x1
                                                           stride-1 conv whose residual (RES == OUT) is the output of row
                                                           r - 1, a LINEAR 1x1 conv (any stride, no bias-free form) of the
                                                           same output shape -- a projection shortcut and the expansion it
                                                           is added to (resnet.py:60-75).  DUALW: the concatenated matrix
                                                           [COUT][CIN(r) + CIN(r-1)] = [W(r) | W(r-1)], DUALB: b(r) + b(r-1).
                                                           The library may then compute both rows as ONE GEMM over the two
                                                           inputs (row r - 1's output is never materialised); it falls back
                                                           to the two rows whenever it cannot.  Both CIN % 32 == 0. */
    ISS_C_ACTPARAM,                                     /* ISS_OP_ACT: the bits of the activation's float parameter (alpha of elu / leaky relu) */
    ISS_C_ACTPARAM2, ISS_C_ACTPARAM3,                   /* ISS_OP_ACT code 9: max_value, threshold */
};
#define ISS_BUF_INPUT  (-2)   /* IN: the network input (patch source or iss_cnn_forward input) */

/* nbuf activation buffers with buf_elems[i] floats per sample; the last op's OUT
 * buffer holds the (out_dim,) result per sample.                                */
int iss_cnn_load(iss_ctx* ctx, int net_id, const int32_t* prog, int32_t nrows,
                 const float* blob, int64_t blob_floats,
                 int32_t nbuf, const int64_t* buf_elems,
                 int32_t in_h, int32_t in_w, int32_t in_c, int32_t out_dim);
/* Load a program whose parameter blob is byte-identical to net src_id's (e.g. the same ResNet compiled for another window
 * width): iss_cnn_load minus the blob.  No parameter upload and no hi / lo split: the device parameter arrays (f32 and the
 * bf16 / fp16 halves) are shared and reference-counted, so unloading either net leaves the other valid.  The rows are
 * validated against the source's blob size; f16 eligibility is the source's; the precision state starts as a fresh load's.
 * Per-program state (im2col tables, weight sums, packed dense weights, buffer plan) is the new net's own.  Replaces, for the
 * shorter last window of every file (vbx_segmenter.py:234-243), a full reload of the same ResNet-101 parameters.       */
int iss_cnn_load_shared(iss_ctx* ctx, int net_id, int src_id, const int32_t* prog, int32_t nrows,
                        int32_t nbuf, const int64_t* buf_elems,
                        int32_t in_h, int32_t in_w, int32_t in_c, int32_t out_dim);

/* Class probabilities of n 20 ms slots.  win_row[i] = first mspec row of the 68-frame
 * window feeding slot i (the host applies the 17-left/16(+1)-right edge replication of
 * segmenter.py:83-84 when it builds this list); nmel columns are used (21 or 24,
 * segmenter.py:146-147).  Per window: z-normalisation with population std
 * (segmenter.py:82) and finite_out[i] = all(isfinite(normalised patch)) (:86); windows
 * that are not finite get probs 0.5 (segmenter.py:175).                         */
int iss_cnn_probs(iss_ctx* ctx, int net_id, const int32_t* win_row, int32_t n,
                  float* probs_out /* n*out_dim */, uint8_t* finite_out /* n */);

/* Asynchronous form: enqueues the same work on the context's stream and returns; win_row
 * is consumed before the call returns, probs_out / finite_out (page-locked memory from
 * iss_host_alloc if the copy is to overlap host work) are valid after iss_wait(ctx, ticket)
 * (or any other call that synchronises the context), and front to back as iss_wait_slots reports.  The resident mel spectrogram must not
 * be replaced before iss_wait.  Lets the host run the Viterbi of one network
 * (segmenter.py:176) while the device already evaluates the next one.
 *
 * Dead windows.  A window that holds a non-finite log-mel value (digital silence gives whole -inf rows) is certainly not finite:
 * its mean is non-finite.  Both calls leave such windows out of the network's passes and write their 0.5 / finite = 0 rows directly; the
 * live windows run as a shorter list in the caller's order (their arithmetic is unchanged; tile boundaries move as they do with
 * the pass size, and the shared-first-layer decision is taken on the live list, so a list with many dead windows may run the
 * per-window first layer where compute-then-mask shares it: the same values to float32 rounding), and a call without a dead window runs exactly as before.  Windows of finite values that do not normalise
 * (std = 0, overflow) stay in the list and are decided on the device as ever.  Which windows are dead is known on the host from
 * one byte per log-mel row (row_flags_kernel; iss_set_mspec scans its argument instead).  iss_sidekit enqueues that kernel and its
 * read-back behind the feature kernel, and the wait of iss_get_loge brings the bytes along with the log-energy: no further wait.
 * Features that came another way have them fetched at the FIRST of these calls, with ONE wait for the stream.  The
 * precision guard probes the live list.  ISS_DIAG_NO_SKIP_DEAD restores compute-then-mask.  iss_cnn_dead_stats: windows
 * these calls were given, and how many of them were left out, since the context was created (0 left out under the switch). */
int iss_cnn_probs_async(iss_ctx* ctx, int net_id, const int32_t* win_row, int32_t n,
                        float* probs_out /* n*out_dim */, uint8_t* finite_out /* n */, int64_t* ticket_out);
int iss_cnn_dead_stats(iss_ctx* ctx, int64_t* windows, int64_t* dead);
/* Block until the work of `ticket` (and everything enqueued before it) is complete; ticket < 0 = the whole stream.  A wait for
 * the newest ticket, or for the whole stream, retires every ticket given out so far. */
int iss_wait(iss_ctx* ctx, int64_t ticket);
/* Landings.  The result of an iss_cnn_probs_async call reaches probs_out / finite_out front to back.  When both arrays are
 * page-locked (iss_host_alloc), every pass of the call (the workspace limit decides how many windows a pass holds) stores its rows
 * straight into them -- they are device-visible; scatter_probs_kernel writes each element once, 0.5 where the window did not
 * normalise -- and an event behind the pass says that its slots are there: its own windows' and the dead slots up to the next live
 * window, which the call itself wrote before it returned.  No copy follows a pass or the call, and the values are those of the
 * synchronous call.  With a pageable array the call gathers its result on the device and copies it out once, behind the last
 * pass, one landing: a copy into pageable memory would hold the submitting thread.
 * iss_wait_slots blocks until slots [0, upto) of call `ticket` are in the caller's arrays and reports in *landed_out how many
 * slots are: >= min(upto, n), never less than an earlier answer for the ticket, n once the call is complete.  upto <= 0 does not
 * block (hipEventQuery).  A ticket that iss_wait has retired, or that was never given out, answers 2^31 - 1: everything has
 * landed.  Tickets are retired by iss_wait alone. */
int iss_wait_slots(iss_ctx* ctx, int64_t ticket, int32_t upto, int32_t* landed_out);

/* Generic batched forward on caller-supplied host input (n, in_h, in_w, in_c) f32 NHWC:
 * replaces vbx_segmenter.py:262-266 `OnnxBackendExtractor.get_embedding` (ResNet-101
 * of resnet.py:78-135, one launch sequence for many windows instead of batch 1).  */
int iss_cnn_forward(iss_ctx* ctx, int net_id, const float* x, int32_t n, float* out /* n*out_dim */);

/* Arithmetic mode of the conv/dense GEMMs.  gfx950 has no xf32 / TF32 and its f32-input MFMA runs at 1/16 of the 16-bit rate, so
 * both operands are split x = hi + lo into 16-bit halves and every k-step issues three MFMAs (lo.hi + hi.lo + hi.hi, f32 accumulate):
 *   ISS_PREC_F16X3   (default since round 6) fp16 halves, 11 + 11 mantissa bits, v_mfma_f32_32x32x16_f16, in the kernels that carry the
 *                    segmenter nets' arithmetic (conv_x3_wq_kernel, conv_x3_wq3h_kernel, conv_x3_pw_kernel, and the per-window first
 *                    layer of scattered window lists, conv1_patch_x3_kernel); exact f32 for their
 *                    small trailing layers; bf16 halves in every kernel without an fp16 instantiation.  Needs parameters and
 *                    activations inside fp16's range (|x| < 65504; beyond it a result is NaN).  Parameters are checked at load, and
 *                    activations can only be checked by the precision guard's probe, which runs on iss_cnn_probs /
 *                    iss_cnn_probs_async: so fp16 halves are taken by PATCH networks with every parameter in range, run through
 *                    those two calls, and by nothing else.  A network with a larger parameter, and every network run through
 *                    iss_cnn_forward or iss_vbx_embed (the x-vector ResNet among them), runs ISS_PREC_BF16X3 in this mode, and
 *                    iss_cnn_precision_info reports that.  max |d log p| against exact f32 on the stand-ins: 4.7e-5
 *                    (profiles/r06_f16_ab.txt), the speed of ISS_PREC_BF16X3 within 1 %;
 *   ISS_PREC_BF16X3  bf16 halves, 8 + 8 mantissa bits, v_mfma_f32_32x32x16_bf16, in every GEMM kernel: operand error 2^-16 relative,
 *                    max |d log p| 2.9e-4 on the same data (the default of rounds 1-5);
 *   ISS_PREC_F32     v_mfma_f32_32x32x2_f32, bit-wise an fmaf chain (reference-grade, ~3 x slower).                          */
#define ISS_PREC_BF16X3 0
#define ISS_PREC_F32    1
#define ISS_PREC_F16X3  2
int iss_set_precision(iss_ctx* ctx, int mode);

/* Precision guard for weights nobody has measured (north star: "frame logits within 1e-3 fp32"; segmenter.py:163,176 --
 * the reference's emissions are log(predict(...)) in f32).  How far inside that bound a split mode sits depends on the activation
 * ranges of the weights actually loaded (tests/precision_emulation.py, profiles/r06_precision_emulation.txt).  So the FIRST
 * iss_cnn_probs / iss_cnn_probs_async call of a patch network in a split mode first runs up to 256 of the call's own windows
 * (four runs of consecutive slots spread over the list) in that mode and in exact f32, records max |log p_split - log p_f32| over
 * every class of every finite window, and -- when that exceeds `threshold` (default 5e-4, half the bound; a NaN, i.e. an activation
 * beyond fp16's range, always does) -- switches THIS network until the context's mode changes: to the other split mode if that one
 * passes the same probe (the same speed), else to ISS_PREC_F32.  A call none of whose probed windows is finite (e.g. all over -inf
 * mel rows) gives the probe nothing to compare: the network stays ISS_GUARD_PENDING (0 windows compared) and its next call probes again.
 * iss_set_precision with a mode other than the context's current one re-arms every loaded network the caller has not pinned with
 * iss_cnn_set_net_precision: the guard's decision is dropped (ISS_GUARD_PENDING, probe figures -1 / 0 windows), the network runs the
 * new mode, and its next iss_cnn_probs call probes it again (a network whose first call ran in exact f32 included).
 * iss_set_precision_guard: threshold <= 0 disables the probe (networks loaded later are not probed; already decided ones keep their
 * mode).  A threshold change is not a mode change: it re-arms nothing.
 * iss_cnn_precision_info: mode in use for the network (ISS_PREC_*, the one it actually runs: see ISS_PREC_F16X3), the probe's figure
 * for the mode that was asked for (-1 if not probed), the windows it compared, ISS_GUARD_* state, and the figure of the mode in use
 * (0 for exact f32).
 * iss_cnn_set_net_precision: caller's override for one network (-1 = follow the context again); marks it decided, and the override
 * survives iss_set_precision (it is never probed). */
#define ISS_GUARD_PENDING   0   /* not probed yet                                              */
#define ISS_GUARD_PASSED    1   /* probed: within the threshold, mode kept                     */
#define ISS_GUARD_ESCALATED 2   /* probed: above the threshold, the network runs another mode  */
#define ISS_GUARD_FIXED     3   /* mode set by the caller (iss_cnn_set_net_precision) or the context was in exact-f32 mode at the first call */
int iss_set_precision_guard(iss_ctx* ctx, float threshold);
int iss_cnn_precision_info(iss_ctx* ctx, int id, int32_t* mode, float* max_dlogp, int32_t* slots, int32_t* state, float* dlogp_in_use);
int iss_cnn_set_net_precision(iss_ctx* ctx, int id, int mode);

/* Kernel-selection switches for same-box A/B measurements and for the tests that compare two device paths with each
 * other (e.g. the shared first layer against the per-window one).  0 (default) = production selection.  The library never
 * reads the environment for these: inaspeechsegmenter_amd/_native.py maps the ISS_DIAG environment variable (a
 * comma-separated list of the names below, lower case, without the prefix) onto this call when a context is created.  */
#define ISS_DIAG_NO_SHARED_FIRST 0x001u  /* per-window first layer instead of the shared one (segmenter.py:82 per window)   */
#define ISS_DIAG_NO_FLROWS       0x002u  /* first_layer_raw_kernel instead of first_layer_rows_kernel                        */
#define ISS_DIAG_NO_WS           0x004u  /* no weight-stationary footprint kernel (conv_x3_fp_kernel everywhere)             */
#define ISS_DIAG_NO_WS3          0x008u  /* no NH = 2 weight-stationary kernel for the 3x3 layers                            */
#define ISS_DIAG_NO_DIRECT1      0x010u  /* no direct f32 kernel for one-channel 3x3 first layers                            */
#define ISS_DIAG_NO_NH2          0x020u  /* conv_x3_fp_kernel: 64 output channels per workgroup                              */
#define ISS_DIAG_NO_TR           0x040u  /* conv_x3_fp_kernel: row-major epilogue                                            */
#define ISS_DIAG_NO_PW           0x080u  /* 1x1 layers on the generic gather kernel                                          */
#define ISS_DIAG_NO_PWS          0x100u  /* 1x1 layers on the round-2 pointwise kernel                                       */
#define ISS_DIAG_NO_PWS2         0x200u  /* 1x1 layers: 64-column tiles only                                                 */
#define ISS_DIAG_NO_WQ           0x400u  /* conv_x3_ws_kernel (two waves per SIMD) instead of conv_x3_wq_kernel for the fused 5x3 layer */
#define ISS_DIAG_NO_DUAL         0x800u  /* projection shortcut + expansion as two launches (ISS_C_DUALW ignored)            */
#define ISS_DIAG_NO_CHAIN        0x1000u /* identity-residual expansion and the next block's reduction as two launches       */
#define ISS_DIAG_NO_RING         0x2000u /* no ring form of the weight-stationary kernel (second convs with > 16 taps: gather kernel) */
#define ISS_DIAG_NO_FSAME        0x4000u /* a zero-padded ('same') first layer is run per window, not shared between windows  */
#define ISS_DIAG_NO_F32WS        0x8000u /* exact-f32 mode: conv_igemm_kernel everywhere (no F32 form of the weight-stationary kernel) */
#define ISS_DIAG_NO_NCB1         0x10000u /* layers with <= 32 output channels on the 64-column forms (no NCB = 1 form)                 */
#define ISS_DIAG_NO_WSU3         0x20000u /* unpadded 3x3 layers with 64 / 96 output channels on conv_x3_fp_kernel                      */
#define ISS_DIAG_NO_GFUSED       0x40000u /* the generic gather kernel never reads the shared first-layer rows (per-window first layer)  */
#define ISS_DIAG_NO_HL           0x80000u /* f32 NHWC activations between the footprint kernels (no CHL layout: conv_x3_wq3_kernel instead of conv_x3_wq3h_kernel) */
#define ISS_DIAG_NO_SKIP_DEAD    0x100000u /* windows over non-finite log-mel values run through the network and are masked afterwards   */
#define ISS_DIAG_ALL             0x1fffffu
int iss_set_diag(iss_ctx* ctx, uint32_t flags);

/* FLOPs (2*MAC of the conv/dense outputs actually computed) per sample of a loaded network. */
int iss_cnn_flops(iss_ctx* ctx, int net_id, double* flops_per_sample);

/* ------------------------------------------------ VBx 64-band fbank front end
 * replaces vbx_segmenter.py:72-89 `get_features` (features_vbx.py:62-149).
 * window = povey_window(400) f64; melbank = mel_fbank_mx(...) (257,64) f64 row-major.
 * sig_i32 = (signal * 2**15).astype(int) (vbx_segmenter.py:85); dither_u = the
 * np.random.seed(3) uniform stream of n doubles (features_vbx.py:127-128), generated
 * on the host because it is an MT19937 stream.  out = (T,64) f32, T = n/160 style
 * count *T_out = (n + 320 - 400)/160 + 1.                                        */
int iss_vbx_tables(iss_ctx* ctx, const double* window400, const double* melbank_257x64);
int iss_vbx_features(iss_ctx* ctx, const int32_t* sig_i32, const double* dither_u, int64_t n,
                     float* fea_out /* T*64, may be NULL to keep on device */, int32_t* T_out);
/* Same for PCM16 sources (what io.py's ffmpeg hop yields: (signal * 2**15).astype(int) is then the PCM itself) with a
 * dither stream cached on the device: np.random.seed(3) gives every file the same stream, so upload its longest prefix
 * once (iss_vbx_set_dither) and send 2 bytes per sample afterwards.                                                    */
int iss_vbx_set_dither(iss_ctx* ctx, const double* dither_u, int64_t n);
int iss_vbx_features_pcm16(iss_ctx* ctx, const int16_t* pcm, int64_t n,
                           float* fea_out /* T*64 or NULL */, int32_t* T_out);
/* F files of PCM16 concatenated (file f = pcm[sample_off[f] .. sample_off[f+1]), F+1 offsets), each >= 200 samples; dither =
 * the cached stream (iss_vbx_set_dither), long enough for the LONGEST file: every file restarts at u[0] (vbx_segmenter.py:84).
 * Leaves ONE resident (sum T_f, 64) f32 arena for iss_vbx_embed (window starts are arena rows); frame_off_out[f] = first
 * frame of file f (F+1 entries).  The frames of file f are bit-identical to iss_vbx_features_pcm16 on that file alone.
 * Three launches per batch (fbank over all frames, one cumsum wavefront per file, one ragged CMN), where a loop over
 * iss_vbx_features_pcm16 makes three per file.  ISS_EINVAL: a file under 200 samples or over the per-file limit, or more than
 * 2^31 - 8192 frames in all.  Replaces a per-file loop over get_features (vbx_segmenter.py:72-89).                      */
int iss_vbx_features_batch_pcm16(iss_ctx* ctx, const int16_t* pcm, const int64_t* sample_off, int32_t nfiles,
                                 int32_t* frame_off_out, float* fea_out /* (sum T_f)*64, or NULL: stay resident */);
/* The same batch front end on parts of the RESIDENT PCM16 signal (iss_signal_pcm16*, or what a decode / resample pass wrote
 * there): part p = samples [sample_begin[p], sample_begin[p] + sample_count[p]) of the signal.  Nothing is uploaded but the part
 * table.  The parts need not touch and may come in any order: a pass leaves a gap up to the next multiple of 160 behind every
 * part, so each part carries its own length; none is derived from the next offset.  Per part: its own framing, reflect padding,
 * cumsum and CMN; the cached dither stream restarts at u[0].  Leaves the resident (sum T_p, 64) f32 arena iss_vbx_embed reads,
 * parts in the order given; frame_off_out[p] = first arena row of part p (nparts + 1 entries).  Three launches per call.
 * Contract:
 *   - the frames of part p are bit-identical to iss_vbx_features_pcm16 on those samples alone;
 *   - no sample outside a part is read: not the gap behind it, not a neighbouring part, not what lies past the signal's end;
 *   - ISS_EINVAL, nothing launched and nothing resident changed: a part under 200 samples or over the per-file limit, a part
 *     outside the signal, two parts that overlap, more than 2^31 - 8192 frames in all;
 *   - ISS_ESTATE, likewise: no tables (iss_vbx_tables), a cached dither stream shorter than the longest part, a resident
 *     signal that is not PCM16 (iss_signal_f32) or none.
 * iss_vbx_resident_stats: calls that launched (one fbank launch each) and parts they took, since the context was created.  */
int iss_vbx_features_resident(iss_ctx* ctx, const int64_t* sample_begin, const int64_t* sample_count, int32_t nparts,
                              int32_t* frame_off_out, float* fea_out /* (sum T_p)*64, or NULL: stay resident */);
int iss_vbx_resident_stats(iss_ctx* ctx, int64_t* launches, int64_t* parts);
/* x-vectors of n windows [starts[i], starts[i] + frames) of the RESIDENT features (frames = the loaded network's input
 * width; its first conv must be a window-mode conv, ISS_C_INMODE 2): replaces the window loop of
 * vbx_segmenter.py:222-231 + get_embedding (:262-266) without copying windows through the host.                        */
int iss_vbx_embed(iss_ctx* ctx, int net_id, const int32_t* starts, int32_t n, float* out /* n*out_dim */);

/* ------------------------------------------- multi-GPU: the single exchange step
 * Long archives shard file-parallel over the GPUs of one node (one process per GPU; files
 * are independent units, segmenter.py:314-327 / scripts/ina_speech_segmenter_pyro_server.py:
 * 34-68).  After local processing every rank holds a table of int32 rows
 * (file_id, label_id, start_slot, stop_slot); ONE ncclAllGather (RCCL over xGMI) of
 * fixed-capacity buffers with a header row (n_rows, capacity, rank, 0) leaves every
 * rank's rows on every rank.  librccl is dlopen'ed on first use: single-GPU users do not
 * need it.  Rendezvous: rank 0 calls iss_comm_unique_id and hands the 128 bytes to the
 * other ranks by any out-of-band means (inaspeechsegmenter_amd/sharding.py uses a TCP
 * socket on MASTER_ADDR); then every rank calls iss_comm_init.                        */
#define ISS_COMM_ID_BYTES 128
int iss_comm_unique_id(iss_ctx* ctx, uint8_t id_out[ISS_COMM_ID_BYTES]);
int iss_comm_init(iss_ctx* ctx, const uint8_t id[ISS_COMM_ID_BYTES], int32_t rank, int32_t world);
int iss_comm_destroy(iss_ctx* ctx);
/* local_rows: (n_local,4) int32.  all_rows: (world*capacity,4) int32, rank r's rows start at
 * r*capacity; counts[r] = rows rank r HAS (may exceed capacity: then only the first
 * `capacity` arrived and the caller repeats the call with capacity >= max(counts)).
 * Failure handling (the reference's Pyro workers fail independently, scripts/ina_speech_segmenter_pyro_client.py:64-74;
 * a collective cannot): a rank whose local work failed still takes part with n_local = -1, every rank then sees
 * counts[r] == -1 and raises; a rank that is GONE makes the others wait ISS_COMM_TIMEOUT_S seconds (environment,
 * default 1800), after which the communicator is aborted (ncclCommAbort) and the call returns ISS_ETIMEOUT.          */
int iss_allgather_segments(iss_ctx* ctx, const int32_t* local_rows, int32_t n_local, int32_t capacity,
                           int32_t* all_rows, int32_t* counts /* world */);
/* max over ranks of a double (bench timing) and a barrier, on the same communicator */
int iss_comm_allreduce_max(iss_ctx* ctx, double* value);
/* what RCCL itself reports for the communicator: ncclCommCount / ncclCommUserRank / ncclGetVersion and the path of
 * the librccl that was bound (audit trail of the multi-GPU bench line) */
int iss_comm_info(iss_ctx* ctx, int32_t* world, int32_t* rank, int32_t* version, char* lib_path, int32_t lib_path_len);

/* ------------------------------------------------------------ profiling hooks */
/* Accumulated device time (ms, hipEvent-timed on the context's stream), launch count and algorithmic flops of the
 * kernel classes since the last reset.  kind: 0 = all conv/dense implicit-GEMM kernels, 1 = sidekit / vbx fbank front
 * end, 2 = everything else; 3.. = the GEMM kernels one by one (each launch counted in 0 AND in its own class).       */
#define ISS_PROF_GEMM      0
#define ISS_PROF_FRONTEND  1
#define ISS_PROF_OTHER     2
#define ISS_PROF_WS        3   /* conv_x3_ws_kernel   (weight-stationary footprint kernel) */
#define ISS_PROF_FP        4   /* conv_x3_fp_kernel   (streaming-weights footprint kernel) */
#define ISS_PROF_PW        5   /* conv_x3_pw_kernel   (1x1 / dense persistent GEMM) */
#define ISS_PROF_GATHER    6   /* conv_x3_kernel      (generic gather GEMM) */
#define ISS_PROF_PATCH1    7   /* conv1_patch_x3_kernel (per-window first layer) */
#define ISS_PROF_F32       8   /* conv_igemm_kernel   (exact-f32 MFMA mode) */
#define ISS_PROF_KINDS     9
int iss_prof_enable(iss_ctx* ctx, int on);
int iss_prof_get(iss_ctx* ctx, int kind, double* ms, int64_t* launches, double* flops);
int iss_prof_reset(iss_ctx* ctx);
/* Per-layer view of the same HIP-event brackets: time and launch count of op-program row `row` (the conv / dense row of
 * the loaded network that a launch executed; rows of different networks share the index space) since the last reset. */
#define ISS_PROF_ROWS      512
int iss_prof_get_row(iss_ctx* ctx, int row, double* ms, int64_t* launches);
/* Per kernel INSTANTIATION: entry `index` (0, 1, ... until ISS_EINVAL) of the list of distinct kernel instantiations
 * launched since the last reset -- name with its template arguments spelled out (e.g.
 * "conv_x3_ws_kernel<5,3,false,false,true,1,1>"), accumulated HIP-event time, launches and algorithmic flops.  This is what
 * bench.py's roofline.dominant is computed from.                                                                        */
int iss_prof_get_instance(iss_ctx* ctx, int index, char* name_out, int32_t name_len, double* ms, int64_t* launches, double* flops);

/* ------------------------------------------------------------------ test aid
 * Overwrites scratch, not state.  After a stream sync, fills the full CAPACITY (not the used size) of every device
 * buffer of the context that holds no state with the 32-bit `word`: the activation buffers with their slack, the shared
 * first-layer rows, statistics, finite flags, window lists, row flags, the CNN input / output staging, the x-vector
 * front end's sample / filter-bank / offset buffers, and the source, job, status and staging buffers of the resampler
 * and the decoders.  Untouched: the resident signal and features (log-mel, log-energy, x-vector features), the cached
 * dither stream, every table and every network's parameters.  The row flags of the resident features are recomputed at
 * the next call that needs them.  A result of the library is a function of its inputs, parameters, mode and switches
 * only, so no call made afterwards may return anything else than before: the tests use this entry with NaN, -inf, 0 and
 * FLT_MAX to hold that.  What iss_flac_get_stage / iss_adpcm_get_stage would return is gone, and so is every payload an
 * origin of iss_resample_staged_mix held: that call is ISS_ESTATE until a new survey or decode call.  Not for production. */
int iss_scribble(iss_ctx* ctx, uint32_t word);

/* The operand split of the conv kernels over an array: x[i] = hi + lo with hi = rne16(x[i]), lo = rne16(x[i] - hi), the
 * halves fp16 (f16 != 0) or bf16, as 16-bit patterns in hi_out[i] / lo_out[i] (n values each, host memory like x).
 * form 0: four values at a time, the way the kernels split an f32 input (split4_pk); form 1: one value at a time, the
 * way their epilogues split an output.  Not for production.                                                          */
int iss_diag_split16(iss_ctx* ctx, const float* x, int64_t n, int32_t f16, int32_t form, uint16_t* hi_out, uint16_t* lo_out);

/* ------------------------------------------------------------------ host only
 * Viterbi smoothing, replaces pyannote_viterbi.py:118-224 `viterbi_decoding` on the
 * unconstrained path the segmenter uses (segmenter.py:72-73,176): float64 scores,
 * uniform initial log(1/K), argmax takes the FIRST maximum, back-tracking :217-220.
 * emission (T,K) row-major; f32 variant promotes each value to double exactly like
 * numpy does when `np.log(r)` (float32) is added to float64 (segmenter.py:176).
 * transition (K,K) row-major, T[i][j] = i -> j.  K <= 16.                        */
int iss_viterbi_f64(const double* emission, int64_t T, int32_t K, const double* transition,
                    int32_t* states_out);
int iss_viterbi_f32(const float* emission, int64_t T, int32_t K, const double* transition,
                    int32_t* states_out);
/* nseg consecutive segments of one (sum(seg_len), K) emission array, each smoothed on its own like iss_viterbi_f32
 * (the per-segment loop of segmenter.py:168-178 in one call).                                                          */
int iss_viterbi_segments_f32(const float* emission, const int64_t* seg_len, int64_t nseg, int32_t K,
                             const double* transition, int32_t* states_out);
/* `_energy_activity` behind its threshold (segmenter.py:69-73): raw activity loge[t] > threshold (float64 compare),
 * pred2logemission (viterbi_utils.py:29-34; the caller passes numpy's log(eps) and log(1 - eps)), two-state Viterbi with the
 * (2,2) transition matrix of log_trans_exp (viterbi_utils.py:36-42).  states_out[t] in {0, 1}.                         */
int iss_energy_viterbi(const float* loge, int64_t T, double threshold, double log_eps, double log_1m_eps,
                       const double* transition, int32_t* states_out);

#ifdef __cplusplus
}
#endif
#endif /* ISS_H */
