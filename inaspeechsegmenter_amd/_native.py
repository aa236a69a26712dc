"""ctypes binding of libiss_hip.so (include/iss.h).  No fallback: if the shared library is
missing, or a device call is made without a usable gfx950 GPU, this raises.

The library is built in-tree by `__graft_entry__.build()` (hipcc, --offload-arch=gfx950).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ISS_LIB') or os.path.join(_HERE, 'libiss_hip.so')      # ISS_LIB: another build of the library (A/B runs)

PROG_COLS = 32
OP_CONV, OP_POOL, OP_SOFTMAX, OP_STATPOOL, OP_ACT, OP_ELT = 1, 2, 3, 4, 5, 6
(ELT_COPY, ELT_ADD, ELT_SUB, ELT_MUL, ELT_MAX, ELT_MIN, ELT_AVG, ELT_ZERO, ELT_PERMUTE) = range(9)     # ISS_OP_ELT kinds (ISS_C_ACT)
(C_OP, C_IN, C_OUT, C_RES, C_H, C_W, C_CIN, C_HO, C_WO, C_COUT, C_KH, C_KW, C_SH, C_SW, C_PT, C_PL,
 C_ACT, C_WOFF, C_BOFF, C_PSOFF, C_PTOFF, C_INMODE, C_POOLKIND, C_ORDER, C_FPOOLH, C_FPOOLW, C_DUALW, C_DUALB, C_ACTPARAM, C_ACTPARAM2, C_ACTPARAM3) = range(31)
PREC_BF16X3, PREC_F32, PREC_F16X3 = 0, 1, 2
K_ALIGN = 32          # conv weight rows are padded to a multiple of this many k
BUF_INPUT = -2
MAX_NETS = 8
# iss_resample_job (include/iss.h) and the ISS_RS_* format of each stored sample dtype
RS_JOB = np.dtype([('src_offset', '<i8'), ('frames_in', '<i8'), ('channels', '<i4'), ('format', '<i4'), ('filter', '<i4'),
                   ('reserved', '<i4'), ('dst_offset', '<i8'), ('frames_out', '<i8')])
RS_FORMAT = {np.dtype(np.uint8): 0, np.dtype('<i2'): 1, np.dtype('<i4'): 2, np.dtype('<f4'): 3, np.dtype('<f8'): 4}
# formats a dtype does not tell: signed 8-bit, G.711 mu-law / A-law bytes, and the big-endian flag of the 2/4/8-byte formats
RS_I8, RS_ULAW, RS_ALAW, RS_SWAP = 8, 9, 10, 0x100
# iss_adpcm_job (include/iss.h) and the ISS_ADPCM_* block status codes
ADPCM_JOB = np.dtype([('src_offset', '<i8'), ('block_begin', '<i8'), ('nblocks', '<i8'), ('frames_total', '<i8'), ('channels', '<i4'),
                      ('block_align', '<i4'), ('output', '<i4'), ('filter', '<i4'), ('dst_offset', '<i8'), ('frames_out', '<i8')])
ADPCM_TO_SIGNAL, ADPCM_TO_STAGE = 0, 1
ADPCM_STATUS = {1: 'step index above 88', 2: 'predictor index above 6'}
# iss_flac_info / iss_flac_frame / iss_flac_job (include/iss.h)
FLAC_INFO = np.dtype([('sample_rate', '<i4'), ('channels', '<i4'), ('bps', '<i4'), ('min_block', '<i4'), ('max_block', '<i4'),
                      ('reserved', '<i4'), ('total_samples', '<i8')])
FLAC_FRAME = np.dtype([('offset', '<i8'), ('length', '<i8'), ('first_sample', '<i8'), ('block_size', '<i4'),
                       ('channel_mode', '<i4'), ('bps', '<i4'), ('header_bytes', '<i4')])
FLAC_JOB = np.dtype([('src_offset', '<i8'), ('frame_begin', '<i8'), ('nframes', '<i8'), ('frames_total', '<i8'), ('channels', '<i4'),
                     ('bps', '<i4'), ('output', '<i4'), ('filter', '<i4'), ('dst_offset', '<i8'), ('frames_out', '<i8')])
FLAC_TO_SIGNAL, FLAC_TO_STAGE = 0, 1
# iss_window (include/iss.h): the row beside a job row of the *_windows entry points
WINDOW = np.dtype([('s_begin', '<i8'), ('s_end', '<i8'), ('frames_total', '<i8'), ('out_begin', '<i8'), ('out_count', '<i8')])
# iss_split (include/iss.h): the row beside a job row of the *_split entry points
SPLIT = np.dtype([('dst_stride', '<i8'), ('sel_begin', '<i4'), ('sel_count', '<i4')])
# iss_mixset / iss_mix / iss_mix_term (include/iss.h): the row beside a job row of the *_mix entry points, and the call's two tables
MIXSET = np.dtype([('dst_stride', '<i8'), ('mix_begin', '<i4'), ('mix_count', '<i4')])
MIX = np.dtype([('term_begin', '<i4'), ('term_count', '<i4'), ('divisor', '<f8')])
MIX_TERM = np.dtype([('channel', '<i4'), ('reserved', '<i4'), ('weight', '<f8')])
# iss_sched / iss_sched_run (include/iss.h, "Schedules"): the row beside a job row of the *_sched entry points, and the call's run rows
SCHED = np.dtype([('run_begin', '<i4'), ('run_count', '<i4')])
SCHED_RUN = np.dtype([('begin_frame', '<i8'), ('mix', '<i4'), ('reserved', '<i4')])
# iss_survey_job (include/iss.h): a row of the survey entry points
SET =np.dtype([('member_begin', '<i4'), ('member_count', '<i4')])                                       # iss_set, beside every job
SET_MEMBER = np.dtype([('src_offset', '<i8'), ('frames', '<i8'), ('channels', '<i4'), ('reserved', '<i4')])   # iss_set_member
SURVEY_JOB = np.dtype([('src_offset', '<i8'), ('frames_in', '<i8'), ('channels', '<i4'), ('format', '<i4'), ('full', '<f8')])
# ISS_FLAC_* frame status codes -> reason
FLAC_STATUS = {1: 'reserved subframe type', 2: 'subframe header padding bit set', 3: 'wasted bits exceed the sample size',
               4: 'reserved residual coding method', 5: 'residual partition order does not fit the block',
               6: 'invalid LPC precision', 7: 'negative LPC shift', 8: 'residual overruns the frame',
               9: 'nonzero padding before the footer', 10: 'subframes end before the footer', 11: 'CRC-16 mismatch'}


STAGED_ORIGIN = {None: 0, 'flac': 1, 'adpcm': 2, 'msadpcm': 3}      # ISS_STAGED_*: the origins of iss_resample_staged_mix


class NativeError(RuntimeError):
    pass


def _window_rows(windows, njobs):
    """WINDOW rows for a *_windows entry point: one beside every job."""
    wn = np.ascontiguousarray(np.array(windows, dtype=WINDOW).reshape(-1))
    if wn.size != njobs:
        raise ValueError(f'{wn.size} windows for {njobs} jobs')
    return wn


def _split_rows(splits, njobs):
    """(SPLIT rows, int32 channel table) for a *_split entry point from one `(dst_stride, [channels])` or None (downmix) per
    job; a pair of arrays (SPLIT rows, channel table) is handed on as given."""
    if isinstance(splits, tuple) and len(splits) == 2 and isinstance(splits[0], np.ndarray):
        rows, sel = np.ascontiguousarray(splits[0], dtype=SPLIT).reshape(-1), np.ascontiguousarray(splits[1], dtype=np.int32)
    else:
        rows, sel = np.zeros(len(splits), dtype=SPLIT), []
        for k, sp in enumerate(splits):
            if sp is not None:
                rows[k] = (int(sp[0]), len(sel), len(sp[1]))
                sel.extend(int(ch) for ch in sp[1])
        sel = np.array(sel, dtype=np.int32)
    if rows.size != njobs:
        raise ValueError(f'{rows.size} splits for {njobs} jobs')
    return rows, sel


def _mix_rows(mixes, njobs):
    """(MIXSET rows, MIX rows, MIX_TERM rows) for a *_mix entry point from one `(dst_stride, [mix, ...])` or None (downmix) per
    job, a mix being a resample.Mix or a channel index (that channel alone); a triple of arrays is handed on as given."""
    if isinstance(mixes, tuple) and len(mixes) == 3 and isinstance(mixes[0], np.ndarray):
        sets, rows, terms = (np.ascontiguousarray(a, dtype=dt).reshape(-1) for a, dt in zip(mixes, (MIXSET, MIX, MIX_TERM)))
    else:
        sets, rows, terms = np.zeros(len(mixes), dtype=MIXSET), [], []
        for k, ms in enumerate(mixes):
            if ms is not None:
                sets[k] = (int(ms[0]), len(rows), len(ms[1]))
                for m in ms[1]:
                    t, d = (((m, 1.0),), 1.0) if isinstance(m, (int, np.integer)) else (m.terms, m.divisor)
                    rows.append((len(terms), len(t), float(d)))
                    terms.extend((int(ch), 0, float(w)) for ch, w in t)
        rows, terms = np.array(rows, dtype=MIX).reshape(-1), np.array(terms, dtype=MIX_TERM).reshape(-1)
    if sets.size != njobs:
        raise ValueError(f'{sets.size} mix sets for {njobs} jobs')
    return sets, rows, terms


def _sched_rows(scheds, njobs):
    """(SCHED rows, SCHED_RUN rows, MIX rows, MIX_TERM rows) for a *_sched entry point from one schedule per job: a
    resample.Schedule, or a sequence of (begin_frame, mix) with mix a resample.Mix or None (the plain downmix: -1).  Equal mixes of
    a call share a row.  A 4-tuple of arrays is handed on as given."""
    if isinstance(scheds, tuple) and len(scheds) == 4 and isinstance(scheds[0], np.ndarray):
        sc, runs, rows, terms = (np.ascontiguousarray(a, dtype=dt).reshape(-1) for a, dt in zip(scheds, (SCHED, SCHED_RUN, MIX, MIX_TERM)))
    else:
        sc, runs, rows, terms, seen = np.zeros(len(scheds), dtype=SCHED), [], [], [], {}
        for k, s in enumerate(scheds):
            mine = list(s)
            sc[k] = (len(runs), len(mine))
            for begin, m in mine:
                if m is not None and m not in seen:
                    seen[m] = len(rows)
                    rows.append((len(terms), len(m.terms), float(m.divisor)))
                    terms.extend((int(ch), 0, float(w)) for ch, w in m.terms)
                runs.append((int(begin), -1 if m is None else seen[m], 0))
        runs = np.array(runs, dtype=SCHED_RUN).reshape(-1)
        rows, terms = np.array(rows, dtype=MIX).reshape(-1), np.array(terms, dtype=MIX_TERM).reshape(-1)
    if sc.size != njobs:
        raise ValueError(f'{sc.size} schedules for {njobs} jobs')
    return sc, runs, rows, terms


def _sched_fades(scheds, fades, nruns):
    """The half-widths of a *_sched_fade entry point (include/iss.h, "Fades"), one int32 per run row, or None where no run
    fades in: then the *_sched entry point is called.  fades: None -- what the resample.Schedule objects among `scheds` carry --,
    or the array itself (with schedules given as arrays, or to hand the library rows a Schedule would refuse)."""
    given = fades is not None
    if not given:
        if isinstance(scheds, tuple) and len(scheds) == 4 and isinstance(scheds[0], np.ndarray):
            return None
        fades = [h for s in scheds for h in (getattr(s, 'fades', None) or (0,) * len(list(s)))]
    fades = np.ascontiguousarray(fades, dtype=np.int32).reshape(-1)
    if fades.size != nruns:
        raise ValueError(f'{fades.size} fades for {nruns} runs')
    return fades if given or fades.any() else None      # (an array given goes to the library as it is, all 0 or not)


def _set_rows(jb, members):
    """(job rows, SET rows, SET_MEMBER rows) for a *_set entry point (include/iss.h, "File sets").  members: per job a list of
    `(byte offset, frames, channels)`, the offset counted from the job row's src_offset -- where the job's payload lies in the
    source, as a source's `row` states it --, which then becomes the 0 a set job states.  A pair of arrays (SET rows,
    SET_MEMBER rows) is handed on as given, and so are the job rows."""
    if isinstance(members, tuple) and len(members) == 2 and isinstance(members[0], np.ndarray):
        return (np.ascontiguousarray(jb), np.ascontiguousarray(members[0], dtype=SET).reshape(-1),
                np.ascontiguousarray(members[1], dtype=SET_MEMBER).reshape(-1))
    if len(members) != jb.size:
        raise ValueError(f'{len(members)} member lists for {jb.size} jobs')
    jb = jb.copy()
    sets, rows = np.zeros(jb.size, dtype=SET), []
    for k, ms in enumerate(members):
        sets[k] = (len(rows), len(ms))
        base = int(jb['src_offset'][k])
        rows.extend((base + int(off), int(frames), int(ch), 0) for off, frames, ch in ms)
    jb['src_offset'] = 0
    return jb, sets, np.array(rows, dtype=SET_MEMBER).reshape(-1)


_lib = None


def lib():
    """The loaded shared library; raises NativeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback for the feature/CNN path.")
    # PyTorch-ROCm ships its own HIP runtime (libamdhip64 with the same SONAME as /opt/rocm's).  Two HIP runtimes
    # in one process do not both see the GPU ("No HIP GPUs are available" in whichever initialises second), so make
    # the order deterministic: if torch is installed, let it load its runtime first and bind to that one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    pf, pd, pi32, pi64, pu8, pi16 = (C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_int16))
    sig = {
        'iss_create': (C.c_int, [C.c_int, C.POINTER(vp)]),
        'iss_destroy': (None, [vp]),
        'iss_last_error': (C.c_char_p, [vp]),
        'iss_version': (C.c_char_p, []),
        'iss_set_workspace_limit': (C.c_int, [vp, u64]),
        'iss_synchronize': (C.c_int, [vp]),
        'iss_sidekit_tables': (C.c_int, [vp, pd, pf]),
        'iss_signal_pcm16': (C.c_int, [vp, pi16, i64]),
        'iss_signal_f32': (C.c_int, [vp, pf, i64]),
        'iss_signal_pcm16_device': (C.c_int, [vp, vp, i64]),
        'iss_signal_pcm16_device_stream': (C.c_int, [vp, vp, i64, vp]),
        'iss_resample_filter': (C.c_int, [vp, i32, i32, pd, i64, pi32]),
        'iss_resample_pcm16': (C.c_int, [vp, vp, i64, vp, i32, i64]),
        'iss_resample_pcm16_windows': (C.c_int, [vp, vp, i64, vp, vp, i32, i64]),
        'iss_flac_decode_windows': (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i32, i64, pi32]),
        'iss_adpcm_decode_windows': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32]),
        'iss_msadpcm_decode_windows': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32]),
        'iss_resample_pcm16_split': (C.c_int, [vp, vp, i64, vp, i32, i64, vp, vp, i64]),
        'iss_flac_decode_split': (C.c_int, [vp, vp, i64, vp, i64, vp, i32, i64, pi32, vp, vp, i64]),
        'iss_adpcm_decode_split': (C.c_int, [vp, vp, i64, vp, i32, i64, i64, pi32, vp, vp, i64]),
        'iss_msadpcm_decode_split': (C.c_int, [vp, vp, i64, vp, i32, i64, i64, pi32, vp, vp, i64]),
        'iss_resample_pcm16_windows_split': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, vp, vp, i64]),
        'iss_flac_decode_windows_split': (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i32, i64, pi32, vp, vp, i64]),
        'iss_adpcm_decode_windows_split': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32, vp, vp, i64]),
        'iss_msadpcm_decode_windows_split': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32, vp, vp, i64]),
        'iss_resample_split_geometry': (C.c_int, [vp, i32, i32, pi32, pi32]),
        'iss_resample_pcm16_mix': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, vp, vp, i64, vp, i64]),
        'iss_flac_decode_mix': (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i32, i64, pi32, vp, vp, i64, vp, i64]),
        'iss_adpcm_decode_mix': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32, vp, vp, i64, vp, i64]),
        'iss_msadpcm_decode_mix': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, i64, pi32, vp, vp, i64, vp, i64]),
        'iss_staged_payload': (C.c_int, [vp, i32, pi64]),
        'iss_resample_staged_mix': (C.c_int, [vp, i32, i64, vp, vp, i32, i64, vp, vp, i64, vp, i64]),
        'iss_resample_pcm16_sched': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, vp, vp, i64, vp, i64, vp, i64]),
        'iss_resample_staged_sched': (C.c_int, [vp, i32, i64, vp, vp, i32, i64, vp, vp, i64, vp, i64, vp, i64]),
        'iss_resample_pcm16_sched_fade': (C.c_int, [vp, vp, i64, vp, vp, i32, i64, vp, vp, i64, vp, vp, i64, vp, i64]),
        'iss_resample_staged_sched_fade': (C.c_int, [vp, i32, i64, vp, vp, i32, i64, vp, vp, i64, vp, vp, i64, vp, i64]),
        'iss_survey_blocks': (C.c_int, [vp, vp, i64, vp, i32, pi32, vp, vp]),
        'iss_flac_survey_blocks': (C.c_int, [vp, vp, i32, pi32, vp, vp]),
        'iss_adpcm_survey_blocks': (C.c_int, [vp, vp, i32, pi32, vp, vp]),
        'iss_msadpcm_survey_blocks': (C.c_int, [vp, vp, i32, pi32, vp, vp]),
        'iss_upload_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_resample_pcm16_set': (C.c_int, [vp, vp, i64, vp, i32, i64, vp, vp, i64, vp, vp, i64, vp, i64]),
        'iss_survey_set': (C.c_int, [vp, vp, i64, vp, i32, vp, vp, i64, vp]),
        'iss_resample_staged_set': (C.c_int, [vp, i32, i64, vp, i32, i64, vp, vp, i64, vp, vp, i64, vp, i64]),
        'iss_survey': (C.c_int, [vp, vp, i64, vp, vp, i32, vp]),
        'iss_flac_survey': (C.c_int, [vp, vp, vp, i32, vp]),
        'iss_adpcm_survey': (C.c_int, [vp, vp, vp, i32, vp]),
        'iss_msadpcm_survey': (C.c_int, [vp, vp, vp, i32, vp]),
        'iss_survey_geometry': (C.c_int, [pi32, pi32, pi32]),
        'iss_survey_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_get_signal_pcm16': (C.c_int, [vp, pi16, i64, i64]),
        'iss_resample_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_flac_index': (C.c_int, [vp, i64, i64, vp, vp, i64, pi64, pi64, C.c_char_p, i32]),
        'iss_flac_crc': (C.c_int, [vp, i64, pi32, pi32]),
        'iss_flac_decode_host': (C.c_int, [vp, i64, vp, i64, i32, i32, i64, vp, pi32]),
        'iss_flac_decode': (C.c_int, [vp, vp, i64, vp, i64, vp, i32, i64, pi32]),
        'iss_flac_get_stage': (C.c_int, [vp, i32, vp, i64]),
        'iss_flac_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_adpcm_decode_host': (C.c_int, [vp, i64, i64, i32, i32, i64, pi16, pi32]),
        'iss_adpcm_decode': (C.c_int, [vp, vp, i64, vp, i32, i64, i64, pi32]),
        'iss_adpcm_get_stage': (C.c_int, [vp, i32, vp, i64]),
        'iss_adpcm_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_msadpcm_decode_host': (C.c_int, [vp, i64, i64, i32, i32, i64, pi16, pi32]),
        'iss_msadpcm_decode': (C.c_int, [vp, vp, i64, vp, i32, i64, i64, pi32]),
        'iss_msadpcm_get_stage': (C.c_int, [vp, i32, vp, i64]),
        'iss_msadpcm_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_host_alloc': (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        'iss_host_free': (C.c_int, [vp, vp]),
        'iss_cnn_probs_async': (C.c_int, [vp, C.c_int, pi32, i32, pf, pu8, pi64]),
        'iss_cnn_dead_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_wait': (C.c_int, [vp, i64]),
        'iss_wait_slots': (C.c_int, [vp, i64, i32, pi32]),
        'iss_comm_unique_id': (C.c_int, [vp, pu8]),
        'iss_comm_init': (C.c_int, [vp, pu8, i32, i32]),
        'iss_comm_destroy': (C.c_int, [vp]),
        'iss_allgather_segments': (C.c_int, [vp, pi32, i32, i32, pi32, pi32]),
        'iss_comm_allreduce_max': (C.c_int, [vp, pd]),
        'iss_comm_info': (C.c_int, [vp, pi32, pi32, pi32, C.c_char_p, i32]),
        'iss_sidekit': (C.c_int, [vp, pi32]),
        'iss_get_loge': (C.c_int, [vp, pf]),
        'iss_get_mspec': (C.c_int, [vp, pf]),
        'iss_set_mspec': (C.c_int, [vp, pf, i32]),
        'iss_cnn_load': (C.c_int, [vp, C.c_int, pi32, i32, pf, i64, i32, pi64, i32, i32, i32, i32]),
        'iss_cnn_load_shared': (C.c_int, [vp, C.c_int, C.c_int, pi32, i32, i32, pi64, i32, i32, i32, i32]),
        'iss_cnn_probs': (C.c_int, [vp, C.c_int, pi32, i32, pf, pu8]),
        'iss_cnn_forward': (C.c_int, [vp, C.c_int, pf, i32, pf]),
        'iss_cnn_flops': (C.c_int, [vp, C.c_int, pd]),
        'iss_set_precision': (C.c_int, [vp, C.c_int]),
        'iss_set_precision_guard': (C.c_int, [vp, C.c_float]),
        'iss_cnn_precision_info': (C.c_int, [vp, C.c_int, pi32, pf, pi32, pi32, pf]),
        'iss_cnn_set_net_precision': (C.c_int, [vp, C.c_int, C.c_int]),
        'iss_vbx_tables': (C.c_int, [vp, pd, pd]),
        'iss_vbx_features': (C.c_int, [vp, pi32, pd, i64, pf, pi32]),
        'iss_vbx_set_dither': (C.c_int, [vp, pd, i64]),
        'iss_vbx_features_pcm16': (C.c_int, [vp, pi16, i64, pf, pi32]),
        'iss_vbx_features_batch_pcm16': (C.c_int, [vp, pi16, pi64, i32, pi32, pf]),
        'iss_vbx_features_resident': (C.c_int, [vp, pi64, pi64, i32, pi32, pf]),
        'iss_vbx_resident_stats': (C.c_int, [vp, pi64, pi64]),
        'iss_vbx_embed': (C.c_int, [vp, C.c_int, pi32, i32, pf]),
        'iss_prof_enable': (C.c_int, [vp, C.c_int]),
        'iss_prof_get': (C.c_int, [vp, C.c_int, pd, pi64, pd]),
        'iss_prof_reset': (C.c_int, [vp]),
        'iss_prof_get_row': (C.c_int, [vp, C.c_int, pd, pi64]),
        'iss_prof_get_instance': (C.c_int, [vp, C.c_int, C.c_char_p, i32, pd, pi64, pd]),
        'iss_set_diag': (C.c_int, [vp, C.c_uint32]),
        'iss_scribble': (C.c_int, [vp, C.c_uint32]),
        'iss_diag_split16': (C.c_int, [vp, pf, i64, i32, i32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
        'iss_viterbi_f64': (C.c_int, [pd, i64, i32, pd, pi32]),
        'iss_viterbi_f32': (C.c_int, [pf, i64, i32, pd, pi32]),
        'iss_energy_viterbi': (C.c_int, [pf, i64, C.c_double, C.c_double, C.c_double, pd, pi32]),
        'iss_viterbi_segments_f32': (C.c_int, [pf, pi64, i64, i32, pd, pi32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    L._iss_symbols = tuple(sig)
    _lib = L
    return L


DIAG_BITS = {'no_shared_first': 0x001, 'no_flrows': 0x002, 'no_ws': 0x004, 'no_ws3': 0x008, 'no_direct1': 0x010,
             'no_nh2': 0x020, 'no_tr': 0x040, 'no_pw': 0x080, 'no_pws': 0x100, 'no_pws2': 0x200, 'no_wq': 0x400,
             'no_dual': 0x800, 'no_chain': 0x1000, 'no_ring': 0x2000, 'no_fsame': 0x4000, 'no_f32ws': 0x8000, 'no_ncb1': 0x10000, 'no_wsu3': 0x20000, 'no_gfused': 0x40000, 'no_hl': 0x80000,
             'no_skip_dead': 0x100000}                                                                                         # include/iss.h ISS_DIAG_*


def diag_flags(names):
    """'no_shared_first,no_pws2' -> ISS_DIAG_* bit mask (unknown names raise)."""
    flags = 0
    for nm in str(names).replace(' ', '').replace('+', ',').lower().split(','):
        if nm:
            flags |= DIAG_BITS[nm]
    return flags


def _ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def viterbi(emission, transition):
    """Host Viterbi (iss_viterbi_f32/f64): emission (T,K) float32|float64 log-scores,
    transition (K,K) float64.  Returns int32 state ids (T,)."""
    L = lib()
    em = np.ascontiguousarray(emission)
    if em.dtype not in (np.float32, np.float64):
        em = em.astype(np.float64)
    tr = np.ascontiguousarray(transition, dtype=np.float64)
    T, K = em.shape
    out = np.empty(T, dtype=np.int32)
    if em.dtype == np.float32:
        rc = L.iss_viterbi_f32(_ptr(em, C.c_float), T, K, _ptr(tr, C.c_double), _ptr(out, C.c_int32))
    else:
        rc = L.iss_viterbi_f64(_ptr(em, C.c_double), T, K, _ptr(tr, C.c_double), _ptr(out, C.c_int32))
    if rc != 0:
        raise NativeError(f"iss_viterbi failed ({rc}): T={T} K={K}")
    return out


def viterbi_segments(emission, seg_len, transition):
    """iss_viterbi_segments_f32: emission (n,K) float32 log-scores of consecutive segments of lengths seg_len, each smoothed on
    its own.  Returns int32 state ids (n,)."""
    L = lib()
    em = np.ascontiguousarray(emission, dtype=np.float32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    tr = np.ascontiguousarray(transition, dtype=np.float64)
    n, K = em.shape
    assert int(sl.sum()) == n
    out = np.empty(n, dtype=np.int32)
    rc = L.iss_viterbi_segments_f32(_ptr(em, C.c_float), _ptr(sl, C.c_int64), sl.size, K, _ptr(tr, C.c_double), _ptr(out, C.c_int32))
    if rc != 0:
        raise NativeError(f"iss_viterbi_segments_f32 failed ({rc}): n={n} K={K} segments={sl.size}")
    return out


_LOG_EPS = np.log(np.full(1, 1e-10))[0], np.log(np.full(1, 1 - 1e-10))[0]     # as pred2logemission's np.log(ret) yields them


def energy_viterbi(loge, threshold, transition):
    """iss_energy_viterbi: smoothed activity (T,) int32 of `loge > threshold` (see include/iss.h)."""
    L = lib()
    x = np.ascontiguousarray(loge, dtype=np.float32)
    tr = np.ascontiguousarray(transition, dtype=np.float64)
    out = np.empty(x.size, dtype=np.int32)
    rc = L.iss_energy_viterbi(_ptr(x, C.c_float), x.size, float(threshold), float(_LOG_EPS[0]), float(_LOG_EPS[1]),
                              _ptr(tr, C.c_double), _ptr(out, C.c_int32))
    if rc != 0:
        raise NativeError(f"iss_energy_viterbi failed ({rc}): T={x.size}")
    return out


def flac_crc(buf):
    """(CRC-8, CRC-16) of `buf` as the FLAC frame header / footer computes them (iss_flac_crc)."""
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    c8, c16 = C.c_int32(), C.c_int32()
    if lib().iss_flac_crc(C.c_void_p(b.ctypes.data), b.size, C.byref(c8), C.byref(c16)) != 0:
        raise NativeError('iss_flac_crc failed')
    return c8.value, c16.value


def flac_index(buf, first_frame, info):
    """iss_flac_index: buf = uint8 array of the whole stream, info = one FLAC_INFO record -> FLAC_FRAME rows.
    Raises ValueError(offset, reason) for a malformed stream."""
    L = lib()
    inf = np.ascontiguousarray(np.array(info, dtype=FLAC_INFO).reshape(1))
    cap = max(16, int(inf['total_samples'][0]) // max(1, int(inf['min_block'][0]) or 1) + 2) if inf['total_samples'][0] > 0 \
        else buf.size // 64 + 16
    err = C.create_string_buffer(256)
    n, off = C.c_int64(), C.c_int64()
    for _ in range(2):
        rows = np.zeros(cap, dtype=FLAC_FRAME)
        rc = L.iss_flac_index(C.c_void_p(buf.ctypes.data), buf.size, int(first_frame), C.c_void_p(inf.ctypes.data),
                              C.c_void_p(rows.ctypes.data), cap, C.byref(n), C.byref(off), err, 256)
        if rc != -5:                                   # ISS_ENOMEM: more frames than room
            break
        cap = buf.size // 9 + 16                       # a frame is at least 9 bytes
    if rc != 0:
        raise ValueError(off.value, err.value.decode())
    return rows[:n.value].copy()


def flac_decode_host(buf, frames, channels, bps, frames_total):
    """iss_flac_decode_host -> (stored samples (n,) or (n, channels) int16 / int32, per-frame ISS_FLAC_* status)."""
    fr = np.ascontiguousarray(frames, dtype=FLAC_FRAME)
    out = np.empty((int(frames_total), int(channels)), dtype=np.int32 if bps > 16 else np.int16)
    st = np.zeros(len(fr), dtype=np.int32)
    rc = lib().iss_flac_decode_host(C.c_void_p(buf.ctypes.data), buf.size, C.c_void_p(fr.ctypes.data), len(fr), int(channels),
                                    int(bps), int(frames_total), C.c_void_p(out.ctypes.data), _ptr(st, C.c_int32))
    if rc != 0:
        raise NativeError(f'iss_flac_decode_host failed ({rc}): bad frame rows')
    return (out[:, 0] if channels == 1 else out), st


def adpcm_decode_host(buf, nblocks, channels, block_align, frames_total, fn='iss_adpcm_decode_host'):
    """iss_adpcm_decode_host -> (PCM16 samples (n,) or (n, channels), per-block ISS_ADPCM_* status)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    out = np.empty((int(frames_total), int(channels)), dtype=np.int16)
    st = np.zeros(int(nblocks), dtype=np.int32)
    rc = getattr(lib(), fn)(C.c_void_p(buf.ctypes.data), buf.size, int(nblocks), int(channels), int(block_align),
                            int(frames_total), _ptr(out, C.c_int16), _ptr(st, C.c_int32))
    if rc != 0:
        raise NativeError(f'{fn} failed ({rc}): bad block geometry')
    return (out[:, 0] if channels == 1 else out), st


def msadpcm_decode_host(buf, nblocks, channels, block_align, frames_total):
    """iss_msadpcm_decode_host: as adpcm_decode_host, Microsoft ADPCM blocks."""
    return adpcm_decode_host(buf, nblocks, channels, block_align, frames_total, 'iss_msadpcm_decode_host')


class Context:
    """One device context (stream + resident signal/features + loaded networks)."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.iss_create(int(device), C.byref(h))
        if rc != 0:
            raise NativeError(f"iss_create(device={device}) failed ({rc}): "
                              f"{self._L.iss_last_error(None).decode()}")
        self._h = h
        self.device = device
        self.T = 0
        self._net_out = {}
        self._dither_n = 0          # length of the dither stream cached on the device (vbx)
        self._pinned = {}           # data address -> hipHostMalloc pointer of pinned_empty() arrays
        self.comm_rank, self.comm_world = 0, 1
        self.precision = None       # last value given to set_precision / set_workspace_limit (None = library default)
        self.workspace_limit = None
        self.diag = 0
        env = os.environ.get('ISS_DIAG', '')
        if env:                     # A/B tooling only (tools/ab_env.sh): the library itself never reads the environment
            self.set_diag(diag_flags(env))
        self.guard_threshold = None # last value given to set_precision_guard (None = library default, 5e-4)
        env = os.environ.get('ISS_PREC_GUARD', '')
        if env:                     # A/B tooling only: timing-only experiment builds compute wrong results on purpose
            self.set_precision_guard(float(env))

    def close(self):
        if getattr(self, '_h', None):
            for p in list(self._pinned.values()):
                self._L.iss_host_free(self._h, C.c_void_p(p))
            self._pinned.clear()
            self._L.iss_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise NativeError(f"{what} failed ({rc}): {self._L.iss_last_error(self._h).decode()}")

    # ---- SIDEKIT front end
    def sidekit_tables(self, window, melbank):
        w = np.ascontiguousarray(window, dtype=np.float64)
        b = np.ascontiguousarray(melbank, dtype=np.float32)
        assert w.shape == (400,) and b.shape == (24, 257)
        self._ck(self._L.iss_sidekit_tables(self._h, _ptr(w, C.c_double), _ptr(b, C.c_float)), 'iss_sidekit_tables')

    def set_signal(self, sig):
        """sig: 1-D int16 (PCM) or float32 array, 16 kHz mono."""
        sig = np.ascontiguousarray(sig)
        if sig.dtype == np.int16:
            self._ck(self._L.iss_signal_pcm16(self._h, _ptr(sig, C.c_int16), sig.size), 'iss_signal_pcm16')
        elif sig.dtype == np.float32:
            self._ck(self._L.iss_signal_f32(self._h, _ptr(sig, C.c_float), sig.size), 'iss_signal_f32')
        else:
            raise TypeError(f"signal dtype {sig.dtype}: need int16 or float32")
        self._keep = sig            # the async H2D copy reads it until the next sync

    def set_signal_device(self, dev_ptr, n, producer_stream=None):
        """PCM16 samples already in this GPU's HBM.  The library's stream is made to wait for everything submitted so
        far to `producer_stream` (a hipStream_t handle as int, e.g. torch.cuda.current_stream().cuda_stream; None = the
        legacy default stream); see include/iss.h for the ordering contract."""
        self._ck(self._L.iss_signal_pcm16_device_stream(self._h, C.c_void_p(int(dev_ptr)), int(n),
                                                        C.c_void_p(int(producer_stream)) if producer_stream else None),
                 'iss_signal_pcm16_device')

    # ---- resampler (iss_resample_*): WAV sources at other rates / channel counts -> resident 16 kHz mono PCM16
    def resample_filter(self, sr):
        """Register the filter of source rate `sr` (resample.plan; cached by the library) -> (filter id, up, down)."""
        from . import resample
        up, down, h = resample.plan(sr)
        fid = C.c_int32()
        self._ck(self._L.iss_resample_filter(self._h, up, down, _ptr(h, C.c_double), h.size, C.byref(fid)), 'iss_resample_filter')
        return fid.value, up, down

    def resample_job(self, x, sr, src_offset, dst_offset, fmt=None):
        """One iss_resample_job row for stored samples x ((n,) or (n, C)) placed at byte `src_offset` of the source buffer.
        fmt: the ISS_RS_* format code where the dtype does not tell it (RS_I8 / RS_ULAW / RS_ALAW bytes, | RS_SWAP)."""
        fid, up, down = self.resample_filter(sr)
        n = x.shape[0]
        return (src_offset, n, 1 if x.ndim == 1 else x.shape[1], RS_FORMAT[x.dtype] if fmt is None else int(fmt), fid, 0,
                dst_offset, -(-n * up // down))

    def resample(self, src, jobs, n_signal=-1, windows=None, splits=None, mixes=None):
        """iss_resample_pcm16: src = 1-D uint8 array of the stored samples of every job, jobs = rows of RS_JOB; one H2D copy,
        one launch.  n_signal >= 0: a new resident signal of that many samples; < 0: into the signal of the last set_signal.
        windows: rows of WINDOW, one beside every job (iss_resample_pcm16_windows): src holds frames [s_begin, s_end) of each
        file, and the outputs [out_begin, out_begin + out_count) are written.
        splits: `(dst_stride, [channels])` or None per job (iss_resample_pcm16_split): the selected channels of a job are written
        apart, channel k of the selection at dst_offset + k * dst_stride; None downmixes as ever.  With windows
        (iss_resample_pcm16_windows_split): the window's outputs of each selected channel, dst_stride >= out_count.
        mixes (not with splits): `(dst_stride, [mix, ...])` or None per job (iss_resample_pcm16_mix, with or without windows): mix
        k of a job -- a resample.Mix, or a channel index for that channel alone -- is written at dst_offset + k * dst_stride;
        None downmixes as ever."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        jb = np.ascontiguousarray(np.array(jobs, dtype=RS_JOB))
        self._decode_call('iss_resample_pcm16', (C.c_void_p(src.ctypes.data), src.size, C.c_void_p(jb.ctypes.data)),
                          (jb.size, int(n_signal)), windows, splits, mixes)
        self._keep_rs = src         # the async H2D copy reads it until the next sync

    def _decode_call(self, base, lead, trail, windows, splits, mixes=None):
        """One of the five entry points of `base`: base(ctx, *lead, *trail), or base_windows with the WINDOW rows between
        `lead` (which ends with the job rows) and `trail` (which begins with their count), or base_split with the SPLIT rows,
        the channel table and its length behind `trail`, or base_windows_split with both; or base_mix with the WINDOW rows or
        NULL between `lead` and `trail` and the three mix tables behind `trail`."""
        name, args = base, lead + trail
        if mixes is not None:
            if splits is not None:
                raise ValueError('a call carries splits or mixes, not both')
            wn = None if windows is None else _window_rows(windows, trail[0])
            sets, rows, terms = _mix_rows(mixes, trail[0])
            args = lead + (None if wn is None else C.c_void_p(wn.ctypes.data),) + trail + (
                C.c_void_p(sets.ctypes.data), C.c_void_p(rows.ctypes.data), rows.size, C.c_void_p(terms.ctypes.data), terms.size)
            self._ck(getattr(self._L, base + '_mix')(self._h, *args), base + '_mix')
            return
        if windows is not None:
            wn = _window_rows(windows, trail[0])
            name, args = base + '_windows', lead + (C.c_void_p(wn.ctypes.data),) + trail
        if splits is not None:
            sp, sel = _split_rows(splits, trail[0])
            name, args = name + '_split', args + (C.c_void_p(sp.ctypes.data), C.c_void_p(sel.ctypes.data), sel.size)
        self._ck(getattr(self._L, name)(self._h, *args), name)

    # ---- resampling what a survey or a decode call left on the device (iss_resample_staged_mix)
    def staged_payload(self, coder=None):
        """The id of the payload origin `coder` holds (None: the last survey's upload; 'flac', 'adpcm', 'msadpcm': what the
        coder's last decode call staged).  NativeError (ISS_ESTATE) when it holds none."""
        pid = C.c_int64()
        self._ck(self._L.iss_staged_payload(self._h, STAGED_ORIGIN[coder], C.byref(pid)), 'iss_staged_payload')
        return pid.value

    def resample_staged(self, coder, payload, jobs, n_signal=-1, windows=None, mixes=None):
        """iss_resample_staged_mix: the RS_JOB rows `jobs` over the bytes of payload `payload` of origin `coder`, which are on
        the device already (src_offset of a row: the byte offset of the surveyed job, or for a coder the index of its staged
        job); nothing is uploaded but rows.  windows, mixes: as for `resample`; mixes None is the plain downmix for every job."""
        jb = np.ascontiguousarray(np.array(jobs, dtype=RS_JOB).reshape(-1))
        wn = None if windows is None else _window_rows(windows, jb.size)
        sets, rows, terms = _mix_rows([None] * jb.size if mixes is None else mixes, jb.size)
        self._ck(self._L.iss_resample_staged_mix(
            self._h, STAGED_ORIGIN[coder], int(payload), C.c_void_p(jb.ctypes.data), None if wn is None else C.c_void_p(wn.ctypes.data),
            jb.size, int(n_signal), C.c_void_p(sets.ctypes.data), C.c_void_p(rows.ctypes.data), rows.size,
            C.c_void_p(terms.ctypes.data), terms.size), 'iss_resample_staged_mix')

    # ---- schedules (iss_resample_*_sched): a downmix that differs from one stretch of a file to the next
    @staticmethod
    def _sched_args(scheds, njobs, fades=None):
        """(arrays to keep alive, the entry point's suffix, its arguments from `scheds` on): '_fade' and the half-widths behind the
        run rows where a run fades in, else '' and the arguments of the call without fades."""
        sc, runs, rows, terms = tables = _sched_rows(scheds, njobs)
        fd = _sched_fades(scheds, fades, runs.size)
        mix = (C.c_void_p(rows.ctypes.data), rows.size, C.c_void_p(terms.ctypes.data), terms.size)
        head = (C.c_void_p(sc.ctypes.data), C.c_void_p(runs.ctypes.data), runs.size)
        if fd is None:
            return tables, '', head + mix
        return tables + (fd,), '_fade', head + (C.c_void_p(fd.ctypes.data),) + mix

    def resample_sched(self, src, jobs, scheds, n_signal=-1, windows=None, fades=None):
        """iss_resample_pcm16_sched: `resample` with one schedule per job (a resample.Schedule, or [(begin_frame, mix or None)]) in
        place of splits or mixes: every job writes one signal, frame j of its source mixed by the mix of the run that governs it.
        One H2D copy, one launch.  windows: refused by the library (a schedule governs whole sources).  Where a schedule carries
        a non-zero fade (or `fades`, one half-width per run row of the call, does): iss_resample_pcm16_sched_fade."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        jb = np.ascontiguousarray(np.array(jobs, dtype=RS_JOB).reshape(-1))
        wn = None if windows is None else _window_rows(windows, jb.size)
        keep, sfx, args = self._sched_args(scheds, jb.size, fades)
        self._ck(getattr(self._L, 'iss_resample_pcm16_sched' + sfx)(
            self._h, C.c_void_p(src.ctypes.data), src.size, C.c_void_p(jb.ctypes.data), None if wn is None else C.c_void_p(wn.ctypes.data),
            jb.size, int(n_signal), *args), 'iss_resample_pcm16_sched' + sfx)
        self._keep_rs = src         # the async H2D copy reads it until the next sync

    def resample_staged_sched(self, coder, payload, jobs, scheds, n_signal=-1, windows=None, fades=None):
        """iss_resample_staged_sched (with fades: iss_resample_staged_sched_fade): `resample_sched` over the bytes of payload
        `payload` of origin `coder`, as `resample_staged` reads them; nothing is uploaded but rows."""
        jb = np.ascontiguousarray(np.array(jobs, dtype=RS_JOB).reshape(-1))
        wn = None if windows is None else _window_rows(windows, jb.size)
        keep, sfx, args = self._sched_args(scheds, jb.size, fades)
        self._ck(getattr(self._L, 'iss_resample_staged_sched' + sfx)(
            self._h, STAGED_ORIGIN[coder], int(payload), C.c_void_p(jb.ctypes.data), None if wn is None else C.c_void_p(wn.ctypes.data),
            jb.size, int(n_signal), *args), 'iss_resample_staged_sched' + sfx)

    # ---- file sets (iss_*_set): one file per channel or group of channels, read as the interleaved file they stand for
    def resample_set(self, src, jobs, members, n_signal=-1, mixes=None):
        """iss_resample_pcm16_set: `resample` with `mixes` for file sets, whole sources only.  src = the members' stored bytes,
        jobs = rows of RS_JOB stating each set's frames_in (its longest member's) and channels (all members'), src_offset = where
        the job's payload lies in src; members: per job [(byte offset in that payload, frames, channels)].  mixes: as for
        `resample` (a channel index = that channel alone, so a split rides here too); None, or None for a job, is the plain
        downmix of the set's interleaved twin."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        jb, sets, mem = _set_rows(np.array(jobs, dtype=RS_JOB).reshape(-1), members)
        ms, rows, terms = _mix_rows([None] * jb.size if mixes is None else mixes, jb.size)
        self._ck(self._L.iss_resample_pcm16_set(
            self._h, C.c_void_p(src.ctypes.data), src.size, C.c_void_p(jb.ctypes.data), jb.size, int(n_signal),
            C.c_void_p(sets.ctypes.data), C.c_void_p(mem.ctypes.data), mem.size, C.c_void_p(ms.ctypes.data),
            C.c_void_p(rows.ctypes.data), rows.size, C.c_void_p(terms.ctypes.data), terms.size), 'iss_resample_pcm16_set')
        self._keep_rs = src         # the async H2D copy reads it until the next sync

    def resample_staged_set(self, payload, jobs, members, n_signal=-1, mixes=None):
        """iss_resample_staged_set: `resample_set` over the bytes the last `survey_set` uploaded (payload = staged_payload(None)
        right after it); jobs and members as that call's.  Nothing is uploaded but rows."""
        jb, sets, mem = _set_rows(np.array(jobs, dtype=RS_JOB).reshape(-1), members)
        ms, rows, terms = _mix_rows([None] * jb.size if mixes is None else mixes, jb.size)
        self._ck(self._L.iss_resample_staged_set(
            self._h, STAGED_ORIGIN[None], int(payload), C.c_void_p(jb.ctypes.data), jb.size, int(n_signal),
            C.c_void_p(sets.ctypes.data), C.c_void_p(mem.ctypes.data), mem.size, C.c_void_p(ms.ctypes.data),
            C.c_void_p(rows.ctypes.data), rows.size, C.c_void_p(terms.ctypes.data), terms.size), 'iss_resample_staged_set')

    def upload_stats(self):
        """(payload H2D copies, their bytes) since the context was created: stored and compressed bytes, not rows or signals."""
        return self._counters('iss_upload_stats')

    def resample_signal(self, x, sr, fmt=None):
        """A single source resampled on its own: the resident signal becomes its 16 kHz mono PCM16 -> its length.  (For arrays in
        hand, as the tests have them; the product places a file through sources.RawSource.place: the same job row, the same call.)"""
        x = np.ascontiguousarray(x)
        job = self.resample_job(x, sr, 0, 0, fmt)
        self.resample(x.reshape(-1).view(np.uint8), [job], n_signal=job[-1])
        return job[-1]

    def resample_split_geometry(self, sr, nsel):
        """(outputs per tile, channels per group) the planner gives a selection of `nsel` channels at source rate `sr`."""
        fid, _, _ = self.resample_filter(sr)
        tile, group = C.c_int32(), C.c_int32()
        self._ck(self._L.iss_resample_split_geometry(self._h, fid, int(nsel), C.byref(tile), C.byref(group)),
                 'iss_resample_split_geometry')
        return tile.value, group.value

    def get_signal_pcm16(self, offset, n):
        """Samples [offset, offset + n) of the resident PCM16 signal (e.g. what `resample` wrote)."""
        out = np.empty(int(n), dtype=np.int16)
        self._ck(self._L.iss_get_signal_pcm16(self._h, _ptr(out, C.c_int16), int(offset), int(n)), 'iss_get_signal_pcm16')
        return out

    def _counters(self, fn):        # (launches, units) the stats entry point `fn` reports
        a, b = C.c_int64(), C.c_int64()
        self._ck(getattr(self._L, fn)(self._h, C.byref(a), C.byref(b)), fn)
        return a.value, b.value

    def _get_stage(self, fn, job, frames_total, channels, dtype):        # a decoder's read-back `fn`: (n,) or (n, channels)
        out = np.empty((int(frames_total), int(channels)), dtype=dtype)
        self._ck(getattr(self._L, fn)(self._h, int(job), C.c_void_p(out.ctypes.data), out.nbytes), fn)
        return out[:, 0] if channels == 1 else out

    def resample_stats(self):
        """(resample launches, resample jobs) since the context was created."""
        return self._counters('iss_resample_stats')

    def _status(self, name, n):
        """This context's page-locked status array `name` of a decoder, grown on demand to hold n entries."""
        st, n = self.__dict__.get(name), max(int(n), 1)
        if st is None or st.size < n:
            if st is not None:
                self.pinned_free(st)
            st = self.__dict__[name] = self.pinned_empty((int(n * 1.25) + 256,), np.int32)
        return st

    # ---- FLAC decoder (iss_flac_*): compressed frames -> resident signal (PCM16), staging buffer, or resampled
    def flac_decode(self, src, frames, jobs, n_signal=-1, windows=None, splits=None, mixes=None):
        """iss_flac_decode: src = 1-D uint8 array of the compressed bytes of every job, frames = FLAC_FRAME rows, jobs = rows
        of FLAC_JOB; one H2D copy, one decode launch (+ one resample launch).  -> the per-frame status array (page-locked,
        this context's): valid after the next synchronising call (get_loge, flac_get_stage, synchronize).
        windows: rows of WINDOW, one beside every job (iss_flac_decode_windows): each job's rows are a run of its file's frames
        that covers [s_begin, s_end), and only those samples are produced.
        splits: as for `resample` (iss_flac_decode_split), for TO_STAGE jobs with a filter; None for every other job.
        mixes: as for `resample` (iss_flac_decode_mix), for the same jobs."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        fr = np.ascontiguousarray(frames, dtype=FLAC_FRAME)
        jb = np.ascontiguousarray(np.array(jobs, dtype=FLAC_JOB).reshape(-1))
        st = self._status('_flac_status', len(fr))
        self._decode_call('iss_flac_decode', (C.c_void_p(src.ctypes.data), src.size, C.c_void_p(fr.ctypes.data), len(fr),
                                              C.c_void_p(jb.ctypes.data)), (jb.size, int(n_signal), _ptr(st, C.c_int32)),
                          windows, splits, mixes)
        self._keep_flac = (src, fr)    # the async H2D copy reads them until the next sync
        return st[:len(fr)]

    def flac_get_stage(self, job, frames_total, channels, bps):
        """Stored-format samples of staged job `job` of the last flac_decode: (n,) or (n, channels) int16 / int32."""
        return self._get_stage('iss_flac_get_stage', job, frames_total, channels, np.int32 if bps > 16 else np.int16)

    def flac_stats(self):
        """(FLAC decode launches, frames decoded) since the context was created."""
        return self._counters('iss_flac_stats')

    # ---- IMA ADPCM decoder (iss_adpcm_*): stored blocks -> resident signal (PCM16), staging buffer, or resampled
    def adpcm_decode(self, src, jobs, nblocks, n_signal=-1, windows=None, splits=None, mixes=None):
        """iss_adpcm_decode: src = 1-D uint8 array of the blocks of every job, jobs = rows of ADPCM_JOB, nblocks = their
        sum; one H2D copy, one decode launch (+ one resample launch).  -> the per-block status array (page-locked, this
        context's): valid after the next synchronising call (get_loge, adpcm_get_stage, synchronize).
        windows: rows of WINDOW, one beside every job (iss_adpcm_decode_windows): each job holds exactly the blocks that its
        samples [s_begin, s_end) lie in, and only those samples are produced.
        splits: as for `resample` (iss_adpcm_decode_split), for TO_STAGE jobs with a filter; None for every other job.
        mixes: as for `resample` (iss_adpcm_decode_mix), for the same jobs."""
        return self._block_decode('adpcm', src, jobs, nblocks, n_signal, windows, splits, mixes)

    def _block_decode(self, coder, src, jobs, nblocks, n_signal, windows, splits, mixes=None):
        """iss_<coder>_decode.  Status array and kept source bytes are the coder's own: a pass launches both coders before it
        reads either's status."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        jb = np.ascontiguousarray(np.array(jobs, dtype=ADPCM_JOB).reshape(-1))
        st = self._status(f'_{coder}_status', nblocks)
        self._decode_call(f'iss_{coder}_decode', (C.c_void_p(src.ctypes.data), src.size, C.c_void_p(jb.ctypes.data)),
                          (jb.size, int(nblocks), int(n_signal), _ptr(st, C.c_int32)), windows, splits, mixes)
        setattr(self, f'_keep_{coder}', src)         # the async H2D copy reads it until the next sync
        return st[:int(nblocks)]

    def adpcm_get_stage(self, job, frames_total, channels):
        """PCM16 samples of staged job `job` of the last adpcm_decode: (n,) or (n, channels) int16."""
        return self._get_stage('iss_adpcm_get_stage', job, frames_total, channels, np.int16)

    def adpcm_stats(self):
        """(ADPCM decode launches, blocks decoded) since the context was created."""
        return self._counters('iss_adpcm_stats')

    # ---- Microsoft ADPCM decoder (iss_msadpcm_*): the IMA decoder's rows and contracts, state of its own
    def msadpcm_decode(self, src, jobs, nblocks, n_signal=-1, windows=None, splits=None, mixes=None):
        """iss_msadpcm_decode: as adpcm_decode, for Microsoft ADPCM blocks (status ISS_ADPCM_PREDICTOR for a bad block)."""
        return self._block_decode('msadpcm', src, jobs, nblocks, n_signal, windows, splits, mixes)

    def msadpcm_get_stage(self, job, frames_total, channels):
        """PCM16 samples of staged job `job` of the last msadpcm_decode: (n,) or (n, channels) int16."""
        return self._get_stage('iss_msadpcm_get_stage', job, frames_total, channels, np.int16)

    def msadpcm_stats(self):
        """(Microsoft ADPCM decode launches, blocks decoded) since the context was created."""
        return self._counters('iss_msadpcm_stats')

    # ---- channel survey (iss_survey*): level figures and cross-products of stored frames, nothing else of the context touched
    def survey(self, src, jobs, windows=None, coder=None):
        """iss_survey: src = 1-D uint8 array of the stored bytes of every job, jobs = rows of SURVEY_JOB; one H2D copy, one
        launch of each survey kernel -> one resample.SurveyFields per job, valid on return.  windows: rows of WINDOW, one
        beside every job: its bytes hold frames [s_begin, s_end) of the file and frames [out_begin, out_begin + out_count) are
        surveyed.  coder ('flac', 'adpcm', 'msadpcm'; src is then None): iss_<coder>_survey over what the coder's last decode
        call staged, src_offset of a row the index of the staged job."""
        jb = np.ascontiguousarray(np.array(jobs, dtype=SURVEY_JOB).reshape(-1))
        wn = None if windows is None else _window_rows(windows, jb.size)
        out = self._survey_out(jb)
        tail = (C.c_void_p(jb.ctypes.data), None if wn is None else C.c_void_p(wn.ctypes.data), jb.size, C.c_void_p(out.ctypes.data))
        if coder is None:
            src = np.ascontiguousarray(src, dtype=np.uint8)
            self._ck(self._L.iss_survey(self._h, C.c_void_p(src.ctypes.data), src.size, *tail), 'iss_survey')
        else:
            self._ck(getattr(self._L, f'iss_{coder}_survey')(self._h, *tail), f'iss_{coder}_survey')
        return self._survey_fields(jb, wn, out)

    def survey_blocks(self, src, jobs, block_chunks, coder=None):
        """iss_survey_blocks (coder: iss_<coder>_survey_blocks, src None): `survey` without windows, and the same figures per
        block of block_chunks[k] chunks of job k's frames (include/iss.h, "Survey blocks") -> (one resample.SurveyFields per job,
        per job the list of its blocks' SurveyFields); one H2D copy, one survey launch, valid on return."""
        from .resample import SURVEY_CHUNK, SURVEY_PAIR_CHANNELS, SurveyFields
        jb = np.ascontiguousarray(np.array(jobs, dtype=SURVEY_JOB).reshape(-1))
        ks = np.ascontiguousarray(np.array(block_chunks, dtype=np.int32).reshape(-1))
        if ks.size != jb.size:
            raise ValueError(f'{ks.size} block sizes for {jb.size} jobs')
        out = self._survey_out(jb)
        chs, ns = [int(c) for c in jb['channels']], [int(n) for n in jb['frames_in']]
        width = [6 * c + (c * (c - 1) // 2 if c <= SURVEY_PAIR_CHANNELS else 0) for c in chs]
        nblk = [-(-(-(-n // SURVEY_CHUNK)) // max(int(k), 1)) if n > 0 else 0 for n, k in zip(ns, ks)]
        blk = np.zeros(max(sum(w * b for w, b in zip(width, nblk)), 1), dtype=np.float64)
        tail = (C.c_void_p(jb.ctypes.data), jb.size, _ptr(ks, C.c_int32), C.c_void_p(out.ctypes.data), C.c_void_p(blk.ctypes.data))
        if coder is None:
            src = np.ascontiguousarray(src, dtype=np.uint8)
            self._ck(self._L.iss_survey_blocks(self._h, C.c_void_p(src.ctypes.data), src.size, *tail), 'iss_survey_blocks')
        else:
            self._ck(getattr(self._L, f'iss_{coder}_survey_blocks')(self._h, *tail), f'iss_{coder}_survey_blocks')
        blocks, pos = [], 0
        for c, w, n, k, nb in zip(chs, width, ns, ks, nblk):
            per = int(k) * SURVEY_CHUNK
            rows = np.zeros(nb, dtype=SURVEY_JOB)
            rows['channels'], rows['frames_in'] = c, [min(per, n - b * per) for b in range(nb)]
            blocks.append(self._survey_fields(rows, None, blk[pos:pos + nb * w]))
            pos += nb * w
        return self._survey_fields(jb, None, out), blocks

    def survey_set(self, src, jobs, members):
        """iss_survey_set: iss_survey (without windows) for file sets.  src = the members' stored bytes, jobs = rows of
        SURVEY_JOB stating each set's frames (its longest member's) and channels (all members'), src_offset = where the job's
        payload lies in src; members: per job [(byte offset in that payload, frames, channels)] -> one resample.SurveyFields per
        job, those of the set's interleaved twin."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        jb, sets, mem = _set_rows(np.array(jobs, dtype=SURVEY_JOB).reshape(-1), members)
        out = self._survey_out(jb)
        self._ck(self._L.iss_survey_set(self._h, C.c_void_p(src.ctypes.data), src.size, C.c_void_p(jb.ctypes.data), jb.size,
                                        C.c_void_p(sets.ctypes.data), C.c_void_p(mem.ctypes.data), mem.size,
                                        C.c_void_p(out.ctypes.data)), 'iss_survey_set')
        return self._survey_fields(jb, None, out)

    @staticmethod
    def _survey_out(jb):
        """The result words of the survey jobs `jb`, zeroed."""
        from .resample import SURVEY_PAIR_CHANNELS
        return np.zeros(max(sum(6 * c + (c * (c - 1) // 2 if c <= SURVEY_PAIR_CHANNELS else 0) for c in map(int, jb['channels'])), 1),
                        dtype=np.float64)

    @staticmethod
    def _survey_fields(jb, wn, out):
        """The result rows `out` of the survey jobs `jb` (windows `wn`) -> one resample.SurveyFields per job."""
        from .resample import SurveyFields, SURVEY_PAIR_CHANNELS
        chs = [int(c) for c in jb['channels']]
        width = [6 * c + (c * (c - 1) // 2 if c <= SURVEY_PAIR_CHANNELS else 0) for c in chs]
        res, pos = [], 0
        for k, (c, w) in enumerate(zip(chs, width)):
            r = out[pos:pos + w]
            cnt = r[3 * c:6 * c].view(np.int64)
            n = int(jb['frames_in'][k] if wn is None else wn['out_count'][k])
            res.append(SurveyFields(n, r[2 * c:3 * c].copy(), cnt[:c].copy(), cnt[c:2 * c].copy(), cnt[2 * c:].copy(), r[:c].copy(),
                                    r[c:2 * c].copy(), r[6 * c:].copy() if c <= SURVEY_PAIR_CHANNELS else None))
            pos += w
        return res

    def survey_geometry(self):
        """(frames per chunk, lanes per chunk, channels up to which pairs are computed) of the survey order."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._L.iss_survey_geometry(C.byref(a), C.byref(b), C.byref(c)), 'iss_survey_geometry')
        return a.value, b.value, c.value

    def survey_stats(self):
        """(survey launches, jobs surveyed) since the context was created."""
        return self._counters('iss_survey_stats')

    # ---- page-locked host arrays
    def pinned_empty(self, shape, dtype):
        """numpy array backed by hipHostMalloc memory (freed with the context, or by `pinned_free`)."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        self._ck(self._L.iss_host_alloc(self._h, n, C.byref(p)), 'iss_host_alloc')
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        self._pinned[a.ctypes.data] = p.value
        return a

    def pinned_free(self, a):
        p = self._pinned.pop(a.ctypes.data, None)
        if p is not None and self._h:
            self._ck(self._L.iss_host_free(self._h, C.c_void_p(p)), 'iss_host_free')

    def sidekit(self):
        t = C.c_int32()
        self._ck(self._L.iss_sidekit(self._h, C.byref(t)), 'iss_sidekit')
        self.T = t.value
        return self.T

    def get_loge(self):
        out = np.empty(self.T, dtype=np.float32)
        self._ck(self._L.iss_get_loge(self._h, _ptr(out, C.c_float)), 'iss_get_loge')
        return out

    def get_mspec(self):
        out = np.empty((self.T, 24), dtype=np.float32)
        self._ck(self._L.iss_get_mspec(self._h, _ptr(out, C.c_float)), 'iss_get_mspec')
        return out

    def set_mspec(self, mspec):
        m = np.ascontiguousarray(mspec, dtype=np.float32)
        assert m.ndim == 2 and m.shape[1] == 24
        self._ck(self._L.iss_set_mspec(self._h, _ptr(m, C.c_float), m.shape[0]), 'iss_set_mspec')
        self.T = m.shape[0]

    # ---- CNN engine
    def cnn_load(self, net_id, compiled):
        """compiled: keras_model.CompiledNet."""
        prog = np.ascontiguousarray(compiled.prog, dtype=np.int32)
        blob = np.ascontiguousarray(compiled.blob, dtype=np.float32)
        be = np.ascontiguousarray(compiled.buf_elems, dtype=np.int64)
        h, w, c = compiled.in_shape
        self._ck(self._L.iss_cnn_load(self._h, net_id, _ptr(prog, C.c_int32), prog.shape[0], _ptr(blob, C.c_float),
                                      blob.size, be.size, _ptr(be, C.c_int64), h, w, c, compiled.out_dim),
                 'iss_cnn_load')
        self._net_out[net_id] = compiled.out_dim

    def cnn_load_shared(self, net_id, src_id, compiled):
        """Load `compiled` (keras_model.CompiledNet) on the device parameters of net `src_id`: its blob must be byte-identical
        to the one src_id was loaded with -- the caller's check, the blob is not sent (include/iss.h)."""
        prog = np.ascontiguousarray(compiled.prog, dtype=np.int32)
        be = np.ascontiguousarray(compiled.buf_elems, dtype=np.int64)
        h, w, c = compiled.in_shape
        self._ck(self._L.iss_cnn_load_shared(self._h, net_id, src_id, _ptr(prog, C.c_int32), prog.shape[0], be.size,
                                             _ptr(be, C.c_int64), h, w, c, compiled.out_dim), 'iss_cnn_load_shared')
        self._net_out[net_id] = compiled.out_dim

    def cnn_probs(self, net_id, win_row):
        wr = np.ascontiguousarray(win_row, dtype=np.int32)
        n = wr.size
        probs = np.empty((n, self._net_out[net_id]), dtype=np.float32)
        fin = np.empty(n, dtype=np.uint8)
        self._ck(self._L.iss_cnn_probs(self._h, net_id, _ptr(wr, C.c_int32), n, _ptr(probs, C.c_float),
                                       _ptr(fin, C.c_uint8)), 'iss_cnn_probs')
        return probs, fin.astype(bool)

    def cnn_probs_async(self, net_id, win_row, probs_out=None, finite_out=None):
        """Enqueue iss_cnn_probs and return (ticket, probs, finite_u8); the arrays are valid after wait(ticket).
        Pass pinned_empty() arrays as outputs if the D2H copy is to overlap host work."""
        wr = np.ascontiguousarray(win_row, dtype=np.int32)
        n = wr.size
        if probs_out is None:
            probs_out = np.empty((n, self._net_out[net_id]), dtype=np.float32)
        if finite_out is None:
            finite_out = np.empty(n, dtype=np.uint8)
        assert probs_out.size >= n * self._net_out[net_id] and finite_out.size >= n
        t = C.c_int64(-1)
        self._ck(self._L.iss_cnn_probs_async(self._h, net_id, _ptr(wr, C.c_int32), n, _ptr(probs_out, C.c_float),
                                             _ptr(finite_out, C.c_uint8), C.byref(t)), 'iss_cnn_probs_async')
        return t.value, probs_out, finite_out

    def cnn_dead_stats(self):
        """{'windows', 'dead'}: windows cnn_probs / cnn_probs_async were given since the context was created, and how many of them
        were left out of the passes because they hold a non-finite log-mel value (include/iss.h)."""
        w, d = C.c_int64(0), C.c_int64(0)
        self._ck(self._L.iss_cnn_dead_stats(self._h, C.byref(w), C.byref(d)), 'iss_cnn_dead_stats')
        return {'windows': w.value, 'dead': d.value}

    def wait(self, ticket=-1):
        self._ck(self._L.iss_wait(self._h, int(ticket)), 'iss_wait')

    def wait_slots(self, ticket, upto):
        """iss_wait_slots: block until slots [0, upto) of cnn_probs_async call `ticket` are in its output arrays (upto <= 0: do not
        block) -> how many slots have landed: >= upto, never less than an earlier answer, the call's slot count once it is
        complete.  A ticket that wait() has retired, or that was never given out, answers 2^31 - 1: everything has landed."""
        landed = C.c_int32(0)
        self._ck(self._L.iss_wait_slots(self._h, int(ticket), int(upto), C.byref(landed)), 'iss_wait_slots')
        return landed.value

    # ---- multi-GPU exchange (RCCL)
    def comm_unique_id(self):
        buf = np.zeros(128, dtype=np.uint8)
        self._ck(self._L.iss_comm_unique_id(self._h, _ptr(buf, C.c_uint8)), 'iss_comm_unique_id')
        return buf.tobytes()

    def comm_init(self, uid, rank, world):
        buf = np.frombuffer(bytes(uid), dtype=np.uint8).copy()
        assert buf.size == 128
        self._ck(self._L.iss_comm_init(self._h, _ptr(buf, C.c_uint8), int(rank), int(world)), 'iss_comm_init')
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_destroy(self):
        self._ck(self._L.iss_comm_destroy(self._h), 'iss_comm_destroy')
        self.comm_rank, self.comm_world = 0, 1

    def allgather_segments(self, rows, capacity):
        """rows: (k,4) int32 of this rank, or None = "my local work failed" -> ((world, capacity, 4) int32, counts (world,));
        rank r's first min(counts[r], capacity) rows are valid, counts[r] == -1 marks a rank that reported failure."""
        world = self.comm_world
        out = np.zeros((world, capacity, 4), dtype=np.int32)
        counts = np.zeros(world, dtype=np.int32)
        if rows is None:
            rows, n = np.zeros((1, 4), np.int32), -1
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
            n = rows.shape[0]
        self._ck(self._L.iss_allgather_segments(self._h, _ptr(rows, C.c_int32), n, int(capacity),
                                                _ptr(out, C.c_int32), _ptr(counts, C.c_int32)), 'iss_allgather_segments')
        return out, counts

    def comm_info(self):
        """{'world', 'rank', 'version', 'lib'} as RCCL itself reports them for this context's communicator."""
        w, r, v = C.c_int32(), C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(512)
        self._ck(self._L.iss_comm_info(self._h, C.byref(w), C.byref(r), C.byref(v), buf, 512), 'iss_comm_info')
        return {'world': w.value, 'rank': r.value, 'version': v.value, 'lib': buf.value.decode(errors='replace')}

    def comm_allreduce_max(self, value):
        v = C.c_double(float(value))
        self._ck(self._L.iss_comm_allreduce_max(self._h, C.byref(v)), 'iss_comm_allreduce_max')
        return v.value

    def cnn_forward(self, net_id, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        out = np.empty((n, self._net_out[net_id]), dtype=np.float32)
        self._ck(self._L.iss_cnn_forward(self._h, net_id, _ptr(x, C.c_float), n, _ptr(out, C.c_float)), 'iss_cnn_forward')
        return out

    def cnn_flops(self, net_id):
        f = C.c_double()
        self._ck(self._L.iss_cnn_flops(self._h, net_id, C.byref(f)), 'iss_cnn_flops')
        return f.value

    def set_precision(self, mode):
        """PREC_BF16X3 (default: split-bf16 MFMA, float32-class results) or PREC_F32 (exact f32 MFMA)."""
        self._ck(self._L.iss_set_precision(self._h, int(mode)), 'iss_set_precision')
        self.precision = int(mode)

    def set_precision_guard(self, threshold):
        """Precision guard (include/iss.h): max |d log p| between the split-operand and the exact-f32 arithmetic above which a
        patch network's first call switches it to the other split mode or to exact f32; <= 0 turns the probe off.  Default 5e-4."""
        self._ck(self._L.iss_set_precision_guard(self._h, float(threshold)), 'iss_set_precision_guard')
        self.guard_threshold = float(threshold)

    def cnn_precision_info(self, net_id):
        """{'mode': PREC_*, 'max_dlogp': probe figure or None, 'slots': windows compared, 'state': 'pending' | 'passed' |
        'escalated' | 'fixed'} of one loaded network."""
        mode, slots, state, d, du = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_float(0)
        self._ck(self._L.iss_cnn_precision_info(self._h, int(net_id), C.byref(mode), C.byref(d), C.byref(slots), C.byref(state), C.byref(du)),
                 'iss_cnn_precision_info')
        return {'mode': {PREC_F32: 'f32', PREC_F16X3: 'f16x3'}.get(mode.value, 'bf16x3'), 'max_dlogp': None if d.value < 0 else float(d.value),
                'max_dlogp_in_use': None if du.value < 0 else float(du.value),
                'slots': slots.value, 'state': ('pending', 'passed', 'escalated', 'fixed')[state.value]}

    def cnn_set_net_precision(self, net_id, mode):
        """Arithmetic of ONE network: PREC_BF16X3 / PREC_F32, or -1 to follow the context again (and be probed again)."""
        self._ck(self._L.iss_cnn_set_net_precision(self._h, int(net_id), int(mode)), 'iss_cnn_set_net_precision')

    def set_workspace_limit(self, nbytes):
        self._ck(self._L.iss_set_workspace_limit(self._h, int(nbytes)), 'iss_set_workspace_limit')
        self.workspace_limit = int(nbytes)

    def mirror_settings(self, other):
        """Give this context the arithmetic mode, workspace cap and profiling state of `other` (the extra device
        contexts of the multi-file pipeline follow the Segmenter's own context)."""
        if getattr(other, 'precision', None) is not None and other.precision != getattr(self, 'precision', None):
            self.set_precision(other.precision)
        if getattr(other, 'workspace_limit', None) is not None and other.workspace_limit != getattr(self, 'workspace_limit', None):
            self.set_workspace_limit(other.workspace_limit)
        if getattr(other, 'diag', 0) != getattr(self, 'diag', 0):
            self.set_diag(other.diag)
        if getattr(other, 'guard_threshold', None) is not None and other.guard_threshold != getattr(self, 'guard_threshold', None):
            self.set_precision_guard(other.guard_threshold)

    def set_diag(self, flags):
        """Kernel-selection switches (include/iss.h ISS_DIAG_*): an int, or names like 'no_shared_first,no_pws2'."""
        flags = diag_flags(flags) if isinstance(flags, str) else int(flags)
        self._ck(self._L.iss_set_diag(self._h, flags), 'iss_set_diag')
        self.diag = flags

    def scribble(self, word):
        """Test aid: fill every scratch buffer of the context (capacity, slack included) with the 32-bit `word`; resident
        signal, features, tables and parameters are left alone (include/iss.h iss_scribble)."""
        self._ck(self._L.iss_scribble(self._h, int(word) & 0xFFFFFFFF), 'iss_scribble')

    def diag_split16(self, x, f16, form=0):
        """Test aid: (hi, lo) uint16 patterns of the conv kernels' operand split of the float32 values `x`, fp16 or bf16 halves;
        form 0 / 1 = four at a time / one at a time (include/iss.h iss_diag_split16)."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        hi, lo = np.empty(x.size, np.uint16), np.empty(x.size, np.uint16)
        p16 = C.POINTER(C.c_uint16)
        self._ck(self._L.iss_diag_split16(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, int(bool(f16)), int(form),
                                          hi.ctypes.data_as(p16), lo.ctypes.data_as(p16)), 'iss_diag_split16')
        return hi, lo

    def synchronize(self):
        self._ck(self._L.iss_synchronize(self._h), 'iss_synchronize')

    # ---- VBx front end
    def vbx_tables(self, window, melbank):
        w = np.ascontiguousarray(window, dtype=np.float64)
        b = np.ascontiguousarray(melbank, dtype=np.float64)
        assert w.shape == (400,) and b.shape == (257, 64)
        self._ck(self._L.iss_vbx_tables(self._h, _ptr(w, C.c_double), _ptr(b, C.c_double)), 'iss_vbx_tables')

    def vbx_features(self, sig_i32, dither_u):
        s = np.ascontiguousarray(sig_i32, dtype=np.int32)
        u = np.ascontiguousarray(dither_u, dtype=np.float64)
        assert s.shape == u.shape and s.ndim == 1
        T = (s.size + 320 - 400) // 160 + 1
        out = np.empty((T, 64), dtype=np.float32)
        t = C.c_int32()
        self._ck(self._L.iss_vbx_features(self._h, _ptr(s, C.c_int32), _ptr(u, C.c_double), s.size,
                                          _ptr(out, C.c_float), C.byref(t)), 'iss_vbx_features')
        self._dither_n = 0          # this entry uploads its own stream over the cached one
        assert t.value == T
        return out

    def vbx_set_dither(self, dither_u):
        u = np.ascontiguousarray(dither_u, dtype=np.float64)
        self._ck(self._L.iss_vbx_set_dither(self._h, _ptr(u, C.c_double), u.size), 'iss_vbx_set_dither')
        self._dither_n = u.size

    def vbx_features_pcm16(self, pcm, to_host=True):
        """-> (T, 64) float32, or with to_host=False just T (the features stay on the device for iss_vbx_embed)."""
        s = np.ascontiguousarray(pcm, dtype=np.int16)
        T = (s.size + 320 - 400) // 160 + 1
        t = C.c_int32()
        if not to_host:
            self._ck(self._L.iss_vbx_features_pcm16(self._h, _ptr(s, C.c_int16), s.size, None, C.byref(t)), 'iss_vbx_features_pcm16')
            assert t.value == T
            return T
        out = np.empty((T, 64), dtype=np.float32)
        self._ck(self._L.iss_vbx_features_pcm16(self._h, _ptr(s, C.c_int16), s.size, _ptr(out, C.c_float), C.byref(t)),
                 'iss_vbx_features_pcm16')
        assert t.value == T
        return out

    def vbx_features_batch_pcm16(self, pcms, to_host=True):
        """Many PCM16 files in one call (iss_vbx_features_batch_pcm16; the cached dither stream must cover the longest).
        -> (frame_off, fea): frame_off = (F + 1,) int32 first arena row of every file, fea = the (frame_off[-1], 64) float32
        arena, or None with to_host=False (it stays resident for vbx_embed, whose window starts are then arena rows)."""
        pcms = [np.asarray(p, dtype=np.int16) for p in pcms]
        soff = np.zeros(len(pcms) + 1, dtype=np.int64)
        soff[1:] = np.cumsum([p.size for p in pcms])
        s = np.ascontiguousarray(np.concatenate(pcms) if pcms else np.zeros(0, np.int16))
        foff = np.zeros(len(pcms) + 1, dtype=np.int32)
        T = int(sum((p.size + 320 - 400) // 160 + 1 for p in pcms))
        out = np.empty((T, 64), dtype=np.float32) if to_host else None
        self._ck(self._L.iss_vbx_features_batch_pcm16(self._h, _ptr(s, C.c_int16), _ptr(soff, C.c_int64), len(pcms),
                                                      _ptr(foff, C.c_int32), _ptr(out, C.c_float) if to_host else None),
                 'iss_vbx_features_batch_pcm16')
        return foff, out

    def vbx_features_resident(self, begins, counts, to_host=False):
        """The batch front end on parts of the resident PCM16 signal (iss_vbx_features_resident): part p = its samples
        [begins[p], begins[p] + counts[p]); nothing is uploaded but the two tables.  -> (frame_off, fea) as
        vbx_features_batch_pcm16 returns them, fea None unless to_host."""
        b = np.ascontiguousarray(begins, dtype=np.int64).reshape(-1)
        n = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        if b.size != n.size:
            raise ValueError(f'vbx_features_resident: {b.size} begins, {n.size} counts')
        foff = np.zeros(b.size + 1, dtype=np.int32)
        T = int(sum((int(k) + 320 - 400) // 160 + 1 for k in n if k >= 200))
        out = np.empty((T, 64), dtype=np.float32) if to_host else None
        self._ck(self._L.iss_vbx_features_resident(self._h, _ptr(b, C.c_int64), _ptr(n, C.c_int64), b.size, _ptr(foff, C.c_int32),
                                                   _ptr(out, C.c_float) if to_host else None), 'iss_vbx_features_resident')
        return foff, (out[:foff[-1]] if to_host else None)

    def vbx_resident_stats(self):
        """(vbx_features_resident calls that launched -- one fbank launch each --, parts they took) since the context was created."""
        return self._counters('iss_vbx_resident_stats')

    def vbx_embed(self, net_id, starts):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        out = np.empty((st.size, self._net_out[net_id]), dtype=np.float32)
        self._ck(self._L.iss_vbx_embed(self._h, net_id, _ptr(st, C.c_int32), st.size, _ptr(out, C.c_float)), 'iss_vbx_embed')
        return out

    # ---- profiling
    def prof_enable(self, on=True):
        self._ck(self._L.iss_prof_enable(self._h, 1 if on else 0), 'iss_prof_enable')

    def prof_reset(self):
        self._ck(self._L.iss_prof_reset(self._h), 'iss_prof_reset')

    def prof_get(self, kind):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self._L.iss_prof_get(self._h, kind, C.byref(ms), C.byref(n), C.byref(fl)), 'iss_prof_get')
        return ms.value, n.value, fl.value

    def prof_instances(self):
        """[{'kernel', 'ms', 'launches', 'flops'}] per distinct kernel instantiation launched since the last prof_reset."""
        out = []
        buf = C.create_string_buffer(192)
        i = 0
        while True:
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            if self._L.iss_prof_get_instance(self._h, i, buf, 192, C.byref(ms), C.byref(n), C.byref(fl)) != 0:
                break
            out.append({'kernel': buf.value.decode(), 'ms': ms.value, 'launches': n.value, 'flops': fl.value})
            i += 1
        return out

    def prof_get_row(self, row):
        """(ms, launches) of op-program row `row` since the last prof_reset (per-layer view of the same event brackets)."""
        ms, n = C.c_double(), C.c_int64()
        self._ck(self._L.iss_prof_get_row(self._h, int(row), C.byref(ms), C.byref(n)), 'iss_prof_get_row')
        return ms.value, n.value
