// Which kernel runs a conv row of the op program, decided on the host without touching the device.  Every condition a kernel family
// is taken under is written here once, and the answer names the instantiation once (ConvChoice::inst, a ConvInst of conv_common.h):
// inst_name spells it for the profiler, launch_conv (cnn.hip) hands it to the family's launcher, and a launcher runs the instantiation
// whose template arguments equal it or reports that it holds none -- it has nothing else to choose by.
#pragma once
#include <array>
#include <numeric>
#include "iss_internal.h"
#include "conv_common.h"
#include "conv_ws.h"
#include "conv_wq.h"
#include "conv_wq3.h"
#include "conv_wq3h.h"
#include "conv_dhl.h"
#include "conv_pwc.h"
#include "conv_pw.h"

namespace issk {

// Kernel shapes conv_x3_fp_kernel is instantiated for (the tap loop is unrolled at compile time);
// other shapes run on conv_x3_kernel.
// conv_x3_ws_kernel decomposes a flattened window pixel p < limit as p / W == (p * ceil(2^16 / W)) >> 16: exact iff
// limit * (ceil(2^16 / W) * W - 2^16) < 2^16
inline bool ws_recip_exact(int W, long long limit) {
    const long long m = (65536 + W - 1) / W;
    return limit * (m * W - 65536) < 65536 && limit * m < (1ll << 31);
}
inline bool ws_shape_compiled(int kh, int kw) { ISS_WS_SHAPES(ISS_SHAPE_IS) return false; }
inline bool fp_shape_compiled(int kh, int kw) { ISS_FP_SHAPES(ISS_SHAPE_IS) return false; }
#ifdef ISS_PW_NO_ASM_RING                            // build-time escape (Makefile): none of the asm-load kernels of conv_pw.h / conv_pwc.h
constexpr bool asm_ring_ok = false;
#else
constexpr bool asm_ring_ok = true;
#endif

// fused-pool window of a conv row (1,1 when absent)
inline void fused_pool_of(const int32_t* R, int& ph, int& pw) {
    ph = R[ISS_C_FPOOLH] > 1 ? R[ISS_C_FPOOLH] : 1;
    pw = R[ISS_C_FPOOLW] > 1 ? R[ISS_C_FPOOLW] : 1;
}

// The shape part of ConvArgs from a program row and the pass size (everything kernel selection reads; pointers, tables and the
// grid are the launch's).  Returns `padded`: some tap of some output reads outside the input.
inline bool fill_geometry(ConvArgs& a, const int32_t* R, int bc) {
    a.H = R[ISS_C_H]; a.W = R[ISS_C_W]; a.Cin = R[ISS_C_CIN]; a.Cout = R[ISS_C_COUT];
    fused_pool_of(R, a.ph, a.pw);
    a.pp = a.ph * a.pw;
    a.poolkind = R[ISS_C_POOLKIND];
    a.Hq = R[ISS_C_HO] / a.ph; a.Wq = R[ISS_C_WO] / a.pw;
    a.H_k = R[ISS_C_KH]; a.kw = R[ISS_C_KW];
    a.sh = R[ISS_C_SH]; a.sw = R[ISS_C_SW]; a.pt_ = R[ISS_C_PT]; a.pl_ = R[ISS_C_PL];
    a.act = R[ISS_C_ACT];
    a.M = (long long)bc * a.Hq * a.Wq * a.pp;
    if (R[ISS_C_INMODE] == 1) { a.row_stride = 24; a.pix_stride = 1; a.img_stride = 0; }                 // log-mel patches
    else if (R[ISS_C_INMODE] == 2) { a.row_stride = 1; a.pix_stride = a.H; a.img_stride = 0; }          // x-vector windows
    else { a.row_stride = a.W * a.Cin; a.pix_stride = a.Cin; a.img_stride = (long long)a.H * a.W * a.Cin; }
    return a.pt_ != 0 || a.pl_ != 0 || (R[ISS_C_HO] - 1) * a.sh - a.pt_ + a.H_k > a.H || (R[ISS_C_WO] - 1) * a.sw - a.pl_ + a.kw > a.W;
}
inline double conv_flops(const int32_t* R, double M) { return 2.0 * R[ISS_C_KH] * R[ISS_C_KW] * R[ISS_C_CIN] * (double)R[ISS_C_COUT] * M; }

// Host replica of the device's row mapping / footprint arithmetic: does every 128-row tile of this
// layer touch at most FPIX pixels?  Tiles start at multiples of TM and the pattern repeats every sample, so the tiles
// starting in the first lcm(rows per sample, TM) rows decide.  The answer is that of a launch over any number of samples:
// the call's own count (a.M) is not used, so a call of a few windows, whose only tile ends early, takes the kernel a large
// call takes, and a window's result does not depend on how many windows share its pass.
inline int footprint_pixels(const ConvArgs& a, int TM) {      // largest pixel span of a TM-row tile of this layer (INT_MAX: irregular)
    const long long rows_per_sample = (long long)a.Hq * a.Wq * a.pp;
    const long long lim_rows = std::lcm(rows_per_sample, (long long)TM);
    auto pix_of = [&](long long m, int ky, int kx) {
        long long q = m;
        int dy = 0, dx = 0;
        if (a.pp > 1) { q = m / a.pp; const int j = (int)(m - q * a.pp); dy = j / a.pw; dx = j - dy * a.pw; }
        const int hw = a.Hq * a.Wq;
        const long long b = q / hw;
        const int rem = (int)(q - b * hw);
        const int qy = rem / a.Wq, qx = rem - qy * a.Wq;
        const int oy = qy * a.ph + dy, ox = qx * a.pw + dx;
        return (b * a.H + (oy * a.sh - a.pt_ + ky)) * a.W + (ox * a.sw - a.pl_ + kx);
    };
    long long worst = 0;
    for (long long m0 = 0; m0 < lim_rows; m0 += TM) {
        const long long m_last = m0 + TM - 1;
        const long long lo = pix_of(m0, 0, 0), hi = pix_of(m_last, a.H_k - 1, a.kw - 1);
        worst = std::max<long long>(worst, hi - lo + 1);
        // rows inside the tile never reach below lo / above hi (row-major or pool-window-major order); check anyway
        for (long long m = m0; m <= m_last; ++m)
            if (pix_of(m, 0, 0) < lo || pix_of(m, a.H_k - 1, a.kw - 1) > hi) return 0x7fffffff;
    }
    return (int)std::min<long long>(worst, 0x7fffffff);
}
// IssNet::fp_pix, the footprint cache: the largest pixel span of a TM-row tile of row r (a = its geometry) ...
inline int tile_span(IssNet& n, int r, const ConvArgs& a, int TM) {
    auto it = n.fp_pix.find({r, TM, 0, 0});
    if (it == n.fp_pix.end()) it = n.fp_pix.emplace(std::array<int, 4>{r, TM, 0, 0}, footprint_pixels(a, TM)).first;
    return it->second;
}
// ... and the largest tile height that is a multiple of 4 below `hi`, at least `lo`, and spans at most `cap` pixels (0: none)
inline int tile_rows(IssNet& n, int r, const ConvArgs& a, int hi, int lo, int cap) {
    auto it = n.fp_pix.find({r, hi, lo, cap});
    if (it != n.fp_pix.end()) return it->second;
    int tmr = 0;
    for (int cand = hi; cand >= lo && !tmr; cand -= 4)
        if (footprint_pixels(a, cand) <= cap) tmr = cand;
    return n.fp_pix.emplace(std::array<int, 4>{r, hi, lo, cap}, tmr).first->second;
}

enum class FirstLayer { None, Fused, Gather, Alone };   // a deferred first layer: staged by a footprint kernel, read by the gather kernel, or run by itself first
enum class OutLayout { F32, Chl, ChlDense };
struct ChlState { unsigned np = 0; bool f16 = false, dense = false; };   // np != 0: the buffer holds a CHL tensor of np pixels per plane (fp16 halves; of a dense layer)

struct ConvChoice {
    ConvInst inst;                           // the instantiation: kernel family and template arguments (what inst_name spells and the launcher matches)
    int row = -1, partner = -1, rows = 1;    // the row launched; the chained row behind it / the projection row in front of it; program rows consumed
    int tag = ISS_PROF_GATHER;               // kernel class the profiler counts the launch under
    int tmr = 0;                             // rows per tile where the kernel takes them from the host (ConvArgs::tmr)
    FirstLayer first = FirstLayer::None;
    OutLayout out = OutLayout::F32;
    bool out_f16 = false;                    // CHL output in fp16 (not bf16) halves
    unsigned out_np = 0, in_np = 0;          // ... and its pixels per plane; those of the CHL input the kernel reads (0: f32)
    bool generic_out = false;                // the CHL output goes through the shared pooled epilogue (ConvArgs::out_f16 tells it the halves)
};

// What selection depends on, and nothing else.
struct ConvEnv {
    IssNet& n;                               // host tables only: prog, kpad, wsum_off, wsumx_off (and the footprint cache)
    int bc, rmin, rmax;
    bool share_first;
    int prec;                                // effective precision of this network
    uint32_t diag;
    bool have_winrow, have_input, have_vbx;
    const ChlState* layout;                  // per activation buffer, as earlier rows left it; null: every tensor f32 and no output layout asked for
    double net_flops = 0.0;
    bool x3mode() const { return prec != ISS_PREC_F32; }          // a split-operand mode (bf16 or fp16 halves)
    // ISS_PREC_F16X3: the launches with an fp16 instantiation (the one-wave-per-SIMD conv2 / conv3 / conv4 kernels and the long-K
    // dense kernel: > 99.9 % of the segmenter nets' arithmetic) take fp16 operand halves; a SMALL layer without one runs in exact
    // f32 (conv_igemm_kernel: tests/precision_emulation.py -- the last dense layers in bf16 halves would undo most of the gain),
    // anything else keeps bf16 halves
    bool f16mode() const { return prec == ISS_PREC_F16X3; }
    const int32_t* row(int r) const { return &n.prog[(size_t)r * ISS_PROG_COLS]; }
    ChlState layout_of(int buf) const { return layout && buf != ISS_BUF_INPUT ? layout[buf] : ChlState{}; }
};
inline ConvEnv make_env(IssNet& n, int bc, int rmin, int rmax, bool share_first, int prec, uint32_t diag, bool winrow, bool input, bool vbx, const ChlState* layout) {
    ConvEnv env{n, bc, rmin, rmax, share_first, prec, diag, winrow, input, vbx, layout};
    if (env.f16mode())
        for (int q = 0; q < n.nrows; ++q)
            if (env.row(q)[ISS_C_OP] == ISS_OP_CONV) env.net_flops += conv_flops(env.row(q), (double)env.row(q)[ISS_C_HO] * env.row(q)[ISS_C_WO]);
    return env;
}
// nobody but row r + 1 reads row r's output before the buffer is written again
inline bool sole_reader_is_next(const ConvEnv& env, int r) {
    const int ob = env.row(r)[ISS_C_OUT];
    for (int t = r + 2; t < env.n.nrows; ++t) {
        const int32_t* T = env.row(t);
        if (T[ISS_C_IN] == ob || T[ISS_C_RES] == ob) return false;
        if (T[ISS_C_OUT] == ob) break;
    }
    return true;
}

// A PATCH first layer directly in front of a footprint-kernel conv is not launched per window: it is computed once
// per log-mel row and the second conv normalises it per window while staging its LDS footprint (ConvArgs::f_*,
// conv_fp.h FUSED).  Static part of the test; the footprint-capacity part is decided when the second row is reached
// (the first layer is then launched per window after all).
inline bool can_defer(const ConvEnv& env, int r) {
    const IssNet& n = env.n;
    if (r + 1 >= n.nrows || !env.share_first || env.rmax < env.rmin) return false;
    // exact-f32 mode: only the shape the F32 form of the weight-stationary kernel is instantiated for (conv_ws.h F32, cnn_ws_h.hip)
    const bool x3mode = env.x3mode(), f32defer = !x3mode;
    if (f32defer && (env.diag & (ISS_DIAG_NO_WS | ISS_DIAG_NO_F32WS))) return false;
    const int32_t *R1 = env.row(r), *R2 = env.row(r + 1);
    int ph, pw;
    fused_pool_of(R1, ph, pw);
    const bool pool1 = ph * pw != 1;                 // fused non-overlapping pool behind the first layer: max only, gather path only
    if (R1[ISS_C_OP] != ISS_OP_CONV || R1[ISS_C_INMODE] != 1 || R1[ISS_C_RES] >= 0 || R1[ISS_C_ACT] > 1) return false;
    if (pool1 && (R1[ISS_C_POOLKIND] != 0 || !x3mode || (env.diag & ISS_DIAG_NO_GFUSED))) return false;
    if (R1[ISS_C_CIN] != 1 || R1[ISS_C_SH] != 1 || R1[ISS_C_SW] != 1) return false;
    const bool valid1 = R1[ISS_C_PT] == 0 && R1[ISS_C_PL] == 0 && R1[ISS_C_HO] == R1[ISS_C_H] - R1[ISS_C_KH] + 1 &&
                        R1[ISS_C_WO] == R1[ISS_C_W] - R1[ISS_C_KW] + 1;                                                     // 'valid'
    // 'same' (zero-padded, output = input size): shared through conv_x3_ws_kernel<..., FS> (S table + per-window edge rows)
    const bool same_geo = !valid1 && R1[ISS_C_HO] == R1[ISS_C_H] && R1[ISS_C_WO] == R1[ISS_C_W] && R1[ISS_C_PT] <= R1[ISS_C_KH] - 1 &&
                          R1[ISS_C_PL] <= R1[ISS_C_KW] - 1 && R1[ISS_C_KH] <= R1[ISS_C_H] && n.wsumx_off[r] >= 0 && R1[ISS_C_PSOFF] < 0 &&
                          !(env.diag & ISS_DIAG_NO_FSAME);
    const bool same_ws = same_geo && R1[ISS_C_W] * R1[ISS_C_COUT] * 4 <= WS_STAB && !(env.diag & ISS_DIAG_NO_WS) &&
                         iss_ws_fs_compiled(R2[ISS_C_KH], R2[ISS_C_KW]);
    // ... or through the generic gather kernel (conv_x3_kernel<4>: any second conv)
    const bool same1 = same_ws || (same_geo && x3mode && !(env.diag & ISS_DIAG_NO_GFUSED));
    if (!valid1 && !same1) return false;
    if (pool1 && !valid1) return false;
    if (f32defer && (!valid1 || !iss_ws_f32_fused_compiled(R2[ISS_C_KH], R2[ISS_C_KW]) || R2[ISS_C_SH] != 1 || R2[ISS_C_SW] != 1 ||
                     R2[ISS_C_PT] != 0 || R2[ISS_C_PL] != 0 || R1[ISS_C_PSOFF] >= 0)) return false;
    if (R1[ISS_C_KH] * R1[ISS_C_KW] * R1[ISS_C_COUT] * 4 > 48 * 1024) return false;        // first_layer_raw_kernel's LDS weights
    if (R1[ISS_C_BOFF] < 0 || (R1[ISS_C_PSOFF] >= 0) != (R1[ISS_C_PTOFF] >= 0) || R1[ISS_C_COUT] % 4 != 0 || n.wsum_off[r] < 0) return false;
    if (R2[ISS_C_OP] != ISS_OP_CONV || R2[ISS_C_INMODE] != 0 || R2[ISS_C_IN] != R1[ISS_C_OUT] || R2[ISS_C_RES] >= 0) return false;
    if (R2[ISS_C_CIN] != R1[ISS_C_COUT] || R2[ISS_C_CIN] % XBK != 0 || R2[ISS_C_H] != R1[ISS_C_HO] / ph || R2[ISS_C_W] != R1[ISS_C_WO] / pw) return false;
    const bool ring2 = valid1 && iss_ws_ring_compiled(R2[ISS_C_KH], R2[ISS_C_KW]) && !(env.diag & (ISS_DIAG_NO_RING | ISS_DIAG_NO_WS));
    // a footprint kernel can take it: (a zero-padded second conv is fused by the weight-stationary kernel only; select_row decides);
    // the footprint may touch two windows at most, and the x / W trick of the kernel needs a small W
    const bool foot2 = R2[ISS_C_KH] * R2[ISS_C_KW] >= 8 && (fp_shape_compiled(R2[ISS_C_KH], R2[ISS_C_KW]) || ring2) &&   // (>= 12 unless the weight-stationary kernel takes it, see select_row)
                       R2[ISS_C_H] * R2[ISS_C_W] >= FPIX + 32 && R2[ISS_C_W] <= 128 && (valid1 || same_ws) && !pool1;
    // ... or the generic gather kernel reads the shared rows itself (conv_x3_kernel<3>): any second conv, 'valid' first layer
    const bool gath2 = x3mode && (valid1 || same_geo) && R1[ISS_C_PSOFF] < 0 && !(env.diag & ISS_DIAG_NO_GFUSED);
    if (!foot2 && !gath2) return false;
    return sole_reader_is_next(env, r);                  // nobody else may read the first layer's output
}
// rows r, r + 1: an in-place 1x1 stride-1 expansion with identity residual and relu, then a plain 1x1 stride-1 convolution to
// 32 / 64 / 128 channels that reads it (the next Bottleneck's reduction, resnet.py:48-58) -- the pair conv_x3_pwc_kernel computes
inline bool chain_pair(const ConvEnv& env, int r) {
    const IssNet& n = env.n;
    if (r + 1 >= n.nrows) return false;
    const int32_t *R1 = env.row(r), *R2 = env.row(r + 1);
    int ph, pw, ph2, pw2;
    fused_pool_of(R1, ph, pw), fused_pool_of(R2, ph2, pw2);
    auto plain1x1 = [](const int32_t* R) {
        return R[ISS_C_OP] == ISS_OP_CONV && R[ISS_C_KH] == 1 && R[ISS_C_KW] == 1 && R[ISS_C_SH] == 1 && R[ISS_C_SW] == 1 &&
               R[ISS_C_PT] == 0 && R[ISS_C_PL] == 0 && R[ISS_C_INMODE] == 0 && R[ISS_C_PSOFF] < 0 && R[ISS_C_BOFF] >= 0 &&
               R[ISS_C_HO] == R[ISS_C_H] && R[ISS_C_WO] == R[ISS_C_W];
    };
    return plain1x1(R1) && plain1x1(R2) && ph * pw == 1 && ph2 * pw2 == 1 && R1[ISS_C_DUALW] == 0 &&
           R1[ISS_C_RES] >= 0 && R1[ISS_C_RES] == R1[ISS_C_OUT] && R1[ISS_C_IN] != R1[ISS_C_OUT] && R1[ISS_C_IN] != ISS_BUF_INPUT &&
           R1[ISS_C_ACT] == 1 && R2[ISS_C_IN] == R1[ISS_C_OUT] && R2[ISS_C_RES] < 0 && R2[ISS_C_OUT] != R1[ISS_C_OUT] &&
           R2[ISS_C_OUT] != R1[ISS_C_IN] && R2[ISS_C_ACT] <= 1 && R2[ISS_C_CIN] == R1[ISS_C_COUT] && pwc_compiled(R1[ISS_C_CIN], R2[ISS_C_COUT]) &&
           R2[ISS_C_H] == R1[ISS_C_HO] && R2[ISS_C_W] == R1[ISS_C_WO] && n.kpad[r] == R1[ISS_C_CIN] && n.kpad[r + 1] == R2[ISS_C_CIN];
}
// (fp16 mode) a small layer -- under 0.5 % of the network's arithmetic -- that no fp16 kernel takes: exact f32.  A producer asks
// through the consumer's selection too: it must not hand the CHL layout to a row that then runs an f32 kernel
inline bool small_row_of(const ConvEnv& env, int r, int pend, bool* f16_dense_pw_out) {
    const int32_t* R = env.row(r);
    const double row_flops = conv_flops(R, (double)R[ISS_C_HO] * R[ISS_C_WO]);
    const bool small_cand = env.f16mode() && pend < 0 && row_flops < 0.005 * env.net_flops && row_flops < 2e6 &&     // (and small in absolute terms: a
                            R[ISS_C_INMODE] == 0 && !can_defer(env, r);                                              //  ResNet-101 has 105 layers under 1 %)
    // ... unless it is a dense layer of some width (a 512 -> 512 head: 0.5 MFLOP per window, 66 TFLOP/s on conv_igemm_kernel, 5 % of
    // such a net's step): conv_x3_pw_kernel has an fp16 form for any K, so it takes the layer instead of the streaming kernels
    int ph, pw;
    fused_pool_of(R, ph, pw);
    *f16_dense_pw_out = small_cand && row_flops >= 2.5e5 && R[ISS_C_KH] == 1 && R[ISS_C_KW] == 1 && R[ISS_C_H] == 1 && R[ISS_C_W] == 1 &&
                        R[ISS_C_HO] == 1 && R[ISS_C_WO] == 1 && ph * pw == 1 && R[ISS_C_SH] == 1 && R[ISS_C_SW] == 1 && R[ISS_C_PT] == 0 &&
                        R[ISS_C_PL] == 0 && R[ISS_C_COUT] % 4 == 0 && R[ISS_C_CIN] % XBK == 0 && env.n.kpad[r] == R[ISS_C_CIN] && R[ISS_C_RES] < 0 &&
                        (env.diag & ISS_DIAG_NO_PW) == 0;
    return small_cand && !*f16_dense_pw_out;
}
// the simple transposed epilogue (bias, optional relu; float4 stores) or the pooled relu one: what the exact-f32, the padded NH = 2 and
// the unpadded plain forms of the weight-stationary kernel are compiled with
inline bool epi_tr_simple(const ConvArgs& a) { return a.pp == 1 && a.Cout % 4 == 0 && epi_is_simple_tr(a); }
inline bool epi_pooled_relu(const ConvArgs& a) { return a.pp > 1 && epi_is_pool_relu(a); }

ConvChoice select_conv(const ConvEnv& env, int r, int pend);

// row r's output (Cout channels, `npix` pixels for this call) may be written in the CHL layout: row r + 1 is a conv_x3_wq3h_kernel
// launch that reads it -- on an f32 input its selection is conv_x3_wq3_kernel -- and nobody else does before the buffer is written again
inline bool want_hl_out(const ConvEnv& env, int r, long long npix) {
    if (!env.layout || (env.diag & ISS_DIAG_NO_HL) || r + 1 >= env.n.nrows) return false;
    const int32_t *R = env.row(r), *Q = env.row(r + 1);
    const int ob = R[ISS_C_OUT];
    if (Q[ISS_C_OP] != ISS_OP_CONV || Q[ISS_C_IN] != ob || Q[ISS_C_OUT] == ob || Q[ISS_C_CIN] != R[ISS_C_COUT] || (R[ISS_C_COUT] % (2 * BN) != 0 && R[ISS_C_COUT] != BN)) return false;
    if (npix != (long long)env.bc * Q[ISS_C_H] * Q[ISS_C_W] || !chl_fits(npix, R[ISS_C_COUT])) return false;
    ConvEnv f32in = env;
    f32in.layout = nullptr;
    return select_conv(f32in, r + 1, -1).inst.kernel == ConvKernel::Wq3 && sole_reader_is_next(env, r);
}
// row r is a pooled conv launch (conv_x3_wq3h_kernel<1, ..>) whose output, flattened, is read by the dense layer of row r + 1 and by
// nobody else: it may write the CHL tensor conv_dhl_kernel fetches by LDS-DMA (window = "pixel", feature = "channel").  The selector
// cannot be asked here as want_hl_out asks it: no f32 selection means "conv_dhl_kernel", row r + 1 takes that kernel BECAUSE of the
// layout it is handed (select_row, first test), so these conditions are that kernel's only copy
inline bool want_dhl_out(const ConvEnv& env, int r, int hq, int wq) {
    const IssNet& n = env.n;
    if (!env.layout || (env.diag & ISS_DIAG_NO_HL) || r + 1 >= n.nrows || !env.x3mode()) return false;
    const int32_t *R = env.row(r), *Q = env.row(r + 1);
    const int ob = R[ISS_C_OUT], bc = env.bc;
    const long long K = (long long)hq * wq * R[ISS_C_COUT];
    int qph, qpw;
    fused_pool_of(Q, qph, qpw);
    if (Q[ISS_C_OP] != ISS_OP_CONV || Q[ISS_C_IN] != ob || Q[ISS_C_OUT] == ob || Q[ISS_C_INMODE] != 0 || Q[ISS_C_RES] >= 0 || Q[ISS_C_DUALW] != 0) return false;
    if (Q[ISS_C_KH] != 1 || Q[ISS_C_KW] != 1 || Q[ISS_C_H] != 1 || Q[ISS_C_W] != 1 || Q[ISS_C_HO] != 1 || Q[ISS_C_WO] != 1 || qph * qpw != 1) return false;
    if (Q[ISS_C_CIN] != K || n.kpad[r + 1] != K || hq * wq < 2 || R[ISS_C_COUT] % 8 != 0) return false;
    if (!dhl_supported((int)K, Q[ISS_C_COUT], Q[ISS_C_ACT], Q[ISS_C_PSOFF] >= 0, false)) return false;
    const size_t bytes = (size_t)dhl_npad(bc) * (size_t)K * 4;
    if (bytes > (size_t)bc * K * 4 + ISS_ACT_SLACK || bytes >= 0xFFF00000ull || (long long)bc * hq * wq * (hq * wq) >= (1ll << 32)) return false;
    if ((long long)bc * Q[ISS_C_COUT] * 4 >= (1ll << 32)) return false;
    return sole_reader_is_next(env, r);
}

// One launch: row r alone (dual, chain < 0), rows (dual, r) as the two-source GEMM, or rows (r, chain) as the chained pair.
inline ConvChoice select_row(const ConvEnv& env, int r, int pend, int dual, int chain) {
    IssNet& n = env.n;
    const int32_t* R = env.row(r);
    const int32_t* Rp = pend >= 0 ? env.row(pend) : nullptr;      // the deferred first layer in front
    const int bc = env.bc;
    const uint32_t diag = env.diag;
    // selection asks only whether a row HAS a bias / affine / residual: `has` stands for every such pointer, so the *_supported /
    // epi_is_* helpers it calls may test a ConvArgs pointer for null (and res == out), never read through it or its value
    static const float has = 0.f;
    ConvChoice ch;
    ConvInst& inst = ch.inst;                                     // every field a launch's template fixes ends up here, whichever way it was decided
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    const bool padded = fill_geometry(a, R, bc);
    a.bias = R[ISS_C_BOFF] >= 0 ? &has : nullptr; a.res = R[ISS_C_RES] >= 0 ? &has : nullptr;
    a.ps = R[ISS_C_PSOFF] >= 0 ? &has : nullptr; a.pt = R[ISS_C_PTOFF] >= 0 ? &has : nullptr;
    a.Kpad = n.kpad[r];
    const bool patch = R[ISS_C_INMODE] == 1, window = R[ISS_C_INMODE] == 2;
    auto present = [&](const int32_t* Q) { return Q[ISS_C_IN] != ISS_BUF_INPUT || env.have_input; };
    bool f16_dense_pw = false;
    const bool small_row = small_row_of(env, r, pend, &f16_dense_pw);
    const bool x3 = env.x3mode() && !small_row, f16mode = env.f16mode();
    const ChlState in_l = env.layout_of(R[ISS_C_IN]);            // (only conv_x3_wq3h_kernel and conv_dhl_kernel read the CHL layout)
    ch.row = r; inst.kh = a.H_k; inst.kw = a.kw; inst.padded = padded; inst.window = window;
    if (in_l.np && in_l.dense) {
        // the first dense layer on the flattened-feature CHL tensor conv4 wrote for it (want_dhl_out): both operands by LDS-DMA
        inst.kernel = ConvKernel::Dhl; inst.f16 = in_l.f16; ch.in_np = in_l.np; ch.tag = ISS_PROF_PW;
        return ch;
    }
    a.mode = patch ? 2 : window ? 1 : ((a.Cin % (x3 ? XBK : 4) == 0) ? 0 : 1);
    inst.mode = a.mode;
    const double fl = conv_flops(R, (double)a.M);
    if (chain >= 0) {
        // row r (in-place 1x1 expansion + identity residual + relu) and row `chain` = r + 1 (the next Bottleneck's 1x1 reduction
        // to 128 channels, which reads row r's output) as ONE launch: the reduction consumes x' out of LDS (conv_pwc.h)
        const int32_t* Q = env.row(chain);
        a.bias2 = Q[ISS_C_BOFF] >= 0 ? &has : nullptr;
        a.out = R[ISS_C_RES] == R[ISS_C_OUT] ? const_cast<float*>(a.res) : nullptr;
        a.act2 = Q[ISS_C_ACT]; a.Cout2 = Q[ISS_C_COUT];
        if (!x3 || a.mode != 0 || !present(R) || !pwc_supported(a)) return ch;
        inst.kernel = ConvKernel::Pwc; ch.partner = chain; ch.rows = 2; inst.c1 = a.Cin / 32; inst.c3 = a.Cout2 / 32; ch.tag = ISS_PROF_PW;
        return ch;
    }
    if (dual >= 0) {
        // rows `dual` (a linear 1x1 projection, any stride) and r (the in-place 1x1 expansion it is added to) as ONE GEMM over
        // both inputs on the concatenated weights (ISS_C_DUALW; validated by iss_cnn_load): row `dual`'s output never exists
        const int32_t* P = env.row(dual);
        a.Cin2 = P[ISS_C_CIN]; a.H2 = P[ISS_C_H]; a.W2 = P[ISS_C_W]; a.sh2 = P[ISS_C_SH]; a.sw2 = P[ISS_C_SW];
        a.bias = &has; a.res = nullptr;
        a.Kpad = a.Cin + a.Cin2;
        if (!x3 || a.mode != 0 || !present(R) || !present(P) || !pws2_dual_supported(a)) return ch;
        inst.kernel = ConvKernel::Pws2Dual; inst.simple_pw = true; ch.partner = dual; ch.rows = 2; ch.tag = ISS_PROF_PW;
        return ch;
    }
    const int taps = a.H_k * a.kw;
    const bool unit_stride = a.sh == 1 && a.sw == 1;
    // LDS-footprint kernel usable
    bool fp = x3 && a.mode == 0 && fp_shape_compiled(a.H_k, a.kw) && a.M < (1ll << 31) && tile_span(n, r, a, BM) <= FPIX;
    // weight-stationary kernel (conv_ws.h): the shared-first-layer convolution, 8..16 taps, one N tile of 64 channels
    const bool no_ws = (diag & ISS_DIAG_NO_WS) != 0;
    // the deferred first layer in front is zero-padded ('same'): only the FS form of the weight-stationary kernel can fuse it
    const bool fs1 = Rp && Rp[ISS_C_HO] == Rp[ISS_C_H];
    const bool pool1 = Rp && (Rp[ISS_C_FPOOLH] > 1 || Rp[ISS_C_FPOOLW] > 1);   // the deferred first layer's own fused (max) pool: the gather form only
    const bool affine1 = Rp && Rp[ISS_C_PSOFF] >= 0;             // (a post-activation affine of the first layer stays on conv_x3_fp_kernel)
    bool ws = !no_ws && fp && Rp && taps >= 8 && taps <= WS_MAXNT && ws_shape_compiled(a.H_k, a.kw) &&
              a.Cin % F2_CH == 0 && a.H * a.W >= WS_PIX + 64 + (a.pt_ + 1) * a.W && ws_recip_exact(a.W, a.H * a.W + WS_PIX + a.W) &&
              tile_span(n, r, a, WS_TM) <= WS_PIX && !affine1;
    // ring form (conv_ws.h RING): more than WS_MAXNT taps (7x7), first-layer-fused, one 512-row tile per group on a
    // 1024-pixel footprint; row-major epilogue
    bool ws_ring = false;
    int tmr = 0;
    if (!no_ws && !(diag & ISS_DIAG_NO_RING) && Rp && !fs1 && x3 && a.mode == 0 && iss_ws_ring_compiled(a.H_k, a.kw) &&
        unit_stride && a.Cin % F2_CH == 0 && a.Cin >= 2 * F2_CH && a.M < (1ll << 31) &&
        ws_recip_exact(a.W, a.H * a.W + WS_PIX2 + a.W) && !affine1) {
        // rows per tile: the largest multiple of 4 (<= 512, >= 320) whose footprint fits the 1024 pixels -- a 512-row tile of a
        // pooled 59 x 14 output under a 7-row filter spans 1036 pixels, 496 rows 1002 (ConvArgs::tmr; the rest of the tile idles)
        // ... and reaches into at most ONE following window (the fetch decomposes a footprint position into two windows)
        const int cap = std::min<long long>(WS_PIX2, (long long)a.H * a.W - 64 - (long long)(a.pt_ + 1) * a.W);
        tmr = tile_rows(n, r, a, WS_TM, 320, cap);
        ws_ring = tmr > 0 && a.M % 4 == 0;
        if (ws_ring) { ws = true; fp = true; } else tmr = 0;
    }
    // exact-f32 mode (ISS_PREC_F32): the F32 form of the weight-stationary kernel for the first-layer-fused 5x3 layer
    const bool no_f32ws = (diag & ISS_DIAG_NO_F32WS) != 0;
    bool ws_f32 = !x3 && !no_ws && !no_f32ws && Rp && !fs1 && a.mode == 0 && iss_ws_f32_fused_compiled(a.H_k, a.kw) && !padded &&
                  unit_stride && epi_is_pool_relu(a) && a.Cin % F2_CH == 0 && a.Cin >= 2 * F2_CH && a.M < (1ll << 31) &&
                  a.H * a.W >= WS_PIX + 64 + a.W && ws_recip_exact(a.W, a.H * a.W + WS_PIX + a.W) && !affine1 && tile_span(n, r, a, WS_TM) <= WS_PIX;
    if (ws_f32) { ws = true; fp = true; }
    // FS form: row-major epilogue only.  A second conv WITHOUT a fused pool is not taken: its unpooled output through the row-major
    // epilogue (4-byte stores) measured 3.1 -> 2.3 h/s on conv1_same_nopool against the per-window first layer + transposed kernel
    // ... except the one transposed instantiation: unpadded 5x3 with bias + relu (cnn_ws_f.hip)
    const bool fs_tr = a.pp == 1 && a.Cout % 4 == 0;
    const bool fs_tr_ok = fs_tr && a.H_k == 5 && a.kw == 3 && !padded && epi_is_simple_tr(a);
    const bool ws_fs = fs1 && ws && iss_ws_fs_compiled(a.H_k, a.kw) && (!fs_tr || fs_tr_ok) && unit_stride && a.W * a.Cin * 4 <= WS_STAB &&
                       a.Cin >= 2 * F2_CH && !(diag & ISS_DIAG_NO_FSAME);
    if (fs1 && !ws_fs) ws = false;
    // weight-stationary kernel with two column halves per workgroup (conv_ws.h, NH = 2): unpadded 3x3 stride-1 layers with
    // a multiple of 128 output channels whose 512-row tiles fit a 1024-pixel footprint -- the 3x3 layers of the segmenter nets
    const bool nh2_pad_pool = epi_pooled_relu(a);                // ... and row-major with the pooled relu epilogue
    const bool nh2_pad_ok = epi_tr_simple(a) || nh2_pad_pool;    // the padded form is compiled transposed + simple
    // (exact-f32 mode: the unpadded form with the simple transposed or the pooled relu epilogue only -- cnn_ws_h.hip)
    const bool nh2_f32 = !x3 && !no_f32ws && !padded && (epi_tr_simple(a) || epi_pooled_relu(a));
    // a plain (not first-layer-fused) 3x3 stride-1 weight-stationary launch: 32-bit byte offsets into the input batch
    const bool plain3 = !no_ws && pend < 0 && a.mode == 0 && unit_stride && !a.res && a.Cin % F2_CH == 0 && a.M < (1ll << 31) &&
                        (long long)bc * a.img_stride * 4 < (1ll << 32);
    const bool ws_nh2 = plain3 && !(diag & ISS_DIAG_NO_WS3) && (x3 || nh2_f32) && (!padded || nh2_pad_ok) && a.Cout % (2 * BN) == 0 &&
                        iss_ws_nh2_compiled(a.H_k, a.kw) && tile_span(n, r, a, WS_TM) <= WS_PIX2;
    // plain weight-stationary launch: a padded 3x3 stride-1 layer too wide for the 360-pixel footprint kernel (see conv_ws.h)
    const bool ws_plain = plain3 && !fp && x3 && padded && a.pp == 1 && a.Cout % 4 == 0 && iss_ws_plain_compiled(a.H_k, a.kw) &&
                          tile_span(n, r, a, WS_TM) <= WS_PIX;
    // ... and the UNPADDED 3x3 stride-1 layers the two-column-half form does not take (64 / 96 output channels): they ran on
    // conv_x3_fp_kernel (weights streamed per tap, 215-312 TF); simple transposed epilogue or pooled relu only (cnn_ws_c.hip)
    const bool ws_plain_u = plain3 && !(diag & ISS_DIAG_NO_WSU3) && !ws_nh2 && x3 && !padded && iss_ws_plain_compiled(a.H_k, a.kw) &&
                            a.Cin >= 2 * F2_CH && (epi_tr_simple(a) || epi_pooled_relu(a)) && tile_span(n, r, a, WS_TM) <= WS_PIX;
    bool fused = false;
    if (Rp) {
        const long long edge_rows = fs1 ? (long long)bc * (Rp[ISS_C_KH] - 1) : 0;                          // per-window edge rows behind R
        fused = !pool1 && fp && (ws || (!fs1 && !padded && taps >= 12)) && env.have_winrow &&
                ((long long)(env.rmax - env.rmin) + Rp[ISS_C_HO] + edge_rows) * Rp[ISS_C_WO] * Rp[ISS_C_COUT] * 4 < (1ll << 32);   // 32-bit BYTE offsets into R
        if (ws_ring && !fused) { ws = false; fp = false; ws_ring = false; tmr = 0; }                      // (no footprint kernel of that shape)
        if (ws_f32 && !fused) { ws = false; fp = false; ws_f32 = false; }                                  // (exact-f32 mode has no other one)
    }
    if (!fused && (long long)bc * a.img_stride >= (1ll << 32)) fp = false;        // 32-bit offsets into the input batch
    // no footprint kernel fuses it and none would run this conv anyway: the generic gather kernel reads the shared first-layer
    // rows itself and applies the window's affine map + activation before its operand split (conv_x3_kernel<3>) -- the per-window
    // first-layer tensor (283-333 KB per slot) is neither written nor read for ANY second conv on overlapping windows
    bool gfused = false;
    if (Rp && !fused && x3 && a.mode == 0 && env.have_winrow && !(diag & ISS_DIAG_NO_GFUSED) && !(fs1 && (diag & ISS_DIAG_NO_FSAME))) {
        gfused = (fs1 || (Rp[ISS_C_PT] == 0 && Rp[ISS_C_PL] == 0)) && Rp[ISS_C_PSOFF] < 0 && Rp[ISS_C_ACT] <= 1 && a.M < (1ll << 31) &&
                 (!fs1 || n.wsumx_off[pend] >= 0);
        if (gfused && fp) {
            // conv_x3_fp_kernel would run this conv (unfused) at ~330 TFLOP/s where the gather kernel does ~230, but needs the
            // per-window first-layer tensor, written at ~2.1 TB/s (measured: conv1_patch_x3_kernel): the gather kernel wins when
            // flops * (1/230e12 - 1/330e12) < bytes / 2.1e12, i.e. below ~360 flops per byte of that tensor (narrow nets)
            const double bytes1 = (double)bc * Rp[ISS_C_HO] * Rp[ISS_C_WO] * Rp[ISS_C_COUT] * 4.0;
            gfused = fl < 360.0 * bytes1;
        }
        if (gfused) fp = false;
    }
    if (Rp) ch.first = fused ? FirstLayer::Fused : gfused ? FirstLayer::Gather : FirstLayer::Alone;
    ws = ws && fused;
    if (gfused) inst.mode = a.mode = fs1 ? 4 : 3;
    inst.fused = fused; ch.tmr = tmr;
    ch.tag = ws || ws_plain || ws_plain_u || ws_nh2 ? ISS_PROF_WS : fp ? ISS_PROF_FP : !x3 ? ISS_PROF_F32 : ISS_PROF_GATHER;
    inst.tr = a.pp == 1 && a.Cout % 4 == 0;            // float4 epilogue on transposed accumulators (the families below that differ say so)
    // one-channel 3x3 'same' first layer of a non-PATCH network: direct f32 kernel (either arithmetic mode)
    const bool direct1 = !(diag & ISS_DIAG_NO_DIRECT1) && !patch && pend < 0 && a.Cin == 1 && a.H_k == 3 && a.kw == 3 && unit_stride && a.pt_ == 1 &&
                         a.pl_ == 1 && R[ISS_C_HO] == a.H && R[ISS_C_WO] == a.W && a.pp == 1 && !a.res && !a.ps && a.act <= 1 && a.bias &&
                         a.Cout % 4 == 0 && a.Cout <= 256 && a.M * (long long)(a.Cout / 4) < (1ll << 34);
    if (direct1) {
        inst.kernel = ConvKernel::Direct1; ch.tag = ISS_PROF_GATHER;
    } else if (ws_nh2 && !x3) {
        inst.kernel = ConvKernel::WsNh2F32; inst.tr = a.pp == 1; inst.nh = 2; inst.epi = 1;
    } else if (ws_nh2) {
        // one-wave-per-SIMD variant (conv_wq3.h): unpadded, bias + relu (kind 0) or relu + 2 x 1 max-pool (kind 1)
        int kind = -1;
        if (!(diag & ISS_DIAG_NO_WQ) && !padded && a.bias && a.act == 1 && !a.ps && !a.res && a.Cin >= 2 * F2_CH &&
            ws_recip_exact(a.W, WQ3_PIX + a.W)) {
            if (a.pp == 1 && a.M * (long long)a.Cout * 4 < 0xFFF00000ll) kind = 0;
            else if (a.pp == 2 && a.ph == 2 && a.poolkind == 0 && (a.M / 2) * (long long)a.Cout * 4 < 0xFFF00000ll) kind = 1;
        }
        if (kind >= 0 && (ch.tmr = tile_rows(n, r, a, WQ3_TM, WQ3_TM - 64, WQ3_PIX)) <= 0) kind = -1;
        if (kind >= 0) {
            inst.kernel = in_l.np ? ConvKernel::Wq3h : ConvKernel::Wq3;       // the producer wrote the CHL layout for this launch (want_hl_out)
            inst.kind = kind; ch.in_np = in_l.np; inst.f16 = in_l.np && in_l.f16;
        } else {
            inst.kernel = ConvKernel::WsNh2; inst.nh = 2;
            inst.tr = (padded && !nh2_pad_pool) || (a.pp == 1 && a.Cout % 4 == 0);
            inst.epi = padded ? 1 : (inst.tr ? epi_is_simple_tr(a) : epi_is_pool_relu(a));
        }
    } else if (ws_plain_u) {
        inst.kernel = ConvKernel::WsPlainU; inst.tr = a.pp == 1; inst.epi = 1;
    } else if (ws_plain) {
        inst.kernel = ConvKernel::WsPlain; inst.epi = epi_is_simple_tr(a);
    } else if (ws && ws_f32) {
        inst.kernel = ConvKernel::WsF32Fused; inst.epi = 1;
    } else if (ws && ws_ring) {
        inst.kernel = ConvKernel::WsRing; inst.tr = false; inst.epi = epi_is_pool_relu_any(a);
    } else if (ws && ws_fs) {
        inst.kernel = ConvKernel::WsFs; inst.tr = fs_tr_ok; inst.epi = fs_tr_ok ? 1 : (int)epi_is_pool_relu_any(a);
    } else if (ws) {
        const bool rowmajor_pool = fused && !padded && !inst.tr && epi_is_pool_relu(a) && unit_stride && a.Cin >= 2 * F2_CH;
        // <= 32 output channels: one 32-column block per workgroup (conv_ws.h NCB = 1) instead of half-empty 64-column ones
        if (!(diag & ISS_DIAG_NO_NCB1) && rowmajor_pool && !fs1 && a.Cout <= 32 && iss_ws_ncb1_compiled(a.H_k, a.kw)) {
            inst.kernel = ConvKernel::WsNcb1; inst.epi = 1;
        } else if (!(diag & ISS_DIAG_NO_WQ) && rowmajor_pool && a.pp == 4 && a.ph == 2 && iss_wq_compiled(a.H_k, a.kw) && a.M % 4 == 0 &&
                   (a.M / 4) * (long long)a.Cout * 4 < 0xFFF00000ll && a.Cout <= 256 && (ch.tmr = tile_rows(n, r, a, WS_TM, WS_TM - 32, WQ_PIX)) > 0) {
            // one-wave-per-SIMD, two-footprint variant (conv_wq.h): the dominant launch of the segmenter nets
            // (tmr, rows per tile: the largest multiple of 4 (<= 512) whose footprint fits the kernel's 800 pixels)
            inst.kernel = ConvKernel::Wq; inst.f16 = f16mode;
        } else {
            inst.kernel = ConvKernel::Ws; inst.epi = inst.tr ? epi_is_simple_tr(a) : epi_is_pool_relu_any(a);
        }
    } else if (fp) {
        inst.kernel = ConvKernel::Fp;
        // 128 output channels per workgroup where the layer has them: one LDS footprint serves two 64-column halves
        inst.nh = (!fused && !(diag & ISS_DIAG_NO_NH2) && iss_fp_has_nh2(a.H_k, a.kw) && a.Cout % (2 * BN) == 0) ? 2 : 1;
        inst.tr = !(diag & ISS_DIAG_NO_TR) && inst.tr;       // diagnostic: row-major epilogue everywhere
    } else if (x3 && patch && taps <= XBK && a.M < (1ll << 31)) {
        // fp16 mode: fp16 halves of the normalised window and of the weights here too (|z| <= sqrt(68 * 24), far inside fp16's range)
        inst.kernel = ConvKernel::Patch1; ch.tag = ISS_PROF_PATCH1; inst.tr = inst.tr && !a.res; inst.f16 = f16mode;
    } else if (x3 && gfused) {
        inst.kernel = ConvKernel::Gather;
    } else if (x3) {
        const bool pointwise = !(diag & ISS_DIAG_NO_PW) && a.mode == 0 && inst.tr && taps == 1 && unit_stride && a.pt_ == 0 &&
                               a.pl_ == 0 && R[ISS_C_HO] == a.H && R[ISS_C_WO] == a.W && a.Kpad == a.Cin;
        if (pointwise) ch.tag = ISS_PROF_PW;
        // Streaming pointwise kernels (conv_pw.h) for K <= 2048.  The segmenter nets' first dense layer (K = 4992 / 8320,
        // 192 columns, ~28 k rows per launch) keeps conv_x3_pw_kernel: it runs at 1.7 TB/s of activations on every tiling
        // that was built for it (deeper ring -8 %; one workgroup per 64 rows x all 192 columns +6 %, with split-K +3..+11 %,
        // with non-temporal activation loads +8 %: profiles/HISTORY.md, round 3)
        const bool no_pws = !asm_ring_ok || (diag & ISS_DIAG_NO_PWS) != 0;   // diagnostic: the round-2 pointwise kernel everywhere (or tools/check_ring_regs.py rejected this compiler's cnn_pw.o)
        const bool no_pws2 = (diag & ISS_DIAG_NO_PWS2) != 0;                // diagnostic: 64-column tiles everywhere
        const bool pws_ok = !no_pws && a.Kpad <= 2048 && !f16_dense_pw;      // (fp16 mode: a dense layer that would otherwise run in exact f32)
        // strided 1x1 (the shortcut projections): the 128-column kernel on a strided pixel list
        const bool pw_strided = pws_ok && !no_pws2 && a.mode == 0 && inst.tr && taps == 1 && (a.sh > 1 || a.sw > 1) && a.pt_ == 0 &&
                                a.pl_ == 0 && a.Kpad == a.Cin && pws2_strided_supported(a, R[ISS_C_HO], R[ISS_C_WO]);
        inst.simple_pw = a.act <= 1 && !a.ps; inst.has_res = a.res != nullptr;
        if (pw_strided) { inst.kernel = ConvKernel::Pws2Strided; ch.tag = ISS_PROF_PW; }
        else if (pointwise && pws_ok && !no_pws2 && pws2_supported(a)) inst.kernel = ConvKernel::Pws2;
        else if (pointwise && pws_ok && pws_supported(a)) inst.kernel = ConvKernel::Pws;
        else if (pointwise) { inst.kernel = ConvKernel::Pw; inst.f16 = f16mode; }
        else { inst.kernel = ConvKernel::X3; inst.tr = inst.tr && a.mode != 2; }
    } else {
        inst.kernel = ConvKernel::Igemm;
    }
    // The output layout, once per family.  CHL through the shared pooled epilogue (conv_common.h epilogue_impl / chl_store): every kernel
    // family that ends in it -- the weight-stationary forms, conv_x3_fp_kernel, the generic gather kernel -- can hand its pooled relu
    // output to a conv_x3_wq3h_kernel the way conv_x3_wq_kernel does; the one-wave-per-SIMD kernels have epilogues of their own
    if (inst.kernel == ConvKernel::Wq) {                   // (its own CHL epilogue; the halves follow the launch's operand type)
        if (a.Cout % BN == 0 && want_hl_out(env, r, a.M / 4)) { ch.out = OutLayout::Chl; ch.out_np = chl_npad(a.M / 4); ch.out_f16 = inst.f16; }
        inst.out_hl = ch.out != OutLayout::F32;
    } else if (inst.kernel == ConvKernel::Wq3h) {          // (kind 0 hands on CHL, kind 1 the dense layer's tensor; on an f32 input both write f32)
        if (inst.kind == 0 && want_hl_out(env, r, a.M)) { ch.out = OutLayout::Chl; ch.out_np = chl_npad(a.M); }
        if (inst.kind == 1 && want_dhl_out(env, r, a.Hq, a.Wq)) { ch.out = OutLayout::ChlDense; ch.out_np = dhl_npad(bc); }
        inst.out_hl = ch.out != OutLayout::F32;
        ch.out_f16 = inst.out_hl && inst.f16;
    } else if (inst.kernel != ConvKernel::Wq3 && x3 && !patch && epi_is_pool_relu(a) && a.Cout % 16 == 0 && want_hl_out(env, r, a.M / a.pp)) {
        ch.out = OutLayout::Chl; ch.out_np = chl_npad(a.M / a.pp); ch.out_f16 = f16mode; ch.generic_out = true;
    }
    return ch;
}

// The launch for row r with the deferred first layer `pend` (-1: none) in front.  No HIP call, no launch, no allocation; writes
// nothing but the footprint cache.
inline ConvChoice select_conv(const ConvEnv& env, int r, int pend) {
    const bool pair = asm_ring_ok && pend < 0 && env.x3mode() && !(env.diag & (ISS_DIAG_NO_PW | ISS_DIAG_NO_PWS | ISS_DIAG_NO_PWS2));
    // identity-residual expansion followed by the next block's reduction: one chained launch (conv_pwc.h)
    if (pair && !(env.diag & ISS_DIAG_NO_CHAIN) && chain_pair(env, r)) {
        const ConvChoice ch = select_row(env, r, -1, -1, r + 1);
        if (ch.inst.kernel != ConvKernel::Declined) return ch;
    }
    // projection shortcut followed by its expansion (ISS_C_DUALW on the next row): one two-source launch when the split-bf16
    // streaming kernels are in use (the diagnostic switches that move 1x1 layers elsewhere keep their meaning)
    if (pair && !(env.diag & ISS_DIAG_NO_DUAL) && r + 1 < env.n.nrows && env.row(r + 1)[ISS_C_DUALW] > 0) {
        const ConvChoice ch = select_row(env, r + 1, -1, r, -1);
        if (ch.inst.kernel != ConvKernel::Declined) return ch;
    }
    return select_row(env, r, pend, -1, -1);
}

// The instantiation the profiler reports (bench.py's roofline.dominant and the GPU tests read these): spelled from the ConvInst the
// launcher is keyed on.  The forms of conv_x3_ws_kernel print <KH,KW,PADDED,TR,FUSED,NH,EPI> and a word for the arguments behind them.
inline std::string inst_name(const ConvInst& c) {
    auto B = [](bool b) { return b ? "true" : "false"; };
    char s[160];
    auto ws = [&](const char* form) {
        snprintf(s, sizeof s, "conv_x3_ws_kernel<%d,%d,%s,%s,%s,%d,%d%s>", c.kh, c.kw, B(c.padded), B(c.tr), B(c.fused), c.nh, c.epi, form);
    };
    switch (c.kernel) {
    case ConvKernel::Dhl: snprintf(s, sizeof s, "conv_dhl_kernel<%s,%d>", B(c.f16), ISS_DHL_NW); break;                           // <F16,NW>
    case ConvKernel::Pwc: snprintf(s, sizeof s, "conv_x3_pwc_kernel<%d,%d>", c.c1, c.c3); break;
    case ConvKernel::Pws2Dual: snprintf(s, sizeof s, "conv_x3_pws2_kernel<%s,false,dual>", B(c.simple_pw)); break;
    case ConvKernel::Direct1: snprintf(s, sizeof s, "conv1_direct3x3_kernel<%s>", B(c.window)); break;
    case ConvKernel::Wq3: snprintf(s, sizeof s, "conv_x3_wq3_kernel<%d>", c.kind); break;
    case ConvKernel::Wq3h: snprintf(s, sizeof s, "conv_x3_wq3h_kernel<%d,%s,%s>", c.kind, B(c.out_hl), B(c.f16)); break;           // <KIND,OUT_HL,F16>
    case ConvKernel::WsNh2: case ConvKernel::WsPlain: case ConvKernel::Ws: ws(""); break;
    case ConvKernel::WsNh2F32: case ConvKernel::WsF32Fused: ws(",f32"); break;
    case ConvKernel::WsPlainU: ws(",plain"); break;
    case ConvKernel::WsRing: ws(",ring"); break;
    case ConvKernel::WsFs: ws(",fs"); break;
    case ConvKernel::WsNcb1: ws(",ncb1"); break;
    case ConvKernel::Wq: snprintf(s, sizeof s, "conv_x3_wq_kernel<%d,%d,%s,%s>", c.kh, c.kw, B(c.out_hl), B(c.f16)); break;        // <KH,KW,OUT_HL,F16>
    case ConvKernel::Fp: snprintf(s, sizeof s, "conv_x3_fp_kernel<%d,%d,%s,%s,%s,%d>", c.kh, c.kw, B(c.padded), B(c.tr), B(c.fused), c.nh); break;
    case ConvKernel::Patch1: snprintf(s, sizeof s, "conv1_patch_x3_kernel<%s,%s>", B(c.tr), B(c.f16)); break;                       // <TR,F16>
    case ConvKernel::Gather: case ConvKernel::X3: snprintf(s, sizeof s, "conv_x3_kernel<%d,%s,2>", c.mode, B(c.tr)); break;
    case ConvKernel::Pws2Strided: snprintf(s, sizeof s, "conv_x3_pws2_kernel<%s,true>", B(c.simple_pw)); break;
    case ConvKernel::Pws2: snprintf(s, sizeof s, "conv_x3_pws2_kernel<%s,false>", B(c.simple_pw)); break;
    case ConvKernel::Pws: snprintf(s, sizeof s, "conv_x3_pws_kernel<%s,%s>", B(c.has_res), B(c.simple_pw)); break;
    case ConvKernel::Pw: snprintf(s, sizeof s, "conv_x3_pw_kernel<%s>", B(c.f16)); break;                                          // <F16>
    case ConvKernel::Igemm: snprintf(s, sizeof s, "conv_igemm_kernel<%d>", c.mode); break;
    case ConvKernel::Declined: s[0] = 0; break;
    }
    return s;
}

}  // namespace issk
