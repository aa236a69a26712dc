// Small-CNN / ResNet engine for gfx950: executes a flat op program (include/iss.h) on
// batches of 20 ms slots (or x-vector windows).
//
// Replaces, for the reference: segmenter.py:76-88 `_get_patches` (never materialised here:
// the 68 x nmel window is gathered straight from the resident (T,24) log-mel inside the
// first conv's operand loader, z-normalised on the fly), segmenter.py:156-163 (gather +
// `keras predict`) and vbx_segmenter.py:262-266 (onnxruntime ResNet-101, resnet.py:78-135).
//
// Kernels
//   patch_stats_kernel   per-slot mean / population-std / finite flag     (segmenter.py:82,86)
//   conv_x3_kernel       conv2d + dense as implicit GEMM on v_mfma_f32_32x32x16_bf16 with both
//                        operands split into bf16 hi + lo and three MFMAs per k-step
//                        (hi*hi + hi*lo + lo*hi, f32 accumulate): 2^-16 relative operand error,
//                        i.e. float32-class results at 16/3 x the f32-MFMA rate (gfx950 has no
//                        xf32/TF32).  Default.
//   conv_x3_pw_kernel    1x1 stride-1 convolutions / dense layers: persistent GEMM, prefetch two k-tiles ahead
//   conv_igemm_kernel    the same GEMM on v_mfma_f32_32x32x2_f32 (exact f32, 157 TFLOP/s peak);
//                        iss_set_precision(ctx, ISS_PREC_F32)
//   both: fused bias, residual add, activation, post-activation scale/shift (BatchNorm),
//         optional fused non-overlapping max/avg pooling of 2 or 4 outputs, NHWC in/out
//   pool_kernel          max / average pooling, NHWC (pools that cannot be fused)
//   softmax_kernel       softmax over channels
//   statpool_kernel      mean || std over time                           (resnet.py:123-127)
#include "conv_select.h"      // kernel selection (and, through it, the kernel headers)

using namespace issk;

namespace {

// ------------------------------------------------------------------------------------------
// Implicit-GEMM convolution, exact f32.  C[m][n] = sum_k A[m][k] * Wt[n][k],
//   m = GEMM row (map_row), n = cout, k = (ky, kx, cin)   (NHWC, weights [Cout][Kpad]).
// 256 threads = 4 wavefronts; wave w owns rows [32w, 32w+32) x 64 cols = two 32x32 MFMA tiles.
// MODE: 0 = NHWC with Cin % 4 == 0 (float4 gathers), 1 = NHWC scalar gathers, 2 = z-normed patch.
template <int MODE>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvArgs p) {
    __shared__ __attribute__((aligned(16))) float sA[2][BM * LDK];
    __shared__ __attribute__((aligned(16))) float sB[2][BN * LDK];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned mt, nt;
    gemm_tile_of_block(blockIdx.x, p.nblk, p.nblk_n, mt, nt);
    const long long m0 = (long long)mt * BM;
    const int n0 = (int)nt * BN;

    // this thread fills (row lr, k4) and (row lr+64, k4) of sA
    const int k4 = tid & 3;
    const int lr = tid >> 2;
    RowSrc rs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) rs[j] = row_source<MODE>(p, m0 + lr + 64 * j);
    const int bn = n0 + lr;                       // weight row this thread stages
    const bool bok = bn < p.Cout;
    const float* wrow = p.w + (size_t)(bok ? bn : 0) * p.Kpad + k4 * 4;

    float4 ra[2], rb;
    auto gather = [&](int kt) {
        const int kbase = kt * BK + k4 * 4;
        if (MODE == 0) {
            const int2 e = reinterpret_cast<const int2*>(p.ktab)[kbase];
            const int ky = e.y >> 16, kx = e.y & 0xffff;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int iy = rs[j].iy0 + ky, ix = rs[j].ix0 + kx;
                ra[j] = ld4_or_zero(p.in, rs[j].base + e.x,
                                    rs[j].ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                ra[j] = make_float4(gather_scalar<MODE>(p, rs[j], kbase), gather_scalar<MODE>(p, rs[j], kbase + 1),
                                    gather_scalar<MODE>(p, rs[j], kbase + 2), gather_scalar<MODE>(p, rs[j], kbase + 3));
        }
        rb = *reinterpret_cast<const float4*>(wrow + (size_t)kt * BK);        // rows >= Cout read row 0: never stored
    };
    auto stage = [&](int buf) {
        *reinterpret_cast<float4*>(&sA[buf][lr * LDK + k4 * 4]) = ra[0];
        *reinterpret_cast<float4*>(&sA[buf][(lr + 64) * LDK + k4 * 4]) = ra[1];
        *reinterpret_cast<float4*>(&sB[buf][lr * LDK + k4 * 4]) = rb;
    };

    floatx16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }

    const int nk = p.Kpad / BK;
    gather(0);
    stage(0);
    __syncthreads();

    const int li = lane & 31, lh = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gather(kt + 1);
        const float* a_s = &sA[cur][(wv * 32 + li) * LDK + lh * 4];
        const float* b_s = &sB[cur][li * LDK + lh * 4];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(a_s + g * 8);
            const float4 b0 = *reinterpret_cast<const float4*>(b_s + g * 8);
            const float4 b1 = *reinterpret_cast<const float4*>(b_s + 32 * LDK + g * 8);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
        }
        if (kt + 1 < nk) stage(cur ^ 1);
        __syncthreads();
    }
    epilogue_tile(p, acc0, m0 + wv * 32, n0 + li, lh);
    epilogue_tile(p, acc1, m0 + wv * 32, n0 + 32 + li, lh);
}

// ------------------------------------------------------------------------------------------
// Implicit-GEMM convolution on bf16 MFMA with split operands ("bf16x3").
//   x = hi + lo,  hi = bf16(x),  lo = bf16(x - hi)   (|x - hi - lo| <= 2^-17 |x|)
//   a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi        (dropped a_lo*b_lo <= 2^-16 |a b|)
// Weights are split once on the host side of iss_cnn_load; activations stay f32 in HBM and
// are split while they are staged into LDS (v_cvt_pk_bf16_f32).  Same 128 x 64 tile / wave
// layout / epilogue as the f32 kernel, k-tile 32 = two v_mfma_f32_32x32x16_bf16 steps, i.e.
// 12 MFMAs per wave per k-tile.  LDS: 2 stages x (A hi+lo 20 KB + B hi+lo 10 KB) = 60 KB
// -> two workgroups per CU, one staging while the other is on the matrix pipe.
// MODE: 0 = NHWC with Cin % 32 == 0 (a k-tile is 32 consecutive channels of ONE tap: float4
//           gathers, no table), 1 = NHWC scalar gathers, 2 = z-normed patch.

// NTN = 32-column accumulator tiles per wavefront: the workgroup covers 128 rows x 32*NTN output channels.  NTN = 2 is
// the 128 x 64 tile of the other kernels; NTN = 4 / 8 (Cout >= 128 / 256) stage and split the A tile once for 128 / 256
// channels -- the ResNet 1x1 expansions (K = 32..256, N up to 1024) were bound by re-reading A once per 64 channels.
template <int MODE, bool TR, int NTN>
__global__ __launch_bounds__(256, NTN <= 4 ? 2 : 1) void conv_x3_kernel(const ConvArgs p) {
    constexpr int BNX = 32 * NTN;                    // output channels per workgroup
    constexpr int NBR = BNX / 64;                    // weight rows per thread and k-tile (rows br + 64 j)
    __shared__ __attribute__((aligned(16))) uint16_t sAh[2][BM * XLD];
    __shared__ __attribute__((aligned(16))) uint16_t sAl[2][BM * XLD];
    __shared__ __attribute__((aligned(16))) uint16_t sBh[2][BNX * XLD];
    __shared__ __attribute__((aligned(16))) uint16_t sBl[2][BNX * XLD];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned mt, nt;
    gemm_tile_of_block(blockIdx.x, p.nblk, p.nblk_n, mt, nt);
    const long long m0 = (long long)mt * BM;
    const int n0 = (int)nt * BNX;

    // A staging: thread fills k columns [4*k8, 4*k8+4) of rows lr, lr+32, lr+64, lr+96
    const int k8 = tid & 7;
    const int lr = tid >> 3;
    RowSrc rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rs[j] = row_source<MODE>(p, m0 + lr + 32 * j);
    // B staging: thread fills 8 bf16 (16 B) of weight rows br + 64 j, for hi and lo.  Rows >= Cout read row 0:
    // their output columns are never stored.
    const int br = tid >> 2, bseg = tid & 3;
    size_t boff[NBR];
#pragma unroll
    for (int j = 0; j < NBR; ++j) boff[j] = (size_t)(n0 + br + 64 * j < p.Cout ? n0 + br + 64 * j : 0) * p.Kpad + bseg * 8;

    float4 ra[4];
    uint4 rbh[NBR], rbl[NBR];
    int tap_ky = 0, tap_kx = 0, tap_c = 0;          // MODE 0 / 3: tap walked by the NEXT gather
    // MODE 3 (shared first layer, see row_source): the first layer's weight sums / bias of the 4 channels of this k-tile and which of
    // the 4 rows hold data (a zero-padded tap is a zero of the ACTIVATION, not of the raw row)
    float4 f_s4 = make_float4(0.f, 0.f, 0.f, 0.f), f_b4 = f_s4;
    float4 f_sx[4];                                  // MODE 4: S[x][c] of each row's tap column (the weight sum depends on the column)
    unsigned f_valid = 0;
    const float f_lob = p.f_act == 1 ? 0.f : -INFINITY;
    auto gather = [&](int kt) {
        if (MODE == 4) {
            // zero-padded ('same') first layer, see conv_ws.h FS: row iy of window b is shared row (win_row[b] - rmin) + iy, except the first
            // f_padt / last f_padb rows, which are the window's own edge rows f_erow0 + b * ne + e; the shift uses S[ix][c]
            const int cofs = tap_c + k8 * 4;
            f_b4 = *reinterpret_cast<const float4*>(p.f_bias + cofs);
            f_valid = 0;
            const int ne = p.f_padt + p.f_padb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = rs[j].iy0 + tap_ky, ix = rs[j].ix0 + tap_kx;
                const bool okj = rs[j].ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const int yb = iy - (p.H - p.f_padb);
                const int e = iy < p.f_padt ? iy : (yb >= 0 ? p.f_padt + yb : -1);
                const long long row = e >= 0 ? (long long)p.f_erow0 + (long long)rs[j].b * ne + e : rs[j].base + iy;
                ra[j] = ld4_or_zero(p.in, (row * p.W + ix) * p.Cin + cofs, okj);
                f_sx[j] = *reinterpret_cast<const float4*>(p.f_wsum + (okj ? ix * p.Cin + cofs : cofs));
                f_valid |= okj ? 1u << j : 0u;
            }
            tap_c += XBK;
            if (tap_c >= p.Cin) { tap_c = 0; if (++tap_kx == p.kw) { tap_kx = 0; ++tap_ky; } }
        } else
        if (MODE == 0 || MODE == 3) {
            const int off = (tap_ky * p.W + tap_kx) * p.Cin + tap_c + k8 * 4;
            if (MODE == 3) {
                f_s4 = *reinterpret_cast<const float4*>(p.f_wsum + tap_c + k8 * 4);
                f_b4 = *reinterpret_cast<const float4*>(p.f_bias + tap_c + k8 * 4);
                f_valid = 0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = rs[j].iy0 + tap_ky, ix = rs[j].ix0 + tap_kx;
                const bool okj = rs[j].ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                ra[j] = ld4_or_zero(p.in, rs[j].base + off, okj);
                if (MODE == 3) f_valid |= okj ? 1u << j : 0u;
            }
            tap_c += XBK;
            if (tap_c >= p.Cin) { tap_c = 0; if (++tap_kx == p.kw) { tap_kx = 0; ++tap_ky; } }
        } else {
            const int kbase = kt * XBK + k8 * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                ra[j] = make_float4(gather_scalar<MODE>(p, rs[j], kbase), gather_scalar<MODE>(p, rs[j], kbase + 1),
                                    gather_scalar<MODE>(p, rs[j], kbase + 2), gather_scalar<MODE>(p, rs[j], kbase + 3));
        }
#pragma unroll
        for (int j = 0; j < NBR; ++j) {
            rbh[j] = *reinterpret_cast<const uint4*>(p.wh + boff[j] + (size_t)kt * XBK);
            rbl[j] = *reinterpret_cast<const uint4*>(p.wl + boff[j] + (size_t)kt * XBK);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16x4 h, l;
            if (MODE == 3 || MODE == 4) {                // the window's affine map + activation of the first layer, then the split
                const float sc = rs[j].sd, mr = rs[j].mean;
                if (MODE == 4) f_s4 = f_sx[j];
                float4 v = ra[j];
                v.x = fmaxf(fmaf(v.x, sc, fmaf(f_s4.x, mr, f_b4.x)), f_lob); v.y = fmaxf(fmaf(v.y, sc, fmaf(f_s4.y, mr, f_b4.y)), f_lob);
                v.z = fmaxf(fmaf(v.z, sc, fmaf(f_s4.z, mr, f_b4.z)), f_lob); v.w = fmaxf(fmaf(v.w, sc, fmaf(f_s4.w, mr, f_b4.w)), f_lob);
                ra[j] = (f_valid >> j) & 1u ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            split4(ra[j], h, l);
            *reinterpret_cast<bf16x4*>(&sAh[buf][(lr + 32 * j) * XLD + k8 * 4]) = h;
            *reinterpret_cast<bf16x4*>(&sAl[buf][(lr + 32 * j) * XLD + k8 * 4]) = l;
        }
#pragma unroll
        for (int j = 0; j < NBR; ++j) {
            *reinterpret_cast<uint4*>(&sBh[buf][(br + 64 * j) * XLD + bseg * 8]) = rbh[j];
            *reinterpret_cast<uint4*>(&sBl[buf][(br + 64 * j) * XLD + bseg * 8]) = rbl[j];
        }
    };

    floatx16 acc[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int nk = p.Kpad / XBK;
    gather(0);
    stage(0);
    __syncthreads();

    const int li = lane & 31, lh = lane >> 5;
    const int aoff = (wv * 32 + li) * XLD + lh * 8;
    const int boff_s = li * XLD + lh * 8;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gather(kt + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&sAh[cur][aoff + ks * 16]);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(&sAl[cur][aoff + ks * 16]);
#pragma unroll
            for (int t = 0; t < NTN; ++t) {
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&sBh[cur][boff_s + t * 32 * XLD + ks * 16]);
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&sBl[cur][boff_s + t * 32 * XLD + ks * 16]);
                if (TR) {                                // C^T: rows = channels, columns = pixels (see epilogue_tr)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, al, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, ah, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, ah, acc[t], 0, 0, 0);
                } else {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
                }
            }
        }
        if (kt + 1 < nk) stage(cur ^ 1);
        __syncthreads();
    }
    if (TR) {
#pragma unroll
        for (int t = 0; t < NTN; t += 2) epilogue_tr(p, acc[t], acc[t + 1], m0 + wv * 32 + li, n0 + 32 * t, lh);
    } else {
#pragma unroll
        for (int t = 0; t < NTN; ++t) epilogue_tile(p, acc[t], m0 + wv * 32, n0 + 32 * t + li, lh);
    }
}

// Pointwise (1x1, stride 1, unpadded) convolutions = plain GEMMs on the NHWC pixel list: half of ResNet-101's flops in
// layers with K = 64 .. 512, i.e. 2 - 16 k-tiles per 128 x 64 output tile.  With one tile per workgroup (conv_x3_kernel)
// the first global load of every workgroup (~2 us) and its epilogue are exposed: rocprofv3 --pmc showed those launches at
// 2 TB/s of HBM traffic and 10 % of the matrix peak -- latency-bound, not bandwidth-bound.  Here 2 x 256 persistent
// workgroups walk the XCD-aware tile order and the register prefetch runs ACROSS tiles (the next tile's first k-tile is
// fetched during the current tile's last one, its stores drain behind the next tile's MFMAs); no row decomposition
// (row m of the GEMM is pixel m).
// Round 6: THREE workgroups per CU.  The segmenter nets' first dense layer (K = 4992 / 8320, 192 columns) has 660 tiles per launch;
// on 512 resident workgroups that was two rounds for 1.29 rounds of work, and a timing-only build whose activation loads all hit L2
// ran no faster (profiles/HISTORY.md, round 6: the layer is bound by its per-k-tile barrier structure, not by memory).  768 resident
// workgroups hold every tile at once.  LDS: the 80-byte padded rows (61 KB per workgroup) became unpadded 64-byte rows with the
// 16-byte chunk swizzle of conv_fp.h (chunk c of row r at c ^ ((r >> 2) & 3): the 16 lanes of a ds_read_b128 group hit 16
// different bank groups) = 48 KB.
constexpr int PWLD = XBK;                            // bf16 / fp16 elements per LDS row (64 bytes, swizzled)
template <bool F16>                                // fp16 instead of bf16 operand halves (ISS_PREC_F16X3, conv_common.h)
__global__ __launch_bounds__(256, 3) void conv_x3_pw_kernel(const ConvArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t sAh[2][BM * PWLD];
    __shared__ __attribute__((aligned(16))) uint16_t sAl[2][BM * PWLD];
    __shared__ __attribute__((aligned(16))) uint16_t sBh[2][BN * PWLD];
    __shared__ __attribute__((aligned(16))) uint16_t sBl[2][BN * PWLD];
    auto lds_off = [](int row, int chunk) { return row * PWLD + ((chunk ^ ((row >> 2) & 3)) << 3); };     // in 16-bit elements

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned ntiles = p.nblk * p.nblk_n;
    unsigned t = blockIdx.x;
    if (t >= ntiles) return;
    const int k8 = tid & 7, lr = tid >> 3;           // A staging: k columns [4 k8, 4 k8 + 4) of rows lr + 32 j
    const int br = tid >> 2, bseg = tid & 3;         // B staging: 8 bf16 of weight row br, hi and lo
    const int awr = lds_off(lr, k8 >> 1) + (k8 & 1) * 4, bwr = lds_off(br, bseg);
    // A tile of the GEMM: uniform 64-bit base of its first row + 32-bit per-lane offsets (rows >= M re-read row M - 1:
    // their accumulator rows are never stored).  No masks and no branches around the loads: a select or a branch right
    // behind a load makes hipcc wait for it on the spot, in front of the MFMAs it is meant to overlap.
    struct Tile { long long m0; int n0; const float* abase; unsigned ao[4]; unsigned wo; };
    auto coords = [&](unsigned tt) {
        Tile T;
        unsigned mt, nt;
        gemm_tile_of_block(tt, p.nblk, p.nblk_n, mt, nt);
        T.m0 = (long long)mt * BM;
        T.n0 = (int)nt * BN;
        T.abase = p.in + T.m0 * p.Cin;
        const int left = (int)(p.M - T.m0 < BM ? p.M - T.m0 : BM);            // rows of this tile that exist
#pragma unroll
        for (int j = 0; j < 4; ++j) T.ao[j] = (unsigned)((lr + 32 * j < left ? lr + 32 * j : left - 1) * p.Cin + k8 * 4);
        T.wo = (unsigned)((T.n0 + br < p.Cout ? T.n0 + br : 0) * p.Kpad + bseg * 8);
        return T;
    };
    // Two register sets: a k-tile's loads are issued two iterations before they are converted into LDS.  One iteration is
    // only 12 MFMAs (~0.2 us) against ~2 us of memory latency, so what bounds these layers is the number of bytes in
    // flight; with a one-iteration distance the launches ran at 2 TB/s and 10 % of the matrix peak.
    struct Regs { float4 a[4]; uint4 bh, bl; };
    auto gather = [&](Regs& r, const Tile& T, int kt) {
#ifdef ISS_EXPERIMENTS                                           // timing-only (make EXPERIMENTS=1, ISS_DBG=4): every A load from one 64 KB region
        if (p.dbg & 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r.a[j] = *reinterpret_cast<const float4*>(p.in + ((T.ao[j] + (unsigned)(kt * XBK)) & 0x3FFCu));
        } else
#endif
#pragma unroll
        for (int j = 0; j < 4; ++j) r.a[j] = *reinterpret_cast<const float4*>(T.abase + (T.ao[j] + (unsigned)(kt * XBK)));
        r.bh = *reinterpret_cast<const uint4*>(p.wh + (T.wo + (unsigned)(kt * XBK)));
        r.bl = *reinterpret_cast<const uint4*>(p.wl + (T.wo + (unsigned)(kt * XBK)));
    };
    auto stage = [&](Regs& r, int buf) {
        // opaque pass-through: the conversion can only start here, behind the MFMAs of the iteration
        asm volatile("" : "+v"(r.a[0].x), "+v"(r.a[0].y), "+v"(r.a[0].z), "+v"(r.a[0].w), "+v"(r.a[1].x), "+v"(r.a[1].y), "+v"(r.a[1].z),
                          "+v"(r.a[1].w), "+v"(r.a[2].x), "+v"(r.a[2].y), "+v"(r.a[2].z), "+v"(r.a[2].w), "+v"(r.a[3].x), "+v"(r.a[3].y),
                          "+v"(r.a[3].z), "+v"(r.a[3].w));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (F16) {
                uint2 h, l;
                split4_pk<true>(r.a[j], h.x, h.y, l.x, l.y);
                *reinterpret_cast<uint2*>(&sAh[buf][awr + 32 * j * PWLD]) = h;
                *reinterpret_cast<uint2*>(&sAl[buf][awr + 32 * j * PWLD]) = l;
            } else {
            bf16x4 h, l;
            split4(r.a[j], h, l);
            *reinterpret_cast<bf16x4*>(&sAh[buf][awr + 32 * j * PWLD]) = h;
            *reinterpret_cast<bf16x4*>(&sAl[buf][awr + 32 * j * PWLD]) = l;
            }
        }
        *reinterpret_cast<uint4*>(&sBh[buf][bwr]) = r.bh;
        *reinterpret_cast<uint4*>(&sBl[buf][bwr]) = r.bl;
    };

    floatx16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    const int nk = p.Kpad / XBK;
    const int li = lane & 31, lh = lane >> 5;
    // (rows lr + 32 j share (row >> 2) & 3, so one swizzled offset serves the four staging stores; the second k16 step of a row is
    // its first one's chunk ^ 2 = 16 elements further or nearer)
    const int aoff = lds_off(wv * 32 + li, lh);
    const int boff_s = lds_off(li, lh);

    // load cursor (tile, k-tile), two iterations ahead of the compute cursor; past the last tile it re-reads that tile
    unsigned tl = t;
    Tile TL = coords(t);
    int ktl = 0;
    auto advance_load = [&]() {
        if (++ktl == nk) {
            ktl = 0;
            tl = tl + gridDim.x < ntiles ? tl + gridDim.x : tl;
            TL = coords(tl);
        }
    };
    Tile TC = TL;                                    // compute cursor
    int ktc = 0;
    Regs r0, r1;
    gather(r0, TL, ktl); advance_load();
    gather(r1, TL, ktl); advance_load();
    stage(r0, 0);
    __syncthreads();
    int cur = 0;
    bool done = false;
    auto step = [&](Regs& rload, Regs& rstage) {     // one k-tile: loads for +2, MFMAs on `cur`, convert +1 into the other buffer
        gather(rload, TL, ktl);
        advance_load();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&sAh[cur][aoff ^ (ks * 16)]);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(&sAl[cur][aoff ^ (ks * 16)]);
            const bf16x8 b0h = *reinterpret_cast<const bf16x8*>(&sBh[cur][boff_s ^ (ks * 16)]);
            const bf16x8 b0l = *reinterpret_cast<const bf16x8*>(&sBl[cur][boff_s ^ (ks * 16)]);
            const bf16x8 b1h = *reinterpret_cast<const bf16x8*>(&sBh[cur][(boff_s ^ (ks * 16)) + 32 * PWLD]);
            const bf16x8 b1l = *reinterpret_cast<const bf16x8*>(&sBl[cur][(boff_s ^ (ks * 16)) + 32 * PWLD]);
            // C^T: rows = channels, columns = pixels (epilogue_tr); two independent accumulators alternate
            acc0 = mfma_x3<F16>(b0h, al, acc0);
            acc1 = mfma_x3<F16>(b1h, al, acc1);
            acc0 = mfma_x3<F16>(b0l, ah, acc0);
            acc1 = mfma_x3<F16>(b1l, ah, acc1);
            acc0 = mfma_x3<F16>(b0h, ah, acc0);
            acc1 = mfma_x3<F16>(b1h, ah, acc1);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        stage(rstage, cur ^ 1);
        __syncthreads();
        cur ^= 1;
        if (++ktc == nk) {                           // tile complete
            epilogue_tr<true>(p, acc0, acc1, TC.m0 + wv * 32 + li, TC.n0, lh);
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
            ktc = 0;
            t += gridDim.x;
            if (t >= ntiles) done = true; else TC = coords(t);
        }
    };
    while (true) {
        step(r0, r1);                                // r0 was staged last: free to load; r1 holds the next k-tile
        if (done) break;
        step(r1, r0);
        if (done) break;
    }
}

// ------------------------------------------------------------------------------------------
// First layer on the z-normalised 68 x h log-mel window (PATCH input, Cin = 1, kh*kw <= 32), bf16x3.
//
// conv1 is 1.8 % of the flops but its output is the largest tensor of the net (283-333 KB per slot),
// so the layer is bound by its stores; run through the generic kernel (table-driven scalar gathers into
// an LDS A tile, a barrier per k-tile) it took 18 % of the step at 3.8 % MFMA-busy.  Here:
//   * K fits ONE 32-wide k-tile, so each lane builds its own MFMA A fragments in registers -- 16 cached
//     loads from the (T,24) log-mel (a 128-row tile touches ~11 rows of one window), (x - mean) * (1/std),
//     bf16 hi/lo split -- no LDS A tile, no barrier at all;
//   * the workgroup's 64 x 32 weight block (hi + lo) is loaded once into 32 VGPRs and stays there while
//     the persistent workgroup walks its range of tiles: 12 MFMAs + the fused epilogue per tile.
// TR: operands swapped (C^T = W . A^T): a lane then holds 4 CONSECUTIVE channels of one pixel per register group and
// the epilogue stores float4 (8 x 16-byte stores per lane and tile instead of 32 x 4-byte ones); needs pp == 1.
// F16 (ISS_PREC_F16X3): fp16 halves of the normalised window and of the weights (p.wh / p.wl are then the fp16 split).  With bf16
// halves here the first layer's 2^-16 operand rounding carried the error of a call on scattered windows in that mode (gender
// stand-in, 333 rows: max |d log p| 1.08e-4 against float64, over the mode's 1e-4; overlapping lists take the exact-f32 shared
// first layer and never met it).
template <bool TR, bool F16>
__global__ __launch_bounds__(256, 2) void conv1_patch_x3_kernel(const ConvArgs p) {
    __shared__ int s_delta[XBK];                     // k -> ty * 24 + tx  (or -1 for the K padding)
    __shared__ int s_tap[XBK];                       // k -> (ty << 16) | tx
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int n0 = blockIdx.y * BN;
    const int M = (int)p.M;
    if (tid < XBK) {
        const int K = p.H_k * p.kw;
        const int ty = tid / p.kw, tx = tid - ty * p.kw;
        s_delta[tid] = tid < K ? ty * 24 + tx : -1;
        s_tap[tid] = (ty << 16) | tx;
    }
    // weight fragments of this workgroup's 64 columns: B[k][n] at lane (n = li, k = 8 lh + e), k16 step ks
    bf16x8 b0h[2], b0l[2], b1h[2], b1l[2];
    {
        const int r0 = n0 + li < p.Cout ? n0 + li : 0, r1 = n0 + 32 + li < p.Cout ? n0 + 32 + li : 0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            b0h[ks] = *reinterpret_cast<const bf16x8*>(p.wh + (size_t)r0 * p.Kpad + ks * 16 + lh * 8);
            b0l[ks] = *reinterpret_cast<const bf16x8*>(p.wl + (size_t)r0 * p.Kpad + ks * 16 + lh * 8);
            b1h[ks] = *reinterpret_cast<const bf16x8*>(p.wh + (size_t)r1 * p.Kpad + ks * 16 + lh * 8);
            b1l[ks] = *reinterpret_cast<const bf16x8*>(p.wl + (size_t)r1 * p.Kpad + ks * 16 + lh * 8);
        }
    }
    __syncthreads();
    int dl[16], tp[16];                              // this lane's 16 k values: k = ks * 16 + lh * 8 + e
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int k = (q >> 3) * 16 + lh * 8 + (q & 7);
        dl[q] = s_delta[k];
        tp[q] = s_tap[k];
    }
    const int per = ((int)p.nblk + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile_end = ((int)blockIdx.x + 1) * per < (int)p.nblk ? ((int)blockIdx.x + 1) * per : (int)p.nblk;
    for (int tile = (int)blockIdx.x * per; tile < tile_end; ++tile) {
        const int m = tile * BM + wv * 32 + li;
        int b, oy, ox;
        map_row32(p, m < M ? m : 0, b, oy, ox);
        const int iy0 = oy * p.sh - p.pt_, ix0 = ox * p.sw - p.pl_;
        const float* src = p.in + (size_t)p.win_row[b] * 24 + iy0 * 24 + ix0;
        const float mean = p.stats[2 * b];
        const float rsd = 1.0f / p.stats[2 * b + 1];
        const bool live = m < M && p.finite[b];
        float x[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int iy = iy0 + (tp[q] >> 16), ix = ix0 + (tp[q] & 0xffff);
            const bool ok = live && dl[q] >= 0 && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const float v = src[ok ? dl[q] : 0 - iy0 * 24 - ix0];       // row 0 of the window when masked: always mapped
            x[q] = ok ? (v - mean) * rsd : 0.f;
        }
        bf16x8 ah[2], al[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = x[ks * 8 + e];
                if constexpr (F16) {
                    const _Float16 h = (_Float16)v;
                    ah[ks][e] = __builtin_bit_cast(__bf16, h);
                    al[ks][e] = __builtin_bit_cast(__bf16, (_Float16)(v - (float)h));
                } else {
                    const __bf16 h = (__bf16)v;
                    ah[ks][e] = h;
                    al[ks][e] = (__bf16)(v - (float)h);
                }
            }
        }
        floatx16 acc0, acc1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
        if (!TR) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                acc0 = mfma_x3<F16>(al[ks], b0h[ks], acc0);
                acc1 = mfma_x3<F16>(al[ks], b1h[ks], acc1);
                acc0 = mfma_x3<F16>(ah[ks], b0l[ks], acc0);
                acc1 = mfma_x3<F16>(ah[ks], b1l[ks], acc1);
                acc0 = mfma_x3<F16>(ah[ks], b0h[ks], acc0);
                acc1 = mfma_x3<F16>(ah[ks], b1h[ks], acc1);
            }
            epilogue_tile(p, acc0, (long long)tile * BM + wv * 32, n0 + li, lh);
            epilogue_tile(p, acc1, (long long)tile * BM + wv * 32, n0 + 32 + li, lh);
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {             // rows = channels (weight fragment), columns = pixels
                acc0 = mfma_x3<F16>(b0h[ks], al[ks], acc0);
                acc1 = mfma_x3<F16>(b1h[ks], al[ks], acc1);
                acc0 = mfma_x3<F16>(b0l[ks], ah[ks], acc0);
                acc1 = mfma_x3<F16>(b1l[ks], ah[ks], acc1);
                acc0 = mfma_x3<F16>(b0h[ks], ah[ks], acc0);
                acc1 = mfma_x3<F16>(b1h[ks], ah[ks], acc1);
            }
            epilogue_tr(p, acc0, acc1, m, n0, lh);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Per-slot statistics of the 68 x h log-mel window: mean, population std, finite flag.
// Shared first layer (ConvArgs::f_*): the PATCH conv without its per-window normalisation, once per log-mel row:
//   R[t][x][c] = sum_{ky,kx} w[c][ky * kw + kx] * mspec[(row0 + t + ky) * 24 + x + kx]       (f32, FMA chain in k order)
// One thread per (t, x, 4 channels), grid-stride (the weights are transposed into LDS once per workgroup).  Non-finite results are stored as 0: they only ever reach windows whose finite
// flag is 0, and those are scaled by 0 (their normalised input is all zeros in the reference, segmenter.py:86-88).
template <int KH_, int KW_>                       // compile-time filter shape (0, 0: run-time kh, kw)
__global__ __launch_bounds__(256) void first_layer_raw_kernel(const float* __restrict__ mspec, int row0, long long total,
                                                              int Wout, int Cout, int kh_, int kw_,
                                                              const float* __restrict__ w, int Kpad, float* __restrict__ R) {
    extern __shared__ __attribute__((aligned(16))) float sW[];     // [K][Cout]: a lane's 4 channels of tap k are one ds_read_b128
    const int kh = KH_ ? KH_ : kh_, kw = KW_ ? KW_ : kw_;
    const int K = kh * kw;
    for (int e = threadIdx.x; e < K * Cout; e += 256) {
        const int co = e / K, k = e - co * K;
        sW[k * Cout + co] = w[(size_t)co * Kpad + k];
    }
    __syncthreads();
    const unsigned cg = (unsigned)Cout >> 2, utotal = (unsigned)total;       // total < 2^30 (host: 32-bit offsets into R)
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < utotal; idx += gridDim.x * 256u) {
        const unsigned pix = idx / cg;
        const int c4 = (int)(idx - pix * cg) * 4;
        const unsigned t = pix / (unsigned)Wout;
        const int x = (int)(pix - t * (unsigned)Wout);
        const float* src = mspec + (size_t)(row0 + (int)t) * 24 + x;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        auto tap = [&](int ky, int kx) {
            const float v = src[ky * 24 + kx];
            const float4 wk = *reinterpret_cast<const float4*>(&sW[(ky * kw + kx) * Cout + c4]);
            a0 = fmaf(v, wk.x, a0);
            a1 = fmaf(v, wk.y, a1);
            a2 = fmaf(v, wk.z, a2);
            a3 = fmaf(v, wk.w, a3);
        };
        if constexpr (KH_ > 0) {
#pragma unroll
            for (int ky = 0; ky < KH_; ++ky)
#pragma unroll
                for (int kx = 0; kx < KW_; ++kx) tap(ky, kx);
        } else {
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) tap(ky, kx);
        }
        float4 o;
        o.x = isfinite(a0) ? a0 : 0.f; o.y = isfinite(a1) ? a1 : 0.f; o.z = isfinite(a2) ? a2 : 0.f; o.w = isfinite(a3) ? a3 : 0.f;
        *reinterpret_cast<float4*>(R + (size_t)idx * 4) = o;
    }
}

// A first layer with a fused non-overlapping MAX pool (conv - relu - pool - conv nets), shared between windows: max-pool commutes with the
// per-window map relu(R / std + t) (std > 0), so the pooled per-window activation is the map applied to maxpool(R).  A window's pool
// windows start at its own first row: window rows wr with (wr - rmin) % ph == q pool the pairs of PHASE q, so the pooled rows are kept
// in ph planes, plane q holding max over rows ph * r + q + {0..ph-1}, columns pw * x + {0..pw-1} of R; window b then reads plane q_b from
// row (wr_b - rmin - q_b) / ph on -- winrow_pool_kernel writes that as one row index into the stacked planes, so the consumer
// (conv_x3_kernel<3>) needs nothing but the transformed window list.  One thread per (plane, r, x, 4 channels).
__global__ __launch_bounds__(256) void pool_rows_kernel(const float* __restrict__ R, float* __restrict__ P, long long total, int rrows, int W,
                                                        int C, int ph, int pw, int plane_rows) {
    const unsigned cg = (unsigned)C >> 2, Wp = (unsigned)(W / pw);
    for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const unsigned c4 = (unsigned)(idx % cg) * 4u;
        long long t = idx / cg;
        const unsigned x = (unsigned)(t % Wp); t /= Wp;
        const int r = (int)(t % plane_rows), q = (int)(t / plane_rows);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dy = 0; dy < ph; ++dy) {
            int row = ph * r + q + dy;
            row = row < rrows ? row : rrows - 1;                     // (beyond the last row: never read by a window)
            for (int dx = 0; dx < pw; ++dx) {
                const float4 v = *reinterpret_cast<const float4*>(R + ((size_t)row * W + (x * pw + dx)) * C + c4);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        *reinterpret_cast<float4*>(P + (size_t)idx * 4) = m;
    }
}
__global__ void winrow_pool_kernel(const int32_t* __restrict__ win_row, int32_t* __restrict__ out, int n, int rmin, int ph, int plane_rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int d = win_row[b] - rmin, q = d % ph;
    out[b] = (d - q) / ph + q * plane_rows;
}

// Zero-padded ('same') first layer, the rows every window shares (conv_x3_ws_kernel<..., FS>): output row t of the recording,
// column x, from ALL kh filter rows (input rows t - pt .. t - pt + kh - 1; a window reads row wr + y only for pt <= y < H - pb,
// where these are its own rows) and the filter columns that see data at x (0 <= x - pl + kx < W: the padding of the normalised
// window is worth the window mean in raw units, which the consumer accounts for through S[x][c]).  Rows outside the recording
// are clamped (never read).  One thread per (t, x, 4 channels), run-time filter shape.
__global__ __launch_bounds__(256) void first_layer_same_kernel(const float* __restrict__ mspec, int nrows_mspec, int row0, long long total,
                                                               int W, int Cout, int kh, int kw, int pt, int pl,
                                                               const float* __restrict__ w, int Kpad, float* __restrict__ R) {
    extern __shared__ __attribute__((aligned(16))) float sW[];     // [K][Cout]
    const int K = kh * kw;
    for (int e = threadIdx.x; e < K * Cout; e += 256) {
        const int co = e / K, k = e - co * K;
        sW[k * Cout + co] = w[(size_t)co * Kpad + k];
    }
    __syncthreads();
    const unsigned cg = (unsigned)Cout >> 2, utotal = (unsigned)total;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < utotal; idx += gridDim.x * 256u) {
        const unsigned pix = idx / cg;
        const int c4 = (int)(idx - pix * cg) * 4;
        const unsigned t = pix / (unsigned)W;
        const int x = (int)(pix - t * (unsigned)W);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int ky = 0; ky < kh; ++ky) {
            int r = row0 + (int)t - pt + ky;
            r = r < 0 ? 0 : (r > nrows_mspec - 1 ? nrows_mspec - 1 : r);
            const float* src = mspec + (size_t)r * 24;
            for (int kx = 0; kx < kw; ++kx) {
                const int ix = x - pl + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const float v = src[ix];
                const float4 wk = *reinterpret_cast<const float4*>(&sW[(ky * kw + kx) * Cout + c4]);
                a0 = fmaf(v, wk.x, a0); a1 = fmaf(v, wk.y, a1); a2 = fmaf(v, wk.z, a2); a3 = fmaf(v, wk.w, a3);
            }
        }
        float4 o;
        o.x = isfinite(a0) ? a0 : 0.f; o.y = isfinite(a1) ? a1 : 0.f; o.z = isfinite(a2) ? a2 : 0.f; o.w = isfinite(a3) ? a3 : 0.f;
        *reinterpret_cast<float4*>(R + (size_t)idx * 4) = o;
    }
}

// ... and the rows that are NOT shared: the first pt / last pb output rows of each window see fewer filter rows.  Window b's edge
// row e (e < pt: y = e; else y = H - pb + e - pt) is written per window, already shifted so that the consumer's ordinary map
// rs * X + (bias - mean * rs * S[x][c]) gives the reference's value:  X = partial sum + mean_b * (S[x][c] - S_partial[x][c])
// (partial = the filter rows / columns that lie inside the window).  One thread per (b, e, x, 4 channels).
__global__ __launch_bounds__(256) void first_layer_edge_kernel(const float* __restrict__ mspec, const int32_t* __restrict__ win_row,
                                                               const float* __restrict__ stats, long long total, int H, int W, int Cout,
                                                               int kh, int kw, int pt, int pb, int pl, const float* __restrict__ w, int Kpad,
                                                               const float* __restrict__ S, float* __restrict__ E) {
    extern __shared__ __attribute__((aligned(16))) float sW[];     // [K][Cout]
    const int K = kh * kw;
    for (int e = threadIdx.x; e < K * Cout; e += 256) {
        const int co = e / K, k = e - co * K;
        sW[k * Cout + co] = w[(size_t)co * Kpad + k];
    }
    __syncthreads();
    const unsigned cg = (unsigned)Cout >> 2, utotal = (unsigned)total, ne = (unsigned)(pt + pb);
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < utotal; idx += gridDim.x * 256u) {
        const unsigned pix = idx / cg;
        const int c4 = (int)(idx - pix * cg) * 4;
        const unsigned be = pix / (unsigned)W;
        const int x = (int)(pix - be * (unsigned)W);
        const unsigned b = be / ne;
        const int e = (int)(be - b * ne);
        const int y = e < pt ? e : H - pb + (e - pt);
        const int wr = win_row[b];
        const float mean = stats[2u * b];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int ky = 0; ky < kh; ++ky) {
            const int iy = y - pt + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
            const float* src = mspec + (size_t)(wr + iy) * 24;
            for (int kx = 0; kx < kw; ++kx) {
                const int ix = x - pl + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const float v = src[ix];
                const float4 wk = *reinterpret_cast<const float4*>(&sW[(ky * kw + kx) * Cout + c4]);
                a0 = fmaf(v, wk.x, a0); a1 = fmaf(v, wk.y, a1); a2 = fmaf(v, wk.z, a2); a3 = fmaf(v, wk.w, a3);
                s0 += wk.x; s1 += wk.y; s2 += wk.z; s3 += wk.w;
            }
        }
        const float4 sf = *reinterpret_cast<const float4*>(S + (size_t)x * Cout + c4);
        a0 = fmaf(mean, sf.x - s0, a0); a1 = fmaf(mean, sf.y - s1, a1); a2 = fmaf(mean, sf.z - s2, a2); a3 = fmaf(mean, sf.w - s3, a3);
        float4 o;
        o.x = isfinite(a0) ? a0 : 0.f; o.y = isfinite(a1) ? a1 : 0.f; o.z = isfinite(a2) ? a2 : 0.f; o.w = isfinite(a3) ? a3 : 0.f;
        *reinterpret_cast<float4*>(E + (size_t)idx * 4) = o;
    }
}

// The same R for a compile-time filter shape, one thread per (log-mel row t, 4 channels): the thread keeps the 24 values
// of each of its KH input rows in registers and produces ALL Wout positions of the row from them -- 6 float4
// loads per input row instead of KH * KW scalar loads per OUTPUT (first_layer_raw_kernel issues 20 loads per 16 bytes
// stored and ran at 1.8 TB/s of stores, bound by the load-issue rate of the texture path, not by HBM).  Every output is
// the same fmaf chain in (ky, kx) order: bit-identical results.  A store instruction covers 4 rows x 256 contiguous bytes.
template <int KH_, int KW_, int WOUT>
__global__ __launch_bounds__(256) void first_layer_rows_kernel(const float* __restrict__ mspec, int row0, int nrows, int Cout,
                                                               const float* __restrict__ w, int Kpad, float* __restrict__ R) {
    static_assert(WOUT + KW_ - 1 <= 24, "the log-mel rows are 24 wide");
    extern __shared__ __attribute__((aligned(16))) float sW[];     // [K][Cout]
    constexpr int K = KH_ * KW_;
    for (int e = threadIdx.x; e < K * Cout; e += 256) {
        const int co = e / K, k = e - co * K;
        sW[k * Cout + co] = w[(size_t)co * Kpad + k];
    }
    __syncthreads();
    const unsigned cg = (unsigned)Cout >> 2, total = (unsigned)nrows * cg;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned t = idx / cg;
        const int c4 = (int)(idx - t * cg) * 4;
        float4 acc[WOUT];
#pragma unroll
        for (int x = 0; x < WOUT; ++x) acc[x] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < KH_; ++ky) {
            float v[24];
            const float4* src = reinterpret_cast<const float4*>(mspec + (size_t)(row0 + (int)t + ky) * 24);
#pragma unroll
            for (int q = 0; q < 6; ++q) { const float4 f = src[q]; v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w; }
#pragma unroll
            for (int kx = 0; kx < KW_; ++kx) {
                const float4 wk = *reinterpret_cast<const float4*>(&sW[(ky * KW_ + kx) * Cout + c4]);
#pragma unroll
                for (int x = 0; x < WOUT; ++x) {
                    acc[x].x = fmaf(v[x + kx], wk.x, acc[x].x);
                    acc[x].y = fmaf(v[x + kx], wk.y, acc[x].y);
                    acc[x].z = fmaf(v[x + kx], wk.z, acc[x].z);
                    acc[x].w = fmaf(v[x + kx], wk.w, acc[x].w);
                }
            }
        }
        float* dst = R + ((size_t)t * WOUT) * Cout + c4;
#pragma unroll
        for (int x = 0; x < WOUT; ++x) {
            float4 o;
            o.x = isfinite(acc[x].x) ? acc[x].x : 0.f; o.y = isfinite(acc[x].y) ? acc[x].y : 0.f;
            o.z = isfinite(acc[x].z) ? acc[x].z : 0.f; o.w = isfinite(acc[x].w) ? acc[x].w : 0.f;
            *reinterpret_cast<float4*>(dst + (size_t)x * Cout) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Direct 3x3 convolution of a ONE-channel image (stride 1, zero padding 1, bias, optional relu): ResNet-101's first layer
// (resnet.py:96-99, on the 64 x 144 fbank window of vbx_segmenter.py:262-266).  As a GEMM it has K = 9 padded to a 32-wide
// k-tile of scalar table-driven gathers (conv_x3_kernel<1>: 470 us per 512 windows, 4.5 x the time its 604 MB of output take to
// write).  Here a thread owns 8 consecutive rows x 4 channels of one column: 3 x 10 inputs in registers, 288 fmaf (f32, chain
// in (ky, kx) order), and a wave's store instruction covers 8 neighbouring columns x 128 B = 1 KB contiguous.
// Window input (vbx features, frame-major) and NHWC input share the addressing (row_stride / pix_stride / per-sample base).
template <bool WINDOW>
__global__ __launch_bounds__(256) void conv1_direct3x3_kernel(const ConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sW[];     // [9][Cout]
    for (int e = threadIdx.x; e < 9 * p.Cout; e += 256) {
        const int co = e / 9, k = e - co * 9;
        sW[k * p.Cout + co] = p.w[(size_t)co * p.Kpad + k];
    }
    __syncthreads();
    const unsigned cg = (unsigned)p.Cout >> 2, hb = (unsigned)(p.H + 7) >> 3;
    const unsigned per_img = cg * (unsigned)p.W * hb;
    const unsigned total = per_img * (unsigned)(p.M / ((long long)p.H * p.W));       // host: < 2^32
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned b = idx / per_img;
        unsigned r = idx - b * per_img;
        const unsigned ob = r / (cg * (unsigned)p.W);
        r -= ob * cg * (unsigned)p.W;
        const int ox = (int)(r / cg), c4 = (int)(r - (unsigned)ox * cg) * 4, oy0 = (int)ob * 8;
        const float* src = p.in + (WINDOW ? (long long)p.win_row[b] * p.pix_stride : (long long)b * p.img_stride);
        float v[3][10];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox - 1 + dx;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const int iy = oy0 - 1 + j;
                const bool ok = (unsigned)ix < (unsigned)p.W && (unsigned)iy < (unsigned)p.H;
                const float x = src[ok ? (long long)iy * p.row_stride + (long long)ix * p.pix_stride : 0];
                v[dx][j] = ok ? x : 0.f;
            }
        }
        float4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float4 wk = *reinterpret_cast<const float4*>(&sW[(ky * 3 + kx) * p.Cout + c4]);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    acc[i].x = fmaf(v[kx][i + ky], wk.x, acc[i].x);
                    acc[i].y = fmaf(v[kx][i + ky], wk.y, acc[i].y);
                    acc[i].z = fmaf(v[kx][i + ky], wk.z, acc[i].z);
                    acc[i].w = fmaf(v[kx][i + ky], wk.w, acc[i].w);
                }
            }
        const float4 b4 = *reinterpret_cast<const float4*>(p.bias + c4);
        float* dst = p.out + (((size_t)b * p.H + oy0) * p.W + ox) * p.Cout + c4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (oy0 + i >= p.H) break;
            float4 o = make_float4(acc[i].x + b4.x, acc[i].y + b4.y, acc[i].z + b4.z, acc[i].w + b4.w);
            if (p.act == 1) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
            *reinterpret_cast<float4*>(dst + (size_t)i * p.W * p.Cout) = o;
        }
    }
}

// One wavefront per slot.  segmenter.py:82 (np.mean / np.std over the flattened window) and
// :86 (finite = all(isfinite(normalised))).
__global__ __launch_bounds__(256) void patch_stats_kernel(const float* __restrict__ mspec,
                                                          const int32_t* __restrict__ win_row, int n, int h,
                                                          float* __restrict__ stats, uint8_t* __restrict__ finite) {
    // A lane owns the flattened elements e = lane + 64 k of the 68 x h window (k < 23 for h <= 21, < 26 for h = 24): they are
    // loaded ONCE into registers and the three passes (mean, squared deviations, finite test) run on the registers, in
    // the element order and with the f64 sums of the three-pass form (bit-identical results).  (r, c) of an element
    // advance by (64 / h, 64 % h) with a carry: the run-time division per element and pass was most of this kernel's time.
    constexpr int NV = 26;                           // ceil(68 * 24 / 64)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const float* src = mspec + (size_t)win_row[b] * 24;
    const int cnt = 68 * h;
    const int dr = 64 / h, dc = 64 - dr * h;
    int r = lane / h, c = lane - r * h;
    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int e = lane + 64 * k;
        v[k] = src[e < cnt ? r * 24 + c : 0];        // unconditional load (tail lanes re-read element 0 and are masked below)
        r += dr; c += dc;
        if (c >= h) { c -= h; ++r; }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) if (lane + 64 * k < cnt) s += (double)v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const double mean_d = s / cnt;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < cnt) { const double d = (double)v[k] - mean_d; q += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float meanf = (float)mean_d;
    const float sdf = (float)sqrt(q / cnt);
    int bad = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < cnt) bad |= !isfinite((v[k] - meanf) / sdf);
    bad = __any(bad);
    if (lane == 0) { stats[2 * b] = meanf; stats[2 * b + 1] = sdf; finite[b] = bad ? 0 : 1; }
}

// NHWC pooling; one thread per (sample, oy, ox, c)
__global__ void pool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int H, int W,
                            int C, int Ho, int Wo, int kh, int kw, int sh, int sw, int pt, int pl, int kind) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    long long t = idx / C;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long long b = t / Ho;
    float acc = kind == 0 ? -INFINITY : 0.f;
    int cnt = 0;
    for (int ky = 0; ky < kh; ++ky) {
        const int iy = oy * sh - pt + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < kw; ++kx) {
            const int ix = ox * sw - pl + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float v = in[((b * H + iy) * W + ix) * C + c];
            acc = kind == 0 ? fmaxf(acc, v) : acc + v;
            ++cnt;
        }
    }
    // average: over the window's elements INSIDE the input -- kh * kw unless the pool is zero-padded (Keras / TF 'same' average
    // pooling leaves the padding out of the mean)
    out[idx] = kind == 0 ? acc : acc / (float)(cnt > 0 ? cnt : 1);
}


// Elementwise activations that are not fused into a producer's epilogue (ISS_OP_ACT): elu, leaky relu, selu, softplus, clipped relu.
// One thread per 4 elements (the tail scalar), grid-stride; in place when in == out -- the op program's rows are, so the pointers are
// NOT __restrict__ (iss_cnn_load refuses an ISS_OP_ACT row that reads the network input).
__global__ __launch_bounds__(256) void act_kernel(const float* in, float* out, long long total, int act, float alpha, float p2, float p3) {
    auto f = [&](float v) {
        if (act == 9) return v > p3 ? fminf(v, p2) : alpha * (v - p3);                   // keras.layers.ReLU(max_value = p2, negative_slope = alpha, threshold = p3)
        if (act == 8) return fminf(fmaxf(v, 0.f), alpha);                                // keras.layers.ReLU(max_value = alpha)
        if (act == 4) return v > 0.f ? v : alpha * (expf(v) - 1.f);                       // keras.activations.elu
        if (act == 5) return v > 0.f ? v : alpha * v;                                    // keras.layers.LeakyReLU
        if (act == 6) return 1.05070098f * (v > 0.f ? v : 1.67326324f * (expf(v) - 1.f)); // selu
        return v > 20.f ? v : log1pf(expf(v));                                           // softplus
    };
    const long long n4 = total >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 v = reinterpret_cast<const float4*>(in)[i];
        v.x = f(v.x); v.y = f(v.y); v.z = f(v.z); v.w = f(v.w);
        reinterpret_cast<float4*>(out)[i] = v;
    }
    for (long long i = (n4 << 2) + blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) out[i] = f(in[i]);
}

// Merge / data-movement rows of graph-shaped models (ISS_OP_ELT, include/iss.h): one thread per output element, grid-stride.  `in`,
// `res` and `out` may alias for the binary kinds (each element is read before it is written, by the same thread).
__global__ __launch_bounds__(256) void elt_kernel(const float* in, const float* res, float* out, long long total, int kind,
                                                  int cin, int cout, int nch, int soff, int doff, int d0, int d1, int d2,
                                                  int s0, int s1, int s2, int relu) {
    auto bin = [&](float a, float b) {
        const float v = kind == ISS_ELT_ADD ? a + b : kind == ISS_ELT_SUB ? a - b : kind == ISS_ELT_MUL ? a * b :
                        kind == ISS_ELT_MAX ? fmaxf(a, b) : kind == ISS_ELT_MIN ? fminf(a, b) : (a + b) * 0.5f;
        return relu ? fmaxf(v, 0.f) : v;
    };
    if (kind >= ISS_ELT_ADD && kind <= ISS_ELT_AVG && (total & 3) == 0) {      // float4 at a time (buffers are 256-byte aligned)
        const long long n4 = total >> 2;
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const float4 a = reinterpret_cast<const float4*>(in)[i], b = reinterpret_cast<const float4*>(res)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(bin(a.x, b.x), bin(a.y, b.y), bin(a.z, b.z), bin(a.w, b.w));
        }
        return;
    }
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (kind >= ISS_ELT_ADD && kind <= ISS_ELT_AVG) {
            out[i] = bin(in[i], res[i]);
        } else if (kind == ISS_ELT_COPY || kind == ISS_ELT_ZERO) {       // total = pixels * nch
            const long long p = i / nch;
            const int ch = (int)(i - p * nch);
            out[p * cout + doff + ch] = kind == ISS_ELT_ZERO ? 0.f : in[p * cin + soff + ch];
        } else {                                                         // PERMUTE: output (d0, d1, d2) row-major per sample, input strides s0..s2
            const long long per = (long long)d0 * d1 * d2;
            const long long smp = i / per;
            long long r = i - smp * per;
            const int i2 = (int)(r % d2); r /= d2;
            const int i1 = (int)(r % d1);
            const int i0 = (int)(r / d1);
            out[i] = in[smp * per + (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2];
        }
    }
}

__global__ void softmax_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows, int C) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* x = in + r * C;
    float mx = x[0];
    for (int i = 1; i < C; ++i) mx = fmaxf(mx, x[i]);
    float s = 0.f;
    for (int i = 0; i < C; ++i) s += expf(x[i] - mx);
    for (int i = 0; i < C; ++i) out[r * C + i] = expf(x[i] - mx) / s;
}

// mean || std over W (time) for every (h, c); out[(c*H + h)] and out[C*H + c*H + h]  (resnet.py:123-127)
__global__ void statpool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int H, int W, int C) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    long long t = idx / C;
    const int h = (int)(t % H);
    const long long b = t / H;
    const float* src = in + ((b * H + h) * (long long)W) * C + c;
    float s = 0.f, q = 0.f;
    for (int w = 0; w < W; ++w) { const float v = src[(long long)w * C]; s += v; q += v * v; }
    const float mean = s / W, meansq = q / W;
    float* o = out + b * (2LL * C * H);
    o[c * H + h] = mean;
    o[(long long)C * H + c * H + h] = sqrtf(meansq - mean * mean + 1e-10f);
}

__global__ void fill_half_kernel(float* p, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.5f;
}

// rows whose window was not finite get 0.5 everywhere (segmenter.py:175)
__global__ void mask_probs_kernel(float* probs, const uint8_t* finite, long long n, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * C && !finite[i / C]) probs[i] = 0.5f;
}

// One thread per resident log-mel row: the lowest column that holds a non-finite value, 24 if none.  A window of width w over
// rows [r, r + 68) with such a flag < w has a non-finite mean (patch_stats_kernel) and so is certainly not finite.
__global__ __launch_bounds__(256) void row_flags_kernel(const float* __restrict__ mspec, int T, uint8_t* __restrict__ flag) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float v[24];
#pragma unroll
    for (int k = 0; k < 6; ++k) *reinterpret_cast<float4*>(v + 4 * k) = reinterpret_cast<const float4*>(mspec + (size_t)t * 24)[k];
    flag[t] = (uint8_t)iss_row_flag(v);
}

// The rows of one pass over the live windows to the caller's slots: out[map[i]] = res[i], or 0.5 where the window did not
// normalise to finite values (segmenter.py:175); finite[map[i]] = the device's flag.  The dead slots were filled before.
// map == nullptr: slot i is row i (a pass of a list without dead windows, stored where it lands).  `out` / `finite` may be
// page-locked host memory: every element is stored once, by one thread.
__global__ void scatter_probs_kernel(const float* __restrict__ res, const uint8_t* __restrict__ lfinite, const int32_t* __restrict__ map,
                                     long long n, int C, float* __restrict__ out, uint8_t* __restrict__ finite) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const long long r = i / C;
    const int k = (int)(i - r * C);
    const long long m = map ? map[r] : r;
    const uint8_t f = lfinite[r];
    out[m * C + k] = f ? res[i] : 0.5f;
    if (k == 0) finite[m] = f;
}

inline int roundup(int a, int b) { return (a + b - 1) / b * b; }

// float -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does); weights are finite
inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

}  // namespace

// ============================================================================ host side
IssParamArrays::~IssParamArrays() {
    for (void* p : {(void*)blob, (void*)wh, (void*)wl, (void*)wh16, (void*)wl16}) if (p) (void)hipFree(p);
}

int iss_cnn_free(iss_ctx* c, int id) {
    if (!c || id < 0 || id >= ISS_MAX_NETS) return ISS_EINVAL;
    IssNet& n = c->nets[id];
    if (n.shared_params) {
        n.shared_params.reset();           // shared with another net (iss_cnn_load_shared): freed with the last of them
    } else {
        if (n.d_blob) (void)hipFree(n.d_blob);
        if (n.d_wh) (void)hipFree(n.d_wh);
        if (n.d_wl) (void)hipFree(n.d_wl);
        if (n.d_wh16) (void)hipFree(n.d_wh16);
        if (n.d_wl16) (void)hipFree(n.d_wl16);
    }
    for (auto& kv : n.dhl_wp) if (kv.second) (void)hipFree(kv.second);
    if (n.d_wsum) (void)hipFree(n.d_wsum);
    if (n.d_ktab) (void)hipFree(n.d_ktab);
    n = IssNet();
    return ISS_OK;
}

namespace {
// The op program of a load (iss_cnn_load / iss_cnn_load_shared): rows validated against a blob of blob_floats floats, the
// im2col tables built into ktab.
int cnn_set_program(iss_ctx* c, IssNet& n, const char* who, const int32_t* prog, int32_t nrows, int64_t blob_floats,
                    int32_t nbuf, const int64_t* buf_elems, int32_t in_h, int32_t in_w, int32_t in_c, int32_t out_dim,
                    std::vector<int32_t>& ktab) {
    n.prog.assign(prog, prog + (size_t)nrows * ISS_PROG_COLS);
    n.nrows = nrows; n.nbuf = nbuf; n.buf_elems.assign(buf_elems, buf_elems + nbuf);
    n.in_h = in_h; n.in_w = in_w; n.in_c = in_c; n.out_dim = out_dim;
    n.kpad.assign(nrows, 0); n.ktab_off.assign(nrows, -1);
    double flops = 0;
    for (int r = 0; r < nrows; ++r) {
        const int32_t* R = &n.prog[(size_t)r * ISS_PROG_COLS];
        auto bad = [&](const char* what) { return iss_fail(c, ISS_EINVAL, "%s: row %d: %s", who, r, what); };
        if (R[ISS_C_IN] != ISS_BUF_INPUT && (R[ISS_C_IN] < 0 || R[ISS_C_IN] >= nbuf)) return bad("IN buffer id");
        if (R[ISS_C_OUT] < 0 || R[ISS_C_OUT] >= nbuf) return bad("OUT buffer id");
        if (R[ISS_C_OP] == ISS_OP_CONV) {
            const int K = R[ISS_C_KH] * R[ISS_C_KW] * R[ISS_C_CIN];
            const int Kpad = roundup(K, KALIGN);
            if (K <= 0 || R[ISS_C_COUT] <= 0) return bad("conv shape");
            if (R[ISS_C_WOFF] < 0 || (R[ISS_C_WOFF] & 7) || (int64_t)R[ISS_C_WOFF] + (int64_t)R[ISS_C_COUT] * Kpad > blob_floats)
                return bad("weight offset misaligned or outside blob (weights must be [Cout][roundup32(K)], offset % 8 == 0)");
            if (R[ISS_C_RES] >= nbuf) return bad("RES buffer id");
            if (R[ISS_C_KH] > 32767 || R[ISS_C_KW] > 32767) return bad("kernel too large");
            int fph, fpw;
            fused_pool_of(R, fph, fpw);
            if (fph * fpw != 1 && fph * fpw != 2 && fph * fpw != 4) return bad("fused pool window must cover 2 or 4 outputs");
            if (fph * fpw > 1 && (R[ISS_C_RES] >= 0 || R[ISS_C_HO] / fph < 1 || R[ISS_C_WO] / fpw < 1))
                return bad("fused pool with residual / empty pooled output");
            const bool patch = R[ISS_C_INMODE] == 1;
            const bool window = R[ISS_C_INMODE] == 2;      // (H = features, W = frames) view of the resident (T, H) vbx features
            if (patch && (R[ISS_C_CIN] != 1 || R[ISS_C_H] != 68 || R[ISS_C_W] > 24)) return bad("patch-mode conv must read (68, <=24, 1)");
            if (window && (R[ISS_C_CIN] != 1 || R[ISS_C_H] != 64)) return bad("window-mode conv must read (64, frames, 1)");
            const int rs = patch ? 24 : (window ? 1 : R[ISS_C_W] * R[ISS_C_CIN]);
            const int ps = patch ? 1 : (window ? R[ISS_C_H] : R[ISS_C_CIN]);
            n.kpad[r] = Kpad; n.ktab_off[r] = (int64_t)ktab.size();
            for (int k = 0; k < Kpad; ++k) {
                if (k < K) {
                    const int cc = k % R[ISS_C_CIN], kk = k / R[ISS_C_CIN];
                    const int kx = kk % R[ISS_C_KW], ky = kk / R[ISS_C_KW];
                    ktab.push_back(ky * rs + kx * ps + cc);
                    ktab.push_back((ky << 16) | kx);
                } else {                              // K padding: force the bounds test to fail -> zeros
                    ktab.push_back(0);
                    ktab.push_back((0x7fff << 16) | 0x7fff);
                }
            }
            flops += 2.0 * K * R[ISS_C_COUT] * (double)(R[ISS_C_HO] / fph * fph) * (double)(R[ISS_C_WO] / fpw * fpw);
            if (R[ISS_C_DUALW] != 0 || R[ISS_C_DUALB] != 0) {     // projection shortcut (row r - 1) + expansion (row r) as one GEMM
                if (r < 1) return bad("ISS_C_DUALW on the first row");
                const int32_t* P = &n.prog[(size_t)(r - 1) * ISS_PROG_COLS];
                int pph, ppw;
                fused_pool_of(P, pph, ppw);
                const bool shapes = P[ISS_C_OP] == ISS_OP_CONV && P[ISS_C_KH] == 1 && P[ISS_C_KW] == 1 && R[ISS_C_KH] == 1 && R[ISS_C_KW] == 1 &&
                                    R[ISS_C_SH] == 1 && R[ISS_C_SW] == 1 && P[ISS_C_SH] >= 1 && P[ISS_C_SW] >= 1 &&
                                    R[ISS_C_PT] == 0 && R[ISS_C_PL] == 0 && P[ISS_C_PT] == 0 && P[ISS_C_PL] == 0 &&
                                    R[ISS_C_INMODE] == 0 && P[ISS_C_INMODE] == 0 && fph * fpw == 1 && pph * ppw == 1 &&
                                    R[ISS_C_HO] == R[ISS_C_H] && R[ISS_C_WO] == R[ISS_C_W] && P[ISS_C_HO] == R[ISS_C_HO] &&
                                    P[ISS_C_WO] == R[ISS_C_WO] && P[ISS_C_COUT] == R[ISS_C_COUT] &&
                                    (P[ISS_C_HO] - 1) * P[ISS_C_SH] < P[ISS_C_H] && (P[ISS_C_WO] - 1) * P[ISS_C_SW] < P[ISS_C_W] &&
                                    R[ISS_C_CIN] % 32 == 0 && P[ISS_C_CIN] % 32 == 0;
                const bool chain = R[ISS_C_RES] >= 0 && R[ISS_C_RES] == P[ISS_C_OUT] && R[ISS_C_OUT] == R[ISS_C_RES] &&
                                   R[ISS_C_IN] != P[ISS_C_OUT] && P[ISS_C_IN] != P[ISS_C_OUT] && P[ISS_C_RES] < 0 && P[ISS_C_ACT] == 0 &&
                                   P[ISS_C_PSOFF] < 0 && R[ISS_C_PSOFF] < 0 && P[ISS_C_BOFF] >= 0 && R[ISS_C_BOFF] >= 0;
                const int64_t wo = (int64_t)R[ISS_C_DUALW] - 1, bo = (int64_t)R[ISS_C_DUALB] - 1;
                const bool offs = wo >= 0 && bo >= 0 && (wo & 7) == 0 &&
                                  wo + (int64_t)R[ISS_C_COUT] * (R[ISS_C_CIN] + P[ISS_C_CIN]) <= blob_floats && bo + R[ISS_C_COUT] <= blob_floats;
                if (!shapes || !chain || !offs)
                    return bad("ISS_C_DUALW / ISS_C_DUALB: rows r - 1, r are not a linear 1x1 projection and the in-place 1x1 expansion it is added to, "
                               "or the concatenated parameters lie outside the blob (include/iss.h)");
            }
        } else if (R[ISS_C_OP] == ISS_OP_ACT) {
            if (R[ISS_C_ACT] < 4 || R[ISS_C_ACT] > 9) return bad("ISS_OP_ACT: activation code must be 4 (elu), 5 (leaky relu), 6 (selu), 7 (softplus), 8 (relu with max_value) or 9 (keras ReLU in full)");
            if (R[ISS_C_IN] == ISS_BUF_INPUT) return bad("ISS_OP_ACT: an elementwise activation cannot read the network input (it works in place)");
        } else if (R[ISS_C_OP] == ISS_OP_ELT) {
            const int k = R[ISS_C_ACT];
            const long long hw = (long long)R[ISS_C_H] * R[ISS_C_W];
            if (k < ISS_ELT_COPY || k > ISS_ELT_PERMUTE) return bad("ISS_OP_ELT: unknown kind");
            if (R[ISS_C_HO] < 1 || R[ISS_C_WO] < 1 || R[ISS_C_COUT] < 1 || R[ISS_C_CIN] < 1 || hw < 1) return bad("ISS_OP_ELT: shape");
            if ((long long)R[ISS_C_HO] * R[ISS_C_WO] * R[ISS_C_COUT] > buf_elems[R[ISS_C_OUT]]) return bad("ISS_OP_ELT: output larger than its buffer");
            if (R[ISS_C_IN] != ISS_BUF_INPUT && k != ISS_ELT_ZERO && hw * R[ISS_C_CIN] > buf_elems[R[ISS_C_IN]]) return bad("ISS_OP_ELT: input larger than its buffer");
            if (R[ISS_C_IN] == ISS_BUF_INPUT && k != ISS_ELT_ZERO) return bad("ISS_OP_ELT: a merge row cannot read the network input");
            if (k >= ISS_ELT_ADD && k <= ISS_ELT_AVG) {
                if (R[ISS_C_RES] < 0 || R[ISS_C_RES] >= nbuf) return bad("ISS_OP_ELT: a binary row needs its second operand in ISS_C_RES");
                if (R[ISS_C_HO] != R[ISS_C_H] || R[ISS_C_WO] != R[ISS_C_W] || R[ISS_C_COUT] != R[ISS_C_CIN]) return bad("ISS_OP_ELT: binary rows keep the shape");
                if (hw * R[ISS_C_CIN] > buf_elems[R[ISS_C_RES]]) return bad("ISS_OP_ELT: second operand larger than its buffer");
            } else if (k == ISS_ELT_COPY || k == ISS_ELT_ZERO) {
                if (R[ISS_C_HO] != R[ISS_C_H] || R[ISS_C_WO] != R[ISS_C_W]) return bad("ISS_OP_ELT: COPY / ZERO keep the pixel grid");
                if (R[ISS_C_KH] < 1 || R[ISS_C_PL] < 0 || R[ISS_C_PL] + R[ISS_C_KH] > R[ISS_C_COUT]) return bad("ISS_OP_ELT: destination channel range outside COUT");
                if (k == ISS_ELT_COPY && (R[ISS_C_PT] < 0 || R[ISS_C_PT] + R[ISS_C_KH] > R[ISS_C_CIN] || R[ISS_C_IN] == R[ISS_C_OUT]))
                    return bad("ISS_OP_ELT: COPY source channel range outside CIN, or IN == OUT");
            } else {
                const int pm[3] = {R[ISS_C_KH], R[ISS_C_KW], R[ISS_C_SH]};
                const int dims[3] = {R[ISS_C_H], R[ISS_C_W], R[ISS_C_CIN]};
                if (pm[0] < 0 || pm[0] > 2 || pm[1] < 0 || pm[1] > 2 || pm[2] < 0 || pm[2] > 2 || pm[0] == pm[1] || pm[0] == pm[2] || pm[1] == pm[2])
                    return bad("ISS_OP_ELT: PERMUTE needs a permutation of (0, 1, 2) in KH, KW, SH");
                if (R[ISS_C_HO] != dims[pm[0]] || R[ISS_C_WO] != dims[pm[1]] || R[ISS_C_COUT] != dims[pm[2]] || R[ISS_C_IN] == R[ISS_C_OUT])
                    return bad("ISS_OP_ELT: PERMUTE output shape is not the permuted input shape, or IN == OUT");
            }
        } else if (R[ISS_C_OP] != ISS_OP_POOL && R[ISS_C_OP] != ISS_OP_SOFTMAX && R[ISS_C_OP] != ISS_OP_STATPOOL) {
            return bad("unknown op");
        }
    }
    n.flops_per_sample = flops; n.blob_floats = blob_floats;
    return ISS_OK;
}

// Per-program device tables of a load whose parameters are already on the device (n.d_blob): the weight sums of the
// patch-mode first layers (from the host blob when there is one, else from the device copy) and the im2col tables.
int cnn_upload_tables(iss_ctx* c, IssNet& n, const float* blob, const std::vector<int32_t>& ktab) {
    const int nrows = n.nrows;
    {   // per-channel weight sums of the patch-mode first layers (ConvArgs::f_wsum)
        std::vector<float> wsum;
        n.wsum_off.assign(nrows, -1);
        n.wsumx_off.assign(nrows, -1);
        std::vector<float> wdev;
        for (int r = 0; r < nrows; ++r) {
            const int32_t* R = &n.prog[(size_t)r * ISS_PROG_COLS];
            if (R[ISS_C_OP] != ISS_OP_CONV || R[ISS_C_INMODE] != 1) continue;
            const int K = R[ISS_C_KH] * R[ISS_C_KW] * R[ISS_C_CIN];
            const float* w = blob ? blob + R[ISS_C_WOFF] : nullptr;     // this row's [Cout][Kpad] weights
            if (!w) {
                wdev.resize((size_t)R[ISS_C_COUT] * n.kpad[r]);
                ISS_HIP(c, hipMemcpy(wdev.data(), n.d_blob + R[ISS_C_WOFF], wdev.size() * sizeof(float), hipMemcpyDeviceToHost));
                w = wdev.data();
            }
            n.wsum_off[r] = (int64_t)wsum.size();
            for (int co = 0; co < R[ISS_C_COUT]; ++co) {
                double acc = 0.0;
                for (int k = 0; k < K; ++k) acc += (double)w[(int64_t)co * n.kpad[r] + k];
                wsum.push_back((float)acc);
            }
            while (wsum.size() % 8) wsum.push_back(0.f);         // float4-aligned rows
            // zero-padded first layer: S[x][co] = sum over all filter rows and the filter columns that see data at column x
            // (conv_x3_ws_kernel<..., FS>, first_layer_edge_kernel)
            if ((R[ISS_C_PT] != 0 || R[ISS_C_PL] != 0 || R[ISS_C_WO] == R[ISS_C_W]) && R[ISS_C_CIN] == 1 && R[ISS_C_SW] == 1) {
                n.wsumx_off[r] = (int64_t)wsum.size();
                const int W = R[ISS_C_W], kh = R[ISS_C_KH], kw = R[ISS_C_KW], pl = R[ISS_C_PL];
                for (int x = 0; x < W; ++x)
                    for (int co = 0; co < R[ISS_C_COUT]; ++co) {
                        double acc = 0.0;
                        for (int ky = 0; ky < kh; ++ky)
                            for (int kx = 0; kx < kw; ++kx)
                                if (x - pl + kx >= 0 && x - pl + kx < W) acc += (double)w[(int64_t)co * n.kpad[r] + ky * kw + kx];
                        wsum.push_back((float)acc);
                    }
                while (wsum.size() % 8) wsum.push_back(0.f);
            }
        }
        if (!wsum.empty()) {
            ISS_HIP(c, hipMalloc((void**)&n.d_wsum, wsum.size() * sizeof(float)));
            ISS_HIP(c, hipMemcpy(n.d_wsum, wsum.data(), wsum.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (!ktab.empty()) {
        ISS_HIP(c, hipMalloc((void**)&n.d_ktab, ktab.size() * sizeof(int32_t)));
        ISS_HIP(c, hipMemcpy(n.d_ktab, ktab.data(), ktab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return ISS_OK;
}
}  // namespace

extern "C" int iss_cnn_load(iss_ctx* c, int id, const int32_t* prog, int32_t nrows, const float* blob,
                            int64_t blob_floats, int32_t nbuf, const int64_t* buf_elems, int32_t in_h, int32_t in_w,
                            int32_t in_c, int32_t out_dim) {
    if (!c) return ISS_EINVAL;
    if (id < 0 || id >= ISS_MAX_NETS || !prog || nrows <= 0 || !blob || blob_floats <= 0 || nbuf <= 0 || !buf_elems)
        return iss_fail(c, ISS_EINVAL, "iss_cnn_load: bad argument");
    ISS_HIP(c, hipSetDevice(c->device));
    iss_cnn_free(c, id);
    IssNet& n = c->nets[id];
    std::vector<int32_t> ktab;
    int rc = cnn_set_program(c, n, "iss_cnn_load", prog, nrows, blob_floats, nbuf, buf_elems, in_h, in_w, in_c, out_dim, ktab);
    if (rc) return rc;
    ISS_HIP(c, hipMalloc((void**)&n.d_blob, (size_t)blob_floats * sizeof(float)));
    ISS_HIP(c, hipMemcpy(n.d_blob, blob, (size_t)blob_floats * sizeof(float), hipMemcpyHostToDevice));
    {   // bf16 hi / lo parts of every parameter, same offsets as the f32 blob (conv_x3_kernel operands)
        std::vector<uint16_t> hi((size_t)blob_floats), lo((size_t)blob_floats);
        for (int64_t i = 0; i < blob_floats; ++i) {
            hi[i] = bf16_rne(blob[i]);
            lo[i] = bf16_rne(blob[i] - bf16_to_f32(hi[i]));
        }
        // fp16 split of the same values (ISS_PREC_F16X3); a value outside fp16's range makes the whole network ineligible
        std::vector<uint16_t> hi16((size_t)blob_floats), lo16((size_t)blob_floats);
        n.f16_ok = true;
        for (int64_t i = 0; i < blob_floats; ++i) {
            const float x = blob[i];
            if (!(std::fabs(x) < 65504.f)) { n.f16_ok = false; hi16[i] = lo16[i] = 0; continue; }
            const _Float16 h = (_Float16)x;
            const _Float16 l = (_Float16)(x - (float)h);
            memcpy(&hi16[i], &h, 2); memcpy(&lo16[i], &l, 2);
        }
        ISS_HIP(c, hipMalloc((void**)&n.d_wh16, (size_t)blob_floats * 2 + 16));
        ISS_HIP(c, hipMalloc((void**)&n.d_wl16, (size_t)blob_floats * 2 + 16));
        ISS_HIP(c, hipMemcpy(n.d_wh16, hi16.data(), (size_t)blob_floats * 2, hipMemcpyHostToDevice));
        ISS_HIP(c, hipMemcpy(n.d_wl16, lo16.data(), (size_t)blob_floats * 2, hipMemcpyHostToDevice));
        ISS_HIP(c, hipMalloc((void**)&n.d_wh, (size_t)blob_floats * 2 + 16));
        ISS_HIP(c, hipMalloc((void**)&n.d_wl, (size_t)blob_floats * 2 + 16));
        ISS_HIP(c, hipMemcpy(n.d_wh, hi.data(), (size_t)blob_floats * 2, hipMemcpyHostToDevice));
        ISS_HIP(c, hipMemcpy(n.d_wl, lo.data(), (size_t)blob_floats * 2, hipMemcpyHostToDevice));
    }
    if ((rc = cnn_upload_tables(c, n, blob, ktab))) return rc;
    n.loaded = true;
    return ISS_OK;
}

extern "C" int iss_cnn_load_shared(iss_ctx* c, int id, int src, const int32_t* prog, int32_t nrows, int32_t nbuf,
                                   const int64_t* buf_elems, int32_t in_h, int32_t in_w, int32_t in_c, int32_t out_dim) {
    if (!c) return ISS_EINVAL;
    if (id < 0 || id >= ISS_MAX_NETS || src < 0 || src >= ISS_MAX_NETS || src == id || !prog || nrows <= 0 || nbuf <= 0 || !buf_elems)
        return iss_fail(c, ISS_EINVAL, "iss_cnn_load_shared: bad argument");
    if (!c->nets[src].loaded || !c->nets[src].d_blob)
        return iss_fail(c, ISS_ESTATE, "iss_cnn_load_shared: source net %d not loaded", src);
    ISS_HIP(c, hipSetDevice(c->device));
    iss_cnn_free(c, id);                                  // (id != src: the source's arrays stay)
    IssNet& s = c->nets[src];
    IssNet& n = c->nets[id];
    std::vector<int32_t> ktab;
    int rc = cnn_set_program(c, n, "iss_cnn_load_shared", prog, nrows, s.blob_floats, nbuf, buf_elems, in_h, in_w, in_c, out_dim, ktab);
    if (rc) return rc;
    if (!s.shared_params) {                               // first alias: the source's arrays become reference-counted
        s.shared_params = std::make_shared<IssParamArrays>();
        IssParamArrays& a = *s.shared_params;
        a.blob = s.d_blob; a.wh = s.d_wh; a.wl = s.d_wl; a.wh16 = s.d_wh16; a.wl16 = s.d_wl16;
    }
    n.shared_params = s.shared_params;
    n.d_blob = s.d_blob; n.d_wh = s.d_wh; n.d_wl = s.d_wl; n.d_wh16 = s.d_wh16; n.d_wl16 = s.d_wl16;
    n.f16_ok = s.f16_ok;
    if ((rc = cnn_upload_tables(c, n, nullptr, ktab))) return rc;
    n.loaded = true;
    return ISS_OK;
}

extern "C" int iss_set_precision(iss_ctx* c, int mode) {
    if (!c) return ISS_EINVAL;
    if (mode != ISS_PREC_BF16X3 && mode != ISS_PREC_F32 && mode != ISS_PREC_F16X3) return iss_fail(c, ISS_EINVAL, "iss_set_precision: unknown mode %d", mode);
    if (mode == c->precision) return ISS_OK;
    c->precision = mode;
    // the guard's decision (or its FIXED for a first call in exact f32) was about the old mode: every network the caller has not
    // pinned follows the new one and is probed again on its next iss_cnn_probs call
    for (IssNet& n : c->nets) {
        if (!n.loaded || n.prec_by_caller) continue;
        n.prec_override = -1;
        n.guard_state = ISS_GUARD_PENDING;
        n.guard_dlogp = n.guard_dlogp_chosen = -1.f;
        n.guard_slots = 0;
    }
    return ISS_OK;
}

extern "C" int iss_set_precision_guard(iss_ctx* c, float threshold) {
    if (!c) return ISS_EINVAL;
    if (!(threshold == threshold)) return iss_fail(c, ISS_EINVAL, "iss_set_precision_guard: threshold is NaN");
    c->guard_threshold = threshold;
    return ISS_OK;
}

extern "C" int iss_cnn_set_net_precision(iss_ctx* c, int id, int mode) {
    if (!c || id < 0 || id >= ISS_MAX_NETS) return ISS_EINVAL;
    if (mode != -1 && mode != ISS_PREC_BF16X3 && mode != ISS_PREC_F32 && mode != ISS_PREC_F16X3) return iss_fail(c, ISS_EINVAL, "iss_cnn_set_net_precision: unknown mode %d", mode);
    if (!c->nets[id].loaded) return iss_fail(c, ISS_ESTATE, "net %d not loaded", id);
    c->nets[id].prec_override = mode;
    c->nets[id].prec_by_caller = mode != -1;
    c->nets[id].guard_state = mode == -1 ? ISS_GUARD_PENDING : ISS_GUARD_FIXED;
    return ISS_OK;
}

// A patch network (iss_cnn_probs) reads mspec windows through its first conv; iss_cnn_forward and iss_vbx_embed run every other kind.
static bool net_reads_patches(const IssNet& n) {
    for (int r = 0; r < n.nrows; ++r)
        if (n.prog[(size_t)r * ISS_PROG_COLS + ISS_C_OP] == ISS_OP_CONV && n.prog[(size_t)r * ISS_PROG_COLS + ISS_C_INMODE] == 1) return true;
    return false;
}

// The arithmetic a network actually runs in.  fp16 operand halves overflow on an activation beyond 65504, and only the precision
// guard's probe (iss_cnn_probs) can see that happen: ISS_PREC_F16X3 takes them on patch networks whose parameters are inside
// fp16's range, every other network runs ISS_PREC_BF16X3 (the same MFMA count, f32's range).
static int effective_precision(const iss_ctx* c, const IssNet& n) {
    const int prec = n.prec_override >= 0 ? n.prec_override : c->precision;
    if (prec == ISS_PREC_F16X3 && !(n.f16_ok && n.d_wh16 != nullptr && net_reads_patches(n))) return ISS_PREC_BF16X3;
    return prec;
}

extern "C" int iss_cnn_precision_info(iss_ctx* c, int id, int32_t* mode, float* max_dlogp, int32_t* slots, int32_t* state, float* dlogp_in_use) {
    if (!c || id < 0 || id >= ISS_MAX_NETS) return ISS_EINVAL;
    const IssNet& n = c->nets[id];
    if (!n.loaded) return iss_fail(c, ISS_ESTATE, "net %d not loaded", id);
    if (mode) *mode = effective_precision(c, n);
    if (max_dlogp) *max_dlogp = n.guard_dlogp;
    if (slots) *slots = n.guard_slots;
    if (state) *state = n.guard_state;
    if (dlogp_in_use) *dlogp_in_use = n.guard_dlogp_chosen;
    return ISS_OK;
}

extern "C" int iss_set_diag(iss_ctx* c, uint32_t flags) {
    if (!c) return ISS_EINVAL;
    if (flags & ~(uint32_t)ISS_DIAG_ALL) return iss_fail(c, ISS_EINVAL, "iss_set_diag: unknown bits 0x%x", flags & ~(uint32_t)ISS_DIAG_ALL);
    c->diag = flags;
    return ISS_OK;
}

extern "C" int iss_cnn_flops(iss_ctx* c, int id, double* f) {
    if (!c || id < 0 || id >= ISS_MAX_NETS || !f) return ISS_EINVAL;
    if (!c->nets[id].loaded) return iss_fail(c, ISS_ESTATE, "net %d not loaded", id);
    *f = c->nets[id].flops_per_sample;
    return ISS_OK;
}

namespace {

// what a pass reads: PATCH / window mode (d_winrow + s0, stats, finite), else an NHWC batch
struct PassIo { const int32_t* d_winrow; const float* d_stats; const uint8_t* d_fin; const float* d_input; };

// ConvArgs of the launch `ch`: the geometry selection saw, and the pointers, tables and tile counts it did not look at
int conv_args(iss_ctx* c, IssNet& n, const PassIo& io, int bc, const ConvChoice& ch, ConvArgs& a) {
    const int r = ch.row;
    const int32_t* R = &n.prog[(size_t)r * ISS_PROG_COLS];
    memset(&a, 0, sizeof(a));
    fill_geometry(a, R, bc);
    a.in = R[ISS_C_IN] == ISS_BUF_INPUT ? io.d_input : (const float*)c->act[R[ISS_C_IN]].p;
    a.w = n.d_blob + R[ISS_C_WOFF];
    a.bias = R[ISS_C_BOFF] >= 0 ? n.d_blob + R[ISS_C_BOFF] : nullptr;
    a.ps = R[ISS_C_PSOFF] >= 0 ? n.d_blob + R[ISS_C_PSOFF] : nullptr;
    a.pt = R[ISS_C_PTOFF] >= 0 ? n.d_blob + R[ISS_C_PTOFF] : nullptr;
    a.res = R[ISS_C_RES] >= 0 ? (const float*)c->act[R[ISS_C_RES]].p : nullptr;
    a.out = (float*)c->act[R[ISS_C_OUT]].p;
    a.ktab = n.d_ktab + n.ktab_off[r];
    a.wh = n.d_wh + R[ISS_C_WOFF]; a.wl = n.d_wl + R[ISS_C_WOFF];
    a.Kpad = n.kpad[r]; a.mode = ch.inst.mode; a.tmr = ch.tmr;
    if (ch.inst.kernel == ConvKernel::Dhl) return ISS_OK;
    if (R[ISS_C_INMODE] == 1) {
        if (!io.d_winrow) return iss_fail(c, ISS_ESTATE, "patch-mode network run without a window list");
        a.in = (const float*)c->mspec.p; a.win_row = io.d_winrow; a.stats = io.d_stats; a.finite = io.d_fin;
    } else if (R[ISS_C_INMODE] == 2) {
        if (!io.d_winrow || !c->vbx_out.p) return iss_fail(c, ISS_ESTATE, "window-mode network run without resident vbx features");
        a.in = (const float*)c->vbx_out.p; a.win_row = io.d_winrow;
    } else if (!a.in) return iss_fail(c, ISS_ESTATE, "network input missing");
    a.nblk = (unsigned)((a.M + BM - 1) / BM);
    set_fast_div(a, 0, a.pp); set_fast_div(a, 1, a.pw); set_fast_div(a, 2, a.Hq * a.Wq); set_fast_div(a, 3, a.Wq);
#ifdef ISS_EXPERIMENTS
    { static const int dbg = getenv("ISS_DBG") ? atoi(getenv("ISS_DBG")) : 0; a.dbg = dbg; }     // timing-only experiment bits (never in a release build)
#endif
    a.nblk_n = (unsigned)((a.Cout + BN - 1) / BN);
    if (ch.inst.kernel == ConvKernel::Pwc) {
        const int32_t* Q = &n.prog[(size_t)ch.partner * ISS_PROG_COLS];
        a.wh2 = n.d_wh + Q[ISS_C_WOFF]; a.wl2 = n.d_wl + Q[ISS_C_WOFF];
        a.bias2 = Q[ISS_C_BOFF] >= 0 ? n.d_blob + Q[ISS_C_BOFF] : nullptr;
        a.out2 = (float*)c->act[Q[ISS_C_OUT]].p;
        a.act2 = Q[ISS_C_ACT]; a.Cout2 = Q[ISS_C_COUT];
    } else if (ch.inst.kernel == ConvKernel::Pws2Dual) {
        const int32_t* P = &n.prog[(size_t)ch.partner * ISS_PROG_COLS];
        a.in2 = P[ISS_C_IN] == ISS_BUF_INPUT ? io.d_input : (const float*)c->act[P[ISS_C_IN]].p;
        a.Cin2 = P[ISS_C_CIN]; a.H2 = P[ISS_C_H]; a.W2 = P[ISS_C_W]; a.sh2 = P[ISS_C_SH]; a.sw2 = P[ISS_C_SW];
        const int64_t wo = (int64_t)R[ISS_C_DUALW] - 1;
        a.w = n.d_blob + wo; a.wh = n.d_wh + wo; a.wl = n.d_wl + wo;
        a.bias = n.d_blob + (R[ISS_C_DUALB] - 1); a.res = nullptr;
        a.Kpad = a.Cin + a.Cin2;
    }
    if (ch.inst.f16) { a.f16 = 1; a.wh = n.d_wh16 + R[ISS_C_WOFF]; a.wl = n.d_wl16 + R[ISS_C_WOFF]; }       // fp16 operand halves
    if (ch.inst.kernel == ConvKernel::Wq3h) { a.in_hl = 1; a.in_np = ch.in_np; }
    if (ch.out != OutLayout::F32) { a.out_hl = 1; a.out_np = ch.out_np; a.out_f16 = ch.generic_out && ch.out_f16 ? 1 : 0; }
    return ISS_OK;
}

// The shared first layer `pend` of this pass, into c->raw1: the raw convolution once per log-mel row (zero-padded: the shared rows and
// the per-window edge rows behind them), its fused max-pool where it has one, and the second conv's arguments (ConvArgs::f_*, in,
// win_row) pointed at the result.  *fl gains the first layer's flops.
int launch_shared_first_layer(iss_ctx* c, IssNet& n, const PassIo& io, int pend, int bc, int rmin, int rmax, ConvArgs& a, double* fl) {
    const int32_t* R1 = &n.prog[(size_t)pend * ISS_PROG_COLS];
    const bool fs1 = R1[ISS_C_HO] == R1[ISS_C_H];                        // zero-padded ('same')
    int ph1, pw1;
    fused_pool_of(R1, ph1, pw1);
    const bool pool1 = ph1 * pw1 != 1;
    const long long rrows = (long long)(rmax - rmin) + R1[ISS_C_HO];     // R: rows rmin .. rmax + H1 - 1
    const long long rtot = rrows * R1[ISS_C_WO] * (R1[ISS_C_COUT] / 4);
    const int f_ne = fs1 ? R1[ISS_C_KH] - 1 : 0;                         // zero-padded first layer: edge rows per window
    const long long etot = (long long)bc * f_ne * R1[ISS_C_WO] * (R1[ISS_C_COUT] / 4);
    // pooled planes (ph1 of them) + the transformed window list behind R (see pool_rows_kernel)
    const int plane_rows = pool1 ? (int)(rrows / ph1) + 2 : 0;
    const long long ptot = pool1 ? (long long)ph1 * plane_rows * (R1[ISS_C_WO] / pw1) * (R1[ISS_C_COUT] / 4) : 0;
    { const int rc = iss_reserve(c, c->raw1, (size_t)(rtot + etot + ptot) * 16 + (pool1 ? (size_t)bc * 4 + 16 : 0)); if (rc) return rc; }
    float* Rraw = (float*)c->raw1.p;
    const float* mspec = (const float*)c->mspec.p;
    const float* w1 = n.d_blob + R1[ISS_C_WOFF];
    const size_t lds1 = (size_t)R1[ISS_C_KH] * R1[ISS_C_KW] * R1[ISS_C_COUT] * 4;
    iss_prof_begin(c, 2, 0);
    if (fs1) {
        // shared rows (all filter rows, the filter columns that see data) + the per-window edge rows behind them
        const int pt1 = R1[ISS_C_PT], pl1 = R1[ISS_C_PL], pb1 = R1[ISS_C_KH] - 1 - pt1;
        const float* S = n.d_wsum + n.wsumx_off[pend];
        if (rtot >= (1ll << 31) || etot >= (1ll << 31)) return iss_fail(c, ISS_EINVAL, "internal: shared first layer over %lld + %lld items", rtot, etot);
        hipLaunchKernelGGL(first_layer_same_kernel, dim3((unsigned)std::min<long long>((rtot + 255) / 256, 4096)), dim3(256), lds1, c->stream,
                           mspec, (int)c->T, rmin, rtot, R1[ISS_C_WO], R1[ISS_C_COUT], R1[ISS_C_KH], R1[ISS_C_KW], pt1, pl1, w1, n.kpad[pend], Rraw);
        if (etot > 0)
            hipLaunchKernelGGL(first_layer_edge_kernel, dim3((unsigned)std::min<long long>((etot + 255) / 256, 8192)), dim3(256), lds1, c->stream,
                               mspec, io.d_winrow, io.d_stats, etot, R1[ISS_C_H], R1[ISS_C_WO], R1[ISS_C_COUT], R1[ISS_C_KH],
                               R1[ISS_C_KW], pt1, pb1, pl1, w1, n.kpad[pend], S, Rraw + (size_t)rtot * 4);
        a.f_padt = pt1; a.f_padb = pb1; a.f_erow0 = (int)rrows;
    } else {
        const dim3 rgrid((unsigned)std::min<long long>((rtot + 255) / 256, 4096));
        const bool no_rows = (c->diag & ISS_DIAG_NO_FLROWS) != 0;             // diagnostic: the per-output kernel
        // compiled for the two input widths of the reference's nets: 21 bands (smn / sm) -> 17 positions, 24 (gender) -> 20
        const bool rows_ok = !no_rows && R1[ISS_C_KH] == 4 && R1[ISS_C_KW] == 5 && (R1[ISS_C_WO] == 17 || R1[ISS_C_WO] == 20) &&
                             rrows * (R1[ISS_C_COUT] / 4) < (1ll << 31);
        const dim3 rowgrid((unsigned)std::min<long long>((rrows * (R1[ISS_C_COUT] / 4) + 255) / 256, 4096));
        if (rows_ok && R1[ISS_C_WO] == 17)
            hipLaunchKernelGGL((first_layer_rows_kernel<4, 5, 17>), rowgrid, dim3(256), lds1, c->stream, mspec, rmin, (int)rrows, R1[ISS_C_COUT], w1, n.kpad[pend], Rraw);
        else if (rows_ok)
            hipLaunchKernelGGL((first_layer_rows_kernel<4, 5, 20>), rowgrid, dim3(256), lds1, c->stream, mspec, rmin, (int)rrows, R1[ISS_C_COUT], w1, n.kpad[pend], Rraw);
        else if (R1[ISS_C_KH] == 4 && R1[ISS_C_KW] == 5)
            hipLaunchKernelGGL((first_layer_raw_kernel<4, 5>), rgrid, dim3(256), lds1, c->stream, mspec, rmin, rtot, R1[ISS_C_WO], R1[ISS_C_COUT], 4, 5, w1, n.kpad[pend], Rraw);
        else
            hipLaunchKernelGGL((first_layer_raw_kernel<0, 0>), rgrid, dim3(256), lds1, c->stream, mspec, rmin, rtot, R1[ISS_C_WO], R1[ISS_C_COUT],
                               R1[ISS_C_KH], R1[ISS_C_KW], w1, n.kpad[pend], Rraw);
    }
    a.in = Rraw; a.win_row = io.d_winrow; a.f_rmin = rmin;
    if (pool1) {
        if (ptot >= (1ll << 40)) return iss_fail(c, ISS_EINVAL, "internal: pooled first layer over %lld items", ptot);
        float* P = Rraw + (size_t)(rtot + etot) * 4;
        int32_t* wr2 = reinterpret_cast<int32_t*>(P + (size_t)ptot * 4);
        hipLaunchKernelGGL(pool_rows_kernel, dim3((unsigned)std::min<long long>((ptot + 255) / 256, 8192)), dim3(256), 0, c->stream,
                           (const float*)Rraw, P, ptot, (int)rrows, R1[ISS_C_WO], R1[ISS_C_COUT], ph1, pw1, plane_rows);
        hipLaunchKernelGGL(winrow_pool_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, c->stream, io.d_winrow, wr2, bc, rmin, ph1, plane_rows);
        a.in = P; a.win_row = wr2; a.f_rmin = 0;
    }
    iss_prof_end(c);
    a.stats = io.d_stats; a.finite = io.d_fin;
    a.f_bias = n.d_blob + R1[ISS_C_BOFF];
    a.f_wsum = fs1 ? n.d_wsum + n.wsumx_off[pend] : n.d_wsum + n.wsum_off[pend];
    a.f_ps = R1[ISS_C_PSOFF] >= 0 ? n.d_blob + R1[ISS_C_PSOFF] : nullptr;
    a.f_pt = R1[ISS_C_PTOFF] >= 0 ? n.d_blob + R1[ISS_C_PTOFF] : nullptr;
    a.f_act = R1[ISS_C_ACT];
    *fl += 2.0 * R1[ISS_C_KH] * R1[ISS_C_KW] * (double)R1[ISS_C_COUT] * (double)bc * R1[ISS_C_HO] * R1[ISS_C_WO];
    return ISS_OK;
}

// The instantiations this unit holds itself, keyed like every launcher (conv_common.h ISS_LAUNCH_IF): the branch whose template
// arguments equal `i` runs, and a launcher without one says so.
bool launch_direct1(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t st, const ConvInst& i) {
#define ISS_DIRECT1_TRY(WINDOW_) ISS_LAUNCH_IF(i.kernel == ConvKernel::Direct1 && i.window == WINDOW_, conv1_direct3x3_kernel<WINDOW_>, grid, 256, lds)
    ISS_DIRECT1_TRY(true)
    ISS_DIRECT1_TRY(false)
#undef ISS_DIRECT1_TRY
    return false;
}
bool launch_patch1(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_PATCH1_TRY(TR_, F16_) \
    ISS_LAUNCH_IF(i.kernel == ConvKernel::Patch1 && i.tr == TR_ && i.f16 == F16_, (conv1_patch_x3_kernel<TR_, F16_>), grid, 256, 0)
    ISS_PATCH1_TRY(true, true)
    ISS_PATCH1_TRY(true, false)
    ISS_PATCH1_TRY(false, true)
    ISS_PATCH1_TRY(false, false)
#undef ISS_PATCH1_TRY
    return false;
}
// conv_x3_kernel is instantiated with NTN = 2 (64-column tiles) only: with the XCD-aware order the A tile is re-read from L2, not from
// HBM, and NTN = 4 (128 x 128 tiles: fewer, fatter workgroups) measured 6 % SLOWER on ResNet-101.  The template still takes NTN = 4 / 8,
// but nothing instantiates them: the device code holds the nine <MODE, TR, 2> kernels below and no other.
constexpr int X3_NTN = 2;
bool launch_x3(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_X3_TRY(MODE_, TR_)                                                                                                      \
    ISS_LAUNCH_IF((i.kernel == ConvKernel::X3 || i.kernel == ConvKernel::Gather) && i.mode == MODE_ && i.tr == TR_, \
                  (conv_x3_kernel<MODE_, TR_, X3_NTN>), grid, 256, 0)
    ISS_X3_TRY(4, true)
    ISS_X3_TRY(4, false)
    ISS_X3_TRY(3, true)
    ISS_X3_TRY(3, false)
    ISS_X3_TRY(0, true)
    ISS_X3_TRY(0, false)
    ISS_X3_TRY(1, true)
    ISS_X3_TRY(1, false)
    ISS_X3_TRY(2, false)
#undef ISS_X3_TRY
    return false;
}
bool launch_pw(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_PW_TRY(F16_) ISS_LAUNCH_IF(i.kernel == ConvKernel::Pw && i.f16 == F16_, conv_x3_pw_kernel<F16_>, grid, 256, 0)
    ISS_PW_TRY(true)
    ISS_PW_TRY(false)
#undef ISS_PW_TRY
    return false;
}
bool launch_igemm(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_IGEMM_TRY(MODE_) ISS_LAUNCH_IF(i.kernel == ConvKernel::Igemm && i.mode == MODE_, conv_igemm_kernel<MODE_>, grid, 256, 0)
    ISS_IGEMM_TRY(0)
    ISS_IGEMM_TRY(1)
    ISS_IGEMM_TRY(2)
#undef ISS_IGEMM_TRY
    return false;
}

// One launch, as selected: per kernel family its grid and its launcher, which gets the instantiation (ch.inst) and nothing else to pick
// a template argument by.  A launcher that holds no such instantiation launches nothing and returns false: an error, not another kernel.
int launch_conv(iss_ctx* c, IssNet& n, const ConvChoice& ch, ConvArgs& a, double fl) {
    const int r = ch.row;
    const int32_t* R = &n.prog[(size_t)r * ISS_PROG_COLS];
    const ConvInst& i = ch.inst;
    hipStream_t st = c->stream;
    const dim3 grid(a.nblk, a.nblk_n);
    const unsigned ny = (unsigned)std::max(1, a.Cout / (2 * BN));                                             // NH = 2: column pairs
    const unsigned tiles = (unsigned)((a.M + WS_TM - 1) / WS_TM);                                             // 512-row tiles
    const unsigned groups = (unsigned)((a.M + (long long)WS_TM * WS_G - 1) / ((long long)WS_TM * WS_G));      // ... and groups of WS_G of them
    const unsigned qtiles = ch.tmr > 0 ? (unsigned)((a.M + ch.tmr - 1) / ch.tmr) : 0;                         // tiles of tmr rows
    const dim3 nh2grid(std::min<unsigned>(tiles, std::max(1u, 256u / ny)), ny);                               // NH = 2: one 512-row tile per group
    const dim3 wgrid(std::min<unsigned>(groups, 256u), grid.y);                                               // persistent: one 512-thread workgroup per CU
    bool ok = false;
    iss_prof_begin(c, 0, fl);
    iss_prof_tag(c, ch.tag), iss_prof_row(c, r), iss_prof_inst(c, "%s", inst_name(i).c_str());
    switch (i.kernel) {
    case ConvKernel::Dhl: {
        const int K = R[ISS_C_CIN];
        uint16_t*& wp = n.dhl_wp[{r, i.f16 ? 1 : 0}];
        if (!wp) {
            ISS_HIP(c, hipMalloc((void**)&wp, dhl_packed_elems(K, R[ISS_C_COUT]) * 2));
            iss_dhl_pack((i.f16 ? n.d_wh16 : n.d_wh) + R[ISS_C_WOFF], (i.f16 ? n.d_wl16 : n.d_wl) + R[ISS_C_WOFF], wp, R[ISS_C_COUT], n.kpad[r], K, st);
        }
        DhlArgs d;
        d.a = reinterpret_cast<const uint16_t*>(a.in); d.wp = wp; d.bias = a.bias; d.out = a.out;
        d.np = ch.in_np; d.M = (int)a.M; d.K = K; d.Cout = R[ISS_C_COUT]; d.act = R[ISS_C_ACT];       // (a dense row: one GEMM row per window)
        ok = iss_dhl_launch(d, st, i);
        break;
    }
    case ConvKernel::Pwc: ok = iss_pwc_launch(a, st, i); break;
    case ConvKernel::Pws2Dual: case ConvKernel::Pws2Strided: case ConvKernel::Pws2: ok = iss_pws2_launch(a, st, i); break;
    case ConvKernel::Direct1: {
        const long long items = (long long)(a.M / ((long long)a.H * a.W)) * ((a.H + 7) / 8) * a.W * (a.Cout / 4);
        if (items >= (1ll << 32)) return iss_fail(c, ISS_EINVAL, "internal: direct first layer over %lld work items", items);
        ok = launch_direct1(a, dim3((unsigned)std::min<long long>((items + 255) / 256, 8192)), (size_t)9 * a.Cout * sizeof(float), st, i);
        break;
    }
    case ConvKernel::WsNh2F32: ok = iss_ws_launch_f32_nh2_3x3(a, nh2grid, st, i); break;
    case ConvKernel::WsNh2: ok = iss_ws_launch_nh2_3x3(a, nh2grid, st, i); break;
    case ConvKernel::Wq3: ok = iss_wq3_launch(a, dim3(std::min<unsigned>((qtiles + 1) / 2, std::max(1u, 256u / ny)), ny), st, i); break;
    case ConvKernel::Wq3h: ok = iss_wq3h_launch(a, dim3(std::min<unsigned>((qtiles + 1) / 2, std::max(1u, 256u / ny)), ny), st, i); break;
    case ConvKernel::WsPlainU: case ConvKernel::WsPlain: {
        const dim3 pgrid(std::min<unsigned>(groups, std::max(1u, 256u / grid.y)), grid.y);                    // one 512-thread workgroup per CU in total
        ok = iss_ws_launch_plain_3x3(a, pgrid, st, i);
        break;
    }
    case ConvKernel::WsF32Fused: ok = iss_ws_launch_f32_fused_5x3(a, wgrid, st, i); break;
    case ConvKernel::WsRing: ok = iss_ws_launch_ring(a, dim3(std::min<unsigned>(qtiles, 256u), grid.y), st, i); break;   // one tile of tmr rows per group
    case ConvKernel::WsFs: ok = iss_ws_launch_fs(a, dim3(std::min<unsigned>(tiles, 256u), grid.y), st, i); break;        // FS: one tile per group (conv_ws.h G)
    case ConvKernel::WsNcb1: ok = iss_ws_launch_ncb1_5x3(a, wgrid, st, i); break;
    case ConvKernel::Wq: ok = iss_wq_launch_5x3(a, dim3(std::min<unsigned>((qtiles + 1) / 2, 256u), grid.y), st, i); break;   // persistent: one 256-thread workgroup per CU
    case ConvKernel::Ws:
#define ISS_WS_CASE(KH_, KW_) if (i.kh == KH_ && i.kw == KW_) ok = iss_ws_launch_##KH_##x##KW_(a, wgrid, st, i);
        ISS_WS_SHAPES(ISS_WS_CASE)
#undef ISS_WS_CASE
        break;
    case ConvKernel::Fp: {
        const dim3 pgrid(std::min<unsigned>(a.nblk, 512u), grid.y / i.nh);     // persistent: 2 workgroups per CU
#define ISS_FP_CASE(KH_, KW_) if (i.kh == KH_ && i.kw == KW_) ok = iss_fp_launch_##KH_##x##KW_(a, pgrid, st, i);
        ISS_FP_SHAPES(ISS_FP_CASE)
#undef ISS_FP_CASE
        break;
    }
    // persistent, no barriers: 2 workgroups per CU (blob offsets are multiples of 8 floats, so the float4 loads of bias / scale / shift are aligned)
    case ConvKernel::Patch1: ok = launch_patch1(a, dim3(std::min<unsigned>(a.nblk, 512u), grid.y), st, i); break;
    case ConvKernel::Gather: case ConvKernel::X3:        // A staged once per 32 X3_NTN output channels; 1-D XCD-aware grid
        a.nblk_n = (unsigned)((a.Cout + 32 * X3_NTN - 1) / (32 * X3_NTN));
        ok = launch_x3(a, dim3(a.nblk * a.nblk_n), st, i);
        break;
    case ConvKernel::Pws: ok = iss_pws_launch(a, dim3(std::min<unsigned>(a.nblk * a.nblk_n, 512u)), st, i); break;
    case ConvKernel::Pw: ok = launch_pw(a, dim3(std::min<unsigned>(a.nblk * a.nblk_n, 768u)), st, i); break;
    case ConvKernel::Igemm: ok = launch_igemm(a, dim3(a.nblk * a.nblk_n), st, i); break;      // generic kernels: 1-D, XCD-aware (gemm_tile_of_block)
    case ConvKernel::Declined: return iss_fail(c, ISS_EINVAL, "internal: row %d has no kernel", r);
    }
    if (!ok) return iss_fail(c, ISS_EINVAL, "internal: %s is not compiled", inst_name(i).c_str());
    iss_prof_end(c);
    return ISS_OK;
}

// One selected launch with what goes in front of it: its arguments, the shared first layer where a kernel reads it, the launch.
int run_conv(iss_ctx* c, IssNet& n, const ConvEnv& env, const PassIo& io, const ConvChoice& ch, int pend) {
    const int32_t* R = &n.prog[(size_t)ch.row * ISS_PROG_COLS];
    ConvArgs a;
    int rc = conv_args(c, n, io, env.bc, ch, a);
    if (rc) return rc;
    double fl = conv_flops(R, (double)a.M);
    if (ch.inst.kernel == ConvKernel::Dhl) fl = 2.0 * R[ISS_C_CIN] * (double)R[ISS_C_COUT] * (double)env.bc;
    if (ch.inst.kernel == ConvKernel::Pwc) fl += 2.0 * a.Cout * (double)a.Cout2 * (double)a.M;
    if (ch.inst.kernel == ConvKernel::Pws2Dual) fl += 2.0 * a.Cin2 * (double)a.Cout * (double)a.M;
    if (ch.first == FirstLayer::Fused || ch.first == FirstLayer::Gather)
        if ((rc = launch_shared_first_layer(c, n, io, pend, env.bc, env.rmin, env.rmax, a, &fl))) return rc;
    return launch_conv(c, n, ch, a, fl);
}

// Run the op program on `bc` samples.  src: PATCH mode uses (d_winrow + s0, stats, finite),
// otherwise `d_input` is an NHWC batch.  The result is left in act[last OUT].  [rmin, rmax] = range of the window rows
// of this call; share_first: the caller's (chunking-independent) decision to use the shared first layer.
int run_program(iss_ctx* c, IssNet& n, int bc, const int32_t* d_winrow, const float* d_stats,
                const uint8_t* d_fin, const float* d_input, float** result, int rmin = 0, int rmax = -1,
                bool share_first = false) {
    const PassIo io{d_winrow, d_stats, d_fin, d_input};
    // ---- CHL hand-over between footprint kernels (conv_common.h, round 6): per activation buffer, whether the tensor in it is in
    // the CHL layout.  A producer writes CHL only when the NEXT row is the tensor's only reader and runs on conv_x3_wq3h_kernel
    // (want_hl_out / want_dhl_out, conv_select.h).  effective_precision: one network may run another mode (precision guard)
    std::vector<ChlState> layout(std::max<size_t>(c->act.size(), (size_t)n.nbuf));
    ConvEnv env = make_env(n, bc, rmin, rmax, share_first, effective_precision(c, n), c->diag, d_winrow != nullptr, d_input != nullptr,
                           c->vbx_out.p != nullptr, layout.data());
    int pending = -1;                                            // deferred PATCH first layer (see can_defer)
    for (int r = 0; r < n.nrows; ++r) {
        const int32_t* R = &n.prog[(size_t)r * ISS_PROG_COLS];
        const float* in = R[ISS_C_IN] == ISS_BUF_INPUT ? d_input : (const float*)c->act[R[ISS_C_IN]].p;
        float* out = (float*)c->act[R[ISS_C_OUT]].p;
        const int op = R[ISS_C_OP];
        ChlState out_layout;                                     // of this row's output: f32 unless a conv launch says otherwise
        if (op == ISS_OP_CONV) {
            if (pending < 0 && can_defer(env, r)) { pending = r; *result = out; continue; }
            const ConvChoice ch = select_conv(env, r, pending);
            int rc = ISS_OK;
            if (ch.first == FirstLayer::Alone) rc = run_conv(c, n, env, io, select_row(env, pending, -1, -1, -1), -1);   // (nothing fuses it after all)
            if (!rc) rc = run_conv(c, n, env, io, ch, pending);
            if (pending >= 0) layout[n.prog[(size_t)pending * ISS_PROG_COLS + ISS_C_OUT]] = ChlState{};
            pending = -1;
            if (rc) return rc;
            if (ch.rows == 1 && env.layout_of(R[ISS_C_IN]).np && !ch.in_np)
                return iss_fail(c, ISS_EINVAL, "internal: row %d reads a CHL tensor on a kernel that expects f32", r);
            if (ch.rows == 2) {                                  // the chained pair / the two-source launch: rows r and r + 1 are done
                layout[R[ISS_C_OUT]] = ChlState{};
                R = &n.prog[(size_t)++r * ISS_PROG_COLS];
                out = (float*)c->act[R[ISS_C_OUT]].p;
            }
            if (ch.out != OutLayout::F32) out_layout = ChlState{ch.out_np, ch.out_f16, ch.out == OutLayout::ChlDense};
        } else if (op == ISS_OP_POOL) {
            const long long total = (long long)bc * R[ISS_C_HO] * R[ISS_C_WO] * R[ISS_C_CIN];
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, in, out,
                               total, R[ISS_C_H], R[ISS_C_W], R[ISS_C_CIN], R[ISS_C_HO], R[ISS_C_WO], R[ISS_C_KH],
                               R[ISS_C_KW], R[ISS_C_SH], R[ISS_C_SW], R[ISS_C_PT], R[ISS_C_PL], R[ISS_C_POOLKIND]);
            iss_prof_end(c);
        } else if (op == ISS_OP_SOFTMAX) {
            const long long rows = (long long)bc * R[ISS_C_H] * R[ISS_C_W];
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(softmax_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, in, out,
                               rows, R[ISS_C_CIN]);
            iss_prof_end(c);
        } else if (op == ISS_OP_ACT) {
            const long long total = (long long)bc * R[ISS_C_H] * R[ISS_C_W] * R[ISS_C_CIN];
            float alpha, p2, p3;
            { const int32_t bits = R[ISS_C_ACTPARAM]; memcpy(&alpha, &bits, sizeof(float)); }
            { const int32_t bits = R[ISS_C_ACTPARAM2]; memcpy(&p2, &bits, sizeof(float)); }
            { const int32_t bits = R[ISS_C_ACTPARAM3]; memcpy(&p3, &bits, sizeof(float)); }
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(act_kernel, dim3((unsigned)std::min<long long>((total + 1023) / 1024, 1 << 20)), dim3(256), 0, c->stream, in, out, total,
                               R[ISS_C_ACT], alpha, p2, p3);
            iss_prof_end(c);
        } else if (op == ISS_OP_ELT) {
            const int k = R[ISS_C_ACT];
            const long long hw = (long long)R[ISS_C_H] * R[ISS_C_W];
            const bool chan = k == ISS_ELT_COPY || k == ISS_ELT_ZERO;
            const long long total = (long long)bc * hw * (chan ? R[ISS_C_KH] : R[ISS_C_CIN]);
            const float* res = R[ISS_C_RES] >= 0 ? (const float*)c->act[R[ISS_C_RES]].p : nullptr;
            if (res && layout[R[ISS_C_RES]].np) return iss_fail(c, ISS_EINVAL, "internal: row %d reads a CHL tensor", r);
            int st[3] = {0, 0, 0};
            if (k == ISS_ELT_PERMUTE) {
                const int sin[3] = {R[ISS_C_W] * R[ISS_C_CIN], R[ISS_C_CIN], 1};
                st[0] = sin[R[ISS_C_KH]]; st[1] = sin[R[ISS_C_KW]]; st[2] = sin[R[ISS_C_SH]];
            }
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(elt_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 1 << 20)), dim3(256), 0, c->stream, in, res, out,
                               total, k, R[ISS_C_CIN], R[ISS_C_COUT], R[ISS_C_KH], R[ISS_C_PT], R[ISS_C_PL],
                               R[ISS_C_HO], R[ISS_C_WO], R[ISS_C_COUT], st[0], st[1], st[2], R[ISS_C_ORDER] == 1 ? 1 : 0);
            iss_prof_end(c);
        } else if (op == ISS_OP_STATPOOL) {
            const long long total = (long long)bc * R[ISS_C_H] * R[ISS_C_CIN];
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(statpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, in, out,
                               total, R[ISS_C_H], R[ISS_C_W], R[ISS_C_CIN]);
            iss_prof_end(c);
        }
        ISS_HIP(c, hipGetLastError());
        *result = out;
        layout[R[ISS_C_OUT]] = out_layout;
        if (op != ISS_OP_CONV && R[ISS_C_IN] != ISS_BUF_INPUT && layout[R[ISS_C_IN]].np)
            return iss_fail(c, ISS_EINVAL, "internal: row %d reads a CHL tensor", r);
    }
    return ISS_OK;
}

int plan_chunk(iss_ctx* c, IssNet& n, int total, int* bc_out) {
    int64_t per = 0;
    for (auto e : n.buf_elems) per += e;
    int64_t bc = (int64_t)(c->ws_limit / (uint64_t)(per * sizeof(float)));
    if (bc < 1) bc = 1;
    if (bc > total) bc = total;
    // keep every per-buffer float index below 2^31: several kernels form element offsets in 32 bits (first_layer_raw_kernel's
    // `(unsigned)total`, the footprint kernels' row * Cout offsets), whatever workspace limit the caller has set
    int64_t emax = 1;
    for (auto e : n.buf_elems) emax = std::max<int64_t>(emax, e);
    bc = std::min<int64_t>(bc, ((1ll << 31) - 1) / emax);
    if (bc < 1) return iss_fail(c, ISS_EINVAL, "network activation of %lld floats per sample exceeds the 2^31 element limit", (long long)emax);
    if (bc > 8) bc -= bc % 8;
    if ((int)c->act.size() < n.nbuf) c->act.resize(n.nbuf);
    for (int i = 0; i < n.nbuf; ++i) {
        int rc = iss_reserve(c, c->act[i], (size_t)bc * n.buf_elems[i] * sizeof(float) + issk::ISS_ACT_SLACK);
        if (rc) return rc;
    }
    *bc_out = (int)bc;
    return ISS_OK;
}

}  // namespace

static int cnn_probs_impl(iss_ctx* c, int id, const int32_t* win_row, int32_t nslots, float* probs_out,
                          uint8_t* finite_out, bool async, int64_t* ticket_out);

// Precision guard (include/iss.h): the network's first call in split-bf16 mode.  Up to 256 of the call's windows -- four runs of
// consecutive slots at the quarters of the list, so that each run takes the kernels the call itself will take (the shared first
// layer needs overlapping windows) -- are evaluated in both arithmetic modes; max |d log p| decides.
static int precision_guard(iss_ctx* c, int id, const int32_t* win_row, int32_t nslots) {
    IssNet& n = c->nets[id];
    const int eff = effective_precision(c, n);
    if (eff == ISS_PREC_F32) { n.guard_state = ISS_GUARD_FIXED; return ISS_OK; }
    if (!(c->guard_threshold > 0.f)) return ISS_OK;               // guard off: stays pending
    const int runs = nslots >= 256 ? 4 : 1, per = nslots >= 256 ? 64 : nslots;
    const size_t od = (size_t)n.out_dim;
    std::vector<float> pref((size_t)runs * per * od), pm((size_t)per * od);
    std::vector<uint8_t> fref((size_t)runs * per), fm(per);
    auto window_run = [&](int r) { return win_row + (runs == 1 ? 0 : (size_t)r * (nslots - per) / (runs - 1)); };
    int rc = ISS_OK, compared = 0;
    // max |log p_mode - log p_f32| over every class of every finite window (non-finite ones carry the constant 0.5, segmenter.py:175);
    // a NaN (an activation beyond fp16's range) counts as a failure; classes below 1e-30 in either mode are skipped
    auto probe = [&](int mode, double& worst) {
        worst = 0.0; compared = 0;
        for (int r = 0; r < runs && rc == ISS_OK; ++r) {
            n.prec_override = mode;
            rc = cnn_probs_impl(c, id, window_run(r), per, pm.data(), fm.data(), false, nullptr);
            if (rc != ISS_OK) return;
            for (int i = 0; i < per; ++i) {
                if (!fm[i] || !fref[(size_t)r * per + i]) continue;
                ++compared;
                for (size_t k = 0; k < od; ++k) {
                    const float a = pm[(size_t)i * od + k], b = pref[((size_t)r * per + i) * od + k];
                    if (!(a == a)) { worst = 1e30; continue; }
                    if (!(a > 1e-30f) || !(b > 1e-30f)) continue;      // (an underflowing class: a real disagreement shows in the window's other classes)
                    worst = std::max(worst, std::fabs(std::log((double)a) - std::log((double)b)));
                }
            }
        }
    };
    c->in_guard = true;
    for (int r = 0; r < runs && rc == ISS_OK; ++r) {              // the reference: exact f32
        n.prec_override = ISS_PREC_F32;
        rc = cnn_probs_impl(c, id, window_run(r), per, pref.data() + (size_t)r * per * od, fref.data() + (size_t)r * per, false, nullptr);
    }
    double worst = 0.0;
    int chosen = eff;
    if (rc == ISS_OK) probe(eff, worst);
    const double first = worst;
    if (rc == ISS_OK && worst > (double)c->guard_threshold) {
        chosen = ISS_PREC_F32;
        // the other split mode first (the same speed as the one that failed): fp16 halves where bf16 ones are too coarse, bf16 halves
        // where an activation left fp16's range
        const int other = eff == ISS_PREC_BF16X3 ? ISS_PREC_F16X3 : ISS_PREC_BF16X3;
        if (other == ISS_PREC_BF16X3 || n.f16_ok) {
            double w2 = 0.0;
            probe(other, w2);
            if (rc == ISS_OK && w2 <= (double)c->guard_threshold) { chosen = other; worst = w2; }
        }
    }
    c->in_guard = false;
    n.prec_override = -1;
    if (rc != ISS_OK) return rc;
    if (compared == 0) { n.guard_slots = 0; return ISS_OK; }    // no window finite in both modes: no evidence, stays pending (the next call probes)
    n.guard_dlogp = (float)std::min(first, 1e30); n.guard_slots = compared;
    n.guard_dlogp_chosen = chosen == eff ? n.guard_dlogp : (chosen == ISS_PREC_F32 ? 0.f : (float)worst);
    if (chosen != eff) { n.prec_override = chosen; n.guard_state = ISS_GUARD_ESCALATED; }
    else n.guard_state = ISS_GUARD_PASSED;
    return ISS_OK;
}

// The row flags of the resident features (row_flags_kernel) and their copy to the host, on the stream; no wait.  iss_sidekit puts
// them right behind its feature kernel, so that the one wait of iss_get_loge brings them along with the log-energy.
int iss_enqueue_row_flags(iss_ctx* c) {
    if (c->T <= 0) return ISS_OK;
    int rc;
    if ((rc = iss_reserve(c, c->d_rowflag, (size_t)c->T))) return rc;
    if ((rc = iss_rowflag_host(c, (size_t)c->T))) return rc;
    iss_prof_begin(c, 2, 0);
    hipLaunchKernelGGL(row_flags_kernel, dim3((c->T + 255) / 256), dim3(256), 0, c->stream, (const float*)c->mspec.p, (int)c->T,
                       (uint8_t*)c->d_rowflag.p);
    iss_prof_end(c);
    ISS_HIP(c, hipGetLastError());
    ISS_HIP(c, hipMemcpyAsync(c->h_rowflag, c->d_rowflag.p, (size_t)c->T, hipMemcpyDeviceToHost, c->stream));
    return ISS_OK;
}

// The row flags on the host: already there when the features came from iss_sidekit and iss_get_loge has waited since (or from
// iss_set_mspec, which scans its argument); else one short wait at the first call after the features changed -- for the flags
// iss_sidekit queued, when the caller has not waited through iss_get_loge, or for flags computed here.
static int ensure_row_flags(iss_ctx* c) {
    if (c->flags_epoch == c->feat_epoch) return ISS_OK;
    int rc;
    if (c->flags_queued != c->feat_epoch && (rc = iss_enqueue_row_flags(c))) return rc;
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    c->bad_prefix.clear();
    c->flags_epoch = c->feat_epoch;
    return ISS_OK;
}

// Are the `bytes` at p page-locked host memory?  A device-to-host hipMemcpyAsync into pageable memory holds the submitting thread
// until the copy has run, so copies between the passes of a call would serialise its submission with its execution.
static bool host_pinned(const void* p, size_t bytes) {
    for (const char* q : {(const char*)p, (const char*)p + (bytes ? bytes - 1 : 0)}) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// P[t] = rows below t with a non-finite value in their first w columns: the window at row r is dead iff P[r + 68] != P[r]
static const std::vector<int32_t>& bad_prefix(iss_ctx* c, int w) {
    std::vector<int32_t>& P = c->bad_prefix[w];
    if (P.size() != (size_t)c->T + 1) {
        P.resize((size_t)c->T + 1);
        P[0] = 0;
        for (int32_t t = 0; t < c->T; ++t) P[t + 1] = P[t] + (c->h_rowflag[t] < w ? 1 : 0);
    }
    return P;
}

extern "C" int iss_cnn_dead_stats(iss_ctx* c, int64_t* windows, int64_t* dead) {
    if (!c) return ISS_EINVAL;
    if (windows) *windows = c->win_total;
    if (dead) *dead = c->win_dead;
    return ISS_OK;
}

static int cnn_probs_impl(iss_ctx* c, int id, const int32_t* win_row, int32_t nslots, float* probs_out,
                          uint8_t* finite_out, bool async, int64_t* ticket_out) {
    if (!c) return ISS_EINVAL;
    if (ticket_out) *ticket_out = -1;
    if (id < 0 || id >= ISS_MAX_NETS || nslots < 0 || (nslots > 0 && (!win_row || !probs_out || !finite_out)))
        return iss_fail(c, ISS_EINVAL, "iss_cnn_probs: bad argument");
    IssNet& n = c->nets[id];
    if (!n.loaded) return iss_fail(c, ISS_ESTATE, "iss_cnn_probs: net %d not loaded", id);
    if (!c->have_feats) return iss_fail(c, ISS_ESTATE, "iss_cnn_probs: no mel spectrogram resident");
    if (n.in_h != 68 || n.in_c != 1 || n.in_w > 24) return iss_fail(c, ISS_EINVAL, "net %d is not a (68,h,1) patch network", id);
    if (nslots == 0) return ISS_OK;
    for (int i = 0; i < nslots; ++i)
        if (win_row[i] < 0 || win_row[i] + 68 > c->T)
            return iss_fail(c, ISS_EINVAL, "iss_cnn_probs: window %d (row %d) outside the %d resident frames", i, win_row[i], c->T);
    ISS_HIP(c, hipSetDevice(c->device));
    int rc;
    // Dead windows -- a non-finite log-mel value inside (digital silence: whole -inf rows) -- come back as 0.5 / not finite whatever
    // the network computes, so they are left out of the passes: a pure function of (features, list, width).  `lm` = the live
    // windows' rows, then their slots; empty when no window is dead, and the call then runs exactly as without this step.
    // Windows of finite values that do not normalise (std = 0, overflow) stay in: the device's flag decides them as before.
    std::vector<int32_t> lm;
    int nlive = nslots;
    if (!(c->diag & ISS_DIAG_NO_SKIP_DEAD)) {
        if ((rc = ensure_row_flags(c))) return rc;
        const std::vector<int32_t>& P = bad_prefix(c, n.in_w);
        int dead = 0;
        for (int i = 0; i < nslots; ++i) dead += P[win_row[i] + 68] != P[win_row[i]];
        if (dead) {
            nlive = nslots - dead;
            lm.resize(2 * (size_t)nlive);
            for (int i = 0, j = 0; i < nslots; ++i)
                if (P[win_row[i] + 68] == P[win_row[i]]) { lm[j] = win_row[i]; lm[(size_t)nlive + j] = i; ++j; }
        }
        if (!c->in_guard) c->win_dead += dead;
    }
    if (!c->in_guard) c->win_total += nslots;
    const bool compact = nlive < nslots;
    const int32_t* rows = compact ? lm.data() : win_row;          // the list the network runs on
    if (!c->in_guard && n.guard_state == ISS_GUARD_PENDING && nlive > 0 && (rc = precision_guard(c, id, rows, nlive))) return rc;
    const size_t nup = compact ? 2 * (size_t)nlive : (size_t)nslots;
    if ((rc = iss_reserve(c, c->d_winrow, (nup ? nup : 1) * 4))) return rc;
    if ((rc = iss_reserve(c, c->d_stats, (size_t)nslots * 8))) return rc;
    if ((rc = iss_reserve(c, c->d_finite, (size_t)nslots))) return rc;
    if (compact && (rc = iss_reserve(c, c->d_lfinite, (size_t)(nlive ? nlive : 1)))) return rc;
    if ((rc = iss_reserve(c, c->d_out, (size_t)nslots * n.out_dim * 4))) return rc;
    int bc = 0;
    if (nlive > 0 && (rc = plan_chunk(c, n, nlive, &bc))) return rc;
    // (the device buffers above are shared by calls in flight: one stream orders them, and iss_reserve waits before it frees)
    if (nup == 0) {                                  // every window is dead: nothing to upload, no CNN launch
    } else if (async || compact) {                   // the caller may reuse win_row as soon as we return, and lm ends with this call: stage (pinned)
        void* pinned; int slot;
        if ((rc = iss_stage_host(c, rows, nup * 4, &pinned, &slot))) return rc;
        ISS_HIP(c, hipMemcpyAsync(c->d_winrow.p, pinned, nup * 4, hipMemcpyHostToDevice, c->stream));
        iss_stage_mark(c, slot);
    } else {
        ISS_HIP(c, hipMemcpyAsync(c->d_winrow.p, win_row, (size_t)nslots * 4, hipMemcpyHostToDevice, c->stream));
    }
    const int32_t* d_map = (const int32_t*)c->d_winrow.p + nlive;
    uint8_t* d_fin = compact ? (uint8_t*)c->d_lfinite.p : (uint8_t*)c->d_finite.p;
    const long long tot = (long long)nslots * n.out_dim;
    // Landings (iss_internal.h, iss_ctx::Ticket): an asynchronous call with page-locked outputs stores every pass's rows straight
    // into the caller's arrays (scatter_probs_kernel; the arrays are device-visible) and records an event behind the pass, so that
    // the host can start on the front of the result while the later passes run (iss_wait_slots).  No copy follows a pass, and none
    // the call.  Every other call gathers its result on the device and copies it out once, behind its last pass.
    float* dev_probs = nullptr;
    uint8_t* dev_finite = nullptr;
    const bool per_pass = async && !c->in_guard &&
                          host_pinned(probs_out, (size_t)tot * 4) && host_pinned(finite_out, (size_t)nslots) &&
                          hipHostGetDevicePointer((void**)&dev_probs, probs_out, 0) == hipSuccess &&
                          hipHostGetDevicePointer((void**)&dev_finite, finite_out, 0) == hipSuccess;
    if (per_pass && compact) {                       // the dead slots, by the host: no kernel stores them
        for (int i = 0, j = 0; i < nslots; ++i) {
            if (j < nlive && lm[(size_t)nlive + j] == i) { ++j; continue; }
            for (int k = 0; k < n.out_dim; ++k) probs_out[(size_t)i * n.out_dim + k] = 0.5f;
            finite_out[i] = 0;
        }
    } else if (compact) {                            // the dead slots (the live ones are overwritten by the scatter)
        iss_prof_begin(c, 2, 0);
        hipLaunchKernelGGL(fill_half_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, (float*)c->d_out.p, tot);
        iss_prof_end(c);
        ISS_HIP(c, hipGetLastError());
        ISS_HIP(c, hipMemsetAsync(c->d_finite.p, 0, (size_t)nslots, c->stream));
    }
    if (nlive > 0) {
        iss_prof_begin(c, 2, 0);
        hipLaunchKernelGGL(patch_stats_kernel, dim3((nlive + 3) / 4), dim3(256), 0, c->stream, (const float*)c->mspec.p,
                           (const int32_t*)c->d_winrow.p, nlive, n.in_w, (float*)c->d_stats.p, d_fin);
        iss_prof_end(c);
        ISS_HIP(c, hipGetLastError());
    }
    // Shared first layer (ConvArgs::f_*): decided per call from the whole window list, not per chunk, so that the result
    // does not depend on the workspace limit: on when the windows overlap at least 4-fold on average.
    bool share = !(c->diag & ISS_DIAG_NO_SHARED_FIRST);
    if (nlive > 0) {
        int gmin = rows[0], gmax = rows[0];
        for (int i = 1; i < nlive; ++i) { gmin = std::min(gmin, rows[i]); gmax = std::max(gmax, rows[i]); }
        if ((long long)(gmax - gmin + 68) * 4 > (long long)nlive * 68) share = false;
    }
    iss_ctx::Ticket ticket;
    auto landing = [&](int32_t end) -> int {         // an asynchronous call's event: slots [0, end) are in the caller's arrays behind it
        if (!async) return ISS_OK;
        hipEvent_t ev;
        if (!c->ev_pool.empty()) { ev = c->ev_pool.back(); c->ev_pool.pop_back(); }
        else ISS_HIP(c, hipEventCreate(&ev));
        ticket.land.push_back({end, ev});            // (owned by the ticket from here on, whatever fails below)
        ISS_HIP(c, hipEventRecord(ev, c->stream));
        return ISS_OK;
    };
    auto give_back = [&]() { for (auto& l : ticket.land) c->ev_pool.push_back(l.ev); ticket.land.clear(); };
    for (int s0 = 0; s0 < nlive; s0 += bc) {
        const int cur = std::min(bc, nlive - s0);
        float* res = nullptr;
        int rmin = rows[s0], rmax = rows[s0];
        for (int i = s0 + 1; i < s0 + cur; ++i) { rmin = std::min(rmin, rows[i]); rmax = std::max(rmax, rows[i]); }
        rc = run_program(c, n, cur, (const int32_t*)c->d_winrow.p + s0, (const float*)c->d_stats.p + 2 * (size_t)s0,
                         (const uint8_t*)d_fin + s0, nullptr, &res, rmin, rmax, share);
        if (rc) { give_back(); return rc; }
        if (compact || per_pass) {
            // to the caller's slots: through the map of the live windows, or (no dead window) to slots [s0, s0 + cur); 0.5 where
            // the window did not normalise -- what mask_probs_kernel writes over the gathered result of the other calls
            const long long ct = (long long)cur * n.out_dim;
            float* out = per_pass ? dev_probs : (float*)c->d_out.p;
            uint8_t* fin = per_pass ? dev_finite : (uint8_t*)c->d_finite.p;
            iss_prof_begin(c, 2, 0);
            hipLaunchKernelGGL(scatter_probs_kernel, dim3((unsigned)((ct + 255) / 256)), dim3(256), 0, c->stream, (const float*)res,
                               (const uint8_t*)d_fin + s0, compact ? d_map + s0 : (const int32_t*)nullptr, (long long)cur, n.out_dim,
                               compact ? out : out + (size_t)s0 * n.out_dim, compact ? fin : fin + s0);
            iss_prof_end(c);
            if (hipGetLastError() != hipSuccess) { give_back(); return iss_fail(c, ISS_EHIP, "scatter_probs_kernel launch failed"); }
        } else {
            ISS_HIP(c, hipMemcpyAsync((float*)c->d_out.p + (size_t)s0 * n.out_dim, res, (size_t)cur * n.out_dim * 4,
                                      hipMemcpyDeviceToDevice, c->stream));
        }
        // a landing per pass: its own slots, and with dead windows in the list every slot up to the next live window's -- the dead
        // ones in between hold their 0.5 / 0 already
        if (per_pass && (rc = landing(s0 + cur >= nlive ? nslots : (compact ? lm[(size_t)nlive + s0 + cur] : s0 + cur)))) { give_back(); return rc; }
    }
    if (!per_pass) {                                 // gathered on the device: one copy behind the last pass, one landing
        if (!compact) {
            hipLaunchKernelGGL(mask_probs_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                               (float*)c->d_out.p, (const uint8_t*)c->d_finite.p, (long long)nslots, n.out_dim);
            ISS_HIP(c, hipGetLastError());
        }
        ISS_HIP(c, hipMemcpyAsync(probs_out, c->d_out.p, (size_t)tot * 4, hipMemcpyDeviceToHost, c->stream));
        ISS_HIP(c, hipMemcpyAsync(finite_out, c->d_finite.p, (size_t)nslots, hipMemcpyDeviceToHost, c->stream));
    }
    // (stored where it lands, and every window dead: no pass has recorded the landing of the slots the host wrote)
    if ((!per_pass || nlive == 0) && (rc = landing(nslots))) { give_back(); return rc; }
    if (async) {
        c->tickets.push_back(std::move(ticket));
        if (ticket_out) *ticket_out = c->ticket_base + (int64_t)c->tickets.size() - 1;
        return ISS_OK;
    }
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    iss_prof_collect(c);
    return ISS_OK;
}

extern "C" int iss_cnn_probs(iss_ctx* c, int id, const int32_t* win_row, int32_t nslots, float* probs_out,
                             uint8_t* finite_out) {
    return cnn_probs_impl(c, id, win_row, nslots, probs_out, finite_out, false, nullptr);
}

extern "C" int iss_cnn_probs_async(iss_ctx* c, int id, const int32_t* win_row, int32_t nslots, float* probs_out,
                                   uint8_t* finite_out, int64_t* ticket_out) {
    return cnn_probs_impl(c, id, win_row, nslots, probs_out, finite_out, true, ticket_out);
}

extern "C" int iss_cnn_forward(iss_ctx* c, int id, const float* x, int32_t nsamp, float* out) {
    if (!c) return ISS_EINVAL;
    if (id < 0 || id >= ISS_MAX_NETS || nsamp < 0 || (nsamp > 0 && (!x || !out)))
        return iss_fail(c, ISS_EINVAL, "iss_cnn_forward: bad argument");
    IssNet& n = c->nets[id];
    if (!n.loaded) return iss_fail(c, ISS_ESTATE, "iss_cnn_forward: net %d not loaded", id);
    if (net_reads_patches(n)) return iss_fail(c, ISS_EINVAL, "iss_cnn_forward: net %d reads mspec patches; use iss_cnn_probs", id);
    if (nsamp == 0) return ISS_OK;
    ISS_HIP(c, hipSetDevice(c->device));
    const size_t in_elems = (size_t)n.in_h * n.in_w * n.in_c;
    int rc, bc = 0;
    if ((rc = plan_chunk(c, n, nsamp, &bc))) return rc;
    if ((rc = iss_reserve(c, c->d_in, (size_t)bc * in_elems * 4))) return rc;
    if ((rc = iss_reserve(c, c->d_out, (size_t)nsamp * n.out_dim * 4))) return rc;
    for (int s0 = 0; s0 < nsamp; s0 += bc) {
        const int cur = std::min(bc, nsamp - s0);
        ISS_HIP(c, hipMemcpyAsync(c->d_in.p, x + (size_t)s0 * in_elems, (size_t)cur * in_elems * 4, hipMemcpyHostToDevice, c->stream));
        float* res = nullptr;
        rc = run_program(c, n, cur, nullptr, nullptr, nullptr, (const float*)c->d_in.p, &res);
        if (rc) return rc;
        ISS_HIP(c, hipMemcpyAsync((float*)c->d_out.p + (size_t)s0 * n.out_dim, res, (size_t)cur * n.out_dim * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    }
    ISS_HIP(c, hipMemcpyAsync(out, c->d_out.p, (size_t)nsamp * n.out_dim * 4, hipMemcpyDeviceToHost, c->stream));
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    iss_prof_collect(c);
    return ISS_OK;
}

extern "C" int iss_vbx_embed(iss_ctx* c, int id, const int32_t* starts, int32_t nwin, float* out) {
    if (!c) return ISS_EINVAL;
    if (id < 0 || id >= ISS_MAX_NETS || nwin < 0 || (nwin > 0 && (!starts || !out)))
        return iss_fail(c, ISS_EINVAL, "iss_vbx_embed: bad argument");
    IssNet& n = c->nets[id];
    if (!n.loaded) return iss_fail(c, ISS_ESTATE, "iss_vbx_embed: net %d not loaded", id);
    if (n.prog[ISS_C_OP] != ISS_OP_CONV || n.prog[ISS_C_INMODE] != 2)
        return iss_fail(c, ISS_EINVAL, "iss_vbx_embed: net %d does not start with a window-mode conv", id);
    if (c->vbx_T <= 0) return iss_fail(c, ISS_ESTATE, "iss_vbx_embed: no vbx features resident (iss_vbx_features*)");
    if (nwin == 0) return ISS_OK;
    for (int i = 0; i < nwin; ++i)
        if (starts[i] < 0 || starts[i] + n.in_w > c->vbx_T)
            return iss_fail(c, ISS_EINVAL, "iss_vbx_embed: window %d (frames %d..%d) outside the %d resident frames", i, starts[i],
                            starts[i] + n.in_w, c->vbx_T);
    ISS_HIP(c, hipSetDevice(c->device));
    int rc, bc = 0;
    if ((rc = iss_reserve(c, c->d_winrow, (size_t)nwin * 4))) return rc;
    if ((rc = iss_reserve(c, c->d_out, (size_t)nwin * n.out_dim * 4))) return rc;
    if ((rc = plan_chunk(c, n, nwin, &bc))) return rc;
    ISS_HIP(c, hipMemcpyAsync(c->d_winrow.p, starts, (size_t)nwin * 4, hipMemcpyHostToDevice, c->stream));
    for (int s0 = 0; s0 < nwin; s0 += bc) {
        const int cur = std::min(bc, nwin - s0);
        float* res = nullptr;
        rc = run_program(c, n, cur, (const int32_t*)c->d_winrow.p + s0, nullptr, nullptr, nullptr, &res);
        if (rc) return rc;
        ISS_HIP(c, hipMemcpyAsync((float*)c->d_out.p + (size_t)s0 * n.out_dim, res, (size_t)cur * n.out_dim * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    }
    ISS_HIP(c, hipMemcpyAsync(out, c->d_out.p, (size_t)nwin * n.out_dim * 4, hipMemcpyDeviceToHost, c->stream));
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    iss_prof_collect(c);
    return ISS_OK;
}
