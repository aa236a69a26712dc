// What conv_x3_ws_kernel (conv_ws.h), conv_x3_wq_kernel (conv_wq.h), conv_x3_wq3_kernel (conv_wq3.h) and conv_x3_wq3h_kernel
// (conv_wq3h.h) have in common, each piece written once: the geometry read, the tile bookkeeping, the per-window scalars of a
// fused first layer, the weight-tile slot contract, accumulator zero / MFMA / 8-way pick, the epilogue parameters and the f32
// epilogue pieces of the two 3x3 one-wave-per-SIMD kernels.  Read this first, then conv_wq.h for the scheme; the kernels keep
// their slot schedules and call these.  Everything here is __forceinline__, mutable state comes in by reference, and the
// opaque-register pins inside a piece are part of the schedule.  A piece belongs here only if the kernels compile to the SAME
// instructions with it: tools/device_asm.py on the commit before and after says so (DESIGN.md lists what did not pass).
#pragma once
#include "conv_fp.h"

namespace issk {

typedef const bf16x8 __attribute__((address_space(3)))* LdsR16;
typedef bf16x4 __attribute__((address_space(3)))* LdsW8;
typedef unsigned __attribute__((address_space(3)))* LdsW4;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 __attribute__((address_space(3)))* LdsF4;

// ---- geometry parameters (row decomposition of a tile): read through an opaque copy of the kernel-argument pointer where they
// are needed (once per tile) instead of living in SGPRs through the main loop, reciprocals from the host
struct GeoArgs {
    int H, W, Hq, Wq, ph, pw, pp, sh, sw, pt_, pl_;
    unsigned dv_mul[4];
    int dv_sh[4];
};
typedef const ConvArgs __attribute__((address_space(4)))* KArg;
__device__ __forceinline__ GeoArgs geo_args() {
    KArg q = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    GeoArgs ga;
    ga.H = q->H; ga.W = q->W; ga.Hq = q->Hq; ga.Wq = q->Wq; ga.ph = q->ph; ga.pw = q->pw; ga.pp = q->pp;
    ga.sh = q->sh; ga.sw = q->sw; ga.pt_ = q->pt_; ga.pl_ = q->pl_;
#pragma unroll
    for (int i = 0; i < 4; ++i) { ga.dv_mul[i] = q->dv_mul[i]; ga.dv_sh[i] = q->dv_sh[i]; }
    return ga;
}

// ---- tiles of `tmr` GEMM rows over the M rows of a launch, G of them per group
struct Tiles {
    int M, tmr, n;
    __device__ __forceinline__ Tiles(int M_, int tmr_) : M(M_), tmr(tmr_), n((M_ + tmr_ - 1) / tmr_) {}
    __device__ __forceinline__ int groups(int G) const { return (n + G - 1) / G; }
    __device__ __forceinline__ int clamp(int t) const { return t < n ? t : n - 1; }
    __device__ __forceinline__ int rows_of(int tile) const { const int r = M - tile * tmr; return tile < n ? (r < tmr ? r : tmr) : 0; }   // rows that exist
};

// ---- fused first layer: per-window scalars of the (at most two) windows a footprint touches.  Loaded one block before they are
// used (windows_of), then moved to SGPRs (settle): they are wave-uniform, and VGPRs are what these kernels are short of.
struct Win { int wr0, wr1; float mean0, mean1, sd0, sd1; int live0, live1; };
__device__ __forceinline__ Win windows_of(const ConvArgs& p, int nwin, int b) {       // loads only: nothing here may USE the values (see conv_fp.h)
    Win w;
    const unsigned b0 = (unsigned)(b < nwin ? b : nwin - 1), b1 = (unsigned)(b + 1 < nwin ? b + 1 : nwin - 1);
    w.wr0 = p.win_row[b0]; w.mean0 = p.stats[2u * b0]; w.sd0 = p.stats[2u * b0 + 1u]; w.live0 = p.finite[b0];
    w.wr1 = p.win_row[b1]; w.mean1 = p.stats[2u * b1]; w.sd1 = p.stats[2u * b1 + 1u]; w.live1 = p.finite[b1];
    return w;
}
__device__ __forceinline__ Win settle(const Win& w) {
    Win s;
    s.wr0 = __builtin_amdgcn_readfirstlane(w.wr0); s.wr1 = __builtin_amdgcn_readfirstlane(w.wr1);
    s.mean0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w.mean0)));
    s.mean1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w.mean1)));
    s.sd0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w.sd0)));
    s.sd1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w.sd1)));
    s.live0 = __builtin_amdgcn_readfirstlane(w.live0); s.live1 = __builtin_amdgcn_readfirstlane(w.live1);
    return s;
}

// ---- the weight-tile slot permutation: ONE contract between the LDS-DMA that fills a 4 KB weight tile (`boff_w` in the kernels)
// and the ds_read_b128 that takes its B fragments (`bread`).  A tile is [hi plane 2 KB | lo plane 2 KB], a plane is 64 rows (output
// channels) x 16 k = 128 slots of 16 bytes, and (row n, k half h) lives in slot 2 n + (h ^ ((n >> 3) & 1)): with it the reads of
// the 16 lanes of a group are conflict-free.  Loader: a 1 KB piece is (32-row half, plane) of a tile, lane l of it writes slot
// 64 half + l, so it FETCHES the (n, h) that belongs there: n = 32 half + (l >> 1), h = (l & 1) ^ ((n >> 3) & 1), at byte offset
// 2 (row * Kpad + 8 h) of the weight plane (rows >= Cout read row 0, never stored).  Reader: lane (li, lh) takes row li (+ 32 at
// + 1024), k half lh, of the hi plane (lo at + 2048): base + 16 (2 li + (lh ^ ((li >> 3) & 1))).  Change both or neither.
// (The two expressions stay in the kernels: as functions here they compile to different instructions -- profiles/HISTORY.md.)

// ---- accumulators
__device__ __forceinline__ floatx16 zero16() {
    floatx16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
// one split-operand MFMA; TR: issued transposed (C^T = W A^T)
template <bool TR, bool F16>
__device__ __forceinline__ floatx16 mfma_ab(const bf16x8& a, const bf16x8& b, const floatx16& c) {
    if (TR) return mfma_x3<F16>(b, a, c);
    return mfma_x3<F16>(a, b, c);
}
// accumulator (rb, cb) (compile-time) of a set of eight, named row block major: NCB column blocks per row block
template <int NCB, class T>
__device__ __forceinline__ T& pick8(int rb, int cb, T& a0, T& a1, T& a2, T& a3, T& a4, T& a5, T& a6, T& a7) {
    static_assert(NCB == 2 || NCB == 4, "");
    if (NCB == 4) return rb == 0 ? (cb == 0 ? a0 : cb == 1 ? a1 : cb == 2 ? a2 : a3) : (cb == 0 ? a4 : cb == 1 ? a5 : cb == 2 ? a6 : a7);
    return rb == 0 ? (cb ? a1 : a0) : rb == 1 ? (cb ? a3 : a2) : rb == 2 ? (cb ? a5 : a4) : (cb ? a7 : a6);
}

// ---- epilogue parameters, through the kernel-argument pointer.  Stores go through a buffer descriptor over `out`: an offset
// beyond its size is dropped by the hardware, so rows beyond the tile (tmr) or the launch (M) and columns >= Cout need a select
// on the offset, not a branch.
struct Epi { const float* bias; float* out; int cout; };
__device__ __forceinline__ Epi epi_args() {
    KArg q = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    Epi ep;
    ep.bias = q->bias; ep.out = q->out; ep.cout = q->Cout;
    return ep;
}
constexpr unsigned E_INVALID = 0xFFFF0000u;        // + the largest scalar offset of a store (< 16 KB) stays below 2^32: no wrap-around;
                                                   // the host keeps the output below 0xFFF00000 bytes

// ---- the f32 epilogue of the 3x3 kernels (conv_wq3.h, conv_wq3h.h), 32 units (rb, cb, g) per tile; the kernels hold the state.
// KIND 0 (TR; bias + relu): unit = channels n0 + 32 cb + 8 g + 4 lh + {0..3} of pixel row (wv * 2 + rb) * 32 + li: the bias as a
// float4 from the workgroup's table in LDS (bias_rd: the lane's address in it), one 16-byte store.  KIND 1 (relu + 2 x 1 max-pool):
// unit = rows 8 g + 4 lh + {0..3} of the row block = two pool windows, column n0 + 32 cb + li: two dword stores.
// wrow: the lane's first row inside the tile (row block 0, group 0); rowb: bytes per output row; tile_rows: rows of the tile that exist.
__device__ __forceinline__ void wq3_epi0_relu(float4& e_v, const float4 (&e_bb)[2], const floatx16& acc, int unit) {      // + bias, relu
    const int g = unit & 3;
    const float4 e_b = e_bb[unit & 1];
    e_v = make_float4(fmaxf(acc[4 * g] + e_b.x, 0.f), fmaxf(acc[4 * g + 1] + e_b.y, 0.f),
                      fmaxf(acc[4 * g + 2] + e_b.z, 0.f), fmaxf(acc[4 * g + 3] + e_b.w, 0.f));
    asm volatile("" : "+v"(e_v.x), "+v"(e_v.y), "+v"(e_v.z), "+v"(e_v.w));
}
__device__ __forceinline__ void wq3_epi1_pool(float& e_p0, float& e_p1, const float (&ebias)[4], const floatx16& acc, int cb, int g) {
    e_p0 = fmaxf(fmaxf(acc[4 * g], acc[4 * g + 1]) + ebias[cb], 0.f);
    e_p1 = fmaxf(fmaxf(acc[4 * g + 2], acc[4 * g + 3]) + ebias[cb], 0.f);
    asm volatile("" : "+v"(e_p0), "+v"(e_p1));
}
// vb: byte offset of (pooled row (tile * tmr + wv * 64) / 2 + 2 lh, column n0 + li) in `out`
template <bool X_NOEPI>
__device__ __forceinline__ void wq3_epi1_store(const float& e_p0, const float& e_p1, const __amdgpu_buffer_rsrc_t& orsrc, int& rowb, const int& wrow,
                                               int rb, int cb, int g, unsigned vb, int tile_rows) {
    int wr = wrow;
    asm volatile("" : "+v"(wr), "+s"(rowb));
    const bool ok = wr < tile_rows - (rb * 32 + 8 * g);
    const unsigned off = ok ? vb : E_INVALID;
    if (X_NOEPI) return;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e_p0), orsrc, (int)off, (rb * 16 + 4 * g) * rowb + cb * 128, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e_p1), orsrc, (int)off, (rb * 16 + 4 * g + 1) * rowb + cb * 128, 0);
}
}  // namespace issk
