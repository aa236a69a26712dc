// Test aid (include/iss.h iss_diag_split16): the operand split of conv_common.h, run over an array so that a test can compare
// its 16-bit halves with a host reference bit for bit: a change of the instructions that form the halves (one fused instruction
// for the fp16 residual was measured, profiles/conv2_front_end_ab.md) has its yardstick here.  Nothing here is on a hot path.
#include "conv_common.h"

namespace issk {

template <bool F16>
__global__ __launch_bounds__(256) void diag_split16_kernel(const float* __restrict__ x, long long n, int form,
                                                           uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? x[i0 + k] : 0.f;
    unsigned h[4], l[4];
    if (form == 0) {                                 // four values at a time: split4_pk
        unsigned h01, h23, l01, l23;
        split4_pk<F16>(make_float4(v[0], v[1], v[2], v[3]), h01, h23, l01, l23);
        h[0] = h01; h[1] = h01 >> 16; h[2] = h23; h[3] = h23 >> 16;
        l[0] = l01; l[1] = l01 >> 16; l[2] = l23; l[3] = l23 >> 16;
    } else {                                         // one value at a time: the epilogues that store 16 bits (conv_wq.h epi_s)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[k] = cvt_pk16<F16>(v[k], v[k]);
            const float r = v[k] - unpk16_lo<F16>(h[k]);
            l[k] = cvt_pk16<F16>(r, r);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) { hi[i0 + k] = (uint16_t)(h[k] & 0xffffu); lo[i0 + k] = (uint16_t)(l[k] & 0xffffu); }
}

}  // namespace issk

extern "C" int iss_diag_split16(iss_ctx* c, const float* x, int64_t n, int32_t f16, int32_t form, uint16_t* hi_out, uint16_t* lo_out) {
    if (!c || !x || !hi_out || !lo_out || n < 0 || n > (int64_t)1 << 28 || form < 0 || form > 1) return ISS_EINVAL;
    if (n == 0) return ISS_OK;
    ISS_HIP(c, hipSetDevice(c->device));
    ISS_HIP(c, hipStreamSynchronize(c->stream));
    void* buf = nullptr;
    ISS_HIP(c, hipMalloc(&buf, (size_t)n * 8));      // [n f32][n hi][n lo]
    float* dx = (float*)buf;
    uint16_t* dh = (uint16_t*)(dx + n);
    uint16_t* dl = dh + n;
    hipError_t e = hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned blocks = (unsigned)((n + 1023) / 1024);
        if (f16) hipLaunchKernelGGL(issk::diag_split16_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, dx, (long long)n, (int)form, dh, dl);
        else hipLaunchKernelGGL(issk::diag_split16_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, dx, (long long)n, (int)form, dh, dl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(hi_out, dh, (size_t)n * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(lo_out, dl, (size_t)n * 2, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    ISS_HIP(c, e);
    return ISS_OK;
}
