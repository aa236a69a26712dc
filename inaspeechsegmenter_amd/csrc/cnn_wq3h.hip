// Instantiation unit of conv_x3_wq3h_kernel (conv_wq3h.h): the one-wave-per-SIMD 3x3 kernel on a CHL (pre-split, plane-major)
// input fetched by LDS-DMA; kind 0 = bias + relu with f32 or CHL output, kind 1 = relu + 2 x 1 max-pool with f32 output.
// (The fp16-operand forms are in cnn_wq3h_h.hip.)
#include "conv_wq3h.h"

namespace issk {
bool iss_wq3h_launch_f16(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i);
bool iss_wq3h_launch(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
    ISS_WQ3H_TRY(0, true, false)
    ISS_WQ3H_TRY(0, false, false)
    ISS_WQ3H_TRY(1, true, false)
    ISS_WQ3H_TRY(1, false, false)
    return iss_wq3h_launch_f16(a, grid, st, i);
}
}  // namespace issk
