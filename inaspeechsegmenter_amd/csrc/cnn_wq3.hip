// Instantiation unit of conv_x3_wq3_kernel (conv_wq3.h): one wave per SIMD, the unpadded 3x3 layers with 128 output channels
// per workgroup; kind 0 = bias + relu (transposed accumulators), kind 1 = relu + 2 x 1 max-pool.
#include "conv_wq3.h"

namespace issk {
bool iss_wq3_launch(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_WQ3_TRY(KIND_) ISS_LAUNCH_IF(i.kernel == ConvKernel::Wq3 && i.kind == KIND_, (conv_x3_wq3_kernel<KIND_>), grid, 256, 0)
    ISS_WQ3_TRY(0)
    ISS_WQ3_TRY(1)
#undef ISS_WQ3_TRY
    return false;
}
}  // namespace issk
