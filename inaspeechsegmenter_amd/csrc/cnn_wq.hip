// Instantiation unit of conv_x3_wq_kernel (conv_wq.h): one wave per SIMD, two LDS footprints; the fused 5x3 layer
// (f32 or CHL output; the fp16-operand forms are in cnn_wq_h.hip).
#include "conv_wq.h"

namespace issk {
bool iss_wq_launch_5x3_f16(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i);
bool iss_wq_launch_5x3(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
    ISS_WQ_TRY(5, 3, true, false)
    ISS_WQ_TRY(5, 3, false, false)
    return iss_wq_launch_5x3_f16(a, grid, st, i);
}
}  // namespace issk
