// conv_x3_wq3h_kernel with fp16 operand halves (ISS_PREC_F16X3, conv_common.h).
#include "conv_wq3h.h"

namespace issk {
bool iss_wq3h_launch_f16(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
    ISS_WQ3H_TRY(0, true, true)
    ISS_WQ3H_TRY(0, false, true)
    ISS_WQ3H_TRY(1, true, true)
    ISS_WQ3H_TRY(1, false, true)
    return false;
}
}  // namespace issk
