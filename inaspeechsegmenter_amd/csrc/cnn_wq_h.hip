// conv_x3_wq_kernel with fp16 operand halves (ISS_PREC_F16X3, conv_common.h): its own unit so that `make -j` builds it beside cnn_wq.hip.
#include "conv_wq.h"

namespace issk {
bool iss_wq_launch_5x3_f16(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
    ISS_WQ_TRY(5, 3, true, true)
    ISS_WQ_TRY(5, 3, false, true)
    return false;
}
}  // namespace issk
