// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): the exact-f32 form (F32, v_mfma_f32_32x32x2_f32) for the three layers that carry
// the segmenter nets' arithmetic -- the first-layer-fused 5x3 convolution and the two unpadded 3x3 layers (128 columns per workgroup).
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_f32_fused_5x3) {         // relu + 2x2 max-pool
    ISS_WS_TRY(ConvKernel::WsF32Fused, 5, 3, false, false, true, 1, 1, false, true)
    return false;
}
ISS_WS_LAUNCHER(iss_ws_launch_f32_nh2_3x3) {           // bias + relu, transposed; or pooled relu
    ISS_WS_TRY(ConvKernel::WsNh2F32, 3, 3, false, true, false, 2, 1, false, true)
    ISS_WS_TRY(ConvKernel::WsNh2F32, 3, 3, false, false, false, 2, 1, false, true)
    return false;
}
}  // namespace issk
