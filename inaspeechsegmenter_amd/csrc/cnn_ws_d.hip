// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): the two-column-half (NH = 2) variant for 3x3 layers.
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_nh2_3x3) {
    // zero-padded form (ResNet-101's 128 -> 128 / 256 -> 256 convolutions): transposed, simple epilogue only (host-checked)
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, true, true, false, 2, 1)
    // zero-padded + relu + fused non-overlapping max-pool (a 'same' 3x3 layer in front of a pool: VGG-style stacks), row-major epilogue
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, true, false, false, 2, 1)
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, false, true, false, 2, 1)
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, false, true, false, 2, 0)
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, false, false, false, 2, 1)
    ISS_WS_TRY(ConvKernel::WsNh2, 3, 3, false, false, false, 2, 0)
    return false;
}
}  // namespace issk
