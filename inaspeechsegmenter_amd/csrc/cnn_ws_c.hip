// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): the plain (not first-layer-fused) 3x3 variants, one 64-column tile.
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_plain_3x3) {
    // zero-padded, transposed epilogue
    ISS_WS_TRY(ConvKernel::WsPlain, 3, 3, true, true, false, 1, 1)
    ISS_WS_TRY(ConvKernel::WsPlain, 3, 3, true, true, false, 1, 0)
    // unpadded: 3x3 layers with 64 / 96 output channels (the two-column-half form wants % 128); bias + relu transposed, or pooled relu
    ISS_WS_TRY(ConvKernel::WsPlainU, 3, 3, false, true, false, 1, 1)
    ISS_WS_TRY(ConvKernel::WsPlainU, 3, 3, false, false, false, 1, 1)
    return false;
}
}  // namespace issk
