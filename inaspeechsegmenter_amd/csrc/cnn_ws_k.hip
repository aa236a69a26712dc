// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): NCB = 1 -- one 32-column block per workgroup -- for a first-layer-fused 5x3
// second convolution with <= 32 output channels (relu + 2x2 max-pool).
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_ncb1_5x3) {
    ISS_WS_TRY(ConvKernel::WsNcb1, 5, 3, false, false, true, 1, 1, false, false, 1)
    return false;
}
}  // namespace issk
