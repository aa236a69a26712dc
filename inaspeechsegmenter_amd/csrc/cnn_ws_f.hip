// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): 5x3 behind a zero-padded ('same') shared first layer (FS).
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_fs_5x3) {
    if (launch_ws_fused_rowmajor<5, 3, true>(a, grid, st, i)) return true;
    ISS_WS_TRY(ConvKernel::WsFs, 5, 3, false, true, true, 1, 1, true)       // no fused pool: transposed simple epilogue (bias + relu)
    return false;
}
}  // namespace issk
