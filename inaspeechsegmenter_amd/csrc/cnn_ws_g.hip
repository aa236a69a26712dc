// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): 3x3 behind a zero-padded ('same') shared first layer (FS).
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_fs_3x3) { return launch_ws_fused_rowmajor<3, 3, true>(a, grid, st, i); }
}  // namespace issk
