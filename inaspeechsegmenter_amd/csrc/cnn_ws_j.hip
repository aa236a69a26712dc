// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): the ring form for 4x5 second convolutions (20 taps), first-layer-fused.
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_ring_4x5) { return launch_ws_fused_rowmajor<4, 5, false>(a, grid, st, i); }
}  // namespace issk
