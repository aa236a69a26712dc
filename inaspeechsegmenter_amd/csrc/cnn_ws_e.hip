// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): the ring form for filters with more than 16 taps (7x7), first-layer-fused.
#include "conv_ws.h"

namespace issk {
ISS_WS_LAUNCHER(iss_ws_launch_ring_7x7) { return launch_ws_fused_rowmajor<7, 7, false>(a, grid, st, i); }
}  // namespace issk
