// Instantiation unit of conv_x3_ws_kernel (conv_ws.h): weight-stationary footprint kernel, filter shapes with 8..16 taps.
#include "conv_ws.h"

ISS_WS_SHAPES_A(ISS_WS_DEFINE)
