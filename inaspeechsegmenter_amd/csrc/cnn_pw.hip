// Instantiation unit of conv_x3_pws_kernel (conv_pw.h): streaming pointwise GEMM, four epilogue forms.
#include "conv_pw.h"

namespace issk {
bool iss_pws_launch(const ConvArgs& a, dim3 grid, hipStream_t st, const ConvInst& i) {
#define ISS_PWS_TRY(RES_, SIMPLE_) \
    ISS_LAUNCH_IF(i.kernel == ConvKernel::Pws && i.has_res == RES_ && i.simple_pw == SIMPLE_, (conv_x3_pws_kernel<RES_, SIMPLE_>), grid, 256, 0)
    ISS_PWS_TRY(true, true)
    ISS_PWS_TRY(false, true)
    ISS_PWS_TRY(true, false)
    ISS_PWS_TRY(false, false)
#undef ISS_PWS_TRY
    return false;
}
bool iss_pws2_launch(const ConvArgs& a0, hipStream_t st, const ConvInst& i) {
    ConvArgs a = a0;
    a.nblk_n = (unsigned)(a.Cout / 128);
    const dim3 grid(std::min<unsigned>(a.nblk * a.nblk_n, 512u));
#define ISS_PWS2_TRY(K_, SIMPLE_, STRIDED_, DUAL_) \
    ISS_LAUNCH_IF(i.kernel == K_ && i.simple_pw == SIMPLE_, (conv_x3_pws2_kernel<SIMPLE_, STRIDED_, DUAL_>), grid, 256, 0)
    ISS_PWS2_TRY(ConvKernel::Pws2Dual, true, false, true)
    ISS_PWS2_TRY(ConvKernel::Pws2Strided, true, true, false)
    ISS_PWS2_TRY(ConvKernel::Pws2, true, false, false)
    ISS_PWS2_TRY(ConvKernel::Pws2, false, false, false)
#undef ISS_PWS2_TRY
    return false;
}
}  // namespace issk
