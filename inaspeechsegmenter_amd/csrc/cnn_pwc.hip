// Instantiation unit of conv_x3_pwc_kernel (conv_pwc.h): chained expansion + reduction of two consecutive Bottlenecks.
#include "conv_pwc.h"

namespace issk {
bool iss_pwc_launch(const ConvArgs& a, hipStream_t st, const ConvInst& i) {
    // one workgroup per CU (155 KB of LDS).  K1T = 1: 68 / 73 KB of LDS and <= 252 registers -- TWO workgroups fit a CU, and the second
    // one's waves run their epilogue / split / staging phases under the first one's MFMAs (profiles/r06_pwc_experiments.txt: those
    // phases, not memory, bind the kernel)
#define ISS_PWC_TRY(K1T_, NC3_)                                                                                     \
    ISS_LAUNCH_IF(i.kernel == ConvKernel::Pwc && i.c1 == K1T_ && i.c3 == NC3_, (conv_x3_pwc_kernel<K1T_, NC3_>), \
                  dim3(std::min<unsigned>(a.nblk, K1T_ == 1 ? 512u : 256u)), 256, 0)
    ISS_PWC_PAIRS(ISS_PWC_TRY)
#undef ISS_PWC_TRY
    return false;
}
}  // namespace issk
