// cic2_f.hip -- sixth translation unit of the two-stage CIC decimator (compile time): compiles the stage-1 shapes named below; the kernel
// and the shape table are in cic2_kernels.hpp
#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s16_r4)
ACDSP_CIC2_COMPILE(s16_r3)
ACDSP_CIC2_COMPILE(s32_r7)
ACDSP_CIC2_COMPILE(s32_r6)

}  // namespace acdsp
