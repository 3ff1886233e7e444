// cic2_d.hip -- fourth translation unit of the two-stage CIC decimator (compile time): compiles the stage-1 shapes named below; the kernel
// and the shape table are in cic2_kernels.hpp
#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s16_r15)
ACDSP_CIC2_COMPILE(s16_r5)
ACDSP_CIC2_COMPILE(s32_r5)
ACDSP_CIC2_COMPILE(s32_r4)
ACDSP_CIC2_COMPILE(s32_r3)

}  // namespace acdsp
