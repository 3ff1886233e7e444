// cic2_c.hip -- third translation unit of the two-stage CIC decimator (compile time): compiles the stage-1 shapes named below; the kernel
// and the shape table are in cic2_kernels.hpp
#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s32_r10)
ACDSP_CIC2_COMPILE(s32_r8)

}  // namespace acdsp
