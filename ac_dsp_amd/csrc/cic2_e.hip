// cic2_e.hip -- fifth translation unit of the two-stage CIC decimator (compile time): compiles the stage-1 shapes named below; the kernel
// and the shape table are in cic2_kernels.hpp
#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s16_r12)
ACDSP_CIC2_COMPILE(s16_r6)
ACDSP_CIC2_COMPILE(s16_r7)

}  // namespace acdsp
