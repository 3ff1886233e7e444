// cic2_s8_b.hip -- second translation unit of the byte-row shapes of the two-stage CIC decimator (ACDSP_FLAG_IN_BYTES: 1-byte samples, one sample
// plane on the matrix cores); compiles the stage-1 shape named below; the kernel and the shape table are in cic2_kernels.hpp
#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s8_r8)

}  // namespace acdsp
