// fir_up_s8_b.hip -- translation unit 2 of the interpolating MFMA kernel on byte samples: two K blocks (33 .. 64 - SPC taps per phase), three
// coefficient digit planes.  Only instantiates; the kernel lives in fir_up_kernels.hpp.
#include "fir_up_kernels.hpp"

namespace acdsp {

hipError_t launch_up_b132(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int8_t, 1, 3, 2>(a, d_frag, L, out_eb, epi, grid, s);
}

}  // namespace acdsp
