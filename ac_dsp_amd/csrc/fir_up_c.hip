// fir_up_c.hip -- translation unit 3 of the interpolating MFMA kernel: 32-bit samples (CIC interpolators, two or three coefficient digit
// planes).  Only instantiates; the kernel lives in fir_up_kernels.hpp.
#include "fir_up_kernels.hpp"

namespace acdsp {

hipError_t launch_up_i421(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int32_t, 4, 2, 1>(a, d_frag, L, out_eb, epi, grid, s);
}
hipError_t launch_up_i431(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int32_t, 4, 3, 1>(a, d_frag, L, out_eb, epi, grid, s);
}

}  // namespace acdsp
