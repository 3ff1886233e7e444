// fir_up_b.hip -- translation unit 2 of the interpolating MFMA kernel: 16-bit samples, three coefficient digit planes (ac_poly_intr's pair
// taps, CIC interpolators whose boxcar^N taps pass 2^15).  Only instantiates; the kernel lives in fir_up_kernels.hpp.
#include "fir_up_kernels.hpp"

namespace acdsp {

hipError_t launch_up_s231(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int16_t, 2, 3, 1>(a, d_frag, L, out_eb, epi, grid, s);
}
hipError_t launch_up_s232(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int16_t, 2, 3, 2>(a, d_frag, L, out_eb, epi, grid, s);
}

}  // namespace acdsp
