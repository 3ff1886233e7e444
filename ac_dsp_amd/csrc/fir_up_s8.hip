// fir_up_s8.hip -- the interpolating MFMA kernel on byte samples (ACDSP_FLAG_IN_BYTES on ac_poly_intr): int8 rows are the ONE signed sample
// plane as they are loaded (a step = 512 bytes behind 32 NB bytes of history, one 16-byte load per lane), outputs leave in 1-byte rows
// (ACDSP_FLAG_OUT_BYTES: four results of a lane packed into a dword of the tile) or in int16 rows.  One K block with two or three coefficient
// digit planes here; fir_up_s8_b.hip compiles the two-K-block shape.  Only instantiates; the kernel lives in fir_up_kernels.hpp.
#include "fir_up_kernels.hpp"

namespace acdsp {

hipError_t launch_up_b121(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int8_t, 1, 2, 1>(a, d_frag, L, out_eb, epi, grid, s);
}
hipError_t launch_up_b131(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int8_t, 1, 3, 1>(a, d_frag, L, out_eb, epi, grid, s);
}

}  // namespace acdsp
