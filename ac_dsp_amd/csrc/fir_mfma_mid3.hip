// fir_mfma_mid3.hip -- translation unit 4 of the register-resident shapes of the int8 MFMA FIR: 27 / 29 / 31 K-blocks at one wave per
// SIMD (see fir_mfma_mid.hip).  Only instantiates; the kernels live in fir_mfma_kernels.hpp.
#include "fir_mfma_kernels.hpp"

namespace acdsp {

hipError_t launch_fir_mfma_mid3(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  switch (nb) {
    case 27: return launch_nb_hs<27, 11 + 16 * 11, 1>(p, d_frag, a, epi, grid, s);
    case 29: return launch_nb_hs<29, 12 + 16 * 12, 1>(p, d_frag, a, epi, grid, s);
    case 31: return launch_nb_hs<31, 13 + 16 * 13, 1>(p, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace acdsp
