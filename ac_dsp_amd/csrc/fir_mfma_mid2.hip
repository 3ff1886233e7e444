// fir_mfma_mid2.hip -- translation unit 3 of the register-resident shapes of the int8 MFMA FIR: 19 / 21 / 23 / 25 K-blocks at one wave per
// SIMD (see fir_mfma_mid.hip).  Only instantiates; the kernels live in fir_mfma_kernels.hpp.
#include "fir_mfma_kernels.hpp"

namespace acdsp {

hipError_t launch_fir_mfma_mid2(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  switch (nb) {
    case 19: return launch_nb_hs<19, 7 + 16 * 7, 1>(p, d_frag, a, epi, grid, s);
    case 21: return launch_nb_hs<21, 8 + 16 * 8, 1>(p, d_frag, a, epi, grid, s);
    case 23: return launch_nb_hs<23, 9 + 16 * 9, 1>(p, d_frag, a, epi, grid, s);
    case 25: return launch_nb_hs<25, 10 + 16 * 10, 1>(p, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace acdsp
