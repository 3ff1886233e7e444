// fir_mfma_mid.hip -- second translation unit of the int8 MFMA FIR: the register-resident kernel shapes for 11 / 13 / 15 / 17 K-blocks
// (258 - 513 taps) at one wave per SIMD.  The kernels and launch_nb_hs live in fir_mfma_kernels.hpp; this unit only instantiates them
// (launch_fir_mfma_mid), so that it compiles beside fir_mfma.hip.
#include "fir_mfma_kernels.hpp"

namespace acdsp {

hipError_t launch_fir_mfma_mid(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  switch (nb) {
    case 11: return launch_nb_hs<11, 3 + 16 * 3, 1>(p, d_frag, a, epi, grid, s);
    case 13: return launch_nb_hs<13, 4 + 16 * 4, 1>(p, d_frag, a, epi, grid, s);
    case 15: return launch_nb_hs<15, 5 + 16 * 5, 1>(p, d_frag, a, epi, grid, s);
    case 17: return launch_nb_hs<17, 6 + 16 * 6, 1>(p, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace acdsp
