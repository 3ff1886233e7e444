// fir_mfma_alt2.hip -- translation unit 6 of the int8 MFMA FIR: the NAR instantiations (OUT_TYPEs of fewer than 16 bits, general rounding /
// overflow modes) of the pipelined kernel WITH a band skip, 5 .. 9 K-blocks (see fir_mfma_kernels.hpp: MfmaArgs).  Only instantiates.
//
#include "fir_mfma_kernels.hpp"

namespace acdsp {

// NAR instantiations with a band skip (round 5): band-limited sets into narrow OUT_TYPEs or through the general rounding modes ran every
// high-plane product (36 instead of 24 MFMAs per step at nine blocks) -- that, not the epilogue, was most of their distance to the plain classes
template <int NB, int HS>
static hipError_t launch_alt2_hs(const FirParams &p, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  const v4i *f = (const v4i *)d_frag;
  if (a.gq_on) {
    if (epi == 1) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 1, HS, 1, 2>), grid, dim3(64), 0, s, p, f, a); }
    else { hipLaunchKernelGGL((fir_mfma_kernel<NB, 2, HS, 1, 2>), grid, dim3(64), 0, s, p, f, a); }
  }
  else if (epi == 1) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 1, HS, 1, 1>), grid, dim3(64), 0, s, p, f, a); }
  else { hipLaunchKernelGGL((fir_mfma_kernel<NB, 2, HS, 1, 1>), grid, dim3(64), 0, s, p, f, a); }
  return hipGetLastError();
}
template <int NB>
static hipError_t launch_alt2_nb(const FirParams &p, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  if constexpr (NB >= 7) { if (hs == 3 + 16 * 3) { return launch_alt2_hs<NB, 3 + 16 * 3>(p, d_frag, a, epi, grid, s); } }
  return hs == 2 + 16 * 2 ? launch_alt2_hs<NB, 2 + 16 * 2>(p, d_frag, a, epi, grid, s) : hipErrorInvalidValue;
}
hipError_t launch_fir_mfma_alt2(const FirParams &p, int nb, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  switch (nb) {
    case 5: return launch_alt2_nb<5>(p, hs, d_frag, a, epi, grid, s);
    case 6: return launch_alt2_nb<6>(p, hs, d_frag, a, epi, grid, s);
    case 7: return launch_alt2_nb<7>(p, hs, d_frag, a, epi, grid, s);
    case 8: return launch_alt2_nb<8>(p, hs, d_frag, a, epi, grid, s);
    case 9: return launch_alt2_nb<9>(p, hs, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace acdsp
