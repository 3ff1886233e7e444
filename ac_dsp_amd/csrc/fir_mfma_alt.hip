// fir_mfma_alt.hip -- translation unit 5 of the int8 MFMA FIR: the pipelined kernel's instantiations for OUT_TYPEs of fewer than 16 bits (NAR)
// and for 4-byte output containers (W4), up to 9 K-blocks, without a band skip (see fir_mfma_kernels.hpp: MfmaArgs, launch_nb_hs).  Only
// instantiates.
#include "fir_mfma_kernels.hpp"

namespace acdsp {

template <int NB, int HS>
static hipError_t launch_alt_hs(const FirParams &p, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  const v4i *f = (const v4i *)d_frag;
  if (epi == 3) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 3, HS, 1, 0, true>), grid, dim3(64), 0, s, p, f, a); }
  else if constexpr (HS == 0) {
    // (the general-rounding epilogue has instantiations of its own: inside the narrow-type kernels it spilled 5 - 13 registers at 6 and 9 K-blocks)
    if (a.gq_on) {
      if (epi == 1) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 1, 0, 1, 2>), grid, dim3(64), 0, s, p, f, a); }
      else { hipLaunchKernelGGL((fir_mfma_kernel<NB, 2, 0, 1, 2>), grid, dim3(64), 0, s, p, f, a); }
    }
    else if (epi == 1) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 1, 0, 1, 1>), grid, dim3(64), 0, s, p, f, a); }
    else { hipLaunchKernelGGL((fir_mfma_kernel<NB, 2, 0, 1, 1>), grid, dim3(64), 0, s, p, f, a); }
  } else { return hipErrorInvalidValue; }
  return hipGetLastError();
}
template <int NB>
static hipError_t launch_alt_nb(const FirParams &p, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  if constexpr (NB >= 7) {   // the band-skip codes launch_nb picks
    if (hs == 3 + 16 * 3) { return launch_alt_hs<NB, 3 + 16 * 3>(p, d_frag, a, epi, grid, s); }
    if (hs == 3 + 16 * 2) { return launch_alt_hs<NB, 3 + 16 * 2>(p, d_frag, a, epi, grid, s); }
    if (hs == 2 + 16 * 3) { return launch_alt_hs<NB, 2 + 16 * 3>(p, d_frag, a, epi, grid, s); }
  }
  if constexpr (NB >= 5) { if (hs == 2 + 16 * 2) { return launch_alt_hs<NB, 2 + 16 * 2>(p, d_frag, a, epi, grid, s); } }
  return hs == 0 ? launch_alt_hs<NB, 0>(p, d_frag, a, epi, grid, s) : hipErrorInvalidValue;
}
hipError_t launch_fir_mfma_alt(const FirParams &p, int nb, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  switch (nb) {
    case 1: return launch_alt_nb<1>(p, hs, d_frag, a, epi, grid, s);
    case 2: return launch_alt_nb<2>(p, hs, d_frag, a, epi, grid, s);
    case 3: return launch_alt_nb<3>(p, hs, d_frag, a, epi, grid, s);
    case 4: return launch_alt_nb<4>(p, hs, d_frag, a, epi, grid, s);
    case 5: return launch_alt_nb<5>(p, hs, d_frag, a, epi, grid, s);
    case 6: return launch_alt_nb<6>(p, hs, d_frag, a, epi, grid, s);
    case 7: return launch_alt_nb<7>(p, hs, d_frag, a, epi, grid, s);
    case 8: return launch_alt_nb<8>(p, hs, d_frag, a, epi, grid, s);
    case 9: return launch_alt_nb<9>(p, hs, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace acdsp
