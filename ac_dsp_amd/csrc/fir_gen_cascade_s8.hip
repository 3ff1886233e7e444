// fir_gen_cascade_s8.hip -- the byte-row family of the fused decimator -> FIR cascade (ACDSP_DDC_IN_BYTES): cascade_kernel<int8_t, 1, 3, 6, 5,
// 4, 2, 3, GUARD, LIMB, PART> of fir_gen_kernels.hpp -- one sample plane into stage A (18 MFMAs per step where int16 rows issue 36), an
// INT_TYPE of 25 .. 32 bits on four planes into stage B (24 instead of 30), 264 16-byte pieces per step at R 16 with six K blocks (five per
// lane; int16 rows: nine).  launch_cascade (fir_gen_cascade.hip) decides the shape, the epilogue and the three launches; this unit holds the
// six instantiations it starts, a translation unit of its own so that the library's units keep compiling side by side.
#include "fir_gen_kernels.hpp"

namespace acdsp {

template <bool GUARD, bool LIMB, int PART>
static hipError_t launch_s8(dim3 grid, size_t lds_bytes, hipStream_t s, const FirParams &pa, const FirParams &pb, const v4i *fa, const v4i *fb,
                            const GenArgs &a, const GenArgs &b) {
  hipError_t e = hipFuncSetAttribute((const void *)cascade_kernel<int8_t, 1, 3, 6, 5, 4, 2, 3, GUARD, LIMB, PART>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) { return e; }
  hipLaunchKernelGGL((cascade_kernel<int8_t, 1, 3, 6, 5, 4, 2, 3, GUARD, LIMB, PART>), grid, dim3(64), lds_bytes, s, pa, pb, fa, fb, a, b);
  return hipGetLastError();
}

// the variants launch_cascade starts: interior (PART 1) and edge chunks (PART 2) unguarded, the ragged end (PART 0) guarded
hipError_t launch_cascade_s8(bool guard, bool limb, int part, dim3 grid, size_t lds_bytes, hipStream_t s, const FirParams &pa, const FirParams &pb,
                             const v4i *fa, const v4i *fb, const GenArgs &a, const GenArgs &b) {
  if (guard && part == 0) {
    return limb ? launch_s8<true, true, 0>(grid, lds_bytes, s, pa, pb, fa, fb, a, b) : launch_s8<true, false, 0>(grid, lds_bytes, s, pa, pb, fa, fb, a, b);
  }
  if (!guard && part == 1) {
    return limb ? launch_s8<false, true, 1>(grid, lds_bytes, s, pa, pb, fa, fb, a, b) : launch_s8<false, false, 1>(grid, lds_bytes, s, pa, pb, fa, fb, a, b);
  }
  if (!guard && part == 2) {
    return limb ? launch_s8<false, true, 2>(grid, lds_bytes, s, pa, pb, fa, fb, a, b) : launch_s8<false, false, 2>(grid, lds_bytes, s, pa, pb, fa, fb, a, b);
  }
  return hipErrorInvalidValue;
}

}  // namespace acdsp
