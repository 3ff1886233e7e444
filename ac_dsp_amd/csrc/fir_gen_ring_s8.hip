// fir_gen_ring_s8.hip -- the byte-sample instantiations of fir_gen_ring_kernel (fir_gen_kernels.hpp): ac_poly_dec under ACDSP_FLAG_IN_BYTES at
// DF = 2, 4, 8, 16 into 2- and 8-byte outputs, fir_gen_ring_kernel<int8_t, 1, 2, NBT, R, OEB, SPW, PF, true, FB>.  ONE sample plane: a 16-byte
// piece of a row is a whole slot and goes to LDS as it is (unsigned bytes XOR 0x80).  Only instantiates: the rows are named once, in
// ACDSP_RING_S8_ROWS, and reached through the table of fir_gen_ring.hip; the selection and the launch arguments are fir_gen.hip's.
#include "fir_gen_kernels.hpp"

namespace acdsp {

template <int NBT, int R, int OEB, int SPW, int PF, bool FB>
hipError_t ring_s8_row_launch(int, int, int, int, dim3 grid, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
  hipLaunchKernelGGL((fir_gen_ring_kernel<int8_t, 1, 2, NBT, R, OEB, SPW, PF, true, FB, false>), grid, dim3(64), 0, s, p, frag, a);
  return hipGetLastError();
}

#define ACDSP_RING_S8_INST(ID, NBT, R, OEB, SPW, PF, FB) \
  template hipError_t ring_s8_row_launch<NBT, R, OEB, SPW, PF, (FB != 0)>(int, int, int, int, dim3, hipStream_t, const FirParams &, const v4i *, const GenArgs &);
ACDSP_RING_S8_ROWS(ACDSP_RING_S8_INST)
#undef ACDSP_RING_S8_INST

}  // namespace acdsp
