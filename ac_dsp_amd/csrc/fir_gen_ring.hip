// fir_gen_ring.hip -- the instantiations of fir_gen_ring_kernel (fir_gen_kernels.hpp) and the table of its compiled shapes.  Only
// instantiates: the selection that walks the table and the launch arguments are fir_gen.hip's.
#include "fir_gen_kernels.hpp"

namespace acdsp {

template <typename TIN, int PX, int PCT, int NBT, int R, int OEB, int SPW, int PF, bool NT, bool FB, bool LZ = false>
static hipError_t launch_ring1(dim3 grid, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
  hipLaunchKernelGGL((fir_gen_ring_kernel<TIN, PX, PCT, NBT, R, OEB, SPW, PF, NT, FB, LZ>), grid, dim3(64), 0, s, p, frag, a);
  return hipGetLastError();
}
// variant = spw (steps per chunk), pf (steps the loads run ahead), nt (non-temporal loads), fb (chunk-end store burst)
template <typename TIN, int PX, int PCT, int NBT, int R, int OEB>
static hipError_t launch_ring(int spw, int pf, int nt, int fb, dim3 grid, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
#define ACDSP_RING_CASE(SPWV, PFV, NTV, FBV) \
  if (spw == SPWV && pf == PFV && nt == NTV && fb == FBV) { return launch_ring1<TIN, PX, PCT, NBT, R, OEB, SPWV, PFV, (NTV != 0), (FBV != 0)>(grid, s, p, frag, a); }
  ACDSP_RING_CASE(2, 2, 1, 0) ACDSP_RING_CASE(2, 2, 1, 1)                                 // the defaults (fir_gen_select)
  ACDSP_RING_CASE(1, 1, 1, 0) ACDSP_RING_CASE(4, 1, 1, 0) ACDSP_RING_CASE(4, 2, 1, 1) ACDSP_RING_CASE(4, 4, 1, 1)   // A/B set
#undef ACDSP_RING_CASE
  return hipErrorInvalidValue;
}
template <bool VARIANTS, typename TIN, int PX, int PCT, int NBT, int R, int OEB, int SPW, int PF, bool NT, bool FB, bool LZ>
static hipError_t ring_row_launch(int spw, int pf, int nt, int fb, dim3 grid, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
  if constexpr (VARIANTS) { return launch_ring<TIN, PX, PCT, NBT, R, OEB>(spw, pf, nt, fb, grid, s, p, frag, a); }
  else { return launch_ring1<TIN, PX, PCT, NBT, R, OEB, SPW, PF, NT, FB, LZ>(grid, s, p, frag, a); }
}

// One row per compiled shape, in the order the plans are matched against (RingRow, fir_gen_kernels.hpp): a row stands in front of every
// row whose bounds contain its own -- shape 2 before 16, the one-K-block instantiations before their three-block siblings.
// ENV: env_ok; VAR: the six ACDSP_GEN_RING variants of the shape are compiled, the row's SPW / PF / NT / FB being the default one.
#define ACDSP_RING_ROW(ID, TIN, PX, PCT, NBT, R, OEB, SPW, PF, NT, FB, LZ, ENV, VAR) \
  {ID, (int)sizeof(TIN), PX, PCT, NBT, R, OEB, SPW, PF, NT, FB, LZ, ENV, VAR, ring_row_launch<VAR, TIN, PX, PCT, NBT, R, OEB, SPW, PF, (NT != 0), (FB != 0), (LZ != 0)>},
static const RingRow kRingRows[] = {
  // the decimating BASELINE shapes
  ACDSP_RING_ROW(1, int32_t, 4, 2, 3, 8, 8, 2, 2, 1, 0, 0, true, true)      // CIC R8 N5 on int32 -> int64
  ACDSP_RING_ROW(2, int16_t, 2, 3, 6, 16, 8, 2, 2, 1, 0, 0, true, true)     // CIC R16 N5 on int16 -> int64
  ACDSP_RING_ROW(3, int16_t, 2, 2, 4, 8, 2, 2, 2, 1, 1, 0, true, true)      // 128-tap decimate-by-8 on int16 -> int16
  // further CIC decimator shapes (tools/cic_sweep.py): no BASELINE config, same kernel
  ACDSP_RING_ROW(4, int16_t, 2, 2, 3, 8, 4, 2, 2, 1, 0, 0, true, true)      // CIC R8 on int16 -> int32 (INT_TYPE <= 32 bits)
  ACDSP_RING_ROW(5, int32_t, 4, 2, 2, 4, 8, 4, 4, 1, 0, 0, true, false)     // CIC R4 on int32: 4 KB per step
  // ac_poly_dec on int16 at other factors / output widths (tools/poly_shapes.py): about 8 KB of input per wave, every load up front
  ACDSP_RING_ROW(10, int16_t, 2, 2, 2, 2, 2, 8, 8, 1, 1, 0, false, false)
  ACDSP_RING_ROW(11, int16_t, 2, 2, 2, 2, 8, 8, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(12, int16_t, 2, 2, 3, 4, 2, 4, 4, 1, 1, 0, false, false)
  ACDSP_RING_ROW(13, int16_t, 2, 2, 3, 4, 8, 4, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(14, int16_t, 2, 2, 4, 8, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(15, int16_t, 2, 2, 8, 16, 2, 2, 2, 1, 1, 0, false, false)
  ACDSP_RING_ROW(16, int16_t, 2, 2, 8, 16, 8, 2, 2, 1, 0, 0, false, false)
  // plain (R = 1) FIR on 16-bit samples whose coefficients need more than the int8 kernel's 16 bits (two load groups of two steps per ... ).
  // Plans of ONE K-block -- up to ~49 taps: the reference testbenches' 27 / 29 -- have their own instantiations: the three-block shapes
  // issue 3 x the MFMAs on zero fragments, 36 instead of 12 per 256 outputs on 32-bit samples -- the matrix pipe, not HBM, bounded them
  ACDSP_RING_ROW(23, int16_t, 2, 3, 1, 1, 8, 16, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(23, int16_t, 2, 3, 3, 1, 8, 16, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(24, int16_t, 2, 3, 1, 1, 4, 16, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(24, int16_t, 2, 3, 3, 1, 4, 16, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(25, int16_t, 2, 3, 1, 1, 2, 16, 8, 1, 1, 0, false, false)
  ACDSP_RING_ROW(25, int16_t, 2, 3, 3, 1, 2, 16, 8, 1, 1, 0, false, false)
  // plain (R = 1) FIR on 32-bit samples, up to three coefficient digits and three K-blocks (~130 taps): one 1 KB load per 256-output step
  ACDSP_RING_ROW(20, int32_t, 4, 3, 1, 1, 8, 8, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(20, int32_t, 4, 3, 3, 1, 8, 8, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(21, int32_t, 4, 3, 1, 1, 4, 8, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(21, int32_t, 4, 3, 3, 1, 4, 8, 8, 1, 0, 0, false, false)
  ACDSP_RING_ROW(7, int32_t, 4, 2, 4, 7, 8, 2, 2, 1, 0, 0, false, false)    // CIC R7 (M2 N4: the reference testbench) on int32: 7 KB per step
  ACDSP_RING_ROW(8, int16_t, 2, 2, 3, 5, 4, 4, 2, 1, 0, 0, false, false)    // CIC R5 on int16: 2.5 KB per step, one load group per two steps
  ACDSP_RING_ROW(9, int16_t, 2, 2, 3, 5, 8, 4, 2, 1, 0, 0, false, false)
  // decimal rates: R = 10 on int32 (10 KB per step, two steps per wave) and on int16 (5 KB per step, four steps)
  ACDSP_RING_ROW(30, int32_t, 4, 2, 4, 10, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(31, int16_t, 2, 3, 4, 10, 4, 4, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(32, int16_t, 2, 3, 4, 10, 8, 4, 2, 1, 0, 0, false, false)
  // further small and decimal rates (multistage decimators: 3, 6, 12, 20), same kernel, about 6 - 12 KB of input per wave
  ACDSP_RING_ROW(33, int16_t, 2, 2, 3, 3, 4, 8, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(34, int16_t, 2, 2, 3, 3, 8, 8, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(35, int32_t, 4, 2, 3, 3, 8, 4, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(36, int16_t, 2, 2, 3, 6, 4, 4, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(37, int16_t, 2, 2, 3, 6, 8, 4, 4, 1, 0, 0, false, false)
  ACDSP_RING_ROW(38, int32_t, 4, 2, 3, 6, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(39, int16_t, 2, 2, 5, 12, 4, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(40, int16_t, 2, 2, 5, 12, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(41, int16_t, 2, 3, 8, 20, 4, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(42, int16_t, 2, 3, 8, 20, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(43, int32_t, 4, 2, 3, 5, 8, 2, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(44, int16_t, 2, 2, 4, 7, 4, 4, 2, 1, 0, 0, false, false)
  ACDSP_RING_ROW(45, int16_t, 2, 2, 4, 7, 8, 4, 2, 1, 0, 0, false, false)
  // byte samples (ACDSP_FLAG_IN_BYTES): ac_poly_dec at DF = 2, 4, 8, 16 on one sample plane; instantiated in fir_gen_ring_s8.hip
#define ACDSP_RING_S8_ROW(ID, NBT, R, OEB, SPW, PF, FB) {ID, 1, 1, 2, NBT, R, OEB, SPW, PF, 1, FB, 0, false, false, ring_s8_row_launch<NBT, R, OEB, SPW, PF, (FB != 0)>},
  ACDSP_RING_S8_ROWS(ACDSP_RING_S8_ROW)
#undef ACDSP_RING_S8_ROW
  ACDSP_RING_ROW(6, int32_t, 4, 3, 6, 16, 8, 1, 1, 1, 0, 0, true, false)    // CIC R16 N5 on int32: 16 KB per step = one step per wave (LDS: 18 KB of planes per step)
  // class B: the R = 1 shapes 23 / 24 / 25 / 20 / 21 with the residue loop compiled in (the selection ignores ACDSP_GEN_RING for them)
  ACDSP_RING_ROW(23, int16_t, 2, 3, 1, 1, 8, 16, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(23, int16_t, 2, 3, 3, 1, 8, 16, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(24, int16_t, 2, 3, 1, 1, 4, 16, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(24, int16_t, 2, 3, 3, 1, 4, 16, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(25, int16_t, 2, 3, 1, 1, 2, 16, 8, 1, 1, 1, true, false)
  ACDSP_RING_ROW(25, int16_t, 2, 3, 3, 1, 2, 16, 8, 1, 1, 1, true, false)
  ACDSP_RING_ROW(20, int32_t, 4, 3, 1, 1, 8, 8, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(20, int32_t, 4, 3, 3, 1, 8, 8, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(21, int32_t, 4, 3, 1, 1, 4, 8, 8, 1, 0, 1, true, false)
  ACDSP_RING_ROW(21, int32_t, 4, 3, 3, 1, 4, 8, 8, 1, 0, 1, true, false)
};
#undef ACDSP_RING_ROW

const RingRow *fir_gen_ring_rows(int *n_rows) {
  *n_rows = (int)(sizeof(kRingRows) / sizeof(kRingRows[0]));
  return kRingRows;
}

}  // namespace acdsp
