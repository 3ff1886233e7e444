// fir_gen_cascade.hip -- host side and instantiations of the fused decimator -> FIR cascade (cascade_kernel, fir_gen_kernels.hpp):
// BASELINE config 5, a decimating FIR on int16 input feeding a FIR on its INT_TYPE words without the intermediate leaving the CU.
#include <cstdlib>
#include <cstring>

#include "fir_gen_kernels.hpp"

namespace acdsp {

// pa: stage A (decimator) -- in / x / hist / hl / in_stride / n / n_ch as for launch_fir_gen with out_mode 1;
// pb: stage B formats (in = the INT_TYPE, acc, out, lossless_shift) and the output buffer (y, out_stride, int32 containers).
// Returns hipErrorNotSupported when the shapes are not the compiled ones (the caller then runs the two kernels).
hipError_t launch_cascade(const FirParams &pa, const FirGenPlan &pla, const uint32_t *d_fragA, int w_int, int64_t first,
                          const FirParams &pb, const FirGenPlan &plb, const uint32_t *d_fragB, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) { return hipSuccess; }
  GenArgs a, b;
  memset(&a, 0, sizeof a); memset(&b, 0, sizeof b);
  a.pl = pla; b.pl = plb;
  a.px = (pa.in.W + (pa.in.S ? 0 : 1) + 7) / 8;
  b.px = (w_int + 7) / 8;
  a.n_slots = 15 * pla.R + 4 * pla.nb;
  const int spl = (a.n_slots + 63) / 64;
  const bool shape_ok = pa.in_eb == 2 && a.px == 2 && pla.pc <= 3 && pla.nb <= 6 && spl == 5 && (a.n_slots * 2 + 63) / 64 <= 9 && pla.R >= 2 &&
                        b.px == 5 && plb.pc <= 2 && plb.nb <= 3 && plb.R == 1 && plb.off == 128 && pb.out_eb == 4;
  a.out_mode = 1; a.w_int = w_int; a.out_simple = 2;
  FirParams pint = pa;                       // stage A's "OUT_TYPE" is the INT_TYPE itself: wrap only
  pint.out = pb.in;
  const bool conv_a = gen_conv_params(pint, 1, w_int, &a) && a.e_rs == 0 && a.e_ls2 == 0 && a.e_ko <= a.e_ka && a.e_hi == INT64_MAX;
  const bool conv_b = gen_conv_params(pb, 0, 0, &b);
  const bool out_ok = ((uintptr_t)pb.y % 16 == 0) && ((pb.out_stride * 4) % 16 == 0);
  if (!shape_ok || !conv_a || !conv_b || !out_ok) { return hipErrorNotSupported; }
  a.corr = gen_rebias_corr(a.px, pla.sum_h);
  b.corr = gen_rebias_corr(b.px, plb.sum_h);
  a.first = first; a.n_out = n_out; b.first = 0; b.n_out = n_out;
  a.n_steps = (n_out + 255) / 256;
  int64_t spw = 8;                           // short spans (see launch_fir_gen) against one (half-loaded) warm-up step per chunk: 4: 0.605, 6: 0.642 - 0.667, 8: 0.653 - 0.669 of the roofline (profiles/r3_span_sweep.txt, last block)
  ACDSP_TUNE_ENV(cspw_env, "ACDSP_CASC_SPW");   // tuning knob: steps per wave of the fused cascade
  if (cspw_env && atoi(cspw_env) > 0) { spw = atoi(cspw_env); }
  if (spw < 2) { spw = 2; }
  a.steps_per_wave = spw;
  a.n16 = (pa.n + 15) / 16 * 16;
  a.out_vec_ok = 1; a.chunk0 = 0;
  b.pad = 0; b.rcp = 0; b.n_slots = 0; b.out_mode = 0; b.w_int = 0; b.out_simple = 0; b.n_steps = a.n_steps; b.steps_per_wave = spw;
  b.n16 = 0; b.obuf_off = 0; b.chunk0 = 0; b.out_vec_ok = 1;
  const int slots_alloc = 15 * pla.R + 4 * 6;
  const int phys = gen_slot_map(a, pla.R, slots_alloc);
  a.obuf_off = a.px * (phys + 1) * 16;
  ACDSP_TUNE_ENV(clp_env, "ACDSP_CASC_LDS_PAD");   // diagnostic: extra LDS bytes per wave (lowers the occupancy)
  const size_t lds_bytes = (size_t)a.obuf_off + 5 * 512 + 1024 + (clp_env ? (size_t)atoi(clp_env) : 0);
  const int64_t n_chunks = (a.n_steps + spw - 1) / spw, fast_chunks = n_out / (spw * 256);
  const v4i *fa = (const v4i *)d_fragA, *fb = (const v4i *)d_fragB;

  // 32-bit limb epilogues: the exact stage results are small enough that byte / 16-bit carry chains in 32-bit registers
  // reproduce them (no 64-bit arithmetic per output).  Conditions: the true |y| of both stages bounded well inside int64
  // (sum |h| x the input range), no ACC_TYPE wrap in stage B, a right shift of 0..31 bits into an OUT_TYPE of <= 31 bits,
  // and for AC_SAT an OUT range that reaches into the high limb.
  static const bool no_limb = getenv("ACDSP_NO_LIMB") != nullptr;   // A/B knob
  bool limb = !no_limb && w_int >= 33 && w_int <= 40 && pla.sum_abs_h < (int64_t(1) << 38) && plb.sum_abs_h < (int64_t(1) << 20);
  const int64_t bound_b = limb ? plb.sum_abs_h * (int64_t(1) << (w_int - 1)) + b.e_rnd : 0;   // |stage-B dot product + rounding constant|
  limb = limb && b.e_ls == 0 && b.e_ls2 == 0 && b.e_rs <= 31 && pb.out.W <= 31 && bound_b < (int64_t(1) << 61) &&
         (pb.acc.W >= 63 || bound_b < (int64_t(1) << (pb.acc.W - 1)));
  if (limb) {
    auto digits = [](__int128 c, int nw, int32_t *dig) {   // balanced base-256 digits, the last one takes the rest
      for (int w = 0; w < nw - 1; w++) { dig[w] = pop_balanced_digit(c); }
      dig[nw - 1] = (int32_t)c;
      return c > -(int64_t(1) << 20) && c < (int64_t(1) << 20);
    };
    limb = digits(a.corr, 4, a.dig) && digits(b.corr + b.e_rnd, 6, b.dig);
    if (pb.out.O == ACDSP_SAT) {
      const int hb = pb.out.W - 1 + b.e_rs - 32;           // OUT range in units of the high limb: [-2^hb, 2^hb)
      limb = limb && hb >= 0 && hb <= 29;
      b.l_hb_lo = -(1 << (hb < 0 ? 0 : hb)) - 1; b.l_hb_hi = 1 << (hb < 0 ? 0 : hb);
      b.l_lo = (int32_t)b.e_lo; b.l_hi = (int32_t)b.e_hi; b.l_w = pb.out.W;
    } else {
      b.l_hb_lo = b.l_lo = INT32_MIN; b.l_hb_hi = b.l_hi = INT32_MAX; b.l_w = pb.out.W;
    }
  }
  hipError_t e;
#define ACDSP_CASCADE_LAUNCH(GUARD_, LIMB_, PART_, GRID_)                                                                            \
  e = hipFuncSetAttribute((const void *)cascade_kernel<2, 3, 6, 9, 5, 2, 3, GUARD_, LIMB_, PART_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                          (int)lds_bytes);                                                                                           \
  if (e != hipSuccess) { return e; }                                                                                                 \
  hipLaunchKernelGGL((cascade_kernel<2, 3, 6, 9, 5, 2, 3, GUARD_, LIMB_, PART_>), GRID_, dim3(64), lds_bytes, s, pa, pb, fa, fb, a, b); \
  if ((e = hipGetLastError()) != hipSuccess) { return e; }
  a.xcd_map = 0; a.edge_chunk = 0;
  if (fast_chunks > 0) {
    const dim3 grid((unsigned)fast_chunks, (unsigned)pa.n_ch);
    a.xcd_map = (xcd_map_wanted(false) && ((int64_t)grid.x * grid.y) % 8 == 0) ? 1 : 0;   // off by default here: -3 % on config 5 (profiles/r3_xcd_map.txt)
    {
      if (limb) { ACDSP_CASCADE_LAUNCH(false, true, 1, grid) } else { ACDSP_CASCADE_LAUNCH(false, false, 1, grid) }
      // the complete chunks whose windows leave the call's samples: chunk 0 (history) and possibly the last one (its window ends
      // 16 n_slots - 256 R - off < 16 R samples behind the last output's input: every earlier chunk ends a whole chunk before that)
      a.xcd_map = 0;
      a.edge_chunk = (int32_t)(fast_chunks - 1);
      const dim3 egrid(fast_chunks > 1 ? 2u : 1u, (unsigned)pa.n_ch);
      if (limb) { ACDSP_CASCADE_LAUNCH(false, true, 2, egrid) } else { ACDSP_CASCADE_LAUNCH(false, false, 2, egrid) }
    }
  }
  if (fast_chunks < n_chunks) {
    a.xcd_map = 0;
    a.chunk0 = (int32_t)fast_chunks;
    const dim3 grid((unsigned)(n_chunks - fast_chunks), (unsigned)pa.n_ch);
    if (limb) { ACDSP_CASCADE_LAUNCH(true, true, 0, grid) } else { ACDSP_CASCADE_LAUNCH(true, false, 0, grid) }
  }
#undef ACDSP_CASCADE_LAUNCH
  return hipSuccess;
}

}  // namespace acdsp
