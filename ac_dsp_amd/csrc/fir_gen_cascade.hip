// fir_gen_cascade.hip -- host side and instantiations of the fused decimator -> FIR cascade (cascade_kernel, fir_gen_kernels.hpp):
// BASELINE config 5, a decimating FIR on int16 input feeding a FIR on its INT_TYPE words without the intermediate leaving the CU.
// The same cascade on 1-byte rows (ACDSP_DDC_IN_BYTES) is the family cascade_kernel<int8_t, 1, 3, 6, 5, 4, 2, 3, ...>: this unit decides
// and fills its arguments too, fir_gen_cascade_s8.hip holds those instantiations.
#include <cstdlib>
#include <cstring>

#include "fir_gen_kernels.hpp"

namespace acdsp {

// The compiled shapes and conversions of the cascade: plans, plane counts, slot count, conversion constants and re-bias corrections of both
// stages.  plb == nullptr: stage A and the formats only (what a handle knows before its coefficients).  Two families on the same stage-A plan
// class (R, K blocks, digit planes): int16 rows -- two sample planes, an INT_TYPE of 33 .. 40 bits on five planes -- and 1-byte rows -- one
// sample plane, 25 .. 32 bits on four planes.  (fir_gen_cascade_dec.hip asks with plb == nullptr and adds its own, decimating, stage B.)
bool cascade_args(const FirParams &pa, const FirGenPlan &pla, int w_int, const FirParams &pb, const FirGenPlan *plb, GenArgs &a, GenArgs &b) {
  memset(&a, 0, sizeof a); memset(&b, 0, sizeof b);
  const bool bytes = pa.in_eb == 1;          // one plane whatever the sign: unsigned bytes are re-biased on the way into LDS
  a.pl = pla;
  a.px = bytes ? 1 : (pa.in.W + (pa.in.S ? 0 : 1) + 7) / 8;
  b.px = (w_int + 7) / 8;
  a.n_slots = 15 * pla.R + 4 * pla.nb;
  const int spl = (a.n_slots + 63) / 64;
  bool shape_ok = (bytes ? (pa.in.W <= 8 && b.px == 4) : (pa.in_eb == 2 && a.px == 2 && b.px == 5)) && pla.pc <= 3 && pla.nb <= 6 && spl == 5 &&
                  (a.n_slots * 2 + 63) / 64 <= 9 && pla.R >= 2 && pb.out_eb == 4;
  if (plb) {
    b.pl = *plb;
    shape_ok = shape_ok && plb->pc <= 2 && plb->nb <= 3 && plb->R == 1 && plb->off == 128;
  }
  a.out_mode = 1; a.w_int = w_int; a.out_simple = 2;
  FirParams pint = pa;                       // stage A's "OUT_TYPE" is the INT_TYPE itself: wrap only
  pint.out = pb.in;
  const bool conv_a = gen_conv_params(pint, 1, w_int, &a) && a.e_rs == 0 && a.e_ls2 == 0 && a.e_ko <= a.e_ka && a.e_hi == INT64_MAX;
  const bool conv_b = gen_conv_params(pb, 0, 0, &b);
  if (!shape_ok || !conv_a || !conv_b) { return false; }
  a.corr = gen_rebias_corr(a.px, pla.sum_h);
  if (bytes && !pa.in.S) {                   // x = (x ^ 0x80 as a signed byte) + 128; the kernel takes corr != 0 as the flag of that re-bias
    a.corr = (int64_t)((uint64_t)pla.sum_h * 128);
    if (a.corr == 0) { return false; }
  }
  if (plb) { b.corr = gen_rebias_corr(b.px, plb->sum_h); }
  return true;
}

bool cascade_shape_ok(const FirParams &pa, const FirGenPlan &pla, int w_int, const FirParams &pb, const FirGenPlan *plb) {
  GenArgs a, b;
  return cascade_args(pa, pla, w_int, pb, plb, a, b);
}

// pa: stage A (decimator) -- in / x / hist / hl / in_stride / n / n_ch as for launch_fir_gen with out_mode 1;
// pb: stage B formats (in = the INT_TYPE, acc, out, lossless_shift) and the output buffer (y, out_stride, int32 containers).
// Returns hipErrorNotSupported when the shapes are not the compiled ones (the caller then runs the two kernels).
hipError_t launch_cascade(const FirParams &pa, const FirGenPlan &pla, const uint32_t *d_fragA, int w_int, int64_t first,
                          const FirParams &pb, const FirGenPlan &plb, const uint32_t *d_fragB, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) { return hipSuccess; }
  GenArgs a, b;
  const bool bytes = pa.in_eb == 1;
  const bool out_ok = ((uintptr_t)pb.y % 16 == 0) && ((pb.out_stride * 4) % 16 == 0);
  if (!cascade_args(pa, pla, w_int, pb, &plb, a, b) || !out_ok) { return hipErrorNotSupported; }
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
  const size_t lds_bytes = (size_t)a.obuf_off + (size_t)b.px * 512 + 1024 + (clp_env ? (size_t)atoi(clp_env) : 0);
  const int64_t n_chunks = (a.n_steps + spw - 1) / spw, fast_chunks = n_out / (spw * 256);
  const v4i *fa = (const v4i *)d_fragA, *fb = (const v4i *)d_fragB;

  // 32-bit limb epilogues: the exact stage results are small enough that byte / 16-bit carry chains in 32-bit registers
  // reproduce them (no 64-bit arithmetic per output).  Conditions: the true |y| of both stages bounded well inside int64
  // (sum |h| x the input range), no ACC_TYPE wrap in stage B, a right shift of 0..31 bits into an OUT_TYPE of <= 31 bits,
  // and for AC_SAT an OUT range that reaches into the high limb.
  static const bool no_limb = getenv("ACDSP_NO_LIMB") != nullptr;   // A/B knob
  auto digits = [](__int128 c, int nw, int32_t *dig) {   // balanced base-256 digits, the last one takes the rest
    for (int w = 0; w < nw - 1; w++) { dig[w] = pop_balanced_digit(c); }
    dig[nw - 1] = (int32_t)c;
    return c > -(int64_t(1) << 20) && c < (int64_t(1) << 20);
  };
  bool limb;
  if (bytes) {
    // Byte rows.  Stage A: the word y = acc_0 + (acc_1 << 8) + (acc_2 << 16) stands in ONE 32-bit register: sum|h| x 128 (a re-biased byte
    // is a signed one) plus the correction lies inside int32.  Stage B: five weight classes z = sum_w acc_w 2^(8w) in two limbs with 16-bit
    // carries: |acc_w| <= |dig_w| + 128 x (sum_k |digit_q[k]| over the digit planes q with 0 <= w - q < 4), and every pair
    // acc_w + 256 acc_(w+1) plus a carry below 2^16 must stay inside int32.  The FIR's lossless shift ls = F_acc - F_in - F_coeff (8 with <8,1>
    // samples, <16,1> coefficients and <60,30> sums; 0 on the int16 family's north-star row) is taken out of the rounding shift:
    //   ((z << ls) + rnd) >> rs  =  (z + (rnd >> ls)) >> (rs - ls)   for rs >= ls,
    // the low ls bits of z << ls being zero (rs == ls: the constant 2^(ls-1) never carries and rnd >> ls is 0).
    const __int128 bound_a = (__int128)pla.sum_abs_h * 128 + (a.corr < 0 ? -(__int128)a.corr : (__int128)a.corr);
    const int rs = b.e_rs - b.e_ls;
    const __int128 bound_b = ((__int128)plb.sum_abs_h << (w_int - 1 + b.e_ls)) + b.e_rnd;   // |(stage-B dot product << ls) + rounding constant|
    limb = !no_limb && bound_a < ((__int128)1 << 31) && plb.sum_abs_h < (int64_t(1) << 20) && b.e_ls2 == 0 && rs >= 0 && rs <= 31 && pb.out.W <= 31 &&
           bound_b < ((__int128)1 << 61) && (pb.acc.W >= 63 || bound_b < ((__int128)1 << (pb.acc.W - 1)));
    limb = limb && digits(a.corr, 3, a.dig) && digits((__int128)b.corr + (b.e_rnd >> b.e_ls), 5, b.dig);
    if (limb) {
      int64_t aw[5];
      for (int w = 0; w < 5; w++) {
        aw[w] = b.dig[w] < 0 ? -(int64_t)b.dig[w] : (int64_t)b.dig[w];
        for (int q = 0; q < plb.pc; q++) { if (w - q >= 0 && w - q < 4) { aw[w] += 128 * plb.dig_abs[q]; } }
      }
      const int64_t top = (int64_t(1) << 31) - (int64_t(1) << 16);
      limb = aw[0] + 256 * aw[1] < top && aw[2] + 256 * aw[3] < top && aw[4] < top;
    }
    if (limb) {
      // the high limb H = z >> 32 is clamped to [-2^hb - 1, 2^hb], hb = max(W - 1 + rs - 32, 0), in front of the funnel shift: a clamped H
      // saturates to the side the true one does, and (H : L) >> rs then fits int32 where rs >= hb + 2 (hb > 0: that is W <= 31)
      const int hb0 = pb.out.W - 1 + rs - 32, hb = hb0 < 0 ? 0 : hb0;
      if (pb.out.O == ACDSP_SAT) {
        limb = hb <= 29 && rs >= hb + 2;
        b.l_hb_lo = -(1 << (hb <= 29 ? hb : 0)) - 1; b.l_hb_hi = 1 << (hb <= 29 ? hb : 0);
        b.l_lo = (int32_t)b.e_lo; b.l_hi = (int32_t)b.e_hi; b.l_w = pb.out.W;
      } else {
        b.l_hb_lo = b.l_lo = INT32_MIN; b.l_hb_hi = b.l_hi = INT32_MAX; b.l_w = pb.out.W;
      }
      if (limb) { b.e_rs = rs; }   // (the limb epilogue reads nothing else of the conversion)
    }
  } else {
    limb = !no_limb && w_int >= 33 && w_int <= 40 && pla.sum_abs_h < (int64_t(1) << 38) && plb.sum_abs_h < (int64_t(1) << 20);
    const int64_t bound_b = limb ? plb.sum_abs_h * (int64_t(1) << (w_int - 1)) + b.e_rnd : 0;   // |stage-B dot product + rounding constant|
    limb = limb && b.e_ls == 0 && b.e_ls2 == 0 && b.e_rs <= 31 && pb.out.W <= 31 && bound_b < (int64_t(1) << 61) &&
           (pb.acc.W >= 63 || bound_b < (int64_t(1) << (pb.acc.W - 1)));
    if (limb) {
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
  }
  hipError_t e;
#define ACDSP_CASCADE_LAUNCH(GUARD_, LIMB_, PART_, GRID_)                                                                            \
  if (bytes) {                                                                                                                       \
    if ((e = launch_cascade_s8(GUARD_, LIMB_, PART_, GRID_, lds_bytes, s, pa, pb, fa, fb, a, b)) != hipSuccess) { return e; }          \
  } else {                                                                                                                           \
    e = hipFuncSetAttribute((const void *)cascade_kernel<int16_t, 2, 3, 6, 9, 5, 2, 3, GUARD_, LIMB_, PART_>,                        \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);                                             \
    if (e != hipSuccess) { return e; }                                                                                               \
    hipLaunchKernelGGL((cascade_kernel<int16_t, 2, 3, 6, 9, 5, 2, 3, GUARD_, LIMB_, PART_>), GRID_, dim3(64), lds_bytes, s, pa, pb, fa, fb, a, b); \
    if ((e = hipGetLastError()) != hipSuccess) { return e; }                                                                         \
  }
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
