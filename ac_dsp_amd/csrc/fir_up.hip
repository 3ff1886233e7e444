// fir_up.hip -- exact interpolating (polyphase) FIR on the matrix cores.
//
// The formulation, the mapping onto the matrix cores and the kernel itself are in fir_up_kernels.hpp.  This unit holds the host plan and
// the dispatch and compiles the shape of 16-bit samples with two coefficient digit planes (launch_up_s221); fir_up_b.hip and fir_up_c.hip
// compile the other shapes, for compile time; fir_up_s8.hip / fir_up_s8_b.hip those of byte samples (one sample plane).
#include <stdlib.h>

#include <vector>

#include "fir_up_kernels.hpp"

namespace acdsp {

// ---------------------------------------------------------------------------------------------
// host: digit planes, Toeplitz fragments, correction table
// ---------------------------------------------------------------------------------------------
bool fir_up_plan(const int64_t *E, int L, int nt, int px, FirUpPlan *pl, std::vector<uint32_t> *frag, std::vector<int64_t> *corr) {
  if (L < 2 || L > 16 || (up_spc(L) * L) % 4 != 0 || nt < 1 || px < 1 || px > 4) { return false; }
  // K blocks: the window of a column spans its SPC samples and nt - 1 earlier ones
  const int SPC = up_spc(L);
  int nb = 1;
  while (32 * nb - SPC < nt - 1) { nb++; }
  if (nb > 2) { return false; }
  std::vector<std::vector<int8_t>> dig(kUpMaxPC, std::vector<int8_t>((size_t)L * nt, 0));
  int pc = 1;
  for (int i = 0; i < L * nt; i++) {
    __int128 v = E[i];
    for (int q = 0; q < kUpMaxPC; q++) {
      const int lo = pop_balanced_digit(v);
      dig[q][(size_t)i] = (int8_t)lo;
      if (lo != 0 && q + 1 > pc) { pc = q + 1; }
    }
    if (v != 0) { return false; }
  }
  pl->L = L; pl->nt = nt; pl->pc = pc; pl->nb = nb; pl->hs = 2 * nb;
  frag->assign((size_t)nb * kUpMaxPC * 64 * 4, 0u);
  for (int b = 0; b < nb; b++) {
    for (int q = 0; q < kUpMaxPC; q++) {
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 31, kg = lane >> 5;
        const int d = i / L, j = i % L;
        for (int dw = 0; dw < 4; dw++) {
          uint32_t word = 0;
          for (int bj = 0; bj < 4; bj++) {
            const int kappa = 32 * b + 16 * kg + 4 * dw + bj;
            const int tap = 32 * nb - SPC + d - kappa;
            const int8_t val = (d < SPC && tap >= 0 && tap < nt) ? dig[q][(size_t)j * nt + tap] : (int8_t)0;   // rows past SPC * L: idle
            word |= (uint32_t)(uint8_t)val << (8 * bj);
          }
          (*frag)[((((size_t)b * kUpMaxPC) + q) * 64 + lane) * 4 + dw] = word;
        }
      }
    }
  }
  // re-bias of the px - 1 unsigned planes: x = signed planes + 128 * sum_{p < px-1} 256^p
  unsigned __int128 bias = 0;
  for (int pp = 0; pp < px - 1; pp++) { bias += ((unsigned __int128)128) << (8 * pp); }
  corr->assign((size_t)L, 0);
  for (int j = 0; j < L; j++) {
    unsigned __int128 s = 0;
    for (int k = 0; k < nt; k++) { s += (unsigned __int128)(__int128)E[(size_t)j * nt + k]; }
    (*corr)[(size_t)j] = (int64_t)(uint64_t)(s * bias);
  }
  return true;
}

bool fir_up_shape_ok(int in_eb, int px, int nb, int L, int out_eb) {
  if (nb < 1 || nb > 2 || (L != 2 && L != 4 && L != 8 && L != 16 && L != 7 && L != 3 && L != 5 && L != 6)) { return false; }
  if (in_eb == 2 && px == 2) { return out_eb == 2 || (out_eb == 4 && nb == 1) || out_eb == 8; }
  if (in_eb == 4 && px == 4) { return nb == 1 && out_eb == 8; }
  if (in_eb == 1 && px == 1) { return out_eb == 1 || out_eb == 2; }   // byte samples (fir_up_s8.hip): 4- / 8-byte outputs stay on the VALU kernels
  return false;
}

hipError_t launch_up_s221(const UpArgs &a, const uint32_t *d_frag, int L, int out_eb, int epi, dim3 grid, hipStream_t s) {
  return launch_up_l<int16_t, 2, 2, 1>(a, d_frag, L, out_eb, epi, grid, s);
}

// Input slots [slot0, slot0 + 32 n_steps) of every channel; the caller covers everything else with the VALU kernels.
hipError_t launch_fir_up(const FirParams &p, const FirUpPlan &pl, int px, const uint32_t *d_frag, const int64_t *d_corr, int mode, int w_int,
                         int out_simple, uint32_t sh_mask, int64_t max_abs_v, int64_t slot0, int64_t n_steps, int64_t out_off, hipStream_t s) {
  if (n_steps <= 0) { return hipSuccess; }
  if (!fir_up_shape_ok(p.in_eb, px, pl.nb, pl.L, p.out_eb) || slot0 < pl.hs) { return hipErrorNotSupported; }
  UpArgs a;
  a.p = p; a.slot0 = slot0; a.n_steps = n_steps; a.out_off = out_off; a.mode = mode; a.w_int = w_int; a.out_simple = out_simple;
  a.sh_mask = sh_mask; a.corr = d_corr;
  a.e_rs = a.e_rnd = a.e_w = 0; a.e_lo = INT32_MIN; a.e_hi = INT32_MAX; a.e_mask = ~uint64_t(0);
  a.c_rnd = 0; a.c_lo = INT64_MIN; a.c_hi = INT64_MAX; a.c_rs = a.c_ls2 = a.c_ko = 0;
  int epi = 0;
  const int rs = p.acc.F - p.out.F;
  // bits (sign included) the accumulator value can reach: the host's bound on |V| where it has one, else ACC_TYPE's width
  int acc_bits = p.acc.W;
  if (mode == 0 && max_abs_v >= 0 && p.lossless_shift >= 0 && p.lossless_shift < 32) {
    int vb = 0;
    while (vb < 62 && (int64_t(1) << vb) <= max_abs_v) { vb++; }
    if (vb + p.lossless_shift + 1 < acc_bits) { acc_bits = vb + p.lossless_shift + 1; }
  }
  if (mode == 0 && (px == 2 || px == 1) && p.lossless_shift == 0 && rs >= 0 && rs <= 28 && (p.out_eb == 2 || p.out_eb == 1) &&
      (p.out.Q == ACDSP_TRN || p.out.Q == ACDSP_RND) && (p.out.O == ACDSP_SAT || (p.out.O == ACDSP_WRAP && p.out.W == 8 * p.out_eb)) &&
      max_abs_v >= 0 && max_abs_v < (int64_t(1) << 30)) {
    // 32-bit epilogue: poly_intr, no left shift into ACC_TYPE, |V| (+ rounding constant) inside int32; AC_SAT clamps, AC_WRAP at
    // the container width is the truncation of the 16-bit (1-byte rows: 8-bit) store
    epi = 1;
    a.e_rs = rs;
    a.e_rnd = (p.out.Q == ACDSP_RND && rs > 0) ? (1 << (rs - 1)) : 0;
    if (p.out.O == ACDSP_SAT) { a.e_lo = (int32_t)p.out.lo; a.e_hi = (int32_t)p.out.hi; }
  } else if (mode == 0 && (px == 2 || (px == 4 && p.out_eb == 8)) && (p.out_eb == 8 || (p.out_eb == 4 && pl.nb == 1)) && p.out.S && (p.out.Q == ACDSP_TRN || p.out.Q == ACDSP_RND) &&
             (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT) && p.lossless_shift >= 0 && p.lossless_shift < 32 && rs >= -16 && rs <= 62 &&
             acc_bits + (rs < 0 ? -rs : 0) <= 63 && p.out.W >= 2 && p.out.W <= 8 * p.out_eb) {
    // exact-accumulation class into wider containers: the conversion without the generic epilogue's branches
    epi = 4;
    a.c_rs = rs > 0 ? rs : 0; a.c_ls2 = rs < 0 ? -rs : 0;
    a.c_rnd = (p.out.Q == ACDSP_RND && rs > 0) ? (int64_t(1) << (rs - 1)) : 0;
    if (p.out.O == ACDSP_SAT) { a.c_lo = p.out.lo; a.c_hi = p.out.hi; a.c_ko = 0; }
    else { a.c_lo = INT64_MIN; a.c_hi = INT64_MAX; a.c_ko = 64 - p.out.W; }
  } else if (mode == 1 && out_simple >= 1) {
    // bit-field wrap of the high word: to INT_TYPE, then (out_simple 1) to an OUT_TYPE of the same fraction with AC_WRAP
    const int wo = out_simple == 2 ? w_int : p.out.W, so = out_simple == 2 ? 1 : p.out.S;
    const int wmin = wo < w_int ? wo : w_int;
    if (w_int > 32 && wmin > 32 && wmin < 64 && (so || wo <= w_int)) {
      epi = 2;
      a.e_w = wmin - 32;
      if (!so) { a.e_mask = (uint64_t)(~uint32_t(0) >> (64 - wo)); }
    } else if (w_int <= 32 && p.out_eb == 4 && wmin >= 1 && (so || wo <= w_int)) {
      epi = 3;
      a.e_rs = 32 - wmin;   // (y << rs) >> rs: sign-extending wrap to wmin bits
      if (!so) { a.e_mask = (uint64_t)(~uint32_t(0) >> (32 - wo)); }
    }
  }
  // one-shot waves of about 32 KB of outputs, dispatched in memory order (fir_up_kernel's NST)
  const int64_t spw = up_nst(pl.L, p.out_eb, epi);
  a.steps_per_wave = spw;
  dim3 grid((unsigned)((n_steps + spw - 1) / spw), (unsigned)p.n_ch);
  // XCD-affine chunk order: loses 2 - 5 % on both interpolator rows in the one-shot form (profiles/r4_up_oneshot.txt); ACDSP_XCD_MAP=1 forces it
  a.xcd_map = (xcd_map_wanted(false) && ((int64_t)grid.x * grid.y) % 8 == 0) ? 1 : 0;
  if (p.in_eb == 1) {
    // byte samples: poly_intr only (the CIC interpolator's thin stream is refused under the flag); one sample plane, shapes as for int16
    if (mode != 0) { return hipErrorNotSupported; }
    if (pl.nb == 1 && pl.pc <= 2) { return launch_up_b121(a, d_frag, pl.L, p.out_eb, epi, grid, s); }
    return pl.nb == 1 ? launch_up_b131(a, d_frag, pl.L, p.out_eb, epi, grid, s) : launch_up_b132(a, d_frag, pl.L, p.out_eb, epi, grid, s);
  }
  if (p.in_eb == 2) {
    if (mode == 0) {
      // poly_intr: the pair taps E_j -+ E_cj can have 17 bits = 3 digit planes; sets whose folded taps stay inside two planes
      // (|tap| < 2^15: e.g. any low-pass with sum |c| < 2) skip the third plane's MFMAs and its accumulator
      if (pl.nb == 1 && pl.pc <= 2) { return launch_up_s221(a, d_frag, pl.L, p.out_eb, epi, grid, s); }
      return pl.nb == 1 ? launch_up_s231(a, d_frag, pl.L, p.out_eb, epi, grid, s)
                        : launch_up_s232(a, d_frag, pl.L, p.out_eb, epi, grid, s);
    }
    // CIC: boxcar^N taps in two digit planes (the BASELINE shapes) or three (R^(N-1) past 2^15: R = 16 at N = 5)
    if (pl.nb != 1) { return hipErrorNotSupported; }
    return pl.pc <= 2 ? launch_up_s221(a, d_frag, pl.L, p.out_eb, epi, grid, s) : launch_up_s231(a, d_frag, pl.L, p.out_eb, epi, grid, s);
  }
  if (pl.nb != 1) { return hipErrorNotSupported; }
  return pl.pc <= 2 ? launch_up_i421(a, d_frag, pl.L, p.out_eb, epi, grid, s) : launch_up_i431(a, d_frag, pl.L, p.out_eb, epi, grid, s);
}

}  // namespace acdsp
