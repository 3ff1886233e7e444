// fir_gen.hip -- generalised exact FIR on the matrix cores: wide inputs, wide coefficients, decimation.  This unit holds the host
// planner, the selection of the compiled shape, launch_fir_gen and the instantiations of the window-per-step kernels; the kernels are
// templates of fir_gen_kernels.hpp, the ring kernel's instantiations and shape table are fir_gen_ring.hip's, the cascade fir_gen_cascade.hip's.
//
//     y[m] = sum_k h[k] * x[first + m*R - k]   (mod 2^64),   m = 0, 1, ...
//
// with x in 1..8 byte planes (16/32/64-bit containers), h in 1..4 balanced base-256 digit planes and an
// integer decimation factor R.  It serves
//   * the lossless FIR class for inputs wider than 16 bits (e.g. the 36-bit CIC output feeding the
//     DDC's 127-tap ac_fir_const_coeffs: reference ac_fir_const_coeffs.h:190-199 with IN = <36,21>),
//   * the CIC decimator through its FIR identity  H(z) = z^-(N-1) (1 + ... + z^-(R*M'-1))^N  taken
//     mod 2^outW (reference ac_cic_full_core.h:80-135,198-255; identity checked in
//     tests/test_oracle.py::test_cic_closed_form_fir_identity): the N wide adds per input sample of
//     intStage become a handful of int8 MFMAs per 256 outputs.
//
// Mapping (v_mfma_i32_16x16x64_i8).  One wave = one channel x a chunk of steps; a step is 256 outputs:
// column n = output block m0+16n .. +15, row i = output inside the block.  With W_n = the 16-aligned
// start of column n's input window (W_n = W_0 + 16*R*n) and off = T_n - W_n (constant),
//     D[i][n] = sum_kappa A[i][kappa] * X[kappa][n],   A[i][kappa] = h[off + i*R - kappa],
//     X[kappa][n] = x[W_n + kappa],  kappa in [0, 64*NB).
// Both operands are split into byte planes; plane products with equal weight p+q share one int32
// accumulator (4 VGPRs); the 64-bit recombination, the re-bias correction of the unsigned input planes
// and the OUT_TYPE conversion happen once per output in the epilogue.
//
// Data movement.  Lane <-> 16-sample slot: a lane loads its slot (16*sizeof(TIN) contiguous bytes),
// builds one 16-byte vector per plane (v_perm_b32 byte gathers) and writes it to the plane array in
// LDS; column n / K-group kg / block b then reads slot R*n + 4b + kg.  For even R the slot index is
// padded by slot/R so that the 16 columns of a read hit 16 different 16-byte bank groups.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fir_gen_kernels.hpp"

namespace acdsp {

// ---------------------------------------------------------------------------------------------
// host: coefficient planes and A fragments
// ---------------------------------------------------------------------------------------------
// window geometry: T_n mod 16 == first mod 16; window start is the 16-aligned floor of T_n - (taps-1)
bool fir_gen_window(int n_taps, int R, int first_mod16, int *off, int *nb) {
  if (n_taps < 1 || R < 1 || R > 64) { return false; }
  const int a = ((first_mod16 - (n_taps - 1)) % 16 + 16) % 16;
  *off = (n_taps - 1) + a;
  *nb = (*off + 15 * R + 1 + 63) / 64;
  return *nb <= kGenMaxNB;
}

bool fir_gen_plan(const int64_t *h, int n_taps, int R, int first_mod16, FirGenPlan *pl, std::vector<uint32_t> *frag) {
  // balanced base-256 digits of every tap
  int pc = 1;
  std::vector<std::vector<int8_t>> dig(kGenMaxPC, std::vector<int8_t>(n_taps, 0));
  if (n_taps < 1 || R < 1 || R > 64) { return false; }
  for (int k = 0; k < n_taps; k++) {
    __int128 v = h[k];
    for (int q = 0; q < kGenMaxPC; q++) {
      const int lo = pop_balanced_digit(v);
      dig[q][k] = (int8_t)lo;
      if (lo != 0 && q + 1 > pc) { pc = q + 1; }
    }
    if (v != 0) { return false; }  // needs more than kGenMaxPC digits (dig[][] has exactly kGenMaxPC rows)
  }
  int off, nb;
  if (!fir_gen_window(n_taps, R, first_mod16, &off, &nb)) { return false; }
  pl->pc = pc; pl->nb = nb; pl->off = off; pl->R = R;
  __int128 sum = 0, sum_abs = 0;
  for (int k = 0; k < n_taps; k++) { sum += (__int128)h[k]; sum_abs += h[k] < 0 ? -(__int128)h[k] : (__int128)h[k]; }
  pl->sum_h = (int64_t)(unsigned long long)sum;  // mod 2^64
  pl->sum_abs_h = sum_abs < ((__int128)1 << 62) ? (int64_t)sum_abs : (int64_t(1) << 62);
  for (int q = 0; q < kGenMaxPC; q++) {
    int64_t sa = 0;
    for (int k = 0; k < n_taps; k++) { sa += dig[q][k] < 0 ? -(int64_t)dig[q][k] : (int64_t)dig[q][k]; }
    pl->dig_abs[q] = sa;
  }
  frag->assign((size_t)pc * nb * 64 * 4, 0u);
  for (int q = 0; q < pc; q++) {
    for (int b = 0; b < nb; b++) {
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, kg = lane >> 4;
        for (int dw = 0; dw < 4; dw++) {
          uint32_t word = 0;
          for (int bj = 0; bj < 4; bj++) {
            const int kappa = 64 * b + 16 * kg + 4 * dw + bj;
            const int tap = off + i * R - kappa;
            const int8_t val = (tap >= 0 && tap < n_taps) ? dig[q][tap] : (int8_t)0;
            word |= (uint32_t)(uint8_t)val << (8 * bj);
          }
          (*frag)[(((size_t)q * nb + b) * 64 + lane) * 4 + dw] = word;
        }
      }
    }
  }
  return true;
}

// LDS slot map of a plane.  The MFMA operand read of lane (n_col, kg) is slot R n_col + 4 b + kg, a ds_read_b128, which the LDS
// serves in four NON-contiguous 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, +32: MI355X_MICROARCH.md, LDS) over 64
// dword banks = 16 slots: a group holds eight columns at kg and the other eight at kg + 1.  With R a multiple of 4, TWO empty slots
// after every R make column n start at (R + 2) n: the eight columns of one half land on eight distinct even offsets mod 16 and the
// other half, one slot on, on the odd ones -- no conflict for any K block.  (Round 2 padded ONE slot per R, right for contiguous
// 16-lane groups and 4 extra cycles per K-block read on the real ones: the 24 - 33 % SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of
// configs 3, 5 and poly_dec in profiles/r2_*.)  R = 2 mod 4 is conflict-free as it stands; odd R keeps the identity (one or two
// extra cycles per group).  The staging writes are consecutive slots, 8 of them (32 banks) per bank pass: holes at multiples of 8
// slots leave them conflict-free (R = 4 mod 8: 2-way on some passes).  An XOR map (bits 1 - 3 of the slot ^ the column index) does
// the same without the holes and was measured first; it is not an add, so the cascade kernel could no longer address its ten
// staging pieces as one base register + immediates, and the register allocation of that kernel (255 VGPRs) fell over: +3 .. +35 %
// on the fused DDC depending on the form.  tools/lds_slot_map_check.py replays the lane groups for any R and map.
// Returns the slots a plane must allocate for n slots.
int gen_slot_map(GenArgs &a, int R, int n) {
  a.rcp = (uint32_t)((0x100000000ull + R - 1) / R);
  a.pad = (R % 4 == 0) ? 1 : 0;
  return a.pad ? n + 2 * (n / R) : n;
}

template <typename TIN, int PX, int PCT, int NBT, int NLD, int OEB>
static hipError_t launch_fast(dim3 grid, size_t lds_bytes, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
  hipError_t e = hipFuncSetAttribute((const void *)fir_gen_fast_kernel<TIN, PX, PCT, NBT, NLD, OEB>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) { return e; }
  hipLaunchKernelGGL((fir_gen_fast_kernel<TIN, PX, PCT, NBT, NLD, OEB>), grid, dim3(64), lds_bytes, s, p, frag, a);
  return hipGetLastError();
}

template <typename TIN>
static hipError_t launch_px(int px, dim3 grid, size_t lds_bytes, hipStream_t s, const FirParams &p, const v4i *frag, const GenArgs &a) {
  const bool small = a.pl.nb <= 3 && a.pl.pc <= 2;
#define ACDSP_GEN_CASE(PXV)                                                                                         \
  case PXV: {                                                                                                       \
    if (small) {                                                                                                    \
      hipError_t e = hipFuncSetAttribute((const void *)fir_gen_kernel<TIN, PXV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
      if (e != hipSuccess) { return e; }                                                                            \
      hipLaunchKernelGGL((fir_gen_kernel<TIN, PXV, true>), grid, dim3(64), lds_bytes, s, p, frag, a);             \
    } else {                                                                                                        \
      hipError_t e = hipFuncSetAttribute((const void *)fir_gen_kernel<TIN, PXV, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
      if (e != hipSuccess) { return e; }                                                                            \
      hipLaunchKernelGGL((fir_gen_kernel<TIN, PXV, false>), grid, dim3(64), lds_bytes, s, p, frag, a);            \
    }                                                                                                               \
    return hipGetLastError();                                                                                       \
  }
  // byte planes never exceed the container (launch_fir_gen checks px <= in_eb): only those instantiations exist
  if (px > (int)sizeof(TIN)) { return hipErrorInvalidValue; }
  if constexpr (sizeof(TIN) == 1) {   // byte samples (ACDSP_FLAG_IN_BYTES): one plane
    switch (px) { ACDSP_GEN_CASE(1) default: return hipErrorInvalidValue; }
  } else if constexpr (sizeof(TIN) == 2) {
    switch (px) { ACDSP_GEN_CASE(1) ACDSP_GEN_CASE(2) default: return hipErrorInvalidValue; }
  } else if constexpr (sizeof(TIN) == 4) {
    switch (px) { ACDSP_GEN_CASE(1) ACDSP_GEN_CASE(2) ACDSP_GEN_CASE(3) ACDSP_GEN_CASE(4) default: return hipErrorInvalidValue; }
  } else {
    switch (px) {
      ACDSP_GEN_CASE(1) ACDSP_GEN_CASE(2) ACDSP_GEN_CASE(3) ACDSP_GEN_CASE(4)
      ACDSP_GEN_CASE(5) ACDSP_GEN_CASE(6) ACDSP_GEN_CASE(7) ACDSP_GEN_CASE(8)
      default: return hipErrorInvalidValue;
    }
  }
#undef ACDSP_GEN_CASE
}

// Branch-free output conversion of the fast kernels (GenArgs::e_*): false if the formats need the general requant64.
bool gen_conv_params(const FirParams &p, int out_mode, int w_int, GenArgs *a, int src_bits) {
  bool conv_ok = p.out.S && (p.out.Q == ACDSP_TRN || p.out.Q == ACDSP_RND) && (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT) &&
                 p.out.W >= 2 && p.out.W <= 64;
  int f_src = 0;
  if (out_mode == 1) { a->e_ls = 0; a->e_ka = 64 - w_int; f_src = p.in.F; conv_ok = conv_ok && w_int >= 2 && w_int <= 64; }
  else {
    a->e_ls = p.lossless_shift; a->e_ka = 64 - p.acc.W; f_src = p.acc.F;
    conv_ok = conv_ok && p.acc.S && p.acc.W >= 2 && p.acc.W <= 64 && p.lossless_shift >= 0 && p.lossless_shift < 64;
  }
  // src_bits > 0: the host has bounded the accumulator VALUE to that many bits (sign included), whatever its type's width
  const int rs = f_src - p.out.F, src_w0 = out_mode == 1 ? w_int : p.acc.W, src_w = (src_bits > 0 && src_bits < src_w0) ? src_bits : src_w0;
  a->e_rs = rs > 0 ? rs : 0; a->e_ls2 = rs < 0 ? -rs : 0;
  a->e_rnd = (p.out.Q == ACDSP_RND && rs > 0 && rs < 63) ? (int64_t(1) << (rs - 1)) : 0;
  // neither the rounding add nor the left shift can leave int64 (a 63- / 64-bit source with neither of them -- AC_TRN or rs <= 0, no left shift:
  // the reference testbench's ACC = OUT <64,32> -- is safe as it is)
  conv_ok = conv_ok && a->e_rs <= 62 && (src_w + a->e_ls2 <= 62 || (a->e_rnd == 0 && a->e_ls2 == 0));
  if (p.out.O == ACDSP_SAT) {
    a->e_hi = (int64_t)((uint64_t(1) << (p.out.W - 1)) - 1); a->e_lo = -a->e_hi - 1; a->e_ko = 0;
  } else {
    a->e_hi = INT64_MAX; a->e_lo = INT64_MIN; a->e_ko = 64 - p.out.W;
  }
  return conv_ok;
}

int64_t gen_rebias_corr(int px, int64_t sum_h) {   // 128 * sum(h) * sum_{p < px-1} 256^p  (mod 2^64)
  unsigned __int128 bias = 0;
  for (int q = 0; q < px - 1; q++) { bias += (unsigned __int128)1 << (8 * q); }
  return (int64_t)(unsigned long long)((unsigned __int128)128 * bias * (unsigned long long)sum_h);
}

// Slot tables of the LZ residue loops (see fir_gen_ring_kernel).  With P0 the ring sample of (output r = 0, tap 0) of a lane -- parity
// b = off & 1 for every lane -- iteration m of a loop over taps T0 + i' reads the dwords holding samples P0 + woff - 2 m .. + 5:
//   b' = (b - T0) & 1;  woff = -T0 + b' - 2;  b' = 0: slot D = tap 2m, slot S = tap 2m + 1;  b' = 1: slot S = tap 2m, slot D = tap 2m - 1.
// The mirror sample of tap i is P0 - (N-1-i): a second window that slides UP from voff = -N + 1 - b (N odd: the mirror of a direct
// slot is direct) or -N - b (N even: it is the shifted one and vice versa).
bool fir_gen_lossy_table(const FirGenPlan &pl, const int64_t *coeffs, int n_taps, int n_pair, int n_single, int single0, int neg, int s, bool rnd,
                         FirLossyPlan *out, std::vector<uint32_t> *tab) {
  const uint32_t m1 = (1u << s) - 1, hh = rnd ? (1u << (s - 1)) : 0u;
  auto cl2 = [&](int tap) -> uint32_t { const uint32_t v = (uint32_t)((uint64_t)coeffs[tap] & m1); return v | (v << 16); };
  tab->assign(kLossyTabWords, 0u);
  const int b = pl.off & 1;
  // one loop over `cnt` taps from T0 on: iterations and slot taps
  auto build = [&](int T0, int cnt, int word0, int *n_it, int *woff) {
    const int bp = (b - T0) & 1;
    *woff = -T0 + bp - 2;
    *n_it = cnt <= 0 ? 0 : (bp == 0 ? (cnt + 1) / 2 : cnt / 2 + 1);
    for (int m = 0; m < *n_it; m++) {
      const int iS = bp == 0 ? 2 * m + 1 : 2 * m, iD = bp == 0 ? 2 * m : 2 * m - 1;
      if (word0 + 2 * m + 1 >= kLossyTabWords) { return false; }
      (*tab)[word0 + 2 * m] = (iS >= 0 && iS < cnt) ? cl2(T0 + iS) : 0u;
      (*tab)[word0 + 2 * m + 1] = (iD >= 0 && iD < cnt) ? cl2(T0 + iD) : 0u;
    }
    return true;
  };
  int p_n = 0, p_woff = 0, s_n = 0, s_woff = 0;
  if (!build(0, n_pair, 0, &p_n, &p_woff) || !build(single0, n_single, 2 * p_n, &s_n, &s_woff)) { return false; }
  const int slots = 2 * (p_n + s_n);
  if (slots < 1 || s > 15) { return false; }
  out->flush = (int32_t)(65535u / (2u * m1));      // iterations (two slots each) a 16-bit field holds: >= 1 for s <= 15
  out->s = s; out->neg = neg; out->var_y = (n_taps & 1) ? 0 : 1;
  out->p_n = p_n; out->p_woff = p_woff; out->p_voff = (n_taps & 1) ? -n_taps + 1 - b : -n_taps - b;
  out->s_n = s_n; out->s_woff = s_woff;
  out->h2 = hh | (hh << 16); out->m2 = m1 | (m1 << 16); out->k = (int64_t)slots * hh;
  return true;
}

// Which compiled shapes take a plan: pure host code -- the ACDSP_GEN_RING value is an argument -- so that it can be compared case by case.
//   in_eb / oeb: container bytes, px: byte planes of the samples, pc / nb / R: the plan, lz: class B,
//   conv_ok: the branch-free conversion covers the formats, out_vec_ok: the output rows are 16-byte aligned.
// Ring variant (fir_gen_ring_kernel) for the decimating BASELINE shapes.  ACDSP_GEN_RING=0: the window-per-step kernel (A/B
// reference); ACDSP_GEN_RING=spw,pf,nt,fb picks another compiled variant (steps per chunk, load distance, non-temporal loads,
// chunk-end store burst).  Defaults from same-process sweeps on three boxes (profiles/r4_ring_sweep.txt): TWO-step chunks with
// every load of the chunk issued up front (16 KB bursts on config 3, 8 KB on poly_dec) beat longer chunks by 3 - 5 % and the
// window-per-step kernel by 7 - 11 %; the store burst pays for 2-byte outputs (one 1 KB store per chunk instead of two half-wave
// ones) and costs occupancy for 8-byte outputs.
GenSelect fir_gen_select(int in_eb, int px, int pc, int nb, int oeb, int R, bool lz, bool conv_ok, bool out_vec_ok, const char *ring_env) {
  GenSelect sel = {nullptr, 0, 2, 2, 1, (oeb == 2) ? 1 : 0, px};
  // Fast kernel: table of compiled shapes (BASELINE configs 3, 5a, 5b and the poly_dec row); nbt = K blocks compiled in.
  const int n_slots = 15 * R + 4 * nb, spl = (n_slots + 63) / 64;
  const int npc = (n_slots * in_eb + 63) / 64;   // 16-byte pieces per lane
  if (in_eb == 4 && px == 4 && pc <= 2 && nb <= 3 && spl == 3 && npc <= 9 && oeb == 8) { sel.nbt = 3; }        // CIC R8 N5 on int32 -> int64
  else if (in_eb == 2 && px == 2 && pc <= 3 && nb <= 6 && spl == 5 && npc <= 9 && oeb == 8) { sel.nbt = 6; }   // CIC R16 N5 on int16 -> int64
  else if (in_eb == 8 && px == 5 && pc <= 2 && nb <= 3 && spl == 1 && oeb == 4) { sel.nbt = 3; }   // 127-tap FIR on 36-bit words -> int32
  else if (in_eb == 2 && px == 2 && pc <= 2 && nb <= 4 && spl == 3 && npc <= 5 && oeb == 2) { sel.nbt = 4; }   // 128-tap decimate-by-8 on int16 -> int16
  // ... and a conversion the branch-free form covers: signed wrapping accumulator, signed OUT, TRN/RND, WRAP/SAT
  bool ring_on = true;
  if (ring_env && !lz) {
    int v[4];
    if (sscanf(ring_env, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4) { sel.spw = v[0]; sel.pf = v[1]; sel.nt = v[2]; sel.fb = v[3]; }
    else { ring_on = atoi(ring_env) != 0; }
  }
  if (!conv_ok || !out_vec_ok || (!lz && !ring_on)) { return sel; }
  // 17 .. 24-bit samples in int32 containers (three planes) take the four-plane ring shapes where one fits: the containers are sign-extended, the
  // fourth plane is the sign -- 8 MFMAs more per step against the ring's better stream (CIC R8 M2 N3 on <24,8>: 0.71 on the window kernel)
  const int rpx = (!lz && in_eb == 4 && px == 3) ? 4 : px;
  int n_rows;
  const RingRow *rows = fir_gen_ring_rows(&n_rows);
  for (int i = 0; i < n_rows && !sel.row; i++) {
    const RingRow &r = rows[i];
    if (in_eb == r.in_eb && rpx == r.px && pc <= r.pct && nb <= r.nbt && oeb == r.oeb && R == r.R && (int)lz == r.lz &&
        (lz || !ring_env || r.env_ok)) { sel.row = &r; }
  }
  if (sel.row) {
    sel.px = rpx;
    if (lz || !ring_env) { sel.spw = sel.row->spw; sel.pf = sel.row->pf; }   // (class B ignores ACDSP_GEN_RING)
  }
  return sel;
}

// are this handle's (formats, plan) compiled as a class-B ring shape?
bool fir_gen_lossy_shape_ok(const FirParams &p, const FirGenPlan &pl, int acc_bits) {
  GenArgs a;
  FirParams q = p;
  q.lossless_shift = 0;
  return fir_gen_select(p.in_eb, p.in_eb, pl.pc, pl.nb, p.out_eb, pl.R, true, true, true, nullptr).row != nullptr && gen_conv_params(q, 0, 0, &a, acc_bits);
}

// The kernel argument block of a launch_fir_gen call and what fir_gen_select makes of it; *lds_bytes = dynamic LDS of the window-per-step
// kernels.  false: the planes do not fit the container.
static bool gen_fill_args(const FirParams &p, const FirGenPlan &pl, int out_mode, int w_int, int64_t first, int64_t n_out, const FirLossyPlan *lz,
                          GenArgs *args, GenSelect *select, bool *conv_ok_out, size_t *lds_bytes) {
  GenArgs &a = *args;
  a.pl = pl;
  a.ring_delta = 0;
  const int in_bits = p.in.W + (p.in.S ? 0 : 1);
  a.px = (in_bits + 7) / 8;
  const bool bytes = p.in_eb == 1;   // ACDSP_FLAG_IN_BYTES: one plane whatever the sign -- unsigned bytes are re-biased on the way into LDS
  if (bytes) { a.px = 1; }
  if (a.px > p.in_eb || (bytes && (lz || out_mode != 0))) { return false; }
  if (lz) {
    a.px = p.in_eb;                    // the containers are sign-extended: every byte of them is a plane (the ring shapes are compiled for that)
    a.lz_s = lz->s; a.lz_neg = lz->neg; a.lz_var_y = lz->var_y; a.lz_p_n = lz->p_n; a.lz_p_woff = lz->p_woff; a.lz_p_voff = lz->p_voff;
    a.lz_s_n = lz->s_n; a.lz_s_woff = lz->s_woff; a.lz_flush = lz->flush;
    a.lz_h2 = lz->h2; a.lz_m2 = lz->m2; a.lz_k = lz->k; a.lz_tab = lz->d_tab;
  } else {
    a.lz_s = 0; a.lz_neg = a.lz_var_y = a.lz_p_n = a.lz_p_woff = a.lz_p_voff = a.lz_s_n = a.lz_s_woff = a.lz_flush = 0; a.lz_h2 = a.lz_m2 = 0; a.lz_k = 0; a.lz_tab = nullptr;
  }
  a.n_slots = 15 * pl.R + 4 * pl.nb;
  // (out_mode 1) OUT_TYPE with INT_TYPE's fraction and AC_WRAP converts by bit-field wraps only
  a.out_mode = out_mode; a.w_int = w_int;
  a.out_simple = (out_mode == 1 && p.out.F == p.in.F && p.out.O == ACDSP_WRAP) ? ((p.out.S && p.out.W >= w_int) ? 2 : 1) : 0;
  a.first = first; a.n_out = n_out;
  a.n_steps = (n_out + 255) / 256;
  // Chunk length: four steps per wave (16 - 32 KB of input on the BASELINE shapes).  Workgroups are dispatched in memory order
  // (chunk index fastest), so the bytes the resident waves touch form a compact window that advances through both streams; short
  // spans keep that window small (DRAM page locality: tools/copy_probe2.hip -- 16 - 32 KB spans copy at 5.8 - 6.1 TB/s, 128+ KB
  // spans at 5.2).  The former rule (>= 16384 waves, i.e. 0.5 - 4 MB spans on the BASELINE shapes) ran cic_dec 6 %, polydec 11 %
  // slower; 3 - 4 steps measured best on both, 1 - 2 and 8+ lose 2 - 4 % (profiles/r3_span_sweep.txt).
  int64_t spw = 4;
  ACDSP_TUNE_ENV(spw_env, "ACDSP_GEN_SPW");   // tuning knob: steps (of 256 outputs) per wave
  if (spw_env && atoi(spw_env) > 0) { spw = atoi(spw_env); }
  a.n16 = (p.n + 15) / 16 * 16;
  a.out_vec_ok = ((uintptr_t)p.y % 16 == 0) && ((p.out_stride * p.out_eb) % 16 == 0);
  a.chunk0 = 0;
  const bool conv_ok = gen_conv_params(p, out_mode, w_int, &a, lz ? lz->acc_bits : 0);
  a.e_stages = ((a.e_ls != 0 || a.e_ka != 0) ? 1 : 0) | ((a.e_rnd != 0 || a.e_rs != 0 || a.e_ls2 != 0) ? 2 : 0) |
               ((a.e_lo != INT64_MIN || a.e_hi != INT64_MAX) ? 4 : 0) | (a.e_ko != 0 ? 8 : 0);
  ACDSP_TUNE_ENV(ring_env, "ACDSP_GEN_RING");
  const GenSelect sel = fir_gen_select(p.in_eb, a.px, pl.pc, pl.nb, p.out_eb, pl.R, lz != nullptr, conv_ok, a.out_vec_ok != 0, ring_env);
  a.px = sel.px;
  a.corr = gen_rebias_corr(a.px, pl.sum_h);
  if (bytes && !p.in.S) {   // x = (x ^ 0x80 as a signed byte) + 128; the kernels take corr != 0 as the flag of that re-bias
    a.corr = (int64_t)((uint64_t)pl.sum_h * 128);
    if (a.corr == 0) { return false; }
  }
  {
    // plane accumulator w sums the products of (input plane pp, coefficient digit q), pp + q = w, |plane byte| <= 128
    int64_t bw[kGenMaxPX + kGenMaxPC] = {0};
    for (int w = 0; w < a.px + pl.pc - 1; w++) {
      for (int q = 0; q < pl.pc; q++) { if (w - q >= 0 && w - q < a.px) { bw[w] += 128 * pl.dig_abs[q]; } }
    }
    bool pw_ok = true;
    for (int w = 0; w + 1 < kGenMaxPX + kGenMaxPC; w += 2) { pw_ok = pw_ok && (bw[w + 1] * 256 + bw[w] < (int64_t(1) << 31)); }
    static const bool no_pw = getenv("ACDSP_GEN_NO_PW") != nullptr;   // A/B knob
    a.pw = (pw_ok && !no_pw) ? 1 : 0;
  }
  if (sel.row) {
    spw = sel.spw;
    const int ls = 8 / p.in_eb;
    const int64_t w0slot = (first - pl.off) / 16;                      // exact: the plan aligns the window start to a slot
    a.ring_delta = (int32_t)(((w0slot % ls) + ls) % ls);
  }
  a.steps_per_wave = spw;
  const int phys_nb = sel.nbt > pl.nb ? sel.nbt : pl.nb;             // zero-fragment blocks still read their (stale) slots
  const int slots_alloc = 15 * pl.R + 4 * phys_nb;
  const int phys = gen_slot_map(a, pl.R, slots_alloc);
  a.obuf_off = a.px * (phys + 1) * 16;
  ACDSP_TUNE_ENV(lds_pad_env, "ACDSP_GEN_LDS_PAD");   // diagnostic: extra LDS bytes per wave (lowers the occupancy)
  *lds_bytes = (size_t)a.obuf_off + 2048 + (lds_pad_env ? (size_t)atoi(lds_pad_env) : 0);
  a.xcd_map = 0;
  *select = sel;
  *conv_ok_out = conv_ok;
  return true;
}

// p.n = inputs of this call; outputs m with first + m*R < n.  hist must hold >= off + 16 samples.
hipError_t launch_fir_gen(const FirParams &p_in, const FirGenPlan &pl, const uint32_t *d_frag, int out_mode, int w_int,
                          int64_t first, int64_t n_out, hipStream_t s, const FirLossyPlan *lz, int64_t *covered, int32_t *ring_id) {
  FirParams p = p_in;
  if (covered) { *covered = 0; }
  if (ring_id) { *ring_id = 0; }
  if (lz) { p.lossless_shift = 0; }   // class B: the exact sum is shifted RIGHT by lz->s in front of the ACC_TYPE wrap
  if (n_out <= 0) { return hipSuccess; }
  GenArgs a;
  GenSelect sel;
  bool conv_ok;
  size_t lds_bytes;
  if (!gen_fill_args(p, pl, out_mode, w_int, first, n_out, lz, &a, &sel, &conv_ok, &lds_bytes)) { return hipErrorInvalidValue; }
  if (lz && !sel.row) { return hipSuccess; }   // nothing covered: the caller's exact-order kernel takes the call
  const int in_eb = p.in_eb, oeb = p.out_eb;
  static const bool trace = getenv("ACDSP_GEN_TRACE") != nullptr;   // diagnostic: which compiled shape a launch resolves to
  if (trace) {
    fprintf(stderr, "[acdsp] fir_gen: in_eb %d px %d pc %d nb %d oeb %d R %d conv_ok %d out_vec_ok %d -> ring shape %d, window shape nbt %d\n", in_eb, a.px, pl.pc, pl.nb, oeb,
            pl.R, (int)conv_ok, (int)a.out_vec_ok, sel.row ? sel.row->id : 0, sel.nbt);
  }
  const int64_t spw = a.steps_per_wave;
  const int64_t n_chunks = (a.n_steps + spw - 1) / spw;
  const int64_t fast_chunks = ((sel.nbt || sel.row) && conv_ok && a.out_vec_ok) ? n_out / (spw * 256) : 0;   // chunks made of complete steps only
  const v4i *fr = (const v4i *)d_frag;
  if (fast_chunks > 0) {
    dim3 grid((unsigned)fast_chunks, (unsigned)p.n_ch);
    // XCD-affine chunk order (xcd_remap): measured per shape, same box, three passes (profiles/r3_xcd_map.txt) -- config 3 (CIC R8 on
    // int32, 8 KB of input per step) +2.5 % every time, poly_dec -0.6 % twice and +6.6 % once, the fused DDC -3 %: on for the
    // int32 decimator shape only.  ACDSP_XCD_MAP=0 / 1 forces it off / on for every shape (A/B knob).
    a.xcd_map = (xcd_map_wanted(out_mode == 1 && in_eb == 4) && ((int64_t)grid.x * grid.y) % 8 == 0) ? 1 : 0;
    hipError_t e;
    if (sel.row) {
      e = sel.row->launch(sel.spw, sel.pf, sel.nt, sel.fb, grid, s, p, fr, a);
      if (ring_id) { *ring_id = sel.row->id; }
    }
    else if (in_eb == 4) { e = launch_fast<int32_t, 4, 2, 3, 9, 8>(grid, lds_bytes, s, p, fr, a); }
    else if (in_eb == 8) { e = launch_fast<int64_t, 5, 2, 3, 1, 4>(grid, lds_bytes, s, p, fr, a); }
    else if (oeb == 8) { e = launch_fast<int16_t, 2, 3, 6, 9, 8>(grid, lds_bytes, s, p, fr, a); }
    else { e = launch_fast<int16_t, 2, 2, 4, 5, 2>(grid, lds_bytes, s, p, fr, a); }
    if (e != hipSuccess) { return e; }
  }
  if (lz) {
    if (covered) { *covered = fast_chunks * spw * 256; }
    return hipSuccess;
  }
  if (fast_chunks >= n_chunks) { return hipSuccess; }
  a.xcd_map = 0;
  a.chunk0 = (int32_t)fast_chunks;                                    // ragged tail (and every unlisted shape): general kernel
  dim3 grid((unsigned)(n_chunks - fast_chunks), (unsigned)p.n_ch);
  switch (p.in_eb) {
    case 1: return launch_px<int8_t>(a.px, grid, lds_bytes, s, p, fr, a);
    case 2: return launch_px<int16_t>(a.px, grid, lds_bytes, s, p, fr, a);
    case 4: return launch_px<int32_t>(a.px, grid, lds_bytes, s, p, fr, a);
    default: return launch_px<int64_t>(a.px, grid, lds_bytes, s, p, fr, a);
  }
}

}  // namespace acdsp
