// fir_gen_cascade_dec.hip -- the fused decimator -> ac_poly_dec cascade (acdsp_ddc_create_polydec): cascade_kernel (fir_gen_kernels.hpp) with a
// DECIMATING stage B.  Kernel, host side and instantiations of the one family it has: int16 rows on two sample planes, an INT_TYPE of
// 33 .. 40 bits on five planes, a prototype of NTAPS*DF <= 128 taps in at most two digit planes, DF = 2, int32 output containers.
//
// Stage B is the FIR  y[m] = sum_k h[k] w[first_b + m DF - k]  on the decimator's words w, h[tp DF + df] = c[tp + NTAPS df] (the mapping
// acdsp_polydec_set_coeffs plans with), first_b = DF - 1 - q where q < DF words of the stream wait in front of the call.
//
// A step is 256 final outputs and consumes DF stage-A sub-steps of 256 words (16 ring slots) each:
//
//     sub-step   s0 DF - 1 | s0 DF   s0 DF + 1 | (s0+1) DF  (s0+1) DF + 1 | ...
//     stage A    warm-up   |   A        A      |     A           A        |
//     stage B              |            B(s0)  |                 B(s0+1)  |
//
// The ring holds two steps, 32 DF slots: sub-step ss writes slots (16 ss + column) mod 32 DF, and column n / K-group kg / block b of step st
// reads slot 16 DF st + wb + DF n + 4 b + kg, wb = (first_b - off) / 16 >= -8 the slot of the plan's window start -- the way stage A reads
// R n + 4 b + kg.  A 128-tap prototype reaches 127 words + the window's alignment back: inside the ONE warm-up sub-step, so the history per
// channel, the edge / interior / guard split of the launches and the limb epilogues are cascade_kernel's.
#include <cstdlib>
#include <cstring>

#include "fir_gen_kernels.hpp"

namespace acdsp {

//   GUARD / LIMB / PART: as for cascade_kernel.  PART 1 (interior chunks) is the only form with uniform-base window loads.
//   wb: slot of stage B's window start relative to the step's first word (see above).
template <int DF, bool GUARD, bool LIMB, int PART>
__global__ void __launch_bounds__(64, 2) cascade_dec_kernel(FirParams pa, FirParams pb, const v4i *__restrict__ fragA,
                                                           const v4i *__restrict__ fragB, GenArgs a, GenArgs b, int wb) {
  constexpr int PXA = 2, PCA = 3, NBA = 6, NPCA = 9, PXB = 5, PCB = 2, NBB = 3;
  constexpr int RING = 32 * DF;          // slots: two steps of 16 DF
  constexpr bool FAST = PART == 1;
  static_assert((RING & (RING - 1)) == 0, "the ring is addressed with a mask");
  typedef int16_t TIN;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [A planes][B ring: PXB x RING slots][1 KB output tile]
  const int lane = threadIdx.x;
  const int n_col = lane & 15, kg = lane >> 4;
  // (no xcd_remap: launch_cascade leaves the XCD-affine chunk order off for this class -- it measured -3 % on config 5 -- and this kernel
  // streams the same rows, so the order of the grid is kept and a.xcd_map stays 0)
  int bx = blockIdx.x;
  const int ch = blockIdx.y;
  if constexpr (PART == 2) { bx = blockIdx.x == 0 ? 0 : a.edge_chunk; }
  const int R = a.pl.R;
  const int plane_bytes = a.obuf_off / PXA;
  unsigned char *ring = lds + a.obuf_off;
  unsigned char *ob = ring + PXB * RING * 16;

  v4i AA[NBA][PCA], AB[NBB][PCB];
#pragma unroll
  for (int bb = 0; bb < NBA; bb++) {
#pragma unroll
    for (int q = 0; q < PCA; q++) { AA[bb][q] = (bb < a.pl.nb && q < a.pl.pc) ? fragA[((size_t)q * a.pl.nb + bb) * 64 + lane] : (v4i){0, 0, 0, 0}; }
  }
#pragma unroll
  for (int bb = 0; bb < NBB; bb++) {
#pragma unroll
    for (int q = 0; q < PCB; q++) { AB[bb][q] = (bb < b.pl.nb && q < b.pl.pc) ? fragB[((size_t)q * b.pl.nb + bb) * 64 + lane] : (v4i){0, 0, 0, 0}; }
  }
  const TIN *xrow = (const TIN *)pa.x + (int64_t)ch * pa.in_stride;
  const TIN *hrow = (const TIN *)pa.hist + (int64_t)ch * pa.hl + pa.hl;
  const int64_t s0 = ((int64_t)bx + a.chunk0) * a.steps_per_wave;
  const int64_t s1 = GUARD ? ((s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps) : s0 + a.steps_per_wave;
  const int64_t ss0 = s0 * DF - 1, ss1 = s1 * DF;   // sub-steps [ss0, ss1): the warm-up, then DF per step

  // window loads of a sub-step, coalesced over 16-byte pieces (8 samples; a slot is two pieces), as in cascade_kernel
  v4i pre[NPCA];
  int pc_off[NPCA], pc_ps[NPCA];
#pragma unroll
  for (int k = 0; k < NPCA; k++) {
    int slot = (lane + 64 * k) / 2;
    const int sub = lane & 1;
    if (slot >= a.n_slots) { slot = a.n_slots - 1; }
    pc_off[k] = 16 * slot + 8 * sub;
    pc_ps[k] = phys_slot(slot, a) * 16 + 8 * sub;
  }
  const int64_t W_first = a.first + ss0 * 256 * R - a.pl.off, W_last = a.first + (ss1 - 1) * 256 * R - a.pl.off;
  const bool interior = !GUARD && W_first >= 0 && W_last + 16 * a.n_slots <= a.n16;
  if constexpr (PART == 1) { if (!interior) { return; } }
  if constexpr (PART == 2) { if (interior) { return; } }
  const unsigned lane16 = 16u * (unsigned)lane;
  auto fetch = [&](int64_t ss) {
    const int64_t W0 = a.first + ss * 256 * R - a.pl.off;
    if constexpr (FAST) {
      const char *base = (const char *)(xrow + W0);
#pragma unroll
      for (int k = 0; k < NPCA; k++) {
        const unsigned off = k < NPCA - 2 ? lane16 + 1024u * k : (unsigned)sizeof(TIN) * (unsigned)pc_off[k];
        pre[k] = *(const v4i *)(base + off);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NPCA; k++) {
        const int64_t t = W0 + pc_off[k];
        const TIN *src = (t < 0) ? hrow + t : xrow + ((t < a.n16) ? t : 0);
        pre[k] = *(const v4i *)src;
      }
    }
  };
  auto stage_piece = [&](const v4i &v, int ps) {
#pragma unroll
    for (int pp = 0; pp < PXA; pp++) { put_piece_plane<2, PXA>(v, pp, lds, plane_bytes, ps); }
  };
  int xs_of[NBA];
#pragma unroll
  for (int bb = 0; bb < NBA; bb++) { xs_of[bb] = phys_slot(R * n_col + 4 * bb + kg, a) * 16; }
  const int rb0 = wb + DF * n_col + kg;   // stage B's fragment row of K block 0, relative to the step's first slot
  char *yrow = (char *)pb.y + (int64_t)ch * pb.out_stride * 4;

  auto flush = [&](int64_t st) { tile_flush<4, ACDSP_GEN_ST_NT>(ob, lane, yrow, st * 1024); };   // 256 int32 outputs of a finished step: one 1 KB store
  // One sub-step: stage A, and behind the last sub-step of a step (ss = st DF + DF - 1) stage B of step st -- a wave-uniform branch, so that
  // the chunk's loop holds ONE copy of stage A (a copy per sub-step of a step kept its invariants apart and spilled at 256 registers).
  // WARM: the chunk's warm-up, stage A only.
  auto body = [&](int64_t ss, auto warm_c) {
    constexpr bool WARM = decltype(warm_c)::value;
#pragma unroll
    for (int k = 0; k < NPCA; k++) {
      if constexpr (LIMB) {
        // LDS offsets re-derived per piece rather than ten resident registers (see cascade_kernel)
        int slot = (lane >> 1) + 32 * k;
        if (k >= NPCA - 2 && slot >= a.n_slots) { slot = a.n_slots - 1; }
        stage_piece(pre[k], phys_slot(slot, a) * 16 + 8 * (lane & 1));
      } else {
        stage_piece(pre[k], pc_ps[k]);
      }
    }
    // the next sub-step's loads first, then the store of the previous step's tile, and both in front of this sub-step's arithmetic
    // (cascade_kernel has the measurements behind this order).  The tile of step st - 1 leaves with the FIRST sub-step of step st, before
    // stage B of step st refills it: the store has the whole step to retire
    fetch(ss + 1 < ss1 ? ss + 1 : ss);
    if constexpr (!WARM && !GUARD) { if ((ss & (DF - 1)) == 0 && ss > s0 * DF) { flush(ss / DF - 1); } }
    asm volatile("" ::: "memory");

    // ---- stage A: 256 words of the decimating FIR, wrapped to the INT_TYPE width ----
    v4i accA[PXA + PCA - 1];
#pragma unroll
    for (int w = 0; w < PXA + PCA - 1; w++) { accA[w] = LIMB ? (v4i){a.dig[w], a.dig[w], a.dig[w], a.dig[w]} : (v4i){0, 0, 0, 0}; }
#pragma unroll
    for (int bb = 0; bb < NBA; bb++) {
      v4i X[PXA];
#pragma unroll
      for (int pp = 0; pp < PXA; pp++) { X[pp] = *(const v4i *)(lds + pp * plane_bytes + xs_of[bb]); }
#pragma unroll
      for (int q = 0; q < PCA; q++) {
#pragma unroll
        for (int pp = 0; pp < PXA; pp++) { accA[pp + q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(AA[bb][q], X[pp], accA[pp + q], 0, 0, 0); }
      }
    }
    // byte planes of the four words of this lane -> ring slot (16 ss + n_col) mod RING, bytes 4 kg .. 4 kg + 3
    const int wslot = (((int)(ss & (2 * DF - 1)) * 16 + n_col) & (RING - 1)) * 16 + 4 * kg;
    if constexpr (LIMB) {
      // byte carry chain in 32-bit registers (cascade_kernel): u_w = acc_w + (u_{w-1} >> 8), byte w = u_w & 255
      int u[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        u[0][r] = accA[0][r];
#pragma unroll
        for (int w = 1; w < 4; w++) { u[w][r] = accA[w][r] + (u[w - 1][r] >> 8); }
      }
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const unsigned d = gather4((unsigned)u[pp][0], (unsigned)u[pp][1], (unsigned)u[pp][2], (unsigned)u[pp][3], 0) ^ 0x80808080u;
        *(unsigned *)(ring + pp * (RING * 16) + wslot) = d;
      }
      // top plane: bits 32 .. w_int - 1 of the word, sign-extended (the wrap to INT_TYPE)
      unsigned tb[4];
#pragma unroll
      for (int r = 0; r < 4; r++) { tb[r] = (unsigned)__builtin_amdgcn_sbfe(u[3][r], 8, a.w_int - 32); }
      *(unsigned *)(ring + 4 * (RING * 16) + wslot) = gather4(tb[0], tb[1], tb[2], tb[3], 0);
    } else {
      unsigned lo[4], hi[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint64_t y = planes_to_u64(accA, r, a.corr);
        const int64_t v = (int64_t)(y << a.e_ka) >> a.e_ka;        // INT_TYPE word (signed, w_int bits)
        lo[r] = (unsigned)v; hi[r] = (unsigned)((uint64_t)v >> 32);
      }
#pragma unroll
      for (int pp = 0; pp < PXB; pp++) {
        unsigned d = pp < 4 ? gather4(lo[0], lo[1], lo[2], lo[3], pp) : gather4(hi[0], hi[1], hi[2], hi[3], pp - 4);
        if (pp < PXB - 1) { d ^= 0x80808080u; }
        *(unsigned *)(ring + pp * (RING * 16) + wslot) = d;
      }
    }
    if constexpr (WARM) { return; }
    if ((ss & (DF - 1)) != DF - 1) { return; }

    // ---- stage B: 256 outputs of the decimating FIR on the ring ----
    const int64_t st = (ss + 1) / DF - 1;
    v4i accB[PXB + PCB - 1];
#pragma unroll
    for (int w = 0; w < PXB + PCB - 1; w++) { accB[w] = LIMB ? (v4i){b.dig[w], b.dig[w], b.dig[w], b.dig[w]} : (v4i){0, 0, 0, 0}; }
    const int rbase = (int)(st & 1) * 16 * DF + rb0;
#pragma unroll
    for (int bb = 0; bb < NBB; bb++) {
      v4i X[PXB];
#pragma unroll
      for (int pp = 0; pp < PXB; pp++) { X[pp] = *(const v4i *)(ring + pp * (RING * 16) + (((rbase + 4 * bb) & (RING - 1)) * 16)); }
#pragma unroll
      for (int q = 0; q < PCB; q++) {
#pragma unroll
        for (int pp = 0; pp < PXB; pp++) { accB[pp + q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(AB[bb][q], X[pp], accB[pp + q], 0, 0, 0); }
      }
    }
    int o[4];
    if constexpr (LIMB) {
      // z = sum_w acc_w 2^(8w) as two 32-bit limbs through 16-bit carries; OUT = clamp(z >> rs) (cascade_kernel)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int p01 = accB[0][r] + (int)((unsigned)accB[1][r] << 8);
        const int p23 = accB[2][r] + (int)((unsigned)accB[3][r] << 8);
        const int p45 = accB[4][r] + (int)((unsigned)accB[5][r] << 8);
        const int v1 = p23 + (p01 >> 16);
        int H = p45 + (v1 >> 16);                                                      // z >> 32
        const unsigned L = __builtin_amdgcn_perm((unsigned)v1, (unsigned)p01, 0x05040100u);   // z mod 2^32
        H = H < b.l_hb_lo ? b.l_hb_lo : (H > b.l_hb_hi ? b.l_hb_hi : H);
        int q = (int)__builtin_amdgcn_alignbit((unsigned)H, L, (unsigned)b.e_rs);
        q = q < b.l_lo ? b.l_lo : (q > b.l_hi ? b.l_hi : q);
        o[r] = __builtin_amdgcn_sbfe(q, 0, b.l_w);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        uint64_t y = (uint64_t)b.corr;
#pragma unroll
        for (int w = 0; w < PXB + PCB - 1; w++) { y += (uint64_t)(int64_t)accB[w][r] << (8 * w); }
        int64_t v = (int64_t)(y << b.e_ls);
        v = (int64_t)((uint64_t)v << b.e_ka) >> b.e_ka;
        v = (int64_t)((uint64_t)((v + b.e_rnd) >> b.e_rs) << b.e_ls2);
        v = v < b.e_lo ? b.e_lo : (v > b.e_hi ? b.e_hi : v);
        o[r] = (int)((int64_t)((uint64_t)v << b.e_ko) >> b.e_ko);
      }
    }
    if (GUARD) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int64_t m = st * 256 + 16 * n_col + 4 * kg + r;
        if (m < a.n_out) { *(int *)(yrow + 4 * m) = o[r]; }
      }
    } else {
      tile_put<4>(ob, n_col, kg, o[0], o[1], o[2], o[3]);
    }
  };
  typedef std::integral_constant<bool, true> T;
  typedef std::integral_constant<bool, false> F;
  if constexpr (FAST) {
    // the warm-up feeds stage B's first step with its columns 8 .. 15 only (wb >= -8): the 1 KB pieces entirely below slot 8 R are not loaded
    const int64_t W0 = a.first + ss0 * 256 * R - a.pl.off;
    const char *base = (const char *)(xrow + W0);
    const int kskip = (8 * R * 16 * (int)sizeof(TIN)) / 1024;
#pragma unroll
    for (int k = 0; k < NPCA; k++) {
      const unsigned off = k < NPCA - 2 ? lane16 + 1024u * k : (unsigned)sizeof(TIN) * (unsigned)pc_off[k];
      if (k < NPCA - 2 && k < kskip) { pre[k] = (v4i){0, 0, 0, 0}; }
      else { pre[k] = *(const v4i *)(base + off); }
    }
  } else {
    fetch(ss0);
  }
  body(ss0, T());
  for (int64_t ss = ss0 + 1; ss < ss1; ss++) { body(ss, F()); }
  if (!GUARD) { flush(s1 - 1); }
}

// Does the kernel take the stage-B plan `plb` -- fir_gen_plan(h, NTAPS DF, DF, first_b) -- of a call whose output 0 leaves with local word first_b?
bool cascade_dec_plan_ok(const FirGenPlan &plb, int df, int first_b) {
  if (df != 2 || first_b < 0 || first_b >= df) { return false; }
  const int w0 = first_b - plb.off;   // the window's start, in words from the step's first one: a whole number of slots, at most 8 back
  return plb.R == df && plb.pc <= 2 && plb.nb <= 3 && w0 % 16 == 0 && w0 >= -128 && w0 <= 0;
}

// The arguments of both stages: cascade_args for stage A and the formats (int16 rows only), the plan, correction and window slot of stage B.
static bool cascade_dec_args(const FirParams &pa, const FirGenPlan &pla, int w_int, const FirParams &pb, const FirGenPlan *plb, int df, int first_b,
                             GenArgs &a, GenArgs &b) {
  if (pa.in_eb != 2 || !cascade_args(pa, pla, w_int, pb, nullptr, a, b)) { return false; }
  if (plb) {
    if (!cascade_dec_plan_ok(*plb, df, first_b)) { return false; }
    b.pl = *plb;
    b.corr = gen_rebias_corr(b.px, plb->sum_h);
  }
  return true;
}

bool cascade_dec_shape_ok(const FirParams &pa, const FirGenPlan &pla, int w_int, const FirParams &pb, const FirGenPlan *plb, int df, int first_b) {
  GenArgs a, b;
  return df == 2 && cascade_dec_args(pa, pla, w_int, pb, plb, df, first_b, a, b);
}

// pa / pla / d_fragA / w_int / first: stage A as for launch_cascade.  pb: stage B's formats and the output rows; plb / d_fragB: its plan at
// window phase first_b.  n_out final outputs per channel: the caller has counted them from the words of this call and the q waiting ones.
hipError_t launch_cascade_dec(const FirParams &pa, const FirGenPlan &pla, const uint32_t *d_fragA, int w_int, int64_t first, const FirParams &pb,
                              const FirGenPlan &plb, const uint32_t *d_fragB, int df, int first_b, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) { return hipSuccess; }
  constexpr int DF = 2;
  GenArgs a, b;
  const bool out_ok = ((uintptr_t)pb.y % 16 == 0) && ((pb.out_stride * 4) % 16 == 0);
  if (df != DF || !cascade_dec_args(pa, pla, w_int, pb, &plb, df, first_b, a, b) || !out_ok) { return hipErrorNotSupported; }
  const int wb = (first_b - plb.off) / 16;
  a.first = first; a.n_out = n_out; b.first = first_b; b.n_out = n_out;
  a.n_steps = (n_out + 255) / 256;
  const int64_t spw = 8 / DF;   // a chunk is 8 sub-steps behind its warm-up, the ratio launch_cascade measured for its 8 steps
  a.steps_per_wave = spw;
  a.n16 = (pa.n + 15) / 16 * 16;
  a.out_vec_ok = 1; a.chunk0 = 0; a.xcd_map = 0; a.edge_chunk = 0;
  b.n_steps = a.n_steps; b.steps_per_wave = spw; b.out_vec_ok = 1;
  const int slots_alloc = 15 * pla.R + 4 * 6;
  const int phys = gen_slot_map(a, pla.R, slots_alloc);
  a.obuf_off = a.px * (phys + 1) * 16;
  const size_t lds_bytes = (size_t)a.obuf_off + (size_t)b.px * 32 * DF * 16 + 1024;
  const int64_t n_chunks = (a.n_steps + spw - 1) / spw, fast_chunks = n_out / (spw * 256);
  const v4i *fa = (const v4i *)d_fragA, *fb = (const v4i *)d_fragB;

  // 32-bit limb epilogues: the conditions of launch_cascade's int16 family on this stage B's sums
  static const bool no_limb = getenv("ACDSP_NO_LIMB") != nullptr;   // A/B knob
  auto digits = [](__int128 c, int nw, int32_t *dig) {   // balanced base-256 digits, the last one takes the rest
    for (int w = 0; w < nw - 1; w++) { dig[w] = pop_balanced_digit(c); }
    dig[nw - 1] = (int32_t)c;
    return c > -(int64_t(1) << 20) && c < (int64_t(1) << 20);
  };
  bool limb = !no_limb && w_int >= 33 && w_int <= 40 && pla.sum_abs_h < (int64_t(1) << 38) && plb.sum_abs_h < (int64_t(1) << 20);
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
  hipError_t e;
#define ACDSP_CASCADE_DEC_LAUNCH(GUARD_, LIMB_, PART_, GRID_)                                                                        \
  e = hipFuncSetAttribute((const void *)cascade_dec_kernel<DF, GUARD_, LIMB_, PART_>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                          (int)lds_bytes);                                                                                           \
  if (e != hipSuccess) { return e; }                                                                                                 \
  hipLaunchKernelGGL((cascade_dec_kernel<DF, GUARD_, LIMB_, PART_>), GRID_, dim3(64), lds_bytes, s, pa, pb, fa, fb, a, b, wb);       \
  if ((e = hipGetLastError()) != hipSuccess) { return e; }
  if (fast_chunks > 0) {
    const dim3 grid((unsigned)fast_chunks, (unsigned)pa.n_ch);
    if (limb) { ACDSP_CASCADE_DEC_LAUNCH(false, true, 1, grid) } else { ACDSP_CASCADE_DEC_LAUNCH(false, false, 1, grid) }
    // the complete chunks whose windows leave the call's samples: chunk 0 (history) and possibly the last one (its last window ends fewer
    // than 16 R samples behind the input of the last word it needs: every earlier chunk ends a whole chunk before that)
    a.edge_chunk = (int32_t)(fast_chunks - 1);
    const dim3 egrid(fast_chunks > 1 ? 2u : 1u, (unsigned)pa.n_ch);
    if (limb) { ACDSP_CASCADE_DEC_LAUNCH(false, true, 2, egrid) } else { ACDSP_CASCADE_DEC_LAUNCH(false, false, 2, egrid) }
  }
  if (fast_chunks < n_chunks) {
    a.chunk0 = (int32_t)fast_chunks;
    const dim3 grid((unsigned)(n_chunks - fast_chunks), (unsigned)pa.n_ch);
    if (limb) { ACDSP_CASCADE_DEC_LAUNCH(true, true, 0, grid) } else { ACDSP_CASCADE_DEC_LAUNCH(true, false, 0, grid) }
  }
#undef ACDSP_CASCADE_DEC_LAUNCH
  return hipSuccess;
}

}  // namespace acdsp
