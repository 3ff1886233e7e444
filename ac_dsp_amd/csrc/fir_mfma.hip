// fir_mfma.hip -- many-channel 16-bit FIR on the gfx950 matrix cores (exact integer arithmetic).
//
// Replaces the tap-MAC loops of the reference cores (`acc += reg[i] * coeffs[i]`,
// reference include/ac_dsp/ac_fir_const_coeffs.h:190-199 and the load_/prog_ twins) for the
// arithmetic class in which that loop is an exact integer dot product: accumulator with at least
// F_in + F_coeff fractional bits and AC_WRAP overflow (DESIGN.md "arithmetic classes").  The
// folded architectures (:244-275) enter through their effective direct-form coefficients.
//
// Why MFMA at all: a 255-tap int16 FIR carries 255 MAC per 4 algorithmic bytes; the VALU
// (v_dot2_i32_i16) tops out near 15 % of the HBM roofline, the int8 matrix pipe does not.
//
// The formulation, the data movement and the kernels themselves are in fir_mfma_kernels.hpp.  This unit holds the host plan, the class
// decisions and the dispatch, and compiles the kernels of 1 .. 9 and 33 K-blocks and the LDS-resident ones; the other shapes are compiled
// by fir_mfma_mid.hip / _mid2 / _mid3 and fir_mfma_alt.hip / _alt2 (launch_fir_mfma_*), for compile time.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fir_mfma_kernels.hpp"

namespace acdsp {

int fir_mfma_max_blocks() { return kMaxNB; }
int fir_mfma_max_reg_blocks() { return kMaxRegNB; }

// Host: build frag[plane][b][lane][4 dwords]; plane 0 = high bytes, 1 = low bytes.
// Lane l holds row i = l & 31 and the 16 K-positions k = 16*(l>>5) + j, j = 0..15 (the same
// (lane-group, byte) -> k map is used for the data operand, so any K permutation inside the
// instruction cancels).
// K-blocks of the plan for n_taps: the Toeplitz band of 32 outputs spans n_taps + 31 inputs; 10 .. 32 blocks are padded to the next odd
// count (the register-resident shapes of fir_mfma_mid.hip exist for odd counts; the extra leading block holds zeros).
// ... and the count with the padding applied whatever the ACDSP_NO_MID knob says: the handle's state geometry (history length) must not
// depend on an A/B environment variable
int fir_mfma_plan_blocks_padded(int n_taps) {
  const int nb = (n_taps - 1 + 31) / 32 + 1;
  return (nb >= 10 && nb <= 32 && (nb & 1) == 0) ? nb + 1 : nb;
}
int fir_mfma_plan_blocks(int n_taps) {
  int nb = (n_taps - 1 + 31) / 32 + 1;
  static const bool no_mid = getenv("ACDSP_NO_MID") != nullptr;
  if (!no_mid && nb >= 10 && nb <= 32 && (nb & 1) == 0) { nb++; }
  return nb;
}

bool fir_mfma_build_fragments(const int64_t *c, int n_taps, FirMfmaPlan *plan, uint32_t *frag) {
  const int nb = fir_mfma_plan_blocks(n_taps);
  if (nb > kMaxNB) { return false; }
  return fir_mfma_build_fragments_nb(c, n_taps, nb, plan, frag);
}

bool fir_mfma_build_fragments_nb(const int64_t *c, int n_taps, int nb, FirMfmaPlan *plan, uint32_t *frag) {
  std::vector<int8_t> chi(n_taps), clo(n_taps);
  int64_t sum = 0, sa = 0, sah = 0, sal = 0;
  for (int k = 0; k < n_taps; k++) {
    int64_t v = c[k];
    if (v < -32768 || v > 32767) { return false; }
    int64_t lo = ((v + 128) & 0xff) - 128;
    int64_t hi = (v - lo) / 256;
    if (hi < -128 || hi > 127) { return false; }  // c >= 32640: not representable as two signed bytes
    chi[k] = (int8_t)hi; clo[k] = (int8_t)lo;
    sum += v;
    sa += v < 0 ? -v : v; sah += hi < 0 ? -hi : hi; sal += lo < 0 ? -lo : lo;
  }
  plan->nb = nb;
  plan->sum_abs = sa; plan->sum_abs_hi = sah; plan->sum_abs_lo = sal;
  plan->corr = 128 * sum;
  plan->hi_mask = plan->lo_mask = 0;
  for (int pl = 0; pl < 2; pl++) {
    const int8_t *src = pl == 0 ? chi.data() : clo.data();
    for (int b = 0; b < nb; b++) {
      bool any = false;
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 31, h = lane >> 5;
        for (int dw = 0; dw < 4; dw++) {
          uint32_t word = 0;
          for (int bj = 0; bj < 4; bj++) {
            const int k = 16 * h + 4 * dw + bj;
            const int tap = i - k + 32 * (nb - 1 - b);
            int8_t val = (tap >= 0 && tap < n_taps) ? src[tap] : (int8_t)0;
            any = any || val != 0;
            word |= (uint32_t)(uint8_t)val << (8 * bj);
          }
          frag[(((size_t)pl * nb + b) * 64 + lane) * 4 + dw] = word;
        }
      }
      if (any && b < 64) { (pl == 0 ? plan->hi_mask : plan->lo_mask) |= uint64_t(1) << b; }
    }
  }
  return true;
}

// =============================================================================================
// Large tap counts (NB = 10 .. 33, e.g. the 1023-tap configuration): the 2*NB Toeplitz fragments no
// longer fit the register file, so they live in LDS (2 KB per K-block, one shared coefficient set per
// launch) and are read next to the data fragments: four ds_read_b128 per four MFMAs, ~50 % of the LDS
// bandwidth.  Same one-channel-per-wave mapping, eight free-running waves per workgroup (they share only the A
// fragments; ping-pong barriers measured 20 % slower on the double-wide variant below), run-time K loop.
// =============================================================================================

// EPI 4 (round 4; the LDS-resident kernels only): int16 OUT containers when the 32-bit epilogue's bounds fail -- dense or
// high-gain sets of 258+ taps, where 2^8 mid + ll leaves int32 or the sum may wrap the accumulator.  V = 2^16 hh + 2^8 mid + ll + C
// in 64 bits, then the reference's two conversions branch-free: acc = wrap_ACC(V << lossless_shift); q = (acc + rnd) >> rs2 with
// rs2 = F_acc - F_out >= 1; AC_SAT clamps, AC_WRAP keeps the low W_out bits (host-derived constants in Epi64).  ~35 VALU per output
// instead of 3, still in the shadow of the 132 MFMAs of such a step; results leave through the same LDS tile and 16-byte stores as
// EPI 1 / 2 (the generic class, EPI 0, converts with uniform branches and stores element by element: 4.6 - 6.1 ms on the dense rows
// of profiles/r3_taps_sweep.txt).
struct Epi64 { int64_t corr, rnd, lo, hi; int ls, ka, rs, ko; };
__device__ __forceinline__ Epi64 make_epi64(const FirParams &p, int64_t corr) {
  Epi64 e;
  e.corr = corr; e.ls = p.lossless_shift; e.ka = 64 - p.acc.W; e.rs = p.acc.F - p.out.F;
  e.rnd = q_preload(p.out.Q, e.rs);   // (EPI 4 guarantees the range; the other classes never read it)
  if (p.out.O == ACDSP_SAT) { e.lo = p.out.lo; e.hi = p.out.hi; e.ko = 0; }
  else { e.lo = INT64_MIN; e.hi = INT64_MAX; e.ko = 64 - p.out.W; }
  return e;
}
__device__ __forceinline__ void epi64(const v16i &hh, const v16i &mid, const v16i &ll, const Epi64 &e, int (&o)[16]) {
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int64_t v = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r] + e.corr;
    int64_t acc = (int64_t)((uint64_t)v << e.ls);
    acc = (int64_t)((uint64_t)acc << e.ka) >> e.ka;                   // wrap to ACC_TYPE (signed)
    int64_t q = (acc + e.rnd) >> e.rs;                                // W_acc <= 62: the rounding add cannot leave int64
    q = q < e.lo ? e.lo : (q > e.hi ? e.hi : q);
    o[r] = (int)((int64_t)((uint64_t)q << e.ko) >> e.ko);
  }
}

template <int EPI, bool FAST>
__device__ __forceinline__ void fir_mfma_big_body(const FirParams &p, const v4i *__restrict__ frag, const MfmaArgs &a,
                                                  unsigned char *lds_all) {
  const int NB = a.nb;
  const int HB = NB - 1, NC = 32 + HB, NP = 4 * NC, ARR = staged_array_bytes(NC);
  constexpr int JN = 4;   // NP <= 256
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y * 8 + wave;
  if (ch >= p.n_ch) { ch = p.n_ch - 1; }
  // LDS: [A fragments: 2 planes x NB x 1 KB][per wave: 2 x 4 arrays x ARR staging + 2 KB output tile]
  v4i *ldsA = (v4i *)lds_all;
  const int wave_bytes = 2 * 4 * ARR + 2048;
  unsigned char *lds = lds_all + 2 * NB * 1024 + wave * wave_bytes;
  unsigned char *obuf = lds + 2 * 4 * ARR;
  for (int i = threadIdx.x; i < 2 * NB * 64; i += 512) { ldsA[i] = frag[i]; }

  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;
  const int64_t s0 = a.step0 + (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);

  v4i R[JN];
  auto issue_loads = [&](int64_t T0) {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
      int64_t t = T0 - 32 * HB + 8 * pc;
      const int16_t *src = (t < 0) ? hrow + t : xrow + ((t < a.n8) ? t : 0);
      R[j] = *(const v4i *)src;
    }
  };
  auto stage = [&](unsigned char *buf) {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = lane + 64 * j;
      if (pc < NP) {
        const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
        unsigned hi0 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x07050301u), a.hi_xor);
        unsigned hi1 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x07050301u), a.hi_xor);
        unsigned lo0 = __builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x06040200u) ^ 0x80808080u;
        unsigned lo1 = __builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x06040200u) ^ 0x80808080u;
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        *(v2u *)(buf + (0 * 2 + hh_) * ARR + c * 16 + sub * 8) = (v2u){hi0, hi1};
        *(v2u *)(buf + (1 * 2 + hh_) * ARR + c * 16 + sub * 8) = (v2u){lo0, lo1};
      }
    }
  };

  const int rs = p.in.F + p.cf.F - p.out.F;
  const int64_t corr = a.corr[0];
  const int64_t corr_t = corr + (EPI != 0 ? q_preload(p.out.Q, rs) : 0);
  const int c_ll = (EPI == 1 || EPI == 2) ? (int)corr_t : 0;   // EPI 4 adds C in 64 bits: 128 sum(c) need not fit int32
  const Epi64 e64 = make_epi64(p, corr);
  const v16i ll_init = {c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll};
  int16_t *yrow = (int16_t *)p.y + (int64_t)ch * p.out_stride + 32 * n_col + 4 * h;

  issue_loads(s0 * 1024);
  __syncthreads();          // A fragments visible to every wave (also drains the first loads: once per chunk)
  stage(lds);
  if (FAST || nsteps > 1) { issue_loads((s0 + 1) * 1024); }

  for (int s = 0; s < nsteps; s++) {
    const int64_t T0 = (s0 + s) * 1024;
    const unsigned char *buf = lds + (s & 1) * (4 * ARR);
    const unsigned char *fh = buf + (0 * 2 + h) * ARR + n_col * 16;
    const unsigned char *fl = buf + (1 * 2 + h) * ARR + n_col * 16;
    const v4i *ah = ldsA + lane, *al = ldsA + NB * 64 + lane;

    // ---------------- phase M ----------------
    v16i hh = {0}, mid = {0}, ll = ll_init;
    v4i Ahc = ah[0], Alc = al[0], Bhc = *(const v4i *)fh, Blc = *(const v4i *)fl;
    for (int b = 0; b < NB; b++) {
      v4i Ahn = Ahc, Aln = Alc, Bhn = Bhc, Bln = Blc;
      if (b + 1 < NB) {   // fragments of the next K-block are in flight while this one multiplies
        Ahn = ah[(b + 1) * 64]; Aln = al[(b + 1) * 64];
        Bhn = *(const v4i *)(fh + 16 * (b + 1)); Bln = *(const v4i *)(fl + 16 * (b + 1));
      }
      if (b >= a.hb0 && b <= a.hb1) {
        hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Bhc, hh, 0, 0, 0);
        mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Blc, mid, 0, 0, 0);
      }
      ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Blc, ll, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Bhc, mid, 0, 0, 0);
      Ahc = Ahn; Alc = Aln; Bhc = Bhn; Blc = Bln;
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---------------- phase O ----------------
    int o16[16];
    if (EPI == 4) { epi64(hh, mid, ll, e64, o16); }
    else if (EPI != 0) { epi32<false>(hh, mid, ll, rs - a.nar_d, a, o16); }
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int64_t t0 = T0 + 32 * n_col + 8 * g + 4 * h;
      if (EPI != 0) {
        const int *o = o16 + 4 * g;
        v4s pk;
        if (EPI == 2) {
          typedef short v2s __attribute__((ext_vector_type(2)));
          const v2s p0 = __builtin_amdgcn_cvt_pk_i16(o[0], o[1]), p1 = __builtin_amdgcn_cvt_pk_i16(o[2], o[3]);
          pk = (v4s){p0.x, p0.y, p1.x, p1.y};
        } else {
          pk = (v4s){(short)o[0], (short)o[1], (short)o[2], (short)o[3]};
        }
        int16_t *dst = yrow + T0 + 8 * g;
        if (FAST) {
          const int P = 4 * n_col + g;
          *(v4s *)(obuf + (((P & ~15) | ((P + (P >> 4)) & 15)) * 16 + 8 * h)) = pk;
        } else if (a.out_vec_ok && t0 + 4 <= p.n) {
          *(v4s *)dst = pk;
        } else {
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            if (t0 + rr < p.n) { dst[rr] = pk[rr]; }   // pk: already clamped for AC_SAT
          }
        }
      } else {
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * g + rr;
          int64_t v = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r] + corr;
          int64_t acc = wrap64((int64_t)((uint64_t)v << p.lossless_shift), p.acc.W, p.acc.S);
          int64_t y = requant64(acc, p.acc.F, p.out);
          if (t0 + rr < p.n) { store_raw(p.y, (int64_t)ch * p.out_stride + t0 + rr, p.out_eb, y); }
        }
      }
    }
    if (FAST && EPI != 0) {
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int P = 64 * half + lane;
        const v4i val = *(const v4i *)(obuf + ((P & ~15) | ((P + (P >> 4)) & 15)) * 16);
        *(v4i *)((int16_t *)p.y + (int64_t)ch * p.out_stride + T0 + 512 * half + 8 * lane) = val;
      }
    }
    if (s + 1 < nsteps) {
      stage(lds + ((s + 1) & 1) * (4 * ARR));
      if (FAST || s + 2 < nsteps) { issue_loads(T0 + 2048); }
    }
  }
}

template <int EPI>
__global__ void __launch_bounds__(512, 2)
fir_mfma_big_kernel(FirParams p, const v4i *__restrict__ frag, MfmaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
  const int64_t s0 = a.step0 + (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const bool interior = EPI != 0 && a.out_vec_ok && s1 * 1024 <= p.n;
  if (interior) { fir_mfma_big_body<EPI, true>(p, frag, a, lds_dyn); }
  else { fir_mfma_big_body<EPI, false>(p, frag, a, lds_dyn); }
}

// ---------------------------------------------------------------------------------------------------
// Double-wide variant for complete chunks: a step is 2048 outputs (two column sets of 32 blocks), so every
// A fragment fetched from LDS feeds eight MFMAs instead of four.  With NB = 33 the single-wide kernel moves
// 4 KB of LDS per four MFMAs per wave -- ~220 of the 256 B/clk the LDS delivers, i.e. it is LDS-bound as much as
// MFMA-bound; here it is 6 KB per eight.  The two sets share their halo (one staged array of 64 + NB - 1 chunks,
// single-buffered: a wave stages step s+1 in its own O phase, after its own M phase is done reading).  The eight
// waves of a workgroup share only the A fragments and run free (the ping-pong barriers of the single-wide kernel
// cost 20 % here: 2.86 -> 2.30 ms on config 4).
// Launched over chunks of complete double steps only (EPI 1 / 2); the ragged rest goes to fir_mfma_big_kernel.
template <int EPI>
__global__ void __launch_bounds__(512, 1)
fir_mfma_big2_kernel(FirParams p, const v4i *__restrict__ frag, MfmaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb;
  const int HB = NB - 1, NC = 64 + HB, NP = 4 * NC, ARR = staged_array_bytes(NC);
  constexpr int JN = 6;   // NP <= 4 * 96
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y * 8 + wave;
  if (ch >= p.n_ch) { ch = p.n_ch - 1; }
  v4i *ldsA = (v4i *)lds_all;
  const int wave_bytes = 4 * ARR + 4096;
  unsigned char *lds = lds_all + 2 * NB * 1024 + wave * wave_bytes;
  unsigned char *obuf = lds + 4 * ARR;
  for (int i = threadIdx.x; i < 2 * NB * 64; i += 512) { ldsA[i] = frag[i]; }

  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;
  const int64_t d0 = (int64_t)blockIdx.x * a.steps_per_wave;   // in double steps; the launch covers complete chunks
  const int nsteps = (int)a.steps_per_wave;
  const int64_t t_last = (d0 + nsteps - 1) * 2048;

  v4i R[JN];
  auto issue_loads = [&](int64_t T0) {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
      int64_t t = T0 - 32 * HB + 8 * pc;
      const int16_t *src = (t < 0) ? hrow + t : xrow + ((t < a.n8) ? t : 0);
      R[j] = *(const v4i *)src;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = lane + 64 * j;
      if (pc < NP) {
        const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
        unsigned hi0 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x07050301u), a.hi_xor);
        unsigned hi1 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x07050301u), a.hi_xor);
        unsigned lo0 = __builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x06040200u) ^ 0x80808080u;
        unsigned lo1 = __builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x06040200u) ^ 0x80808080u;
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        *(v2u *)(lds + (0 * 2 + hh_) * ARR + c * 16 + sub * 8) = (v2u){hi0, hi1};
        *(v2u *)(lds + (1 * 2 + hh_) * ARR + c * 16 + sub * 8) = (v2u){lo0, lo1};
      }
    }
  };

  const int rs = p.in.F + p.cf.F - p.out.F;
  const int c_ll = EPI == 4 ? 0 : (int)(a.corr[0] + q_preload(p.out.Q, rs));
  const Epi64 e64 = make_epi64(p, a.corr[0]);
  const v16i ll_init = {c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll};
  int16_t *yout = (int16_t *)p.y + (int64_t)ch * p.out_stride;
  const unsigned char *fh = lds + (0 * 2 + h) * ARR + n_col * 16;
  const unsigned char *fl = lds + (1 * 2 + h) * ARR + n_col * 16;
  const v4i *ah = ldsA + lane, *al = ldsA + NB * 64 + lane;

  issue_loads(d0 * 2048);
  __syncthreads();          // A fragments visible to every wave
  stage();
  issue_loads(nsteps > 1 ? (d0 + 1) * 2048 : t_last);

  for (int s = 0; s < nsteps; s++) {
    const int64_t T0 = (d0 + s) * 2048;
    // ---------------- phase M: column set 0 = chunks n + b, set 1 = chunks 32 + n + b ----------------
    v16i h0 = {0}, m0 = {0}, l0 = ll_init, h1 = {0}, m1 = {0}, l1 = ll_init;
    // fragments of K-block b live in slot b % 3 and are fetched two blocks ahead (one block = 4..8 MFMAs = 128..256
    // cycles, less than an LDS round trip when all eight waves of the workgroup are reading)
    struct Frag { v4i Ah, Al, Bh0, Bl0, Bh1, Bl1; };
    auto fetch = [&](Frag &f, int bb) {
      f.Ah = ah[bb * 64]; f.Al = al[bb * 64];
      f.Bh0 = *(const v4i *)(fh + 16 * bb); f.Bl0 = *(const v4i *)(fl + 16 * bb);
      f.Bh1 = *(const v4i *)(fh + 512 + 16 * bb); f.Bl1 = *(const v4i *)(fl + 512 + 16 * bb);
    };
    auto mac = [&](const Frag &f, int bb) {
      if (bb >= a.hb0 && bb <= a.hb1) {
        h0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Ah, f.Bh0, h0, 0, 0, 0);
        h1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Ah, f.Bh1, h1, 0, 0, 0);
        m0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Ah, f.Bl0, m0, 0, 0, 0);
        m1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Ah, f.Bl1, m1, 0, 0, 0);
      }
      l0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Al, f.Bl0, l0, 0, 0, 0);
      l1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Al, f.Bl1, l1, 0, 0, 0);
      m0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Al, f.Bh0, m0, 0, 0, 0);
      m1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.Al, f.Bh1, m1, 0, 0, 0);
    };
    Frag F0, F1, F2;
    fetch(F0, 0);
    if (NB > 1) { fetch(F1, 1); } else { F1 = F0; }
    F2 = F0;
    for (int b = 0; b < NB; b += 3) {
      if (b + 2 < NB) { fetch(F2, b + 2); }
      mac(F0, b);
      if (b + 1 < NB) {
        if (b + 3 < NB) { fetch(F0, b + 3); }
        mac(F1, b + 1);
      }
      if (b + 2 < NB) {
        if (b + 4 < NB) { fetch(F1, b + 4); }
        mac(F2, b + 2);
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---------------- phase O ----------------
#pragma unroll
    for (int set = 0; set < 2; set++) {
      int o[16];
      if (EPI == 4) { if (set == 0) { epi64(h0, m0, l0, e64, o); } else { epi64(h1, m1, l1, e64, o); } }
      else if (set == 0) { epi32<false>(h0, m0, l0, rs - a.nar_d, a, o); } else { epi32<false>(h1, m1, l1, rs - a.nar_d, a, o); }
#pragma unroll
      // (the permlane32-swap / ds_write_b128 tile of fir_mfma_pipe_body was tried here: conflicts 2.5e7 -> 0 but +0.8 % time,
      // the phase is not in the shadow of MFMAs)
      for (int g = 0; g < 4; g++) {
        v4s pk;
        if (EPI == 2) {
          typedef short v2s __attribute__((ext_vector_type(2)));
          const v2s p0 = __builtin_amdgcn_cvt_pk_i16(o[4 * g], o[4 * g + 1]), p1 = __builtin_amdgcn_cvt_pk_i16(o[4 * g + 2], o[4 * g + 3]);
          pk = (v4s){p0.x, p0.y, p1.x, p1.y};
        } else {
          pk = (v4s){(short)o[4 * g], (short)o[4 * g + 1], (short)o[4 * g + 2], (short)o[4 * g + 3]};
        }
        const int P = 4 * n_col + g;
        *(v4s *)(obuf + 2048 * set + (((P & ~15) | ((P + (P >> 4)) & 15)) * 16 + 8 * h)) = pk;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {   // 4 KB contiguous: four coalesced 16-byte-per-lane stores
      const int P = 64 * (q & 1) + lane;
      const v4i val = *(const v4i *)(obuf + 2048 * (q >> 1) + ((P & ~15) | ((P + (P >> 4)) & 15)) * 16);
#if ACDSP_FIR_NT & 8   // -0.4 % same box (profiles/r2_ab_nt.txt)
      __builtin_nontemporal_store(val, (v4i *)(yout + T0 + 512 * q + 8 * lane));
#else
      *(v4i *)(yout + T0 + 512 * q + 8 * lane) = val;
#endif
    }
    if (s + 1 < nsteps) {
      stage();
      const int64_t tn = T0 + 4096;
      issue_loads(tn < t_last ? tn : t_last);
    }
  }
}

// Waves per workgroup of the register-resident kernel.  8 = ping-pong (MFMA run of waves 0-3 against the
// epilogue / staging of waves 4-7, s_barrier between): measured 4 % SLOWER than independent single-wave
// workgroups on MI355X (1.215 vs 1.163 ms on config 2), because MFMA and VALU issue serialise per SIMD
// whatever the pairing; kept selectable for the record.
constexpr int kSmallWaves = 1;
// engine.hip's small-call path (FirParams::hist_next) relies on the single-wave kernel writing the next history itself
// (`if constexpr (WAVES == 1)` in fir_mfma_kernel): with the 8-wave form selected it would silently drop the state.
static_assert(kSmallWaves == 1, "the fused history update of small host-side calls exists in the single-wave kernel only");

// Band skip code (HS = lo + 16 hi) for the non-zero high-byte blocks: each side skips 2 or 3 blocks when the set allows it
// (instantiated: both sides >= 2), else nothing is skipped.
static int pick_hs(int nb, uint64_t hi_mask) {
  if (hi_mask == 0) { return nb >= 7 ? 3 + 16 * 3 : (nb >= 5 ? 2 + 16 * 2 : 0); }
  int lo = 0, hi = 0;
  while (lo < nb && !((hi_mask >> lo) & 1)) { lo++; }
  while (hi < nb && !((hi_mask >> (nb - 1 - hi)) & 1)) { hi++; }
  lo = lo > 3 ? 3 : lo; hi = hi > 3 ? 3 : hi;
  if (nb < 7) { lo = lo > 2 ? 2 : lo; hi = hi > 2 ? 2 : hi; }
  if (nb < 5 || lo < 2 || hi < 2) { return 0; }
  return lo + 16 * hi;
}

// the NAR instantiations (narrow OUT_TYPEs, general rounding modes) exist for the widest and the narrowest skip only: 3 + 3 where the set
// allows it, else 2 + 2 (fir_mfma_alt2.hip)
static int pick_hs_nar(int nb, uint64_t hi_mask) {
  const int hs = pick_hs(nb, hi_mask);
  return hs == 3 + 16 * 3 ? hs : (hs ? 2 + 16 * 2 : 0);
}

template <int NB>
static hipError_t launch_nb(const FirParams &p, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  static const bool no_nar_hs = getenv("ACDSP_NO_NAR_SKIP") != nullptr;   // A/B knob: the round-4 NAR kernels (every high-plane product issued)
  const int hs = !epi ? 0 : (a.nar_on ? (no_nar_hs ? 0 : pick_hs_nar(NB, a.hi_mask)) : pick_hs(NB, a.hi_mask));
  if (NB >= 7) {
    constexpr int H33 = NB >= 7 ? 3 + 16 * 3 : 0, H32 = NB >= 7 ? 3 + 16 * 2 : 0, H23 = NB >= 7 ? 2 + 16 * 3 : 0;
    if (hs == 3 + 16 * 3) { return launch_nb_hs<NB, H33, kSmallWaves>(p, d_frag, a, epi, grid, s); }
    if (hs == 3 + 16 * 2) { return launch_nb_hs<NB, H32, kSmallWaves>(p, d_frag, a, epi, grid, s); }
    if (hs == 2 + 16 * 3) { return launch_nb_hs<NB, H23, kSmallWaves>(p, d_frag, a, epi, grid, s); }
  }
  if (NB >= 5 && hs == 2 + 16 * 2) { return launch_nb_hs<NB, (NB >= 5 ? 2 + 16 * 2 : 0), kSmallWaves>(p, d_frag, a, epi, grid, s); }
  return launch_nb_hs<NB, 0, kSmallWaves>(p, d_frag, a, epi, grid, s);
}


// NB = 33 (993 .. 1025 taps): the register-resident kernel at one wave per SIMD, for coefficient sets whose high-byte band leaves
// 12 or 14 K-blocks free on either side (any unit-gain low-pass in <16,2>: |c| >= 128 only within ~40 taps of the centre, a
// 5-block band -- BASELINE config 4 issues 76 instead of 132 MFMAs per step).  Fragments that would all be live (dense sets: 264
// registers + two accumulator sets) spill; those sets stay on the LDS-resident kernels below.
// Same-box A/B on config 4 (profiles/r3_fir1023_reg33.txt): 2.32 -> 2.10 ms, 0.45 -> 0.50 of the int8 peak in MFMAs issued.
static int reg33_band_code(uint64_t hi_mask, int epi) {
  if (epi != 1 && epi != 2) { return 0; }
  int lo = 0, hi = 0;
  if (hi_mask == 0) { lo = hi = 16; }
  else {
    while (lo < 33 && !((hi_mask >> lo) & 1)) { lo++; }
    while (hi < 33 && !((hi_mask >> (32 - hi)) & 1)) { hi++; }
  }
  if (lo >= 14 && hi >= 14) { return 14 + 16 * 14; }
  if (lo >= 12 && hi >= 12) { return 12 + 16 * 12; }
  return 0;
}
static hipError_t launch_nb33(const FirParams &p, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  if (reg33_band_code(a.hi_mask, epi) == 14 + 16 * 14) { return launch_nb_hs<33, 14 + 16 * 14, 1>(p, d_frag, a, epi, grid, s); }
  return launch_nb_hs<33, 12 + 16 * 12, 1>(p, d_frag, a, epi, grid, s);
}

static hipError_t launch_big(const FirParams &p, const uint32_t *d_frag, MfmaArgs a, int epi, dim3 grid, hipStream_t s) {
  const int nb = a.nb;
  // contiguous range of non-zero high-byte blocks
  a.hb0 = 0; a.hb1 = nb - 1;
  if (epi) {
    if (a.hi_mask == 0) { a.hb0 = 1; a.hb1 = 0; }
    else {
      while (!((a.hi_mask >> a.hb0) & 1)) { a.hb0++; }
      while (!((a.hi_mask >> a.hb1) & 1)) { a.hb1--; }
    }
  }
  hipError_t e = hipSuccess;
  a.step0 = 0;
  // complete chunks of double steps on the double-wide kernel ...
  const int64_t spw2 = a.steps_per_wave >= 8 ? a.steps_per_wave / 2 : 4;
  const int64_t fast_chunks = (epi == 1 || epi == 2 || epi == 4) && a.out_vec_ok ? (p.n / 2048) / spw2 : 0;
  if (fast_chunks > 0) {
    MfmaArgs a2 = a;
    a2.steps_per_wave = spw2;
    const size_t lds2 = (size_t)2 * nb * 1024 + 8 * ((size_t)4 * staged_array_bytes(64 + nb - 1) + 4096);
    dim3 g2((unsigned)fast_chunks, grid.y);
    if (epi == 1) {
      e = hipFuncSetAttribute((const void *)fir_mfma_big2_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big2_kernel<1>), g2, dim3(512), lds2, s, p, (const v4i *)d_frag, a2); }
    } else if (epi == 4) {
      e = hipFuncSetAttribute((const void *)fir_mfma_big2_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big2_kernel<4>), g2, dim3(512), lds2, s, p, (const v4i *)d_frag, a2); }
    } else {
      e = hipFuncSetAttribute((const void *)fir_mfma_big2_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big2_kernel<2>), g2, dim3(512), lds2, s, p, (const v4i *)d_frag, a2); }
    }
    if (e != hipSuccess) { return e; }
    a.step0 = fast_chunks * spw2 * 2;
    if (a.step0 >= a.n_steps) { return hipGetLastError(); }
    grid.x = (unsigned)((a.n_steps - a.step0 + a.steps_per_wave - 1) / a.steps_per_wave);
  }
  // ... the ragged rest (and the generic epilogue class) on the single-wide kernel
  const size_t lds_bytes = (size_t)2 * nb * 1024 + 8 * ((size_t)2 * 4 * staged_array_bytes(32 + nb - 1) + 2048);
  if (epi == 1) {
    e = hipFuncSetAttribute((const void *)fir_mfma_big_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big_kernel<1>), grid, dim3(512), lds_bytes, s, p, (const v4i *)d_frag, a); }
  } else if (epi == 2) {
    e = hipFuncSetAttribute((const void *)fir_mfma_big_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big_kernel<2>), grid, dim3(512), lds_bytes, s, p, (const v4i *)d_frag, a); }
  } else if (epi == 4) {
    e = hipFuncSetAttribute((const void *)fir_mfma_big_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big_kernel<4>), grid, dim3(512), lds_bytes, s, p, (const v4i *)d_frag, a); }
  } else {
    e = hipFuncSetAttribute((const void *)fir_mfma_big_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) { hipLaunchKernelGGL((fir_mfma_big_kernel<0>), grid, dim3(512), lds_bytes, s, p, (const v4i *)d_frag, a); }
  }
  return e != hipSuccess ? e : hipGetLastError();
}

// Can the all-32-bit epilogue be used for this plan / type combination?  0: no, 1: WRAP, 2: SAT
// a rounding / overflow mode beyond the AC_TRN / AC_RND x AC_WRAP / AC_SAT of the plain fast classes
static bool fir_mfma_general_q(const FirParams &p) {
  return !(q_const_mode(p.out.Q) && (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT));
}
int fir_mfma_epilogue_class(const FirParams &p, const FirMfmaPlan &plan) {
  // an unsigned AC_WRAP accumulator turns every negative sum into 2^W - |v| before OUT_TYPE sees it (the reference's
  // `acc += ...` assignment): only the generic epilogue wraps to ACC_TYPE, the fast ones convert the signed sum
  if (!p.acc.S) { return 0; }
  const int rs = p.in.F + p.cf.F - p.out.F;
  // |y| <= 32768 * sum|c| must fit the accumulator (no AC_WRAP event possible) ...
  const int acc_bits = p.acc.W - (p.acc.S ? 1 : 0) - p.lossless_shift;
  const int64_t x_max = int64_t(1) << (p.in.W > 1 && p.in.W <= 16 ? p.in.W - (p.in.S ? 1 : 0) : 15);   // |x| <= 2^(W_in - 1) (unsigned: < 2^W_in): narrow samples need a narrower accumulator
  const bool acc_wide = acc_bits >= 63 || plan.sum_abs * x_max < (int64_t(1) << (acc_bits > 0 ? acc_bits : 0));
  // ... hh*256 + mid + carry must fit int32, and so must the low plane with corr + rounding constant preloaded
  const int64_t hh_max = 128 * plan.sum_abs_hi, mid_max = 128 * (plan.sum_abs_hi + plan.sum_abs_lo), ll_max = 128 * plan.sum_abs_lo;
  // (the sign- / parity-dependent modes add up to K + |C| <= 2^rs to lo before the shift: epi32_gq)
  const int64_t rnd = q_const_mode(p.out.Q) ? (rs <= 38 ? q_preload(p.out.Q, rs) : 0) : (rs >= 1 && rs <= 31 ? (int64_t(1) << rs) : 0);
  const int64_t corr_abs = (plan.corr < 0 ? -plan.corr : plan.corr) + rnd;
  // lo = 2^8 mid + ll (with the preloaded constant) and the shifted sum must stay inside int32
  // (OUT_TYPEs of W < 16 bits shift by rse = rs - (16 - W) and finish on the packed words: MfmaArgs::nar_*)
  const int nar_d = (p.out_eb == 2 && p.out.W >= 2 && p.out.W < 16) ? 16 - p.out.W : 0, rse = rs - nar_d;
  const bool small = mid_max * 256 + ll_max + corr_abs + 2 < (int64_t(1) << 31) &&
                     (rse <= 16 ? (hh_max << (16 - (rse < 16 ? (rse > 0 ? rse : 0) : 16))) + ((mid_max * 256 + ll_max + corr_abs) >> (rse > 0 ? rse : 0)) + 2
                                : hh_max + ((mid_max * 256 + ll_max + corr_abs) >> 16) + 2) < (int64_t(1) << 31);
  if (p.out_eb == 2 && p.out.S && q_const_mode(p.out.Q) && (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT) &&
      rse >= 1 && rs <= 31 && acc_wide && small && (p.out.W == 16 || (nar_d > 0 && plan.nb <= kMaxRegNB))) {
    return p.out.O == ACDSP_SAT ? 2 : 1;
  }
  // the other rounding modes and AC_SAT_SYM / AC_SAT_ZERO on full 16-bit OUT_TYPEs: the same classes with the increment of the dropped
  // bits (MfmaArgs::gq_*; NAR instantiations: register-resident shapes of up to kMaxRegNB K-blocks).  ACDSP_NO_GQ: generic class (A/B knob)
  static const bool no_gq = getenv("ACDSP_NO_GQ") != nullptr;
  if (!no_gq && fir_mfma_general_q(p) && p.out_eb == 2 && p.out.S && p.out.W == 16 && rs >= 1 && rs <= 31 && acc_wide && small && plan.nb <= kMaxRegNB) {
    return p.out.O == ACDSP_WRAP ? 1 : 2;
  }
  // EPI 4: int16 containers past the 32-bit bounds, on the LDS-resident kernels (more than kMaxRegNB K-blocks): exact 64-bit recombination,
  // ACC_TYPE wrap included, branch-free (epi64).  ACDSP_NO_EPI4: the generic class instead (A/B knob).
  static const bool no_epi4 = getenv("ACDSP_NO_EPI4") != nullptr;
  if (!no_epi4 && plan.nb > kMaxRegNB && p.out_eb == 2 && p.out.S && q_const_mode(p.out.Q) &&
      (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT) && p.acc.W >= 2 && p.acc.W <= 62 && p.lossless_shift >= 0 && p.lossless_shift <= 32 &&
      p.acc.F - p.out.F >= 1 && p.acc.F - p.out.F <= 62 && p.out.W >= 2 && p.out.W <= 16) {
    return 4;
  }
  // 4-byte containers (W_out 17 .. 32): the wide class with an int32 tile; AC_WRAP or AC_SAT
  if (p.out_eb == 4 && p.out.S && q_const_mode(p.out.Q) && (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT) && acc_wide &&
      rs >= 0 && rs <= 38 && p.out.W >= 2 && p.out.W <= 32 && ll_max + corr_abs + 2 < (int64_t(1) << 31) && plan.nb <= kMaxRegNB) {
    return 3;
  }
  // wide rows: 64-bit shift-and-wrap epilogue of the pipelined body (the low plane still carries C in 32 bits)
  if (p.out_eb == 8 && p.out.S && q_const_mode(p.out.Q) && p.out.O == ACDSP_WRAP && acc_wide &&
      rs >= -16 && rs <= 38 && p.out.W >= 2 && p.out.W <= 64 && (rs < 0 ? -rs : 0) + (64 - p.out.W) <= 63 && ll_max + corr_abs + 2 < (int64_t(1) << 31) && plan.nb <= kMaxRegNB) {
    return 3;
  }
  return 0;
}

static bool use_reg33(int nb, uint64_t hi_mask, int epi) {
  static const bool off = getenv("ACDSP_NO_REG33") != nullptr;   // A/B knob: LDS-resident fragments (fir_mfma_big2_kernel) for NB = 33 too
  return nb == 33 && !off && reg33_band_code(hi_mask, epi) != 0;
}

// NB = 10 .. 31 (258 - 961 taps): the register-resident kernel at one wave per SIMD, like NB = 33, for sets whose high-byte band fits the
// five central K-blocks of the instantiated shape.  Shapes exist for odd NB (11 .. 31: fir_mfma_mid.hip, _mid2, _mid3, translation
// units of their own for the compile time); fir_mfma_plan_blocks pads an even plan by one leading zero block (2 MFMAs per step).  Same-box A/B at 319
// taps: 1.27 -> 1.12 ms (profiles/r3_taps_sweep.txt); dense sets and wider bands stay on the LDS-resident kernels.
static int mid_band_code(int nb, uint64_t hi_mask, int epi) {
  if ((epi != 1 && epi != 2) || nb < 11 || nb > 31 || (nb & 1) == 0) { return 0; }
  const int sk = (nb - 5) / 2;
  int lo = 0, hi = 0;
  if (hi_mask == 0) { lo = hi = nb; }
  else {
    while (lo < nb && !((hi_mask >> lo) & 1)) { lo++; }
    while (hi < nb && !((hi_mask >> (nb - 1 - hi)) & 1)) { hi++; }
  }
  return (lo >= sk && hi >= sk) ? sk + 16 * sk : 0;
}
static bool use_mid(int nb, uint64_t hi_mask, int epi) {
  static const bool off = getenv("ACDSP_NO_MID") != nullptr;   // A/B knob: LDS-resident fragments (fir_mfma_big2_kernel)
  return !off && mid_band_code(nb, hi_mask, epi) != 0;
}

static hipError_t launch_switch(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  if (use_reg33(nb, a.hi_mask, epi)) { return launch_nb33(p, d_frag, a, epi, grid, s); }
  if (use_mid(nb, a.hi_mask, epi)) {
    return nb <= 17 ? launch_fir_mfma_mid(p, nb, d_frag, a, epi, grid, s)
                    : (nb <= 25 ? launch_fir_mfma_mid2(p, nb, d_frag, a, epi, grid, s) : launch_fir_mfma_mid3(p, nb, d_frag, a, epi, grid, s));
  }
  if (nb > kMaxRegNB) { return launch_big(p, d_frag, a, epi, grid, s); }
  switch (nb) {
#ifndef ACDSP_FIR_DEV_NB9   // development builds: only the 255-tap shape (compile time 3 min -> 35 s)
    case 1: return launch_nb<1>(p, d_frag, a, epi, grid, s);
    case 2: return launch_nb<2>(p, d_frag, a, epi, grid, s);
    case 3: return launch_nb<3>(p, d_frag, a, epi, grid, s);
    case 4: return launch_nb<4>(p, d_frag, a, epi, grid, s);
    case 5: return launch_nb<5>(p, d_frag, a, epi, grid, s);
    case 6: return launch_nb<6>(p, d_frag, a, epi, grid, s);
    case 7: return launch_nb<7>(p, d_frag, a, epi, grid, s);
    case 8: return launch_nb<8>(p, d_frag, a, epi, grid, s);
#endif
    case 9: return launch_nb<9>(p, d_frag, a, epi, grid, s);
    default: return hipErrorInvalidValue;
  }
}

// 32x32x32 int8 MFMAs the selected kernel issues per 1024 samples of one channel: two low-plane products per K-block plus two
// high-plane products per K-block of the instantiated band (the honest numerator of an MFMA-utilisation figure; the dense
// formulation would be 4 * nb).
int fir_mfma_issued_per_step(const FirParams &p, const FirMfmaPlan &plan) {
  const int epi = fir_mfma_epilogue_class(p, plan), nb = plan.nb;
  int band = nb;
  if (nb <= kMaxRegNB) {
    const bool nar = (epi == 1 || epi == 2) && p.out_eb == 2 && (p.out.W < 16 || fir_mfma_general_q(p));   // NAR instantiations
    static const bool no_nar_hs = getenv("ACDSP_NO_NAR_SKIP") != nullptr;
    const int hs = !epi ? 0 : (nar ? (no_nar_hs ? 0 : pick_hs_nar(nb, plan.hi_mask)) : pick_hs(nb, plan.hi_mask));
    band = nb - (hs & 15) - (hs >> 4);
  } else if (epi) {
    int b0 = 0, b1 = nb - 1;
    if (plan.hi_mask == 0) { band = 0; b0 = nb; b1 = -1; }
    else {
      while (!((plan.hi_mask >> b0) & 1)) { b0++; }
      while (!((plan.hi_mask >> b1) & 1)) { b1--; }
      band = b1 - b0 + 1;
    }
    if (use_reg33(nb, plan.hi_mask, epi)) { const int code = reg33_band_code(plan.hi_mask, epi); band = nb - (code & 15) - (code >> 4); }
    if (use_mid(nb, plan.hi_mask, epi)) { band = 5; }
  }
  return 2 * nb + 2 * band;
}

// true if the plan runs on a kernel that keeps the Toeplitz fragments in registers (the only ones that can take a coefficient set per
// channel): up to 9 K-blocks always, more when the set's high-byte band fits a compiled shape and the fast int16 epilogue applies
bool fir_mfma_register_resident(const FirParams &p, const FirMfmaPlan &plan) {
  if (plan.nb <= kMaxRegNB) { return true; }
  const int epi = fir_mfma_epilogue_class(p, plan);
  return use_mid(plan.nb, plan.hi_mask, epi) || use_reg33(plan.nb, plan.hi_mask, epi);
}

hipError_t launch_fir_mfma(const FirParams &p, const FirMfmaPlan &plan, int frag_per_channel, const uint32_t *d_frag,
                           const int64_t *d_corr, hipStream_t s) {
  if (p.n <= 0) { return hipSuccess; }
  const int epi = fir_mfma_epilogue_class(p, plan);
  MfmaArgs a;
  a.nar_on = 0; a.nar_d = 0; a.nar_lo = INT32_MIN; a.nar_hi = INT32_MAX; a.nar_sh = 0;
  a.gq_on = 0; a.gq_off = 0; a.gq_c = 0; a.gq_k = 0; a.gq_form = 1; a.gq_lo = INT32_MIN; a.gq_hi = INT32_MAX;
  a.hi_xor = p.in_flip ? 0x80808080u : 0u;
  if ((epi == 1 || epi == 2) && p.out_eb == 2 && fir_mfma_general_q(p)) {   // W_out = 16 (fir_mfma_epilogue_class)
    const int rsq = p.in.F + p.cf.F - p.out.F;                               // 1 .. 31 (fir_mfma_epilogue_class)
    const int32_t half = (int32_t)(uint32_t(1) << (rsq - 1)), all = (int32_t)((uint32_t(1) << rsq) - 1u);
    a.nar_on = 1; a.gq_on = 1;
    if (p.out.O == ACDSP_SAT_SYM) { a.gq_lo = -32767; a.gq_hi = 32767; }
    switch (p.out.Q) {   // (the constant modes keep their constant in ll like the plain classes: no increment on top of it)
      case ACDSP_TRN_ZERO:     a.gq_off = 31; a.gq_c = all; a.gq_k = 0; break;
      case ACDSP_RND_ZERO:     a.gq_off = 31; a.gq_c = 1;   a.gq_k = half - 1; break;
      case ACDSP_RND_INF:      a.gq_off = 31; a.gq_c = -1;  a.gq_k = half; break;
      case ACDSP_RND_CONV:     a.gq_off = 0;  a.gq_c = 1;   a.gq_k = half - 1; break;
      case ACDSP_RND_CONV_ODD: a.gq_off = 0;  a.gq_c = -1;  a.gq_k = half; break;
      default: break;
    }
    a.gq_form = p.out.O == ACDSP_SAT_ZERO ? 2 : ((a.gq_off == 0 && rsq < 16) ? 0 : 1);
  }
  a.w4_sat = (epi == 3 && p.out_eb == 4 && p.out.O == ACDSP_SAT) ? 1 : 0; a.w4_lo = p.out.lo; a.w4_hi = p.out.hi;
  if (epi == 3 && p.out_eb == 4 && p.out.O == ACDSP_WRAP) {
    const int rs4 = p.in.F + p.cf.F - p.out.F;
    const int64_t rnd4 = q_preload(p.out.Q, rs4);
    const int64_t lo_max = 128 * (plan.sum_abs_hi + plan.sum_abs_lo) * 256 + 128 * plan.sum_abs_lo + (plan.corr < 0 ? -plan.corr : plan.corr) + rnd4 + 2;
    if (rs4 >= 1 && rs4 <= 31 && lo_max < (int64_t(1) << 31) && 128 * plan.sum_abs_hi + (lo_max >> 16) + 2 < (int64_t(1) << 31)) { a.w4_sat = 2; }
  }
  if ((epi == 1 || epi == 2) && p.out_eb == 2 && p.out.W < 16) {   // (class 1 / 2 with fewer than 16 bits: at most kMaxRegNB K-blocks)
    a.nar_on = 1; a.nar_d = 16 - p.out.W;
    if (epi == 2) { a.nar_lo = (int32_t)p.out.lo; a.nar_hi = (int32_t)p.out.hi; }
    else { a.nar_sh = 32 - p.out.W; }
  }
  a.n_steps = (p.n + 1023) / 1024;
  a.n8 = (p.n + 7) / 8 * 8;
  // >= 16384 waves when the problem allows it; a chunk re-reads NB-1 halo blocks per step anyway
  int64_t spw = (a.n_steps * p.n_ch + 16383) / 16384;
  if (spw < 8) { spw = 8; }
  // Short filters (<= 4 K-blocks, up to 97 taps) are bound by the memory system, not by the MFMAs or the power cap: 32 KB spans per wave,
  // the best span of a bare copy (tools/copy_probe2.hip), run them 13 % faster than 128 KB spans (15 - 95 taps: 0.733 against 0.84 ms per
  // 1024 ch x 2^20 samples, same box; 12 and 24 steps: 0.76 / 0.78).  From 127 taps on 16 .. 64 steps measure alike (profiles/r3_taps_sweep.txt).
  if (plan.nb <= 4 && spw > 16) { spw = 16; }
  // 8-byte outputs (OUT = ACC rows: 2 KB read and 8 KB written per step): 8 steps per wave, 1.96 against 2.07 ms at 64 on the config-2
  // wide row (2 / 4 / 6 / 12 / 16 steps: 2.02 / 1.98 / 1.98 / 2.02 / 2.02; same box, two passes)
  if (epi == 3 && spw > 8) { spw = 8; }
  ACDSP_TUNE_ENV(spw_env, "ACDSP_FIR_SPW");   // tuning knob: 1024-sample steps per wave
  if (spw_env && atoi(spw_env) > 1) { spw = atoi(spw_env); }
  a.steps_per_wave = spw;
  const int oeb = p.out_eb;
  // vector stores at any element-aligned address (gfx950 takes them: 652 parity tests with unaligned rows forced through the vector
  // paths, profiles/r3_unaligned.txt); ACDSP_ALIGNED_ONLY=1 restores the round-2 rule (guarded element-wise stores for such rows)
  static const bool aligned_only = getenv("ACDSP_ALIGNED_ONLY") != nullptr;
  a.out_vec_ok = !aligned_only || (((uintptr_t)p.y % (4 * oeb) == 0) && ((p.out_stride * oeb) % (4 * oeb) == 0));
  a.frag_per_channel = frag_per_channel;
  a.hi_mask = plan.hi_mask;
  a.lo_mask = plan.lo_mask;
  a.nb = plan.nb; a.hb0 = 0; a.hb1 = plan.nb - 1; a.step0 = 0;
  a.corr = d_corr;
  const int wpb = (plan.nb > kMaxRegNB && !use_reg33(plan.nb, plan.hi_mask, epi) && !use_mid(plan.nb, plan.hi_mask, epi)) ? 8 : kSmallWaves;   // channels (waves) per workgroup
  dim3 grid((unsigned)((a.n_steps + spw - 1) / spw), (unsigned)((p.n_ch + wpb - 1) / wpb));
  a.dbg = nullptr;
  static const bool dbg_clock = getenv("ACDSP_DEBUG_CLOCK") != nullptr;
  const size_t n_waves = (size_t)grid.x * grid.y * wpb;
  if (dbg_clock) { if (hipMalloc((void **)&a.dbg, n_waves * 48) != hipSuccess) { a.dbg = nullptr; } else { (void)hipMemsetAsync(a.dbg, 0, n_waves * 48, s); } }
  hipError_t rc = launch_switch(p, plan.nb, d_frag, a, epi, grid, s);
  if (a.dbg) {
    std::vector<int64_t> hd(2 * n_waves);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(hd.data(), a.dbg, n_waves * 16, hipMemcpyDeviceToHost);
    double sc = 0, sr = 0;
    for (size_t i = 0; i < n_waves; i++) { sc += (double)hd[2 * i]; sr += (double)hd[2 * i + 1]; }
    fprintf(stderr, "[acdsp] fir_mfma: %zu waves, mean wave life %.1f us, shader clock %.3f GHz (spw %lld)\n", n_waves,
            sr / n_waves / 100.0, sc / sr * 0.1, (long long)spw);
#ifdef ACDSP_X_PHASES
    {
      std::vector<int64_t> ph(4 * n_waves);
      (void)hipMemcpy(ph.data(), a.dbg + 2 * n_waves, n_waves * 32, hipMemcpyDeviceToHost);
      double t[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < n_waves; i++) { for (int q = 0; q < 4; q++) { t[q] += (double)ph[4 * i + q]; } }
      const double steps = (double)n_waves * (double)spw;
      fprintf(stderr, "[acdsp] cycles per step: M %.0f | barrier %.0f | O %.0f | barrier %.0f\n", t[0] / steps, t[1] / steps, t[2] / steps, t[3] / steps);
    }
#endif
    (void)hipFree(a.dbg);
  }
  return rc;
}

}  // namespace acdsp
