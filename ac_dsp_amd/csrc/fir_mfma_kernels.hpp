// fir_mfma_kernels.hpp -- the kernels of the many-channel 16-bit FIR on the gfx950 matrix cores, shared by the six translation units of the
// family: fir_mfma.hip (host plan, class decisions, dispatch; 1 .. 9 and 33 K-blocks), fir_mfma_mid.hip / _mid2 / _mid3 (11 .. 31
// K-blocks) and fir_mfma_alt.hip / _alt2 (narrow OUT_TYPEs, general rounding modes, 4-byte containers).  A unit compiles the kernels its
// own launchers name and no others.  The LDS-resident kernels for large tap counts have one user and stay in fir_mfma.hip;
// fir_kernels.hpp stays the interface to the engine layer.
//
// Formulation.  For one block of 32 consecutive outputs of one channel,
//     y[T0+i] = sum_k c[k] x[T0+i-k]        i = 0..31
// is a [32 x 32*NB] Toeplitz matrix (built from c, the same for every output block of the
// channel) times the [32*NB] input samples ending at T0+31, NB = ceil((N-1)/32)+1.  The 32 MFMA
// columns are 32 CONSECUTIVE output blocks of the same channel:
//     D[i][n] = y[T0 + 32n + i] = sum_b sum_k A_b[i][k] * X_b[k][n],
//     A_b[i][k] = c[i - k + 32*(NB-1-b)],     X_b[k][n] = x[T0 - 32(NB-1) + 32(n+b) + k],
// so one step (4*NB MFMA 32x32x32) produces 1024 consecutive outputs of one channel from one
// contiguous (32+NB-1)*64-byte stretch of its row.
// MFMA has no int16 operand type, so both operands are split into two signed bytes:
//     c = 256*ch + cl            (cl = sign-extended low byte, ch = (c - cl)/256, both int8)
//     x = 256*xh + xl + 128      (xh = high byte, xl = low byte re-biased to signed)
//     y = 65536*S(ch,xh) + 256*(S(ch,xl) + S(cl,xh)) + S(cl,xl) + 128*sum(c)
// Each S is an int32 MFMA accumulation (|S| <= 32*NB*2^14 < 2^31).  The result is the exact
// integer dot product; rounding/saturation into OUT_TYPE happens once, in the epilogue.
//
// Data movement.  The 2*NB A fragments (4 VGPRs each) stay in registers for the whole kernel.
// Column n of K-block b is "input chunk n+b": the X fragments of the NB K-blocks are lane-shifted
// copies of each other.  The shift is done by LDS addressing: a step's chunks are fetched with fully
// coalesced 16-byte loads (every HBM visit of a row moves 2+ KB -- a first version that put 32
// channels in the columns touched 32 rows x 64 B per step, ~130k interleaved DRAM streams, and
// stalled near 2 TB/s), split into byte planes with v_perm_b32, staged in LDS (2.5 KB per wave) and
// each K-block's fragment is a contiguous, conflict-free ds_read_b128 at offset 16*(n+b).
// One wave = one channel x one time chunk; the Toeplitz fragments are per coefficient set, so
// per-channel coefficients cost nothing extra.
//
// Scheduling.  On gfx950 the int8 MFMA run and the rest of a SIMD's instruction stream serialise: time per
// step ~ (#MFMA x 32 cycles) + (#other instructions x ~4 cycles), whatever the wave pairing (measured:
// two free-running waves per SIMD, an 8-wave ping-pong with s_barrier role swaps, and a software-pipelined
// 1 MFMA : 4 VALU interleave all land within a few percent, the ping-pong 4 % behind).  The kernel therefore
// uses independent single-wave workgroups and spends its effort on instruction count: zero high-byte Toeplitz
// blocks are skipped, the epilogue is 4 VALU ops per output plus a clamping pack, outputs leave through a
// swizzled LDS tile as two 16-byte-per-lane stores.  The 8-wave ping-pong form stays selectable (kSmallWaves)
// and is what the large-tap kernel uses, where the Toeplitz fragments are shared through LDS.
#pragma once

#include "fir_kernels.hpp"

namespace acdsp {

// AC_RND and AC_RND_MIN_INF are "add a constant, then floor" (2^(rs-1) and 2^(rs-1) - 1): the constant rides in the preloaded low-plane
// accumulator of every fast epilogue class, like AC_TRN's zero
__host__ __device__ static inline bool q_const_mode(int q) { return q == ACDSP_TRN || q == ACDSP_RND || q == ACDSP_RND_MIN_INF; }
__host__ __device__ static inline int64_t q_preload(int q, int rs) {
  if (rs <= 0 || rs > 62) { return 0; }
  return q == ACDSP_RND ? (int64_t(1) << (rs - 1)) : (q == ACDSP_RND_MIN_INF ? (int64_t(1) << (rs - 1)) - 1 : 0);
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef short v4s __attribute__((ext_vector_type(4)));

constexpr int kMaxRegNB = 9;  // register-resident Toeplitz fragments: up to 32*8+1 = 257 taps
constexpr int kMaxNB = 33;    // Toeplitz fragments in LDS (shared coefficient set): up to 1025 taps

// Bytes of one staged [plane][half] array of nc 16-byte chunks.  The two halves of a plane are written by one
// ds_write_b64 (lanes alternate between them) and LDS stores see 32 banks: pad so that the arrays sit 16 banks apart
// (size = 64 mod 128), otherwise chunk c of both halves shares its banks (2-way conflict on every staging store:
// SQ_LDS_BANK_CONFLICT was 27 % of SQ_LDS_IDX_ACTIVE).
__host__ __device__ constexpr int staged_array_bytes(int nc) { return ((nc * 16 + 63) / 128) * 128 + 64; }

struct MfmaArgs {
  int64_t steps_per_wave;  // 1024-sample steps per wave
  int64_t n_steps;         // ceil(n / 1024)
  int64_t n8;              // n rounded up to a multiple of 8 (rows are readable that far)
  int32_t out_vec_ok;
  int32_t frag_per_channel;
  uint64_t hi_mask, lo_mask;  // bit b: K-block b of the hi / lo coefficient plane has a non-zero entry (any set)
  int32_t nb, hb0, hb1;       // big-NB kernel: K-blocks, and the range [hb0, hb1] of non-zero high-byte blocks
  int64_t step0;              // big-NB kernels: first 1024-sample step of this launch (split launches)
  const int64_t *corr;     // [n_sets] 128 * sum(c) per coefficient set
  // OUT_TYPEs of W < 16 bits in the 32-bit epilogue classes (round 4).  With d = 16 - W the epilogue shifts by rs - d instead of rs, packs
  // as for 16 bits (AC_SAT: saturating pack, AC_WRAP: truncating pack) and shifts the packed words right by d, arithmetically:
  // sat16(q') >> d == sat_W(q' >> d) and the sign bit of the truncated q' is bit W - 1 of q.  One v_pk_ashrrev_i16 per two outputs, in the
  // NAR instantiations of the pipelined body only; the edge chunks (fir_mfma_body) convert in registers: clamp to [nar_lo, nar_hi],
  // sign-extend the low 32 - nar_sh bits.  nar_on = 0: 16-bit OUT_TYPEs, nothing of this runs.
  int32_t nar_on, nar_d, nar_lo, nar_hi, nar_sh;
  // 16-bit OUT_TYPEs with a sign- / parity-dependent rounding mode or AC_SAT_SYM / AC_SAT_ZERO (round 5), also in the NAR instantiations
  // (nar_d = 0): the truncated quotient of the 32-bit epilogue plus the increment the dropped bits ask for (acdsp_dev.hpp: q_increment),
  // then a clamp to [gq_lo, gq_hi] (AC_SAT_SYM: +-(2^15 - 1)) or, gq_form = 2, zero outside the int16 range.  gq_on = 0: the constant modes
  // (AC_TRN / AC_RND / AC_RND_MIN_INF) into AC_WRAP / AC_SAT, whose rounding constant rides in ll.
  // gq_off / gq_c / gq_k: the mode's bit, increment and constant; gq_form: which copy of the loop (epi32_gq).
  int32_t gq_on, gq_off, gq_c, gq_k, gq_form, gq_lo, gq_hi;
  // unsigned 16-bit samples: 0x80808080 flips the top bit of every high byte as the planes are split (x - 32768 is a signed int16; the
  // host adds 32768 sum(c) to corr); 0 for signed samples.  One v_xor per four samples, in every instantiation.
  uint32_t hi_xor;
  // 4-byte containers in the wide class (W4 instantiations of the pipelined body): w4_sat = 1: AC_SAT bounds, 0: wrap to W_out bits in
  // 64 bits, 2: wrap in 32-bit arithmetic (2^8 mid + ll and, for rs > 16, hh + carry exact in int32: host-checked)
  int32_t w4_sat;
  int64_t w4_lo, w4_hi;
  int64_t *dbg;            // optional: per-wave {shader-clock ticks, 100 MHz real-time ticks} (ACDSP_DEBUG_CLOCK)
};

// 32-bit epilogue of the int16-output fast path.  V = 2^16 hh + 2^8 mid + ll is the exact dot product (ll
// already carries 128*sum(c) and the rounding constant); lo = 2^8 mid + ll fits int32 (host-checked), so
//   V >> rs = (hh << (16 - rs)) + (lo >> rs)            for rs <= 16   (2^16 hh is a multiple of 2^rs)
//   V >> rs = (hh + (lo >> 16)) >> (rs - 16)            for rs  > 16
// i.e. 3 (4) VALU ops per output; rs is wave-uniform.
// high-byte plane of unsigned 16-bit samples (MfmaArgs::hi_xor): in place and from an SGPR.  The nine-block kernels sit at the
// 256-register limit and the allocator's outcome there turns on details: written as `^` this spilled four VGPRs in the HS = 34 kernels of
// classes 1 / 2 and 117 in the dense class-3 one; as a movable asm only the latter (118); as a fixed one (volatile) the class-3 kernel drops
// to 2 spilled VGPRs (9 before the xor existed) but classes 1 / 2 spill 4 in their HS = 0 kernels -- so class 3 pins it, the others do not
// (tests/test_abi.py: test_no_kernel_uses_scratch is the judge of any other arrangement).
template <bool PINNED>
__device__ __forceinline__ unsigned hi_flip(unsigned v, unsigned m) {
  if constexpr (PINNED) { asm volatile("v_xor_b32 %0, %1, %0" : "+v"(v) : "s"(m)); }
  else { asm("v_xor_b32 %0, %1, %0" : "+v"(v) : "s"(m)); }
  return v;
}
template <bool WIDE>   // WIDE: rs > 16
__device__ __forceinline__ void epi32_t(const v16i &hh, const v16i &mid, const v16i &ll, int rs, int (&o)[16]) {
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int lo = (int)(((unsigned)mid[r] << 8) + (unsigned)ll[r]);
    o[r] = WIDE ? (hh[r] + (lo >> 16)) >> (rs - 16) : (int)((unsigned)hh[r] << (16 - rs)) + (lo >> rs);
  }
}
// The same with the increment of a sign- or parity-dependent rounding mode (round 5, second form).  The dropped bits of V >> rs are the low
// rs bits of lo (rs <= 16: 2^16 hh is a multiple of 2^rs), or the low rs - 16 bits of hh + (lo >> 16) above the low half of lo; with
// rem = those bits, m = -1 where the floor quotient q0 is negative (gq_off = 31) or odd (gq_off = 0), every mode is
//   q = q0 + ((rem + (m & C) + K) >> rs)
// (acdsp_dev.hpp: q_increment, written as one carry): AC_TRN_ZERO C = 2^rs - 1, K = 0 on the sign; AC_RND_ZERO C = 1, K = half - 1 and
// AC_RND_INF C = -1, K = half on the sign; AC_RND_CONV C = 1, K = half - 1 and AC_RND_CONV_ODD C = -1, K = half on the parity; the
// constant modes (AC_TRN / AC_RND / AC_RND_MIN_INF: K rides in ll) come here only for AC_SAT_SYM / AC_SAT_ZERO, with C = K = 0.
// Six (seven) VALU per output on top of epi32_t's three (four); the first form tested mask bits per condition, ~24.
// For rs <= 16 the increment can go into lo BEFORE the shift -- (hh << (16 - rs)) + ((lo + (m & C) + K) >> rs), host-checked to stay inside
// int32 -- which saves the separate carry: the parity of q0 is bit rs of lo for rs < 16 (three VALU more than epi32_t), its sign needs q0
// first (five more, one less than the carry form: not worth a third copy of the loop in kernels that sit at the register limit -- with
// it the six- and nine-block NAR kernels spilled five VGPRs).  One uniform branch per step picks the form; the sign modes, rs = 16 on the
// parity and rs > 16 keep the carry form.
// fence between groups of four outputs of epi32_gq: holds the VALU (register pressure) but lets MFMA, SALU, VMEM and DS instructions cross
constexpr int kEpiFence = 0x0008 | 0x0004 | 0x0010 | 0x0080;
// FORM is a compile-time copy of MfmaArgs::gq_form: 0 = increment before the shift on the parity (rs < 16), 1 = carry form, 2 = carry form
// and AC_SAT_ZERO.  The pipelined loop must not branch: a uniform branch per emit splits its body into basic blocks, and the matrix
// products of a group no longer overlap the epilogue next to them (0.29 ms where AC_RND runs 0.21, VALU count almost equal) -- the kernel
// picks one of three copies of the loop instead (fir_mfma_kernel).  Forms 0 / 1 clamp to [gq_lo, gq_hi] (AC_SAT_SYM: +-(2^15 - 1); else the
// whole int32 range) with one v_med3.
template <bool WIDE, int FORM>
__device__ __forceinline__ void epi32_gq(const v16i &hh, const v16i &mid, const v16i &ll, int rs, const MfmaArgs &a, int (&o)[16]) {
  const unsigned C = (unsigned)a.gq_c, K = (unsigned)a.gq_k, off = (unsigned)a.gq_off, mask = (rs >= 32 ? 0u : (1u << rs)) - 1u;
  const int lo_b = a.gq_lo, hi_b = a.gq_hi;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int lo = (int)(((unsigned)mid[r] << 8) + (unsigned)ll[r]);
    int q;
    if constexpr (!WIDE && FORM == 0) {
      const unsigned m = (unsigned)__builtin_amdgcn_sbfe(lo, (unsigned)rs, 1u);
      q = (int)((unsigned)hh[r] << (16 - rs)) + ((int)((unsigned)lo + (m & C) + K) >> rs);
    } else {
      int q0;
      unsigned rem;
      if constexpr (!WIDE) {
        q0 = (int)((unsigned)hh[r] << (16 - rs)) + (lo >> rs);
        rem = (unsigned)lo & mask;
      } else {
        const int t = hh[r] + (lo >> 16);
        q0 = t >> (rs - 16);
        rem = __builtin_amdgcn_perm((unsigned)t, (unsigned)lo, 0x05040100u) & mask;   // t[15:0] : lo[15:0]
      }
      const unsigned m = (unsigned)__builtin_amdgcn_sbfe(q0, off, 1u);
      q = q0 + (int)((rem + (m & C) + K) >> rs);
    }
    if constexpr (FORM == 2) { o[r] = (q < -32768 || q > 32767) ? 0 : q; }
    else { o[r] = q < lo_b ? lo_b : (q > hi_b ? hi_b : q); }
    if ((r & 3) == 3) { __builtin_amdgcn_sched_barrier(kEpiFence); }   // four outputs at a time: the kernels that carry this beside nine blocks of fragments have no registers to interleave sixteen
  }
}
// the same behind uniform branches, for the edge chunks (fir_mfma_body)
template <bool WIDE>
__device__ __forceinline__ void epi32_gq_rt(const v16i &hh, const v16i &mid, const v16i &ll, int rs, const MfmaArgs &a, int (&o)[16]) {
  if (a.gq_form == 0 && !WIDE) { epi32_gq<WIDE, 0>(hh, mid, ll, rs, a, o); }
  else if (a.gq_form == 2) { epi32_gq<WIDE, 2>(hh, mid, ll, rs, a, o); }
  else { epi32_gq<WIDE, 1>(hh, mid, ll, rs, a, o); }
}
__device__ __forceinline__ void epi32_narrow(const MfmaArgs &a, int (&o)[16]) {
  if (a.nar_on) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      int q = o[r] >> a.nar_d;
      q = q < a.nar_lo ? a.nar_lo : (q > a.nar_hi ? a.nar_hi : q);
      o[r] = (int)((unsigned)q << a.nar_sh) >> a.nar_sh;
    }
  }
}
// packed form of the last step (MfmaArgs): four dwords of int16 pairs >> d, arithmetically
__device__ __forceinline__ v4i pk16_ashr(const v4i &v, int d) {
  typedef short v2s_ __attribute__((ext_vector_type(2)));
  const v2s_ d2 = (v2s_){(short)d, (short)d};
  v4i r;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // (the element goes through a scalar first: __builtin_bit_cast applied to a vector-element lvalue reads element 0 whatever the
    // index -- clang 22 / ROCm 7.2 -- and every lane stored four copies of its first dword: round 5, found by disassembly; the round-4
    // parity tests of the narrow OUT_TYPEs never reached this pipelined body)
    const int e = v[i];
    r[i] = __builtin_bit_cast(int, __builtin_bit_cast(v2s_, e) >> d2);
  }
  return r;
}
template <bool GQ = true>   // GQ = false: the kernels of more than kMaxRegNB K-blocks, which the general-rounding class never reaches
__device__ __forceinline__ void epi32(const v16i &hh, const v16i &mid, const v16i &ll, int rs, const MfmaArgs &a, int (&o)[16]) {
  if (GQ && a.gq_on) {
    if (rs <= 16) { epi32_gq_rt<false>(hh, mid, ll, rs, a, o); } else { epi32_gq_rt<true>(hh, mid, ll, rs, a, o); }
    return;
  }
  if (rs <= 16) { epi32_t<false>(hh, mid, ll, rs, o); }   // one uniform branch per step, not one per output
  else { epi32_t<true>(hh, mid, ll, rs, o); }
  epi32_narrow(a, o);
}

// B-fragment read-ahead group size and target waves per SIMD of the register-resident kernel (tuning knobs:
// (3, 2) measured 1.117 ms on config 2, (1, 3) 1.068 ms but spills on dense coefficient sets -> 2.2 ms).
#ifndef ACDSP_GS
#define ACDSP_GS 3
#endif
#ifndef ACDSP_OCC
#define ACDSP_OCC 2
#endif
// non-temporal accesses (A/B knob): bit 0 = ring loads, bit 1 = int16 tile stores, bit 2 = wide tile stores of the pipelined body,
// bit 3 = stores of the double-wide 1023-tap kernel
#ifndef ACDSP_FIR_NT
#define ACDSP_FIR_NT 15
#endif
#ifndef ACDSP_FIR_PRIO
#define ACDSP_FIR_PRIO 0
#endif
// B-fragment read-ahead group of the 33-block shape (one wave per SIMD, 512 registers to spend): same-box A/B on config 4, two passes
// (round 5): 2: 2.067 / 2.068 ms, 3: 2.078, 4: 2.024 / 2.023, 6: 2.029 / 2.030, 8: 2.056 / 2.054.  The 12 + 12 band (nine high-plane blocks) keeps 2: at 4
// the allocator moves eight VGPRs through AGPRs
#ifndef ACDSP_GS_BIG
#define ACDSP_GS_BIG 4
#endif
constexpr int kGroupSize = ACDSP_GS, kOccupancy = ACDSP_OCC;

// EPI 0: any OUT_TYPE / ACC width through requant64.
// EPI 1: OUT container int16, Q in {TRN, RND}, O = WRAP, no accumulator wrap possible, right shift 1..31:
//        32-bit epilogue (epi32).   EPI 2: the same with O = SAT (v_cvt_pk_i16_i32 clamps and packs).
// EPI 3: OUT container int64, signed, Q in {TRN, RND}, O = WRAP, no accumulator wrap possible (the OUT = ACC row
//        of config 2): 64-bit shift-and-wrap epilogue, stored straight from registers; pipelined body only.
// HS:    compile-time band of K-blocks whose high-byte Toeplitz plane is non-zero: HS = lo + 16 hi skips the first `lo` and the
//        last `hi` blocks (0: none; the band of a linear-phase set is centred on tap (N-1)/2, which is not a block centre, so the
//        two sides differ: config 2's set needs blocks 3 .. 6 of 9).
// WAVES: 8 = ping-pong workgroup (see header), 1 = single-wave workgroup.
// FAST:  the chunk is interior: all loads/stores are full vectors, so the loop has no divergent branch
//        around VMEM and the compiler counts outstanding operations exactly (vmcnt(k), not vmcnt(0)).
template <int NB, int EPI, int HS, int WAVES, bool FAST>
__device__ __forceinline__ void fir_mfma_body(const FirParams &p, const v4i *__restrict__ frag, const MfmaArgs &a,
                                              unsigned char *lds_all) {
  constexpr int HB = NB - 1;          // halo chunks
  constexpr int NC = 32 + HB;         // chunks staged per step
  constexpr int NP = 4 * NC;          // 16-byte raw pieces per step
  constexpr int JN = (NP + 63) / 64;  // raw loads per lane per step
  constexpr int ARR = staged_array_bytes(NC);   // bytes of one [plane][half] array
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = (WAVES == 8) ? (wave >> 2) : 0;  // waves w and w+4 share a SIMD
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y * WAVES + wave;
  if (ch >= p.n_ch) { ch = p.n_ch - 1; }  // surplus waves redo the last channel (identical stores): barriers stay uniform
  ch = __builtin_amdgcn_readfirstlane(ch);  // wave-uniform: row bases live in SGPRs
  const int set = a.frag_per_channel ? ch : 0;
  unsigned char *lds = lds_all + wave * (2 * 4 * ARR + 2048);
  unsigned char *obuf = lds + 2 * 4 * ARR;  // 2 KB output tile (FAST path)

  v4i Ah[NB], Al[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    Ah[b] = frag[((int64_t)set * 2 * NB + 0 * NB + b) * 64 + lane];
    Al[b] = frag[((int64_t)set * 2 * NB + 1 * NB + b) * 64 + lane];
  }

  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;  // hrow[t], t < 0
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);

  // raw 16-byte pieces of this lane: piece l + 64 j covers samples T0 - 32 HB + 8 (l + 64 j) ...
  v4i R[JN];
  auto issue_loads = [&](int64_t T0) {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      // every lane loads (surplus lanes repeat the last piece): no divergent branch around VMEM
      const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
      int64_t t = T0 - 32 * HB + 8 * pc;
      const int16_t *src = (t < 0) ? hrow + t : xrow + ((t < a.n8) ? t : 0);  // beyond n: any valid address
      R[j] = *(const v4i *)src;
    }
  };
  // FAST, every fetch but the chunk's first: no history and no end of row in reach (32 HB <= 1024), so the
  // address is a scalar row base plus a loop-invariant 32-bit lane offset -- no per-load VALU.  A fetch past
  // the chunk's last step is redirected to that step (valid, unused).
  auto issue_loads_in = [&](int64_t T0) {
    const int64_t tl = (s1 - 1) * 1024;
    const char *sb = (const char *)(xrow + ((T0 < tl ? T0 : tl) - 32 * HB));
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
      R[j] = *(const v4i *)(sb + (unsigned)(16 * pc));
    }
  };
  // split into byte planes and stage: arrays [plane][half][chunk] of 16 bytes
  auto stage = [&](unsigned char *buf) {
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = lane + 64 * j;
      if (JN * 64 == NP || pc < NP) {
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

  // epilogue constants
  const int rs = p.in.F + p.cf.F - p.out.F;
  const int64_t corr = a.corr[set];
  // EPI 1/2: C = 128*sum(c) + rounding constant rides in as the initial value of the low-plane accumulator;
  // epi32() then needs 3 VALU ops per output and v_cvt_pk_i16_i32 packs (and clamps, for AC_SAT).
  const int64_t corr_t = corr + (EPI != 0 ? q_preload(p.out.Q, rs) : 0);
  const int c_ll = (EPI != 0) ? (int)corr_t : 0;   // preloaded into the low-plane accumulator (int32-safe, host-checked)
  const v16i ll_init = {c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll};
  int16_t *yrow = (int16_t *)p.y + (int64_t)ch * p.out_stride + 32 * n_col + 4 * h;  // EPI 1/2

  // The Toeplitz fragments must have landed before the loop: otherwise the compiler keeps
  // "s_waitcnt vmcnt(k)" for them inside the loop body (simm16: vmcnt 0, expcnt/lgkmcnt untouched).
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __builtin_amdgcn_sched_barrier(0);

  // Fragment reads (conflict-free ds_read_b128) run one group of GS K-blocks ahead of the MFMAs that
  // consume them; sched_barrier(0) pins the "reads of group g+1, then MFMAs of group g" order, which
  // the scheduler would otherwise re-serialise into read-wait-MFMA per block.  Group 0 of a step is
  // read at the end of the previous O phase, so its latency hides behind the barrier.
  constexpr int GS = kGroupSize, NG = (NB + GS - 1) / GS;
  v4i Bh[2][GS], Bl[2][GS];
  auto read_group = [&](const unsigned char *buf, int g, v4i (&dh)[GS], v4i (&dl)[GS]) {
    const unsigned char *fh = buf + (0 * 2 + h) * ARR + n_col * 16;
    const unsigned char *fl = buf + (1 * 2 + h) * ARR + n_col * 16;
#pragma unroll
    for (int i = 0; i < GS; i++) {
      const int b = g * GS + i;
      if (b < NB) {
        dh[i] = *(const v4i *)(fh + 16 * b);
        dl[i] = *(const v4i *)(fl + 16 * b);
      }
    }
  };

  // software pipeline: loads run two steps ahead of the MFMAs, staging one step ahead
  issue_loads(s0 * 1024);
  stage(lds);
  if (FAST) { issue_loads_in((s0 + 1) * 1024); }
  else if (nsteps > 1) { issue_loads((s0 + 1) * 1024); }
  read_group(lds, 0, Bh[0], Bl[0]);
  if (WAVES == 8 && grp == 1) { __builtin_amdgcn_s_barrier(); }  // second half starts one phase later

  for (int s = 0; s < nsteps; s++) {
    const int64_t T0 = (s0 + s) * 1024;
    const unsigned char *buf = lds + (s & 1) * (4 * ARR);

#ifdef ACDSP_X_PHASES
    const uint64_t tp0 = __builtin_readcyclecounter();
#endif
    // ---------------- phase M: MFMA run (four independent accumulators: every one is reused only
    // every fourth MFMA, so a single wave keeps the matrix pipe at its 32-cycle issue rate) ----------------
    v16i hh = {0}, mid = {0}, ll = ll_init;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      __builtin_amdgcn_sched_barrier(0);
      if (g + 1 < NG) { read_group(buf, g + 1, Bh[(g + 1) & 1], Bl[(g + 1) & 1]); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < GS; i++) {
        const int b = g * GS + i;
        if (b < NB) {
          // a Toeplitz block whose high-byte plane is all zero contributes nothing to hh / mid
          if (HS == 0 || (b >= (HS & 15) && b <= NB - 1 - (HS >> 4))) {
            hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bh[g & 1][i], hh, 0, 0, 0);
            mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bl[g & 1][i], mid, 0, 0, 0);
          }
          ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bl[g & 1][i], ll, 0, 0, 0);
          mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bh[g & 1][i], mid, 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#ifdef ACDSP_X_PHASES
    const uint64_t tp1 = __builtin_readcyclecounter();
#endif
    if (WAVES == 8) { __builtin_amdgcn_s_barrier(); }
#ifdef ACDSP_X_PHASES
    const uint64_t tp2 = __builtin_readcyclecounter();
#endif

    // ---------------- phase O: epilogue, stores, staging of the next step, prefetch ----------------
    // D layout: lane (n_col, h), register r: sample T0 + 32 n_col + (r&3) + 8 (r>>2) + 4 h
    int o16[16];
    if (EPI != 0) { epi32(hh, mid, ll, rs - a.nar_d, a, o16); }
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int64_t t0 = T0 + 32 * n_col + 8 * g + 4 * h;
      if (EPI != 0) {
        const int *o = o16 + 4 * g;
        v4s pk;
        if (EPI == 2) {  // OUT_TYPE is a signed 16-bit AC_SAT type: clamp and pack in one instruction
          typedef short v2s __attribute__((ext_vector_type(2)));
          const v2s p0 = __builtin_amdgcn_cvt_pk_i16(o[0], o[1]), p1 = __builtin_amdgcn_cvt_pk_i16(o[2], o[3]);
          pk = (v4s){p0.x, p0.y, p1.x, p1.y};
        } else {
          pk = (v4s){(short)o[0], (short)o[1], (short)o[2], (short)o[3]};
        }
        int16_t *dst = yrow + T0 + 8 * g;
        if (FAST) {
          // stage the 8-byte piece for the row-contiguous write-out below: pair P = 4 n + g holds samples
          // 32 n + 8 g .. +7; its slot is rotated by P >> 4 so that both the ds_write_b64 here and the
          // ds_read_b128 there are bank-conflict free
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
      // 1024 outputs = 2 KB contiguous: two fully coalesced 16-byte-per-lane stores (8 whole 128-byte
      // lines each) instead of four 8-byte scatters that L2 has to merge
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int P = 64 * half + lane;
        const v4i val = *(const v4i *)(obuf + ((P & ~15) | ((P + (P >> 4)) & 15)) * 16);
        *(v4i *)((int16_t *)p.y + (int64_t)ch * p.out_stride + T0 + 512 * half + 8 * lane) = val;
      }
    }
    if (s + 1 < nsteps) {
      unsigned char *nbuf = lds + ((s + 1) & 1) * (4 * ARR);
      stage(nbuf);                                                      // consumes the loads of step s+1
      if (FAST) { issue_loads_in(T0 + 2048); }                          // past the chunk: redirected, harmless
      else if (s + 2 < nsteps) { issue_loads(T0 + 2048); }
      read_group(nbuf, 0, Bh[0], Bl[0]);
    }
#ifdef ACDSP_X_PHASES
    const uint64_t tp3 = __builtin_readcyclecounter();
#endif
    if (WAVES == 8 && (grp == 0 || s + 1 < nsteps)) { __builtin_amdgcn_s_barrier(); }
#ifdef ACDSP_X_PHASES
    if (a.dbg && lane == 0) {
      const int64_t w = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * WAVES + wave;
      int64_t *d = a.dbg + 2 * (int64_t)gridDim.x * gridDim.y * WAVES + 4 * w;
      d[0] += (int64_t)(tp1 - tp0); d[1] += (int64_t)(tp2 - tp1); d[2] += (int64_t)(tp3 - tp2);
      d[3] += (int64_t)(__builtin_readcyclecounter() - tp3);
    }
#endif
  }
}

// ---------------------------------------------------------------------------------------------------
// Software-pipelined body for interior chunks of single-wave workgroups (the steady state of every long
// run).  The plain body above alternates an MFMA run (M) with ~120 dependent VALU/LDS/VMEM instructions
// (O): measured 1290 + 1220 shader cycles per step, i.e. the matrix pipe idles half the time even with two
// waves per SIMD.  Here step s's MFMAs run with everything else of the neighbouring steps interleaved in
// the same instruction stream -- the epilogue and write-out of step s-1 (from a second accumulator set),
// the byte-plane staging of step s+1 and the global loads of step s+2 -- so the wave always has MFMAs to
// issue and the other work hides in their shadow (tools/mfma_probe.hip: 39 cycles/MFMA with the epilogue
// interleaved vs 36 bare).  The loop is unrolled by two so the accumulator sets and the B-fragment
// double buffer swap roles by renaming; it contains no branch.
template <int NB, int EPI, int HS, int NAR = 0, bool W4 = false, int GQF = 1>   // NAR: 1 = OUT_TYPEs of fewer than 16 bits, 2 = general rounding / overflow modes of a 16-bit OUT_TYPE (GQF: epi32_gq's FORM)
__device__ __forceinline__ void fir_mfma_pipe_body(const FirParams &p, const v4i *__restrict__ frag, const MfmaArgs &a,
                                                   unsigned char *lds) {
  static_assert(EPI >= 1 && EPI <= 3, "fast epilogue classes only");
  constexpr int HB = NB - 1, NC = 32 + HB, NP = 4 * NC, JN = (NP + 63) / 64;
  // The staged byte planes live in a RING of 128 chunk slots (four steps of 32) per [plane][half] array, plus HB mirror
  // slots [128, 128 + HB) that repeat slots [0, HB): the window of a step with s % 4 == PAR is the linear slot range
  // [32 PAR, 32 PAR + 32 + HB), so its first HB chunks are the tail the previous step staged -- a step loads and stages only
  // its own 2 KB of new samples (two 16-byte loads per lane) instead of the whole 2.5 KB window with its 25 % halo.
  // The wide-output class (EPI 3) keeps two separate windows per step pair: its loop, unrolled by four, ran 2 - 8 % slower
  // (same-box A/B, profiles/r2_ab_ring.txt) -- that row is bound by its 8-byte stores, not by the input side.
  constexpr bool RINGED = EPI != 3;
  constexpr int RING = 128 + HB, ARR = RINGED ? staged_array_bytes(RING) : staged_array_bytes(NC);
  // two accumulator sets + all Toeplitz fragments leave room for GS = 2 only when some high-byte blocks are skipped
  // (round 4: also NB = 7 dense and the wide-output class with at most two blocks skipped per side -- those spilled 1 - 9 VGPRs at GS = 2)
  constexpr int GS = (NB == 33 && HS == 14 + 16 * 14) ? ACDSP_GS_BIG : (NB > kMaxRegNB ? 2 : (((HS == 0 && NB >= 7) || (EPI == 3 && NB >= 9 && (HS == 0 || HS == 2 + 16 * 2))) ? 1 : 2)), NG = (NB + GS - 1) / GS;
  const int lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y;
  if (ch >= p.n_ch) { ch = p.n_ch - 1; }
  ch = __builtin_amdgcn_readfirstlane(ch);
  const int set = a.frag_per_channel ? ch : 0;
  unsigned char *obuf = lds + (RINGED ? 4 : 2 * 4) * ARR;
  unsigned char *dummy = obuf + (EPI == 3 ? 8192 : 2048);   // 1 KB sink for the surplus lanes of stage()

  // (Round 3 also built a form whose Toeplitz rows were permuted so that a lane held 16 CONSECUTIVE outputs and stored 32 contiguous
  // bytes straight from registers, no LDS tile: 0.907 -> 1.23 ms on config 2, profiles/r3_ab_direct_nt.txt -- each store instruction then
  // writes every other 16-byte piece of a 2 KB run.  Rejected; the code was removed in round 4.)
  v4i Ah[NB], Al[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    Ah[b] = frag[((int64_t)set * 2 * NB + 0 * NB + b) * 64 + lane];
    Al[b] = frag[((int64_t)set * 2 * NB + 1 * NB + b) * 64 + lane];
  }
  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;
  int16_t *yout = (int16_t *)p.y + (int64_t)ch * p.out_stride;
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);

  v4i R[JN];
  auto issue_loads_first = [&](int64_t T0) {   // may reach into the history rows
#pragma unroll
    for (int j = 0; j < JN; j++) {
      const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
      int64_t t = T0 - 32 * HB + 8 * pc;
      const int16_t *src = (t < 0) ? hrow + t : xrow + ((t < a.n8) ? t : 0);
      R[j] = *(const v4i *)src;
    }
  };
  v4i Q[2];
  auto issue_loads_new = [&](int64_t T0) {     // the 1024 new samples of a later step; past the chunk: the last step's (never used)
    const int64_t tl = (s1 - 1) * 1024;
    if constexpr (RINGED) {
      const char *sb = (const char *)(xrow + (T0 < tl ? T0 : tl));
#pragma unroll
      for (int j = 0; j < 2; j++) {
#if ACDSP_FIR_NT & 1   // the ring reads every input byte once: non-temporal loads and stores -2.4 % same box (profiles/r2_ab_nt.txt)
        Q[j] = __builtin_nontemporal_load((const v4i *)(sb + (unsigned)(16 * (lane + 64 * j))));
#else
        Q[j] = *(const v4i *)(sb + (unsigned)(16 * (lane + 64 * j)));
#endif
      }
    } else {                                   // the whole window of that step (see fir_mfma_body)
      const char *sb = (const char *)(xrow + ((T0 < tl ? T0 : tl) - 32 * HB));
#pragma unroll
      for (int j = 0; j < JN; j++) {
        const int pc = (lane + 64 * j < NP) ? lane + 64 * j : NP - 1;
        R[j] = *(const v4i *)(sb + (unsigned)(16 * pc));
      }
    }
  };
  typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
  auto stage_ring = [&](auto par_c) {          // Q -> slots [32 (PAR + 1) + HB, + 32) mod 128 of the step after a step of parity PAR
    constexpr int PAR = decltype(par_c)::value;
    constexpr int base = (PAR == 3) ? HB : 32 * (PAR + 1) + HB;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int pc = lane + 64 * j;
      const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
      const unsigned hi0 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)Q[j].y, (unsigned)Q[j].x, 0x07050301u), a.hi_xor);
      const unsigned hi1 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)Q[j].w, (unsigned)Q[j].z, 0x07050301u), a.hi_xor);
      const unsigned lo0 = __builtin_amdgcn_perm((unsigned)Q[j].y, (unsigned)Q[j].x, 0x06040200u) ^ 0x80808080u;
      const unsigned lo1 = __builtin_amdgcn_perm((unsigned)Q[j].w, (unsigned)Q[j].z, 0x06040200u) ^ 0x80808080u;
      unsigned char *dh = lds + (0 * 2 + hh_) * ARR + (base + c) * 16 + sub * 8;
      unsigned char *dl = lds + (1 * 2 + hh_) * ARR + (base + c) * 16 + sub * 8;
      *(v2u_ *)dh = (v2u_){hi0, hi1};
      *(v2u_ *)dl = (v2u_){lo0, lo1};
      if (PAR == 2 && HB > 0 && 16 * (j + 1) > 32 - HB) {   // slots [128, 128 + HB) also go to [0, HB): the window of parity 0 starts there
        const bool m = c >= 32 - HB;                        // (chunks 32 - HB .. 31 of the step: both loads when HB > 16, i.e. NB = 33)
        *(v2u_ *)(m ? dh - 128 * 16 : dummy + lane * 8) = (v2u_){hi0, hi1};
        *(v2u_ *)(m ? dl - 128 * 16 : dummy + 512 + lane * 8) = (v2u_){lo0, lo1};
      }
    }
  };
  auto stage = [&](unsigned char *buf) {       // prologue: the whole window of the chunk's first step -> slots [0, NC)
#pragma unroll
    for (int j = 0; j < JN; j++) {
      // surplus lanes (last j only) store their copy of the last piece into a private dummy slot: no exec-mask branch
      // in the loop, and no 32 lanes hammering one address (same-address ds_writes serialise: measured as 27 % of
      // the LDS cycles in SQ_LDS_BANK_CONFLICT)
      const int pc = lane + 64 * j;
      const bool live = (64 * (j + 1) <= NP) || pc < NP;
      const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
      unsigned hi0 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x07050301u), a.hi_xor);
      unsigned hi1 = hi_flip<EPI == 3>(__builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x07050301u), a.hi_xor);
      unsigned lo0 = __builtin_amdgcn_perm((unsigned)R[j].y, (unsigned)R[j].x, 0x06040200u) ^ 0x80808080u;
      unsigned lo1 = __builtin_amdgcn_perm((unsigned)R[j].w, (unsigned)R[j].z, 0x06040200u) ^ 0x80808080u;
      typedef unsigned v2u __attribute__((ext_vector_type(2)));
      unsigned char *dh = live ? buf + (0 * 2 + hh_) * ARR + c * 16 + sub * 8 : dummy + lane * 8;
      unsigned char *dl = live ? buf + (1 * 2 + hh_) * ARR + c * 16 + sub * 8 : dummy + 512 + lane * 8;
      *(v2u *)dh = (v2u){hi0, hi1};
      *(v2u *)dl = (v2u){lo0, lo1};
    }
  };

  auto stage_new = [&](auto par_c) {
    if constexpr (RINGED) { stage_ring(par_c); }
    else { stage(lds + ((decltype(par_c)::value & 1) ^ 1) * (4 * ARR)); }
  };

  const int rs = p.in.F + p.cf.F - p.out.F;
  const int c_ll = (int)(a.corr[set] + q_preload(p.out.Q, rs));
  const v16i ll_init = {c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll};

  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // Toeplitz fragments landed (keeps their vmcnt out of the loop)
  __builtin_amdgcn_sched_barrier(0);

  // B fragments: groups of GS K-blocks, double buffered; the group sequence runs on across steps, so the
  // buffer of group g of a step with parity PAR is (PAR * NG + g) & 1.
  v4i Bh[2][GS], Bl[2][GS];
  auto read_group = [&](int woff, int g, v4i (&dh)[GS], v4i (&dl)[GS]) {   // woff: byte offset of the step's window
    const unsigned char *fh = lds + woff + (0 * 2 + h) * ARR + n_col * 16;
    const unsigned char *fl = lds + woff + (1 * 2 + h) * ARR + n_col * 16;
#pragma unroll
    for (int i = 0; i < GS; i++) {
      const int b = g * GS + i;
      if (b < NB) {
        dh[i] = *(const v4i *)(fh + 16 * b);
        dl[i] = *(const v4i *)(fl + 16 * b);
      }
    }
  };
  // epilogue of a finished step: 16 outputs per lane -> packed int16 -> swizzled 2 KB LDS tile (fir_mfma_body)
  int64_t *yout64 = (int64_t *)p.y + (int64_t)ch * p.out_stride;
  const int e3_sr = rs > 0 ? rs : 0, e3_wl = 64 - p.out.W, e3_sl = (rs < 0 ? -rs : 0) + e3_wl;
  auto emit = [&](auto wide_c, int64_t T0, const v16i &hh, const v16i &mid, const v16i &ll, int prsel = 2) {
    if constexpr (EPI == 3 && W4) {
      // 4-byte containers (OUT_TYPEs of 17 .. 32 bits; round 4): the same 64-bit value, wrapped (AC_WRAP) or clamped (AC_SAT: MfmaArgs::w4_*)
      // to W bits, as int32 -- a 4 KB tile of 16-byte slots, slot = 8 n + 2 g + h, XOR-swizzled with n >> 1 so that the ds_write_b128 here
      // (16 lanes = columns n .. n + 15 of one (g, h): two 128-byte rows per column pair, eight distinct 16-byte bank groups in each) and
      // the linear ds_read_b128 of flush() (16 consecutive slots = two whole column rows) are bank-conflict free.
#pragma unroll
      for (int g = 0; g < 4; g++) {
        int o[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * g + rr;
          if (a.w4_sat == 2) {
            // AC_WRAP needs the result mod 2^32 only: lo = 2^8 mid + ll is exact in int32 (host-checked), the rest may wrap
            const int lo = (int)(((unsigned)mid[r] << 8) + (unsigned)ll[r]);
            const unsigned q32 = rs <= 16 ? ((unsigned)hh[r] << (16 - rs)) + (unsigned)(lo >> rs) : (unsigned)((hh[r] + (lo >> 16)) >> (rs - 16));
            o[rr] = (int)(q32 << (32 - p.out.W)) >> (32 - p.out.W);
          } else {
            const int64_t V = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r];
            int64_t q = V >> e3_sr;
            if (a.w4_sat) { q = q < a.w4_lo ? a.w4_lo : (q > a.w4_hi ? a.w4_hi : q); }
            else { q = (int64_t)((uint64_t)q << e3_sl) >> e3_wl; }
            o[rr] = (int)q;
          }
        }
        const int slot = 8 * n_col + ((2 * g + h) ^ ((n_col >> 1) & 7));
        *(v4i *)(obuf + slot * 16) = (v4i){o[0], o[1], o[2], o[3]};
      }
      return;
    }
    if constexpr (EPI == 3) {
      // y = wrap_W((V + rnd) >> rs) (or V << -rs), V = 2^16 hh + 2^8 mid + ll.  The 1024 outputs of the step form an
      // 8 KB tile of 16-byte slots (slot = 16 n + 4 g + 2 h + half), XOR-swizzled with the column so that both the
      // ds_write_b128 here (8 consecutive columns per LDS cycle) and the row-contiguous ds_read_b128 of flush() are
      // bank-conflict free; the write-out is then whole 128-byte lines (32-byte pieces straight from registers ran
      // at 2.9 TB/s).
      typedef long v2l __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int g = 0; g < 4; g++) {
        int64_t v[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * g + rr;
          const int64_t V = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r];
          v[rr] = (int64_t)((uint64_t)(V >> e3_sr) << e3_sl) >> e3_wl;
        }
        const int slot = 16 * n_col + ((4 * g + 2 * h) ^ (n_col & 15));
        *(v2l *)(obuf + slot * 16) = (v2l){v[0], v[1]};
        *(v2l *)(obuf + (slot ^ 1) * 16) = (v2l){v[2], v[3]};
      }
      return;
    }
    int o[16];
    if constexpr (NAR == 2 && GQF < 0) { epi32_gq_rt<decltype(wide_c)::value>(hh, mid, ll, rs, a, o); }
    else if constexpr (NAR == 2) { epi32_gq<decltype(wide_c)::value, GQF>(hh, mid, ll, rs, a, o); }   // (general rounding modes: 16-bit OUT_TYPEs only)
    else { epi32_t<decltype(wide_c)::value>(hh, mid, ll, NAR == 1 ? rs - a.nar_d : rs, o); }
    // A lane holds rows 8 g + 4 h .. + 3 of column n: 8 bytes per g, and the 16 lanes of a ds_write_b64 group share h, so
    // they can reach only half of the 32 banks (2-way conflict on every store: the 16.6 % SQ_LDS_BANK_CONFLICT of round 1).
    // v_permlane32_swap trades g-odd of the h = 0 lanes for g-even of the h = 1 lanes: every lane then owns 16 contiguous
    // bytes (slot P = 4 n + 2 pr + h), written as two ds_write_b128; slot ^ ((n >> 1) & 3) spreads the 8 lanes of a store
    // group over the 8 slots of a 128-byte bank row and keeps the aligned 4-slot sets flush() reads conflict-free.
    unsigned d[4][2];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      if (EPI == 2) {
        d[g][0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(o[4 * g], o[4 * g + 1]));
        d[g][1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(o[4 * g + 2], o[4 * g + 3]));
      } else {
        d[g][0] = __builtin_amdgcn_perm((unsigned)o[4 * g + 1], (unsigned)o[4 * g], 0x05040100u);
        d[g][1] = __builtin_amdgcn_perm((unsigned)o[4 * g + 3], (unsigned)o[4 * g + 2], 0x05040100u);
      }
    }
#pragma unroll
    for (int pr = 0; pr < 2; pr++) {
      if (prsel != 2 && prsel != pr) { continue; }
      const auto a0 = __builtin_amdgcn_permlane32_swap(d[2 * pr][0], d[2 * pr + 1][0], false, false);
      const auto a1 = __builtin_amdgcn_permlane32_swap(d[2 * pr][1], d[2 * pr + 1][1], false, false);
      const int P = 4 * n_col + 2 * pr + h;
      *(v4i *)(obuf + (P ^ ((n_col >> 1) & 3)) * 16) = (v4i){(int)a0[0], (int)a1[0], (int)a0[1], (int)a1[1]};
    }
  };
  // ... and its row-contiguous write-out: two coalesced 16-byte-per-lane stores
  auto flush = [&](int64_t T0) {
    if constexpr (EPI == 3 && W4) {
      char *yout32 = (char *)((int32_t *)p.y + (int64_t)ch * p.out_stride + T0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int P = 64 * k + lane;
        const v4i val = *(const v4i *)(obuf + ((P & ~7) | ((P & 7) ^ ((P >> 4) & 7))) * 16);
#if ACDSP_FIR_NT & 4
        __builtin_nontemporal_store(val, (v4i *)(yout32 + (unsigned)(16 * P)));
#else
        *(v4i *)(yout32 + (unsigned)(16 * P)) = val;
#endif
      }
      return;
    }
    if constexpr (EPI == 3) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int P = 64 * k + lane;
        const v4i val = *(const v4i *)(obuf + (P ^ ((P >> 4) & 15)) * 16);
#if ACDSP_FIR_NT & 4
        __builtin_nontemporal_store(val, (v4i *)((char *)(yout64 + T0) + (unsigned)(16 * P)));
#else
        *(v4i *)((char *)(yout64 + T0) + (unsigned)(16 * P)) = val;
#endif
      }
      return;
    }
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const int P = 64 * half + lane;
      v4i val = *(const v4i *)(obuf + (P ^ ((P >> 3) & 3)) * 16);
      if constexpr (NAR == 1) { val = pk16_ashr(val, a.nar_d); }   // OUT_TYPEs of fewer than 16 bits (MfmaArgs::nar_*)
#if ACDSP_FIR_NT & 2
      __builtin_nontemporal_store(val, (v4i *)(yout + T0 + 512 * half + 8 * lane));
#else
      *(v4i *)(yout + T0 + 512 * half + 8 * lane) = val;
#endif
    }
  };

  // One step.  PAR: step parity (selects buffers by renaming); PREV: there is a finished step in (ph, pm, pl).
  auto run_step = [&](auto wide_c, auto par_c, auto prev_c, int s, v16i &hh, v16i &mid, v16i &ll, const v16i &ph, const v16i &pm,
                      const v16i &pl) {
    constexpr int PAR = decltype(par_c)::value;
    constexpr bool PREV = decltype(prev_c)::value;
    const int64_t T0 = (s0 + s) * 1024;
    // byte offsets of this step's and the next step's window: ring slots 32 PAR, or one of the two separate windows
    constexpr int buf = RINGED ? 512 * PAR : (PAR & 1) * (4 * ARR), nbuf = RINGED ? 512 * ((PAR + 1) & 3) : ((PAR & 1) ^ 1) * (4 * ARR);
    hh = (v16i){0}; mid = (v16i){0}; ll = ll_init;
    // side work, spread over the first groups: S = stage step s+1, L = fetch step s+2, E1 = epilogue of step
    // s-1 into the LDS tile, E2 = its write-out
    // loads first (longest latency), the epilogue under the widest MFMA groups: same-box A/B of seven placements in
    // profiles/r2_ab_place.txt (round-2 start: L 1, E1 1, E2 2; this one -1.3 % on config 2, -0.6 % dense, -0.5 % wide).
    // With five or more groups the int16 epilogue is split over two of them (halves of the tile), write-out one group
    // later: another -0.9 % (profiles/r2_ab_place.txt, last section).
    constexpr bool kSplitEmit = NG > 4 && EPI != 3;
    constexpr int gS = 0, gL = 0, gE1 = (NG > 2) ? 2 : NG - 1, gE2 = kSplitEmit ? 4 : ((NG > 3) ? 3 : NG - 1);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      __builtin_amdgcn_sched_barrier(0);
      constexpr int dummy = 0; (void)dummy;
      const int cb = (PAR * NG + g) & 1, nb_ = cb ^ 1;
      // ACDSP_ABL_*: timing-only ablation builds (wrong results) behind the table in profiles/r2_fir255_clock.txt (d)
#ifndef ACDSP_ABL_STAGE
      if (NG == 1 && g == gS) { stage_new(par_c); }
#endif
#ifdef ACDSP_ABL_BREAD
      if (g == 0) {
#endif
      if (g + 1 < NG) { read_group(buf, g + 1, Bh[nb_], Bl[nb_]); }
      else { read_group(nbuf, 0, Bh[nb_], Bl[nb_]); }          // first group of the next step (staged in group 0)
#ifdef ACDSP_ABL_BREAD
      }
#endif
#ifndef ACDSP_ABL_STAGE
      if (NG > 1 && g == gS) { stage_new(par_c); }
#endif
#ifndef ACDSP_ABL_LOAD
      if (g == gL) { issue_loads_new(T0 + 2048); }
#endif
#ifndef ACDSP_ABL_EMIT
      if (PREV && kSplitEmit) {
        if (g == gE1) { emit(wide_c, T0 - 1024, ph, pm, pl, 0); }
        if (g == gE1 + 1) { emit(wide_c, T0 - 1024, ph, pm, pl, 1); }
      } else if (PREV && g == gE1) { emit(wide_c, T0 - 1024, ph, pm, pl); }
#else
      if (PREV && g == gE1) { asm volatile("" :: "v"(ph[0]), "v"(pm[0]), "v"(pl[0])); }   // keeps the MFMAs of the step alive
#endif
#ifndef ACDSP_ABL_FLUSH
      if (PREV && g == gE2) { flush(T0 - 1024); }
#endif
#if ACDSP_FIR_PRIO   // A/B knob: raise the wave's issue priority over its MFMA runs (round-2 review item 1c)
      __builtin_amdgcn_s_setprio(ACDSP_FIR_PRIO);
#endif
#pragma unroll
      for (int i = 0; i < GS; i++) {
        const int b = g * GS + i;
        if (b < NB) {
#if ACDSP_FIR_BORDER
          // (round 6 A/B) the sample operand stays for two consecutive products of a band block: Bh, Bh, Bl, Bl instead of Bh, Bl, Bl, Bh
          if (HS == 0 || (b >= (HS & 15) && b <= NB - 1 - (HS >> 4))) {
            hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bh[cb][i], hh, 0, 0, 0);
            mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bh[cb][i], mid, 0, 0, 0);
            ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bl[cb][i], ll, 0, 0, 0);
            mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bl[cb][i], mid, 0, 0, 0);
          } else {
            ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bl[cb][i], ll, 0, 0, 0);
            mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bh[cb][i], mid, 0, 0, 0);
          }
#else
          if (HS == 0 || (b >= (HS & 15) && b <= NB - 1 - (HS >> 4))) {
            hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bh[cb][i], hh, 0, 0, 0);
            mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah[b], Bl[cb][i], mid, 0, 0, 0);
          }
          ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bl[cb][i], ll, 0, 0, 0);
          mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al[b], Bh[cb][i], mid, 0, 0, 0);
#endif
        }
      }
#if ACDSP_FIR_PRIO
      __builtin_amdgcn_s_setprio(0);
#endif
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using std::integral_constant;
  typedef integral_constant<int, 0> P0; typedef integral_constant<int, 1> P1;
  typedef integral_constant<int, 2> P2; typedef integral_constant<int, 3> P3;
  typedef integral_constant<bool, true> WithPrev; typedef integral_constant<bool, false> NoPrev;

  auto go = [&](auto wide_c) {   // the loop exists once per epilogue shift class: no branch inside it
    // prologue: step s0 staged, step s0+1 in flight, first B group read.  Inside the arm: hoisted above the branch on the shift class,
    // the first B fragments were live across the OTHER arm's loop and spilled around it (4 VGPRs of scratch in eight instantiations).
    issue_loads_first(s0 * 1024);
    stage(lds);
    issue_loads_new((s0 + 1) * 1024);
    read_group(0, 0, Bh[0], Bl[0]);
    v16i hA, mA, lA, hB, mB, lB;
    run_step(wide_c, P0(), NoPrev(), 0, hA, mA, lA, hA, mA, lA);
    int s = 1;
    auto last = [&](int sl, const v16i &h_, const v16i &m_, const v16i &l_) {
      emit(wide_c, (s0 + sl) * 1024, h_, m_, l_);
      flush((s0 + sl) * 1024);
    };
    if constexpr (!RINGED) {
      for (; s + 1 < nsteps; s += 2) {
        run_step(wide_c, P1(), WithPrev(), s, hB, mB, lB, hA, mA, lA);
        run_step(wide_c, P0(), WithPrev(), s + 1, hA, mA, lA, hB, mB, lB);
      }
      if (s < nsteps) {
        run_step(wide_c, P1(), WithPrev(), s, hB, mB, lB, hA, mA, lA);
        last(s, hB, mB, lB);
      } else {
        last(s - 1, hA, mA, lA);
      }
    } else {
      for (; s + 3 < nsteps; s += 4) {      // ring parity = s % 4, accumulator set = s % 2
        run_step(wide_c, P1(), WithPrev(), s, hB, mB, lB, hA, mA, lA);
        run_step(wide_c, P2(), WithPrev(), s + 1, hA, mA, lA, hB, mB, lB);
        run_step(wide_c, P3(), WithPrev(), s + 2, hB, mB, lB, hA, mA, lA);
        run_step(wide_c, P0(), WithPrev(), s + 3, hA, mA, lA, hB, mB, lB);
      }
      if (s < nsteps) {                     // up to three more steps; each arm ends with the write-out of its own last step
        run_step(wide_c, P1(), WithPrev(), s, hB, mB, lB, hA, mA, lA);
        if (s + 1 < nsteps) {
          run_step(wide_c, P2(), WithPrev(), s + 1, hA, mA, lA, hB, mB, lB);
          if (s + 2 < nsteps) {
            run_step(wide_c, P3(), WithPrev(), s + 2, hB, mB, lB, hA, mA, lA);
            last(s + 2, hB, mB, lB);
          } else {
            last(s + 1, hA, mA, lA);
          }
        } else {
          last(s, hB, mB, lB);
        }
      } else {
        last(s - 1, hA, mA, lA);
      }
    }
  };
  if (EPI == 3 || (NAR == 1 ? rs - a.nar_d : rs) <= 16) { go(integral_constant<bool, false>()); }
  else { go(integral_constant<bool, true>()); }
}

// NB > kMaxRegNB (the 1023-tap shape, NB = 33): one wave per SIMD with the whole 512-entry register file -- 2 * 33 Toeplitz
// fragments are 264 registers (fewer with a high-byte band), next to two accumulator sets and the B-fragment double buffer.
template <int NB, int EPI, int HS, int WAVES, int NAR = 0, bool W4 = false>
__global__ void __launch_bounds__(64 * WAVES, (NB > kMaxRegNB ? 1 : kOccupancy))
fir_mfma_kernel(FirParams p, const v4i *__restrict__ frag, MfmaArgs a) {
  // WAVES == 1: the pipelined body keeps a 4-step ring of staged planes (4 arrays of 128 + NB - 1 slots), the plain body two windows
  constexpr int kStaged = (WAVES == 1 && EPI != 0 && EPI != 3 && 4 * staged_array_bytes(128 + NB - 1) > 2 * 4 * staged_array_bytes(32 + NB - 1))
                              ? 4 * staged_array_bytes(128 + NB - 1) : 2 * 4 * staged_array_bytes(32 + NB - 1);
  __shared__ __attribute__((aligned(16))) unsigned char lds[WAVES * (kStaged + (EPI == 3 ? 8192 : 2048)) + 1024];
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  // (a lone first step has no in-row window to park the unused prefetch on: see issue_loads_in)
  const bool interior = EPI != 0 && a.out_vec_ok && s1 * 1024 <= p.n && (s0 > 0 || s1 >= 2);
  const uint64_t c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
  if constexpr (WAVES == 1 && EPI != 0) {
    if (interior) {
      // one copy of the loop per form of the increment (epi32_gq); the eight- and nine-block kernels with most of their fragments live
      // spill 6 - 18 VGPRs that way and keep one loop with the form behind uniform branches
      if constexpr (NAR == 2 && NB >= 8 && HS != 3 + 16 * 3) { fir_mfma_pipe_body<NB, EPI, HS, NAR, W4, -1>(p, frag, a, lds); }
      else if constexpr (NAR == 2) {
        if (a.gq_form == 0) { fir_mfma_pipe_body<NB, EPI, HS, NAR, W4, 0>(p, frag, a, lds); }
        else if (a.gq_form == 2) { fir_mfma_pipe_body<NB, EPI, HS, NAR, W4, 2>(p, frag, a, lds); }
        else { fir_mfma_pipe_body<NB, EPI, HS, NAR, W4, 1>(p, frag, a, lds); }
      } else { fir_mfma_pipe_body<NB, EPI, HS, NAR, W4>(p, frag, a, lds); }
    }
    else if constexpr (EPI == 3) { fir_mfma_body<NB, 0, 0, WAVES, false>(p, frag, a, lds); }   // edges: generic epilogue
    else { fir_mfma_body<NB, EPI, HS, WAVES, false>(p, frag, a, lds); }
  } else {
    if (interior) { fir_mfma_body<NB, EPI, HS, WAVES, true>(p, frag, a, lds); }
    else { fir_mfma_body<NB, EPI, HS, WAVES, false>(p, frag, a, lds); }
  }
  if constexpr (WAVES == 1) {
    // small host-side calls (FirParams::hist_next set): the first chunk's wave also writes the channel's next history, so that a
    // one-sample run() of the drop-in classes is ONE launch (cf. fir_hist_update_kernel)
    if (p.hist_next && blockIdx.x == 0 && (int)blockIdx.y < p.n_ch) {
      const int64_t row = (int64_t)blockIdx.y;
      for (int j = threadIdx.x; j < p.hl; j += 64) {
        const int64_t g = p.n - p.hl + j;
        const int64_t v = (g >= 0) ? load_raw(p.x, row * p.in_stride + g, p.in_eb, p.in.S) : load_raw(p.hist, row * p.hl + p.hl + g, p.in_eb, p.in.S);
        store_raw(p.hist_next, row * p.hl + j, p.in_eb, v);
      }
    }
  }
  if (a.dbg && (threadIdx.x & 63) == 0) {
    const int64_t w = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * WAVES + (threadIdx.x >> 6);
    a.dbg[2 * w] = (int64_t)(__builtin_readcyclecounter() - c0);
    a.dbg[2 * w + 1] = (int64_t)(__builtin_amdgcn_s_memrealtime() - r0);
  }
}

// ---- launchers defined in the other translation units of the family (split for compile time) ----
// NAR (OUT_TYPEs of fewer than 16 bits, general rounding / overflow modes) and W4 (4-byte containers) instantiations of up to kMaxRegNB
// K-blocks: fir_mfma_alt.hip without a band skip, fir_mfma_alt2.hip with one
hipError_t launch_fir_mfma_alt(const FirParams &p, int nb, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s);
hipError_t launch_fir_mfma_alt2(const FirParams &p, int nb, int hs, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s);
// the register-resident shapes for 11 .. 17, 19 .. 25 and 27 .. 31 K-blocks (odd counts): fir_mfma_mid.hip, _mid2, _mid3
hipError_t launch_fir_mfma_mid(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s);
hipError_t launch_fir_mfma_mid2(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s);
hipError_t launch_fir_mfma_mid3(const FirParams &p, int nb, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s);

// the plain instantiations of one shape (classes 1 / 2 / 3 and the generic one): whichever unit calls it compiles them
template <int NB, int HS, int WAVES>
static hipError_t launch_nb_hs(const FirParams &p, const uint32_t *d_frag, const MfmaArgs &a, int epi, dim3 grid, hipStream_t s) {
  const dim3 blk(64 * WAVES);
  if constexpr (WAVES == 1 && NB <= kMaxRegNB) {
    if ((HS == 0 && a.nar_on && (epi == 1 || epi == 2)) || (epi == 3 && p.out_eb == 4)) { return launch_fir_mfma_alt(p, NB, HS, d_frag, a, epi, grid, s); }
    if (HS != 0 && a.nar_on && (epi == 1 || epi == 2)) { return launch_fir_mfma_alt2(p, NB, HS, d_frag, a, epi, grid, s); }
  }
  if (epi == 1) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 1, HS, WAVES>), grid, blk, 0, s, p, (const v4i *)d_frag, a); }
  else if (epi == 2) { hipLaunchKernelGGL((fir_mfma_kernel<NB, 2, HS, WAVES>), grid, blk, 0, s, p, (const v4i *)d_frag, a); }
  else if (epi == 3 && WAVES == 1 && NB <= kMaxRegNB) {
    if constexpr (NB <= kMaxRegNB) {
      hipLaunchKernelGGL((fir_mfma_kernel<NB, 3, HS, WAVES>), grid, blk, 0, s, p, (const v4i *)d_frag, a);
    }
  }
  else { hipLaunchKernelGGL((fir_mfma_kernel<NB, 0, 0, WAVES>), grid, blk, 0, s, p, (const v4i *)d_frag, a); }
  return hipGetLastError();
}

}  // namespace acdsp
