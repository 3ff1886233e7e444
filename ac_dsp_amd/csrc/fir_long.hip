// fir_long.hip -- long 16-bit FIRs (1026 .. 16384 taps) on the gfx950 matrix cores, exact integer arithmetic; and the host helpers the three
// long units share (long_blocks, long_phase_fragments, long_geometry, long_grid).  The segment geometry kLong* is in fir_long_kernels.hpp.
//
// The formulation is that of fir_mfma_kernels.hpp (header comment there): one step is 1024 consecutive outputs of one channel, the 32 MFMA columns
// are 32 consecutive output blocks, K-block b of the [32 x 32 NB] Toeplitz matrix meets "input chunk n + b", both operands are split into
// two signed bytes and the four int32 plane sums are recombined in 64 bits.  |plane sum| <= 32 NB 2^14: 2^28 at NB = 513 (2^29 with the
// re-biased low sample byte), so the accumulators of a step stay live across the WHOLE coefficient set and the recombination, the wrap to
// ACC_TYPE and the conversion to OUT_TYPE run once per output, as in the generic epilogue of fir_mfma_big_body.
//
// What differs is where the A (coefficient) fragments live.  2 KB per K-block: 66 KB at 1025 taps still fit LDS in one piece
// (fir_mfma_big_kernel), 1 MB at 16384 taps do not.  The K-blocks are therefore walked in SEGMENTS of kLongSB = 16 blocks:
//   * the eight waves of a workgroup (eight channels, the same steps) share one 32 KB A segment in LDS, double-buffered: while segment g
//     multiplies, every thread holds its 64 bytes of segment g + 1 in registers (global loads issued before the products of g) and
//     writes them into the other buffer at the top of the next iteration -- ONE __syncthreads() per segment;
//   * each wave stages its own sample window of the segment, 32 + 16 - 1 = 47 chunks from T0 - 32 (NB - 1) + 32 * 16 g on, split into byte
//     planes with v_perm_b32 exactly like fir_mfma_big_body (also double-buffered, private to the wave: no barrier involved).  The window
//     is re-read per segment (3 KB against 64 MFMAs = 2048+ matrix-pipe cycles per wave): left to the L2.
// LDS: 2 x 32 KB + 8 waves x 2 x 4 x 832 B = 116 KB, one workgroup per CU, two waves per SIMD.
//
// Barrier uniformity.  The loop that contains the barrier runs nsteps * NSEG times.  NSEG = ceil(nb / 16) is a launch argument; nsteps is
// min(steps_per_wave, n_steps - blockIdx.x * steps_per_wave): launch arguments and blockIdx only.  Nothing a wave owns -- its channel
// (clamped to the last one past n_ch), the raggedness of its last step, the high-byte range -- enters a loop bound or guards a barrier,
// and no thread leaves the kernel before the loop ends.
//
// One kernel, no template parameters: every ACC_TYPE / OUT_TYPE of up to 64 bits goes through wrap64 / requant64 / store_raw behind
// wave-uniform branches.  Measured (profiles/long_fir_taps_sweep.txt): about 2.5 ms per 2^30 outputs, visible below ~4000 taps.
#include <cstdlib>
#include <vector>

#include "fir_long_kernels.hpp"

namespace acdsp {

struct LongArgs {
  int64_t steps_per_wave;   // 1024-sample steps per workgroup row
  int64_t n_steps;          // ceil(n / 1024)
  int64_t n8;               // n rounded up to a multiple of 8 (rows are readable that far)
  int32_t nb, hb0, hb1;     // K-blocks; the high-plane products of blocks [hb0, hb1] only are issued
  uint32_t hi_xor;          // unsigned 16-bit samples: 0x80808080 flips the top bit of every high byte (fir_mfma_kernels.hpp, MfmaArgs::hi_xor)
  const int64_t *corr;      // [1] 128 * sum(c) (+ 32768 * sum(c) with hi_xor)
};

__global__ void __launch_bounds__(512, 1)
fir_long_kernel(FirParams p, const v4i *__restrict__ frag, LongArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb, NSEG = (NB + kLongSB - 1) / kLongSB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y * 8 + wave;
  if (ch >= p.n_ch) { ch = p.n_ch - 1; }   // (the wave still runs every iteration and barrier; its stores repeat the last channel's)
  // LDS: [2 A segments: 2 planes x 16 blocks x 1 KB][per wave: 2 staged windows of 4 arrays]
  v4i *ldsA = (v4i *)lds_all;
  unsigned char *ldsX = lds_all + (size_t)2 * kLongAWords * 16 + (size_t)wave * 2 * kLongXBytes;

  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;
  // loop bounds: launch arguments and blockIdx only (see "Barrier uniformity" above)
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);
  const int total = nsteps * NSEG;

  v4i RA[kLongAPerThread], RX[kLongJN];
  // global loads of iteration (step s, segment g): this thread's share of the A segment, this lane's share of the wave's window
  auto issue_loads = [&](int s, int g) {
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) {
      const int idx = threadIdx.x + 512 * q, pl = idx / (kLongSB * 64), bl = (idx >> 6) % kLongSB, ln = idx & 63;
      int bg = g * kLongSB + bl;
      if (bg >= NB) { bg = NB - 1; }   // blocks past the set in the last segment: never multiplied, any in-bounds fragment will do
      RA[q] = frag[((size_t)pl * NB + bg) * 64 + ln];
    }
    // window base >= -32 (NB - 1) >= -hl (asserted at create); t is a multiple of 8, so a load never straddles history and row
    const int64_t base = (s0 + s) * 1024 - 32 * (int64_t)(NB - 1) + 32 * kLongSB * (int64_t)g;
#pragma unroll
    for (int j = 0; j < kLongJN; j++) {
      const int pc = (lane + 64 * j < kLongNP) ? lane + 64 * j : kLongNP - 1;
      const int64_t t = base + 8 * pc;
      const int16_t *src = (t < 0) ? hrow + t : xrow + ((t < a.n8) ? t : 0);
      RX[j] = *(const v4i *)src;
    }
  };
  // registers -> LDS: the A segment (all waves, read after the barrier) and the wave's byte planes
  auto commit = [&](int buf) {
    v4i *dstA = ldsA + buf * kLongAWords;
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) { dstA[threadIdx.x + 512 * q] = RA[q]; }
    unsigned char *xb = ldsX + buf * kLongXBytes;
#pragma unroll
    for (int j = 0; j < kLongJN; j++) {
      const int pc = lane + 64 * j;
      if (pc < kLongNP) {
        const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
        const unsigned hi0 = __builtin_amdgcn_perm((unsigned)RX[j].y, (unsigned)RX[j].x, 0x07050301u) ^ a.hi_xor;
        const unsigned hi1 = __builtin_amdgcn_perm((unsigned)RX[j].w, (unsigned)RX[j].z, 0x07050301u) ^ a.hi_xor;
        const unsigned lo0 = __builtin_amdgcn_perm((unsigned)RX[j].y, (unsigned)RX[j].x, 0x06040200u) ^ 0x80808080u;
        const unsigned lo1 = __builtin_amdgcn_perm((unsigned)RX[j].w, (unsigned)RX[j].z, 0x06040200u) ^ 0x80808080u;
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        *(v2u *)(xb + (0 * 2 + hh_) * kLongARR + c * 16 + sub * 8) = (v2u){hi0, hi1};
        *(v2u *)(xb + (1 * 2 + hh_) * kLongARR + c * 16 + sub * 8) = (v2u){lo0, lo1};
      }
    }
  };

  const int64_t corr = a.corr[0];
  v16i hh = {0}, mid = {0}, ll = {0};
  if (total > 0) { issue_loads(0, 0); }
  int s = 0, g = 0;
  for (int it = 0; it < total; it++) {
    const int buf = it & 1;
    // buffer `buf` was last read in iteration it - 2; every wave has passed the barrier of it - 1 since
    commit(buf);
    int sn = s, gn = g + 1;
    if (gn == NSEG) { gn = 0; sn++; }
    if (it + 1 < total) { issue_loads(sn, gn); }   // in flight behind this segment's products
    __syncthreads();

    if (g == 0) { hh = (v16i){0}; mid = (v16i){0}; ll = (v16i){0}; }
    const int b0 = g * kLongSB, nbs = (NB - b0 < kLongSB) ? NB - b0 : kLongSB;
    const v4i *ah = ldsA + buf * kLongAWords + lane, *al = ah + kLongSB * 64;
    const unsigned char *xb = ldsX + buf * kLongXBytes;
    const unsigned char *fh = xb + (0 * 2 + h) * kLongARR + n_col * 16;   // chunk n_col + bl <= 46
    const unsigned char *fl = xb + (1 * 2 + h) * kLongARR + n_col * 16;
    v4i Ahc = ah[0], Alc = al[0], Bhc = *(const v4i *)fh, Blc = *(const v4i *)fl;
    for (int bl = 0; bl < nbs; bl++) {
      v4i Ahn = Ahc, Aln = Alc, Bhn = Bhc, Bln = Blc;
      if (bl + 1 < nbs) {   // fragments of the next K-block are in flight while this one multiplies
        Ahn = ah[(bl + 1) * 64]; Aln = al[(bl + 1) * 64];
        Bhn = *(const v4i *)(fh + 16 * (bl + 1)); Bln = *(const v4i *)(fl + 16 * (bl + 1));
      }
      if (b0 + bl >= a.hb0 && b0 + bl <= a.hb1) {
        hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Bhc, hh, 0, 0, 0);
        mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Blc, mid, 0, 0, 0);
      }
      ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Blc, ll, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Bhc, mid, 0, 0, 0);
      Ahc = Ahn; Alc = Aln; Bhc = Bhn; Blc = Bln;
    }

    if (g == NSEG - 1) {
      // V = 2^16 hh + 2^8 mid + ll + corr, exact in 64 bits; then the reference's two conversions (`acc += ...`, `data_out = acc`)
      const int64_t T0 = (s0 + s) * 1024;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t t0 = T0 + 32 * n_col + 8 * q + 4 * h;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int64_t v = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r] + corr;
          const int64_t acc = wrap64((int64_t)((uint64_t)v << p.lossless_shift), p.acc.W, p.acc.S);
          const int64_t y = requant64(acc, p.acc.F, p.out);
          if (t0 + rr < p.n) { store_raw(p.y, (int64_t)ch * p.out_stride + t0 + rr, p.out_eb, y); }
        }
      }
    }
    s = sn; g = gn;
  }
}

int long_blocks(int taps) {
  const int nb = (taps - 1 + 31) / 32 + 1;
  return nb < 2 ? 2 : nb;
}

bool long_phase_fragments(const int64_t *c, int phases, int nt, std::vector<uint32_t> *frag, std::vector<int64_t> *corr) {
  const int nb = long_blocks(nt);
  const size_t blk = (size_t)64 * 4, plane = (size_t)phases * nb * blk;
  frag->assign(2 * plane, 0u);
  corr->assign((size_t)phases, 0);
  std::vector<uint32_t> one((size_t)2 * nb * blk);
  for (int d = 0; d < phases; d++) {
    FirMfmaPlan mp;
    if (!fir_mfma_build_fragments_nb(c + (size_t)nt * d, nt, nb, &mp, one.data())) { return false; }
    (*corr)[(size_t)d] = mp.corr;
    for (int pl = 0; pl < 2; pl++) {   // [plane][nb] of the phase -> [plane][d][nb] of the set
      std::copy(one.begin() + (size_t)pl * nb * blk, one.begin() + (size_t)(pl + 1) * nb * blk, frag->begin() + pl * plane + (size_t)d * nb * blk);
    }
  }
  return true;
}

LongGeom long_geometry(uint64_t sample_bytes, uint64_t head, int n_ch, uint64_t cap) {
  auto b = [&](uint64_t G) { return sample_bytes * (head + G); };   // bytes of one channel's phase rows
  uint64_t C = (uint64_t)n_ch;
  if (C * b(1024) > cap) {
    C = cap / b(1024) / 8 * 8;
    if (C < 8) { C = 8; }
    if (C > (uint64_t)n_ch) { C = (uint64_t)n_ch; }
  }
  // largest multiple of 1024 with C * b(G) <= cap, inside 1024 .. 65536
  const uint64_t fit = cap / (C * sample_bytes);   // slab samples + head that fit
  uint64_t G = fit > head ? (fit - head) / 1024 * 1024 : 0;
  if (G < 1024) { G = 1024; }
  if (G > 65536) { G = 65536; }
  return {(int64_t)G, (int32_t)C, C * b(G)};
}

LongGrid long_grid(int64_t n_steps, int rows, int64_t min_steps) {
  // a workgroup is eight rows x steps_per_wave steps; >= 2048 workgroups (8 per CU) when the problem allows it
  const int64_t wg_rows = ((int64_t)rows + 7) / 8;
  int64_t spw = (n_steps * wg_rows + 2047) / 2048;
  if (spw < min_steps) { spw = min_steps; }
  return {spw, (unsigned)((n_steps + spw - 1) / spw), (unsigned)wg_rows};
}

bool long_plan_blocks(const int64_t *c, int n_taps, FirLongPlan *plan, std::vector<uint32_t> *frag, int64_t *sum_abs) {
  const int nb = long_blocks(n_taps);
  frag->assign((size_t)2 * nb * 64 * 4, 0u);
  FirMfmaPlan mp;
  if (!fir_mfma_build_fragments_nb(c, n_taps, nb, &mp, frag->data())) { return false; }
  plan->nb = nb;
  plan->corr = mp.corr;
  if (sum_abs) { *sum_abs = mp.sum_abs; }
  // K-block b holds taps i - k + 32 (nb - 1 - b), i, k = 0 .. 31: tap t sits in the blocks b with |32 (nb - 1 - b) - t| <= 31.  The range
  // of blocks with a non-zero high byte follows from the first and the last such tap (the 64-bit masks of FirMfmaPlan end at block 63).
  int t_first = -1, t_last = -1;
  for (int t = 0; t < n_taps; t++) {
    const int64_t lo = ((c[t] + 128) & 0xff) - 128;
    if (c[t] != lo) {
      if (t_first < 0) { t_first = t; }
      t_last = t;
    }
  }
  if (t_first < 0) { plan->hb0 = 1; plan->hb1 = 0; return true; }
  // smallest b: 32 (nb - 1 - b) <= t_last + 31; largest b: 32 (nb - 1 - b) >= t_first - 31
  plan->hb0 = nb - 1 - (t_last + 31) / 32;
  plan->hb1 = nb - 1 - (t_first > 31 ? (t_first - 31 + 31) / 32 : 0);
  if (plan->hb0 < 0) { plan->hb0 = 0; }
  return true;
}

bool fir_long_plan(const int64_t *c, int n_taps, FirLongPlan *plan, std::vector<uint32_t> *frag) {
  if (n_taps < kFirLongMinTaps || n_taps > kFirLongMaxTaps) { return false; }
  return long_plan_blocks(c, n_taps, plan, frag, nullptr);
}

int fir_long_issued_per_step(const FirLongPlan &plan) {
  return 2 * plan.nb + (plan.hb1 >= plan.hb0 ? 2 * (plan.hb1 - plan.hb0 + 1) : 0);
}

hipError_t launch_fir_long(const FirParams &p, const FirLongPlan &plan, const uint32_t *d_frag, const int64_t *d_corr, hipStream_t s) {
  if (p.n <= 0) { return hipSuccess; }
  if (plan.nb < 2 || 32 * (plan.nb - 1) > p.hl || p.in_eb != 2) { return hipErrorInvalidValue; }   // the first step reaches 32 (nb - 1) samples back
  LongArgs a;
  a.n_steps = (p.n + 1023) / 1024;
  a.n8 = (p.n + 7) / 8 * 8;
  const LongGrid lg = long_grid(a.n_steps, p.n_ch, 8);   // at least 8 steps each
  a.steps_per_wave = lg.steps_per_wave;
  a.nb = plan.nb; a.hb0 = plan.hb0; a.hb1 = plan.hb1;
  a.hi_xor = p.in_flip ? 0x80808080u : 0u;
  a.corr = d_corr;
  hipError_t e = hipFuncSetAttribute((const void *)fir_long_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLongLdsBytes);
  if (e != hipSuccess) { return e; }
  hipLaunchKernelGGL(fir_long_kernel, dim3(lg.gx, lg.gy), dim3(512), kLongLdsBytes, s, p, (const v4i *)d_frag, a);
  return hipGetLastError();
}

}  // namespace acdsp
