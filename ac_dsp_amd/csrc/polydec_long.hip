// polydec_long.hip -- long polyphase decimators (ac_poly_dec, NTAPS * DF up to 16384, DF up to 256) on the gfx950 matrix cores, exact
// integer arithmetic.  Takes the exact-sum shapes the ring kernel of fir_gen.hip cannot plan (DF > 64, or a window of more than 8 K-blocks).
//
// Formulation.  With c[tp + NTAPS d] the reference's coefficient array (ac_poly_dec.h:119-121) and the phase streams
//   z_d[m] = x[m DF + DF-1 - d],  d = 0 .. DF-1   (m < 0 reaches into the history)
// the output is  y[g] = sum_d sum_tp c[tp + NTAPS d] z_d[g - tp]:  DF plain FIRs of NTAPS taps on the DF phase streams, summed in one
// accumulator.  Each of them is the Toeplitz product of fir_long.hip (header comment there and in fir_mfma_kernels.hpp): nb = max(2,
// ceil((NTAPS-1)/32) + 1) K-blocks per phase, H = 32 (nb - 1) samples of reach, both operands split into two signed bytes, four int32 plane
// sums recombined in 64 bits.  At most 16384 real taps contribute 2^14 each to a plane sum (the padding of a phase to nb K-blocks is zero
// coefficients): the bound of fir_long.hip, so the accumulators stay live across ALL phases and the recombination, the wrap to ACC_TYPE and
// the conversion to OUT_TYPE run once per output.  The reference's per-phase accumulators acc1[d] are ACC_TYPE sums of exact products: with
// a wrapping accumulator (or a saturating one no partial sum can reach -- decided by the host) their sum mod 2^W is this sum.
//
// Two kernels per time slab of a channel group:
//   1. polydec_phase_split_kernel writes the phase streams into the handle's scratch, int16 [group channel][d][L], L = H + G_slab; element
//      j of a row is z_d[g0 - H + j] with g0 the slab's first output.  The [m][d] -> [d][m] transpose goes through LDS (odd row pitch), so
//      both the reads of the caller's rows and the writes of the phase rows are coalesced.  It writes every element the second kernel
//      multiplies: H + 1024 * ceil(slab outputs / 1024) per row, zeros behind the end of the call and in front of the history.
//   2. fir_long_dec_kernel is fir_long_kernel with another iteration space: (step of 1024 outputs, phase d, segment gs of <= 16 K-blocks of
//      that phase), nsteps * DF * ceil(nb / 16) iterations with one __syncthreads() each.  Same workgroup (eight waves = eight channels),
//      same LDS plan (two 32 KB A segments + eight private double-buffered 47-chunk windows, 116 KB), same generic 64-bit epilogue.  A
//      segment never straddles phases, so a window is 47 chunks of ONE phase row: the B operand of (d, K-block b, column n) is
//      z_d[G0 - H + 32 (n + b) + 0..31], a contiguous read.  The accumulators are cleared at (d, gs) = (0, 0); the epilogue runs behind the
//      last (d, gs) of a step.  Every high-plane product is issued (no high-byte range).
//      At nb = 2 (NTAPS <= 33) an iteration is 8 MFMAs per barrier; two phases per segment would halve the barriers (not built).
//
// Barrier uniformity, as in fir_long.hip: the loop that contains the barrier runs nsteps * DF * NSEG times; DF and NSEG are launch
// arguments, nsteps follows from launch arguments and blockIdx.  A wave's channel is clamped to the group's last one, never exited.
#include <cstdlib>
#include <numeric>
#include <vector>

#include "fir_long_kernels.hpp"

namespace acdsp {

// ---------------------------------------------------------------------------------------------
// kernel 1: phase split
// ---------------------------------------------------------------------------------------------
constexpr int kSplitThreads = 256;
constexpr int kSplitTileElems = 16384;             // samples of one tile: J groups x DF, J = 64 .. 1024 (a power of two)
constexpr int kSplitLdsElems = kSplitTileElems + 1024;   // ... at a row pitch of DF | 1

struct SplitArgs {
  const int16_t *x, *hist;   // the caller's rows and the handle's history [n_ch][hl]
  int16_t *z;                // scratch [n_grp][df][L]
  int64_t in_stride, n_in;
  int64_t L, Lw;             // row length; elements written per row (a multiple of 32)
  int64_t m0;                // phase-stream index of element 0 of a row: g0 - H
  int32_t hl, df, ch0, J;    // J: groups per tile
};

__global__ void __launch_bounds__(kSplitThreads)
polydec_phase_split_kernel(SplitArgs a) {
  __shared__ int16_t tile[kSplitLdsElems];
  const int DF = a.df, P = DF | 1;   // odd pitch: the column reads below fall on distinct banks
  const int chl = blockIdx.y, ch = a.ch0 + chl;
  const int64_t j0 = (int64_t)blockIdx.x * a.J;
  const int jn = (int)((a.Lw - j0 < a.J) ? a.Lw - j0 : a.J);   // even (Lw and J are multiples of 32)
  const int16_t *xrow = a.x + (int64_t)ch * a.in_stride;
  const int16_t *hrow = a.hist + (int64_t)ch * a.hl + a.hl;
  // input samples t = tb + i, i = jj DF + r: consecutive threads read consecutive samples
  const int64_t tb = (a.m0 + j0) * DF;
  const int total = jn * DF;
  const int qs = kSplitThreads / DF, rs = kSplitThreads % DF;
  int jj = threadIdx.x / DF, r = threadIdx.x % DF;
  for (int i = threadIdx.x; i < total; i += kSplitThreads) {
    const int64_t t = tb + i;
    int16_t v = 0;
    if (t >= 0) { if (t < a.n_in) { v = xrow[t]; } }
    else if (t >= -(int64_t)a.hl) { v = hrow[t]; }
    tile[jj * P + r] = v;
    jj += qs; r += rs;
    if (r >= DF) { r -= DF; jj++; }
  }
  __syncthreads();
  // phase rows: element pairs (2 pj, 2 pj + 1) of row d, consecutive threads write consecutive dwords of one row
  const int hp = jn >> 1, totp = hp * DF;
  const int qd = kSplitThreads / hp, rd = kSplitThreads % hp;
  int d = threadIdx.x / hp, pj = threadIdx.x % hp;
  int16_t *zc = a.z + (int64_t)chl * DF * a.L + j0;
  for (int o = threadIdx.x; o < totp; o += kSplitThreads) {
    const int c = DF - 1 - d;
    const uint32_t lo = (uint16_t)tile[(2 * pj) * P + c], hi = (uint16_t)tile[(2 * pj + 1) * P + c];
    *(uint32_t *)(zc + (int64_t)d * a.L + 2 * pj) = lo | (hi << 16);
    d += qd; pj += rd;
    if (pj >= hp) { pj -= hp; d++; }
  }
}

// ---------------------------------------------------------------------------------------------
// kernel 2: the Toeplitz products over (step, phase, segment)
// ---------------------------------------------------------------------------------------------
struct LongDecArgs {
  int64_t steps_per_wave;   // 1024-output steps per workgroup row
  int64_t n_steps;          // ceil(slab outputs / 1024)
  int64_t L;                // elements of a phase row
  int64_t g0, g_end;        // the slab's outputs [g0, g_end) of the call
  int32_t nb, df;           // K-blocks per phase, phases
  int32_t ch0, n_grp;       // the group's first channel and channel count
  uint32_t hi_xor;          // unsigned 16-bit samples: 0x80808080 flips the top bit of every high byte (fir_mfma_kernels.hpp, MfmaArgs::hi_xor)
  const int64_t *corr;      // [1] 128 * sum(c) (+ 32768 * sum(c) with hi_xor)
  const int16_t *z;         // phase streams [n_grp][df][L]
};

__global__ void __launch_bounds__(512, 1)
fir_long_dec_kernel(FirParams p, const v4i *__restrict__ frag, LongDecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb, NSEG = (NB + kLongSB - 1) / kLongSB, DF = a.df;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int chl = blockIdx.y * 8 + wave;
  if (chl >= a.n_grp) { chl = a.n_grp - 1; }   // (the wave still runs every iteration and barrier; its stores repeat the last channel's)
  const int ch = a.ch0 + chl;
  // LDS: [2 A segments: 2 planes x 16 blocks x 1 KB][per wave: 2 staged windows of 4 arrays]
  v4i *ldsA = (v4i *)lds_all;
  unsigned char *ldsX = lds_all + (size_t)2 * kLongAWords * 16 + (size_t)wave * 2 * kLongXBytes;

  const int16_t *zch = a.z + (int64_t)chl * DF * a.L;
  // loop bounds: launch arguments and blockIdx only (see "Barrier uniformity" above)
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);
  const int total = nsteps * DF * NSEG;
  const size_t plane_words = (size_t)DF * NB * 64;

  v4i RA[kLongAPerThread], RX[kLongJN];
  // global loads of iteration (step s, phase d, segment g): this thread's share of the A segment, this lane's share of the wave's window
  auto issue_loads = [&](int s, int d, int g) {
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) {
      const int idx = threadIdx.x + 512 * q, pl = idx / (kLongSB * 64), bl = (idx >> 6) % kLongSB, ln = idx & 63;
      int bg = g * kLongSB + bl;
      if (bg >= NB) { bg = NB - 1; }   // blocks past the phase in its last segment: never multiplied, any in-bounds fragment will do
      RA[q] = frag[(size_t)pl * plane_words + ((size_t)d * NB + bg) * 64 + ln];
    }
    // the window of segment g starts 32 * 16 g elements behind the step's first one; the chunks a product reads end at H + 1024 (s0 + s + 1)
    // <= L, the others are clamped to the row's start.  e and L are multiples of 8: a load never straddles the end of the row
    const int16_t *zrow = zch + (int64_t)d * a.L;
    const int64_t base = (s0 + s) * 1024 + 32 * kLongSB * (int64_t)g;
#pragma unroll
    for (int j = 0; j < kLongJN; j++) {
      const int pc = (lane + 64 * j < kLongNP) ? lane + 64 * j : kLongNP - 1;
      const int64_t e = base + 8 * pc;
      RX[j] = *(const v4i *)(zrow + ((e < a.L) ? e : 0));
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
  if (total > 0) { issue_loads(0, 0, 0); }
  int s = 0, d = 0, g = 0;
  for (int it = 0; it < total; it++) {
    const int buf = it & 1;
    // buffer `buf` was last read in iteration it - 2; every wave has passed the barrier of it - 1 since
    commit(buf);
    int sn = s, dn = d, gn = g + 1;
    if (gn == NSEG) { gn = 0; dn++; }
    if (dn == DF) { dn = 0; sn++; }
    if (it + 1 < total) { issue_loads(sn, dn, gn); }   // in flight behind this segment's products
    __syncthreads();

    if (d == 0 && g == 0) { hh = (v16i){0}; mid = (v16i){0}; ll = (v16i){0}; }
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
      hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Bhc, hh, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Blc, mid, 0, 0, 0);
      ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Blc, ll, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Bhc, mid, 0, 0, 0);
      Ahc = Ahn; Alc = Aln; Bhc = Bhn; Blc = Bln;
    }

    if (d == DF - 1 && g == NSEG - 1) {
      // V = 2^16 hh + 2^8 mid + ll + corr, exact in 64 bits; then the reference's two conversions (`acc += ...`, `data_out = acc`)
      const int64_t G0 = a.g0 + (s0 + s) * 1024;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t t0 = G0 + 32 * n_col + 8 * q + 4 * h;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int64_t v = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r] + corr;
          const int64_t acc = wrap64((int64_t)((uint64_t)v << p.lossless_shift), p.acc.W, p.acc.S);
          const int64_t y = requant64(acc, p.acc.F, p.out);
          if (t0 + rr < a.g_end) { store_raw(p.y, (int64_t)ch * p.out_stride + t0 + rr, p.out_eb, y); }
        }
      }
    }
    s = sn; d = dn; g = gn;
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
bool polydec_long_plan(const int64_t *c, int ntaps, int df, PolyDecLongPlan *plan, std::vector<uint32_t> *frag) {
  if (ntaps < 1 || df < 1 || df > kPolyDecLongMaxDf || (int64_t)ntaps * df > kPolyDecLongMaxTaps) { return false; }
  std::vector<int64_t> corr;
  if (!long_phase_fragments(c, df, ntaps, frag, &corr)) { return false; }
  plan->ntaps = ntaps; plan->df = df; plan->nb = long_blocks(ntaps);
  plan->corr = std::accumulate(corr.begin(), corr.end(), (int64_t)0);   // one accumulator over all phases: one constant
  return true;
}

hipError_t launch_polydec_long(const FirParams &p, const PolyDecLongPlan &plan, const LongGeom &geo, const uint32_t *d_frag,
                               const int64_t *d_corr, void *d_scratch, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) { return hipSuccess; }
  if (p.in_eb != 2 || plan.nb < 2 || geo.slab < 1024 || geo.slab % 1024 || geo.group < 1 || !d_scratch) { return hipErrorInvalidValue; }
  const int64_t H = 32 * (int64_t)(plan.nb - 1), L = H + geo.slab;
  hipError_t e = hipFuncSetAttribute((const void *)fir_long_dec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLongLdsBytes);
  if (e != hipSuccess) { return e; }
  int J = 1024;
  while (J > 64 && J * plan.df > kSplitTileElems) { J >>= 1; }
  for (int ch0 = 0; ch0 < p.n_ch; ch0 += geo.group) {
    const int n_grp = (p.n_ch - ch0 < geo.group) ? p.n_ch - ch0 : geo.group;
    for (int64_t g0 = 0; g0 < n_out; g0 += geo.slab) {
      const int64_t n_slab = (n_out - g0 < geo.slab) ? n_out - g0 : geo.slab;
      const int64_t n_steps = (n_slab + 1023) / 1024;
      SplitArgs sa;
      sa.x = (const int16_t *)p.x; sa.hist = (const int16_t *)p.hist; sa.z = (int16_t *)d_scratch;
      sa.in_stride = p.in_stride; sa.n_in = p.n;
      sa.L = L; sa.Lw = H + 1024 * n_steps; sa.m0 = g0 - H;
      sa.hl = p.hl; sa.df = plan.df; sa.ch0 = ch0; sa.J = J;
      hipLaunchKernelGGL(polydec_phase_split_kernel, dim3((unsigned)((sa.Lw + J - 1) / J), (unsigned)n_grp), dim3(kSplitThreads), 0, s, sa);
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
      LongDecArgs a;
      a.n_steps = n_steps; a.L = L; a.g0 = g0; a.g_end = g0 + n_slab;
      a.nb = plan.nb; a.df = plan.df; a.ch0 = ch0; a.n_grp = n_grp;
      a.hi_xor = p.in_flip ? 0x80808080u : 0u;
      a.corr = d_corr; a.z = (const int16_t *)d_scratch;
      const LongGrid lg = long_grid(n_steps, n_grp, 1);
      a.steps_per_wave = lg.steps_per_wave;
      hipLaunchKernelGGL(fir_long_dec_kernel, dim3(lg.gx, lg.gy), dim3(512), kLongLdsBytes, s, p, (const v4i *)d_frag, a);
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
    }
  }
  return hipSuccess;
}

}  // namespace acdsp
