// polyintr_long.hip -- long polyphase interpolators (ac_poly_intr, 65 .. 16384 taps per phase, IF up to 255) on the gfx950 matrix cores,
// exact integer arithmetic.  Takes the exact-sum shapes on 16-bit types fir_up.hip cannot plan (more than two K-blocks per phase).
//
// Formulation.  The host folds the three cores, the one-sample lag of the folded cores and the symmetric-pair combination into IF linear
// filters of the SAME input stream (polyintr_linear_taps, engine_poly.hip):
//   group(n)[j] = sum_k E_j[k] x[n - k],  k = 0 .. nt - 1,  nt = NTAPS + lag,
// halved (arithmetic >> 1) for the phases of a pair.  Each E_j is a plain FIR: the Toeplitz product of fir_long.hip (header comment there
// and in fir_mfma_kernels.hpp) with nb = max(2, ceil((nt-1)/32) + 1) K-blocks, both operands split into two signed bytes, four int32 plane
// sums recombined in 64 bits.  At most 16384 taps contribute 2^14 each to a plane sum: the bound of fir_long.hip.
//
// Two kernels per time slab of a channel group:
//   1. fir_long_intr_kernel is fir_long_kernel with another iteration space: (step of 1024 input samples, phase j, segment gs of <= 16
//      K-blocks of that phase), nsteps * IF * ceil(nb / 16) iterations with one __syncthreads() each.  Same workgroup (eight waves = eight
//      channels), same LDS plan (two 32 KB A segments + eight private double-buffered 47-chunk windows, 116 KB), same generic 64-bit
//      epilogue.  The B operand is the caller's row plus the handle's history, the same window for every phase of a step (re-read per
//      phase: left to the L2, as fir_long.hip leaves the re-read per segment).  A row may start at any element-aligned address and have any
//      stride: a 16-byte load that would pass the row's last sample is assembled from guarded element loads, samples behind the call and in
//      front of the history read as 0.  The accumulators are cleared at (j, gs = 0); the epilogue runs behind the last segment of (step, j)
//      and stores phase j of the step into the handle's scratch, OUT containers [group channel][j][slab sample].  Every high-plane product
//      is issued (no high-byte range).
//   2. polyintr_phase_merge_kernel interleaves the IF phase rows into the caller's rows, y[ch][(n - skip) IF + j].  The [j][n] -> [n][j]
//      transpose goes through LDS (odd row pitch), so both the reads of the phase rows and the writes of the output rows are coalesced; 2-byte
//      containers leave as aligned dwords.  It writes the outputs [o_lo, n_out) of the call only: the group of the call's sample 0 on the
//      folded cores belongs to the exact kernel (it carries the sums saved by the previous call) or does not exist (the stream's first sample).
//
// Barrier uniformity, as in fir_long.hip: the loop that contains the barrier runs nsteps * IF * NSEG times; IF and NSEG are launch
// arguments, nsteps follows from launch arguments and blockIdx.  A wave's channel is clamped to the group's last one, never exited.
#include <cstdlib>
#include <vector>

#include "fir_long_kernels.hpp"

namespace acdsp {

// ---------------------------------------------------------------------------------------------
// kernel 1: the Toeplitz products over (step, phase, segment)
// ---------------------------------------------------------------------------------------------
struct LongIntrArgs {
  int64_t steps_per_wave;   // 1024-sample steps per workgroup row
  int64_t n_steps;          // ceil(slab samples / 1024)
  int64_t n0, n_end;        // the slab's input samples [n0, n_end) of the call (n0 a multiple of 1024)
  int64_t G;                // elements of a scratch row (the geometry's slab)
  int32_t nb, ifac;         // K-blocks per phase, phases
  int32_t ch0, n_grp;       // the group's first channel and channel count
  const int64_t *corr;      // [ifac] 128 * sum(E_j)
  const uint8_t *halve;     // [ifac] 1: the phase is half of a symmetric pair, its sum leaves >> 1
  void *z;                  // scratch [n_grp][ifac][G], OUT containers
};

__global__ void __launch_bounds__(512, 1)
fir_long_intr_kernel(FirParams p, const v4i *__restrict__ frag, LongIntrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb, NSEG = (NB + kLongSB - 1) / kLongSB, IF = a.ifac;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int chl = blockIdx.y * 8 + wave;
  if (chl >= a.n_grp) { chl = a.n_grp - 1; }   // (the wave still runs every iteration and barrier; its stores repeat the last channel's)
  const int ch = a.ch0 + chl;
  // LDS: [2 A segments: 2 planes x 16 blocks x 1 KB][per wave: 2 staged windows of 4 arrays]
  v4i *ldsA = (v4i *)lds_all;
  unsigned char *ldsX = lds_all + (size_t)2 * kLongAWords * 16 + (size_t)wave * 2 * kLongXBytes;

  const int16_t *xrow = (const int16_t *)p.x + (int64_t)ch * p.in_stride;
  const int16_t *hrow = (const int16_t *)p.hist + (int64_t)ch * p.hl + p.hl;
  // loop bounds: launch arguments and blockIdx only (see "Barrier uniformity" above)
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);
  const int total = nsteps * IF * NSEG;
  const size_t plane_words = (size_t)IF * NB * 64;

  v4i RA[kLongAPerThread], RX[kLongJN];
  // global loads of iteration (step s, phase j, segment g): this thread's share of the A segment, this lane's share of the wave's window
  auto issue_loads = [&](int s, int j, int g) {
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) {
      const int idx = threadIdx.x + 512 * q, pl = idx / (kLongSB * 64), bl = (idx >> 6) % kLongSB, ln = idx & 63;
      int bg = g * kLongSB + bl;
      if (bg >= NB) { bg = NB - 1; }   // blocks past the phase in its last segment: never multiplied, any in-bounds fragment will do
      RA[q] = frag[(size_t)pl * plane_words + ((size_t)j * NB + bg) * 64 + ln];
    }
    // t is a multiple of 8 and so is hl: a load never straddles history and row, nor the history's first sample
    const int64_t base = a.n0 + (s0 + s) * 1024 - 32 * (int64_t)(NB - 1) + 32 * kLongSB * (int64_t)g;
#pragma unroll
    for (int jx = 0; jx < kLongJN; jx++) {
      const int pc = (lane + 64 * jx < kLongNP) ? lane + 64 * jx : kLongNP - 1;
      const int64_t t = base + 8 * pc;
      v4i v = {0, 0, 0, 0};
      if (t < 0) {
        if (t >= -(int64_t)p.hl) { v = *(const v4i *)(hrow + t); }
      } else if (t + 8 <= p.n) {
        v = *(const v4i *)(xrow + t);
      } else if (t < p.n) {   // the row's last samples: nothing behind sample n - 1 is read
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        const int m = (int)(p.n - t);   // 1 .. 7
        const uint16_t *xs = (const uint16_t *)xrow + t;
        w0 = xs[0];
        if (m > 1) { w0 |= (unsigned)xs[1] << 16; }
        if (m > 2) { w1 = xs[2]; }
        if (m > 3) { w1 |= (unsigned)xs[3] << 16; }
        if (m > 4) { w2 = xs[4]; }
        if (m > 5) { w2 |= (unsigned)xs[5] << 16; }
        if (m > 6) { w3 = xs[6]; }
        v = (v4i){(int)w0, (int)w1, (int)w2, (int)w3};
      }
      RX[jx] = v;
    }
  };
  // registers -> LDS: the A segment (all waves, read after the barrier) and the wave's byte planes
  auto commit = [&](int buf) {
    v4i *dstA = ldsA + buf * kLongAWords;
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) { dstA[threadIdx.x + 512 * q] = RA[q]; }
    unsigned char *xb = ldsX + buf * kLongXBytes;
#pragma unroll
    for (int jx = 0; jx < kLongJN; jx++) {
      const int pc = lane + 64 * jx;
      if (pc < kLongNP) {
        const int c = pc >> 2, hh_ = (pc >> 1) & 1, sub = pc & 1;
        const unsigned hi0 = __builtin_amdgcn_perm((unsigned)RX[jx].y, (unsigned)RX[jx].x, 0x07050301u);
        const unsigned hi1 = __builtin_amdgcn_perm((unsigned)RX[jx].w, (unsigned)RX[jx].z, 0x07050301u);
        const unsigned lo0 = __builtin_amdgcn_perm((unsigned)RX[jx].y, (unsigned)RX[jx].x, 0x06040200u) ^ 0x80808080u;
        const unsigned lo1 = __builtin_amdgcn_perm((unsigned)RX[jx].w, (unsigned)RX[jx].z, 0x06040200u) ^ 0x80808080u;
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        *(v2u *)(xb + (0 * 2 + hh_) * kLongARR + c * 16 + sub * 8) = (v2u){hi0, hi1};
        *(v2u *)(xb + (1 * 2 + hh_) * kLongARR + c * 16 + sub * 8) = (v2u){lo0, lo1};
      }
    }
  };

  v16i hh = {0}, mid = {0}, ll = {0};
  if (total > 0) { issue_loads(0, 0, 0); }
  int s = 0, j = 0, g = 0;
  for (int it = 0; it < total; it++) {
    const int buf = it & 1;
    // buffer `buf` was last read in iteration it - 2; every wave has passed the barrier of it - 1 since
    commit(buf);
    int sn = s, jn = j, gn = g + 1;
    if (gn == NSEG) { gn = 0; jn++; }
    if (jn == IF) { jn = 0; sn++; }
    if (it + 1 < total) { issue_loads(sn, jn, gn); }   // in flight behind this segment's products
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
      hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Bhc, hh, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Blc, mid, 0, 0, 0);
      ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Blc, ll, 0, 0, 0);
      mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Bhc, mid, 0, 0, 0);
      Ahc = Ahn; Alc = Aln; Bhc = Bhn; Blc = Bln;
    }

    if (g == NSEG - 1) {
      // V = 2^16 hh + 2^8 mid + ll + corr_j, exact in 64 bits; the pair halving (the host's bound: nothing wraps in front of it), then the
      // reference's conversions to ACC_TYPE and OUT_TYPE
      const int64_t corr = a.corr[j];
      const int hv = a.halve[j];
      const int64_t N0 = (s0 + s) * 1024;   // slab sample of the step's first output
      const int64_t zrow = ((int64_t)chl * IF + j) * a.G;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t t0 = N0 + 32 * n_col + 8 * q + 4 * h;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int64_t v = ((int64_t)hh[r] << 16) + ((int64_t)mid[r] << 8) + (int64_t)ll[r] + corr;
          const int64_t sh = (int64_t)((uint64_t)v << p.lossless_shift) >> hv;
          const int64_t acc = wrap64(sh, p.acc.W, p.acc.S);
          const int64_t y = requant64(acc, p.acc.F, p.out);
          if (a.n0 + t0 + rr < a.n_end) { store_raw(a.z, zrow + t0 + rr, p.out_eb, y); }
        }
      }
    }
    s = sn; j = jn; g = gn;
  }
}

// ---------------------------------------------------------------------------------------------
// kernel 2: phase merge
// ---------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 256;
constexpr int kMergeLdsBytes = 40 * 1024;   // J samples x (IF | 1) containers, J = 16 .. 1024 (a power of two): at most 20480 elements

struct MergeArgs {
  const void *z;             // scratch [n_grp][ifac][G]
  void *y;                   // the caller's rows
  int64_t out_stride, G;
  int64_t n0, n_cnt;         // the slab's first input sample and its sample count
  int64_t o_lo, n_out;       // outputs [o_lo, n_out) of the call are written
  int32_t ifac, skip, ch0, J;
  uint32_t rcp;              // ceil(2^32 / ifac): i / ifac = umulhi(i, rcp) for i < 2^16 (ifac > 1)
};

template <typename T>
__global__ void __launch_bounds__(kMergeThreads)
polyintr_phase_merge_kernel(MergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];
  T *tile = (T *)merge_lds;
  const int IF = a.ifac, P = IF | 1;   // odd pitch: the column writes below fall on distinct banks
  const int chl = blockIdx.y, ch = a.ch0 + chl;
  const int64_t jl0 = (int64_t)blockIdx.x * a.J;
  const int jn = (int)((a.n_cnt - jl0 < a.J) ? a.n_cnt - jl0 : a.J);
  const int total = jn * IF;
  // phase rows: consecutive threads read consecutive samples of one row
  const T *zc = (const T *)a.z + (int64_t)chl * IF * a.G + jl0;
  {
    const int qs = kMergeThreads / jn, rs = kMergeThreads % jn;
    int j = threadIdx.x / jn, jj = threadIdx.x % jn;
    for (int i = threadIdx.x; i < total; i += kMergeThreads) {
      tile[jj * P + j] = zc[(int64_t)j * a.G + jj];
      j += qs; jj += rs;
      if (jj >= jn) { jj -= jn; j++; }
    }
  }
  __syncthreads();
  // output element i of the tile = (sample i / IF, phase i % IF): consecutive threads write consecutive words of the caller's row
  const int64_t o0 = (a.n0 + jl0 - a.skip) * IF;   // output index of element 0 (negative for the stream's first sample)
  T *yrow = (T *)a.y + (int64_t)ch * a.out_stride;
  auto elem = [&](int i) -> T {
    const unsigned dg = IF == 1 ? (unsigned)i : __umulhi((unsigned)i, a.rcp);
    return tile[dg * P + (i - (int)dg * IF)];
  };
  auto live = [&](int i) -> bool { return i >= 0 && i < total && o0 + i >= a.o_lo && o0 + i < a.n_out; };
  if (sizeof(T) == 2) {
    // dwords on the 4-byte grid of the row: pair p holds the elements 2 p - par and 2 p - par + 1
    const int par = (int)(((uintptr_t)(yrow + o0) >> 1) & 1);
    for (int pi = threadIdx.x; 2 * pi - par < total; pi += kMergeThreads) {
      const int i = 2 * pi - par;
      const bool l0 = live(i), l1 = live(i + 1);
      if (l0 && l1) {
        const uint32_t lo = (uint16_t)elem(i), hi = (uint16_t)elem(i + 1);
        *(uint32_t *)(yrow + o0 + i) = lo | (hi << 16);
      } else if (l0) {
        yrow[o0 + i] = elem(i);
      } else if (l1) {
        yrow[o0 + i + 1] = elem(i + 1);
      }
    }
  } else {
    for (int i = threadIdx.x; i < total; i += kMergeThreads) {
      if (live(i)) { yrow[o0 + i] = elem(i); }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
bool polyintr_long_plan(const int64_t *E, int ifac, int nt, const uint8_t *halve, PolyIntrLongPlan *plan, std::vector<uint32_t> *frag,
                        std::vector<int64_t> *corr, std::vector<uint8_t> *flags) {
  if (nt < 1 || nt > kPolyIntrLongMaxTaps || ifac < 1 || ifac > 255) { return false; }
  const int nb = long_blocks(nt);
  if ((int64_t)ifac * nb > kPolyIntrLongMaxBlocks) { return false; }
  flags->assign(halve, halve + ifac);
  if (!long_phase_fragments(E, ifac, nt, frag, corr)) { return false; }   // accumulators per phase: every phase keeps its constant
  plan->nt = nt; plan->ifac = ifac; plan->nb = nb;
  return true;
}

hipError_t launch_polyintr_long(const FirParams &p, const PolyIntrLongPlan &plan, const LongGeom &geo, const uint32_t *d_frag,
                                const int64_t *d_corr, const uint8_t *d_halve, void *d_scratch, int skip, int64_t o_lo, int64_t n_out,
                                hipStream_t s) {
  if (p.n <= 0 || n_out <= o_lo) { return hipSuccess; }
  if (p.in_eb != 2 || plan.nb < 2 || 32 * (plan.nb - 1) > p.hl || p.hl % 8 || geo.slab < 1024 || geo.slab % 1024 || geo.group < 1 || geo.group > 65535 || !d_scratch ||
      (p.out_eb != 2 && p.out_eb != 4 && p.out_eb != 8)) {
    return hipErrorInvalidValue;
  }
  hipError_t e = hipFuncSetAttribute((const void *)fir_long_intr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLongLdsBytes);
  if (e != hipSuccess) { return e; }
  const int IF = plan.ifac, P = IF | 1;
  int J = 1024;
  while (J > 16 && (int64_t)J * P * p.out_eb > kMergeLdsBytes) { J >>= 1; }
  for (int ch0 = 0; ch0 < p.n_ch; ch0 += geo.group) {
    const int n_grp = (p.n_ch - ch0 < geo.group) ? p.n_ch - ch0 : geo.group;
    for (int64_t n0 = 0; n0 < p.n; n0 += geo.slab) {
      const int64_t n_slab = (p.n - n0 < geo.slab) ? p.n - n0 : geo.slab;
      if ((n0 + n_slab - skip) * IF <= o_lo) { continue; }   // (a slab that holds the call's sample 0 alone)
      LongIntrArgs a;
      a.n_steps = (n_slab + 1023) / 1024;
      a.n0 = n0; a.n_end = n0 + n_slab; a.G = geo.slab;
      a.nb = plan.nb; a.ifac = IF; a.ch0 = ch0; a.n_grp = n_grp;
      a.corr = d_corr; a.halve = d_halve; a.z = d_scratch;
      // no floor of 8 steps as in launch_fir_long: a step is IF * NSEG iterations here, not NSEG, and a slab may hold one step only
      // (launch_polydec_long has none either)
      const LongGrid lg = long_grid(a.n_steps, n_grp, 1);
      a.steps_per_wave = lg.steps_per_wave;
      hipLaunchKernelGGL(fir_long_intr_kernel, dim3(lg.gx, lg.gy), dim3(512), kLongLdsBytes, s, p, (const v4i *)d_frag, a);
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
      MergeArgs m;
      m.z = d_scratch; m.y = p.y; m.out_stride = p.out_stride; m.G = geo.slab;
      m.n0 = n0; m.n_cnt = n_slab; m.o_lo = o_lo; m.n_out = n_out;
      m.ifac = IF; m.skip = skip; m.ch0 = ch0; m.J = J;
      m.rcp = (uint32_t)((0x100000000ull + IF - 1) / IF);
      const dim3 mgrid((unsigned)((n_slab + J - 1) / J), (unsigned)n_grp);
      const size_t lds = (size_t)J * P * p.out_eb;
      if (p.out_eb == 2) { hipLaunchKernelGGL(polyintr_phase_merge_kernel<uint16_t>, mgrid, dim3(kMergeThreads), lds, s, m); }
      else if (p.out_eb == 4) { hipLaunchKernelGGL(polyintr_phase_merge_kernel<uint32_t>, mgrid, dim3(kMergeThreads), lds, s, m); }
      else { hipLaunchKernelGGL(polyintr_phase_merge_kernel<uint64_t>, mgrid, dim3(kMergeThreads), lds, s, m); }
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
    }
  }
  return hipSuccess;
}

}  // namespace acdsp
