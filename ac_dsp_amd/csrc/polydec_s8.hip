// polydec_s8.hip -- long polyphase decimators (ac_poly_dec, NTAPS * DF up to 16384, DF up to 256) on 1-byte sample containers
// (ACDSP_FLAG_IN_BYTES: IN_TYPE of up to 8 bits) on the gfx950 matrix cores, exact integer arithmetic.  The byte sibling of polydec_long.hip:
// the same exact-sum shapes the ring kernel of fir_gen.hip cannot plan (DF > 64, or a window of more than 8 K-blocks), the same formulation
// (header comment there): DF plain FIRs of NTAPS taps on the phase streams z_d[m] = x[m DF + DF-1 - d], summed in one accumulator; the same
// coefficient fragments (two signed bytes per coefficient, long_phase_fragments), channel groups and time slabs.  What differs:
//   * ONE sample plane, as in fir_s8.hip.  A chunk is 32 bytes of a phase row as it lies in the scratch: no v_perm split, the window of a
//     segment sits in LDS in memory order (lane (column n, half h) reads the 16 bytes at 32 (n + b) + 16 h).  Signed samples are the B operand
//     as they are; unsigned ones are XOR-ed with 0x80 on the way into LDS (x - 128 as a signed byte) and 128 * sum(c) rides in the correction
//     constant.  A K-block costs two products where polydec_long.hip issues four.
//   * Two accumulator sets: V = (hi << 8) + lo + corr.  |plane sum| <= 16384 * 2^14 = 2^28 at 16384 real taps (the padding of a phase to nb
//     K-blocks is zero coefficients): the bound of fir_s8.hip, so the accumulators stay live across ALL phases.
//   * The phase streams are int8 rows: DF bytes of scratch per slab output, half of polydec_long.hip's.
//
// Two kernels per time slab of a channel group:
//   1. polydec_phase_split_s8_kernel writes the phase streams into the handle's scratch, int8 [group channel][d][L], L = H + G_slab, H =
//      32 (nb - 1); element j of a row is z_d[g0 - H + j] with g0 the slab's first output.  The [m][d] -> [d][m] transpose goes through LDS, so
//      both the reads of the caller's rows and the writes of the phase rows (one dword = four outputs per thread) are coalesced.  It writes
//      every element the second kernel multiplies: H + 1024 * ceil(slab outputs / 1024) per row, zeros behind the end of the call and in front
//      of the history (those meet zero coefficients or outputs that are not stored).
//   2. polydec_s8_kernel walks (step of 1024 outputs, phase d, segment gs of <= 16 K-blocks of that phase) like fir_long_dec_kernel: eight
//      waves = eight channels share one double-buffered 32 KB A segment, each wave stages its own 47-chunk window (1504 bytes, two 16-byte
//      loads per lane), one __syncthreads() per iteration.  LDS: 2 x 32 KB + 8 x 2 x 1.5 KB = 88 KB.
//
// Barrier uniformity, as in polydec_long.hip and fir_long.hip: every loop bound and every branch around __syncthreads() is made of launch
// arguments and blockIdx only -- the loop that contains the barrier runs nsteps * DF * NSEG times; DF and NSEG are launch arguments, nsteps
// follows from launch arguments and blockIdx.  A wave past the group's last channel is clamped to that channel, never exited: it runs every
// iteration and barrier, and its stores repeat the last channel's.
#include <cstdlib>
#include <vector>

#include "fir_long_kernels.hpp"

namespace acdsp {

// ---------------------------------------------------------------------------------------------
// kernel 1: phase split
// ---------------------------------------------------------------------------------------------
constexpr int kSplit8Threads = 256;
constexpr int kSplit8TileElems = 16384;             // samples of one tile: J groups x DF, J = 64 .. 1024 (a power of two)
constexpr int kSplit8LdsElems = kSplit8TileElems + 1024;   // ... at a row pitch of DF | 1

struct Split8Args {
  const int8_t *x, *hist;    // the caller's rows and the handle's history [n_ch][hl]
  int8_t *z;                 // scratch [n_grp][df][L]
  int64_t in_stride, n_in;
  int64_t L, Lw;             // row length; elements written per row (a multiple of 32)
  int64_t m0;                // phase-stream index of element 0 of a row: g0 - H
  int32_t hl, df, ch0, J;    // J: groups per tile
};

__global__ void __launch_bounds__(kSplit8Threads)
polydec_phase_split_s8_kernel(Split8Args a) {
  __shared__ int8_t tile[kSplit8LdsElems];
  const int DF = a.df, P = DF | 1;
  const int chl = blockIdx.y, ch = a.ch0 + chl;
  const int64_t j0 = (int64_t)blockIdx.x * a.J;
  const int jn = (int)((a.Lw - j0 < a.J) ? a.Lw - j0 : a.J);   // a multiple of 32 (Lw and J are)
  const int8_t *xrow = a.x + (int64_t)ch * a.in_stride;
  const int8_t *hrow = a.hist + (int64_t)ch * a.hl + a.hl;
  // input samples t = tb + i, i = jj DF + r: consecutive threads read consecutive samples
  const int64_t tb = (a.m0 + j0) * DF;
  const int total = jn * DF;
  const int qs = kSplit8Threads / DF, rs = kSplit8Threads % DF;
  int jj = threadIdx.x / DF, r = threadIdx.x % DF;
  for (int i = threadIdx.x; i < total; i += kSplit8Threads) {
    const int64_t t = tb + i;
    int8_t v = 0;
    if (t >= 0) { if (t < a.n_in) { v = xrow[t]; } }
    else if (t >= -(int64_t)a.hl) { v = hrow[t]; }
    tile[jj * P + r] = v;
    jj += qs; r += rs;
    if (r >= DF) { r -= DF; jj++; }
  }
  __syncthreads();
  // phase rows: elements 4 pj .. 4 pj + 3 of row d as one dword, consecutive threads write consecutive dwords of one row
  const int hp = jn >> 2, totp = hp * DF;
  const int qd = kSplit8Threads / hp, rd = kSplit8Threads % hp;
  int d = threadIdx.x / hp, pj = threadIdx.x % hp;
  int8_t *zc = a.z + (int64_t)chl * DF * a.L + j0;
  for (int o = threadIdx.x; o < totp; o += kSplit8Threads) {
    const int c = DF - 1 - d;
    const int8_t *tp = tile + (4 * pj) * P + c;
    const uint32_t w = (uint32_t)(uint8_t)tp[0] | ((uint32_t)(uint8_t)tp[P] << 8) | ((uint32_t)(uint8_t)tp[2 * P] << 16) | ((uint32_t)(uint8_t)tp[3 * P] << 24);
    *(uint32_t *)(zc + (int64_t)d * a.L + 4 * pj) = w;
    d += qd; pj += rd;
    if (pj >= hp) { pj -= hp; d++; }
  }
}

// ---------------------------------------------------------------------------------------------
// kernel 2: the Toeplitz products over (step, phase, segment), one sample plane
// ---------------------------------------------------------------------------------------------
constexpr int kDec8NP = 2 * kLongNC;                         // 16-byte loads of a segment's window: 47 chunks of 32 bytes
constexpr int kDec8JN = (kDec8NP + 63) / 64;                 // ... per lane
constexpr int kDec8XBytes = (kDec8NP * 16 + 63) / 64 * 64;   // one staged window of a wave
constexpr size_t kDec8LdsBytes = (size_t)2 * kLongAWords * 16 + (size_t)8 * 2 * kDec8XBytes;
static_assert(kDec8JN == 2, "two window loads per lane");
static_assert(kDec8XBytes >= 32 * kLongNC, "staged window holds the 47 chunks");
static_assert(kDec8LdsBytes <= 160 * 1024, "LDS of one gfx950 CU");

struct Dec8Args {
  int64_t steps_per_wave;   // 1024-output steps per workgroup row
  int64_t n_steps;          // ceil(slab outputs / 1024)
  int64_t L;                // elements (= bytes) of a phase row, a multiple of 32
  int64_t g0, g_end;        // the slab's outputs [g0, g_end) of the call
  int32_t nb, df;           // K-blocks per phase, phases
  int32_t ch0, n_grp;       // the group's first channel and channel count
  uint32_t x_xor;           // unsigned samples: 0x80808080 turns every byte into x - 128; else 0
  const int64_t *corr;      // [1] 128 * sum(c) for unsigned samples, else 0
  const int8_t *z;          // phase streams [n_grp][df][L]
};

__global__ void __launch_bounds__(512, 1)
polydec_s8_kernel(FirParams p, const v4i *__restrict__ frag, Dec8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb, NSEG = (NB + kLongSB - 1) / kLongSB, DF = a.df;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int chl = blockIdx.y * 8 + wave;
  if (chl >= a.n_grp) { chl = a.n_grp - 1; }   // (the wave still runs every iteration and barrier; its stores repeat the last channel's)
  const int ch = a.ch0 + chl;
  // LDS: [2 A segments: 2 planes x 16 blocks x 1 KB][per wave: 2 staged windows]
  v4i *ldsA = (v4i *)lds_all;
  unsigned char *ldsX = lds_all + (size_t)2 * kLongAWords * 16 + (size_t)wave * 2 * kDec8XBytes;

  const int8_t *zch = a.z + (int64_t)chl * DF * a.L;
  // loop bounds: launch arguments and blockIdx only (see "Barrier uniformity" above)
  const int64_t s0 = (int64_t)blockIdx.x * a.steps_per_wave;
  const int64_t s1 = (s0 + a.steps_per_wave < a.n_steps) ? s0 + a.steps_per_wave : a.n_steps;
  const int nsteps = (int)(s1 - s0);
  const int total = nsteps * DF * NSEG;
  const size_t plane_words = (size_t)DF * NB * 64;

  v4i RA[kLongAPerThread], RX[kDec8JN];
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
    // <= L, the others are clamped to the row's start.  e and L are multiples of 16: a load never straddles the end of the row
    const int8_t *zrow = zch + (int64_t)d * a.L;
    const int64_t base = (s0 + s) * 1024 + 32 * kLongSB * (int64_t)g;
#pragma unroll
    for (int j = 0; j < kDec8JN; j++) {
      const int pc = (lane + 64 * j < kDec8NP) ? lane + 64 * j : kDec8NP - 1;
      const int64_t e = base + 16 * pc;
      RX[j] = *(const v4i *)(zrow + ((e < a.L) ? e : 0));
    }
  };
  // registers -> LDS: the A segment (all waves, read after the barrier) and the wave's window, in memory order
  auto commit = [&](int buf) {
    v4i *dstA = ldsA + buf * kLongAWords;
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) { dstA[threadIdx.x + 512 * q] = RA[q]; }
    unsigned char *xb = ldsX + buf * kDec8XBytes;
#pragma unroll
    for (int j = 0; j < kDec8JN; j++) {
      const int pc = lane + 64 * j;
      if (pc < kDec8NP) {
        v4i v = RX[j];
        v.x ^= (int)a.x_xor; v.y ^= (int)a.x_xor; v.z ^= (int)a.x_xor; v.w ^= (int)a.x_xor;
        *(v4i *)(xb + 16 * pc) = v;
      }
    }
  };

  const int64_t corr = a.corr[0];
  v16i hi = {0}, lo = {0};
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

    if (d == 0 && g == 0) { hi = (v16i){0}; lo = (v16i){0}; }
    const int b0 = g * kLongSB, nbs = (NB - b0 < kLongSB) ? NB - b0 : kLongSB;
    const v4i *ah = ldsA + buf * kLongAWords + lane, *al = ah + kLongSB * 64;
    const unsigned char *fx = ldsX + buf * kDec8XBytes + 32 * n_col + 16 * h;   // chunk n_col + bl <= 46
    v4i Ahc = ah[0], Alc = al[0], Bc = *(const v4i *)fx;
    for (int bl = 0; bl < nbs; bl++) {
      v4i Ahn = Ahc, Aln = Alc, Bn = Bc;
      if (bl + 1 < nbs) {   // fragments of the next K-block are in flight while this one multiplies
        Ahn = ah[(bl + 1) * 64]; Aln = al[(bl + 1) * 64];
        Bn = *(const v4i *)(fx + 32 * (bl + 1));
      }
      hi = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, Bc, hi, 0, 0, 0);
      lo = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, Bc, lo, 0, 0, 0);
      Ahc = Ahn; Alc = Aln; Bc = Bn;
    }

    if (d == DF - 1 && g == NSEG - 1) {
      // V = 2^8 hi + lo + corr, exact in 64 bits; then the reference's two conversions (`acc += ...`, `data_out = acc`)
      const int64_t G0 = a.g0 + (s0 + s) * 1024;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t t0 = G0 + 32 * n_col + 8 * q + 4 * h;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int64_t v = ((int64_t)hi[r] << 8) + (int64_t)lo[r] + corr;
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
hipError_t launch_polydec_s8(const FirParams &p, const PolyDecLongPlan &plan, const LongGeom &geo, const uint32_t *d_frag,
                             const int64_t *d_corr, void *d_scratch, int64_t n_out, hipStream_t s) {
  if (n_out <= 0) { return hipSuccess; }
  if (p.in_eb != 1 || p.in.W > 8 || plan.nb < 2 || geo.slab < 1024 || geo.slab % 1024 || geo.group < 1 || !d_scratch) { return hipErrorInvalidValue; }
  const int64_t H = 32 * (int64_t)(plan.nb - 1), L = H + geo.slab;
  hipError_t e = hipFuncSetAttribute((const void *)polydec_s8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDec8LdsBytes);
  if (e != hipSuccess) { return e; }
  int J = 1024;
  while (J > 64 && J * plan.df > kSplit8TileElems) { J >>= 1; }
  for (int ch0 = 0; ch0 < p.n_ch; ch0 += geo.group) {
    const int n_grp = (p.n_ch - ch0 < geo.group) ? p.n_ch - ch0 : geo.group;
    for (int64_t g0 = 0; g0 < n_out; g0 += geo.slab) {
      const int64_t n_slab = (n_out - g0 < geo.slab) ? n_out - g0 : geo.slab;
      const int64_t n_steps = (n_slab + 1023) / 1024;
      Split8Args sa;
      sa.x = (const int8_t *)p.x; sa.hist = (const int8_t *)p.hist; sa.z = (int8_t *)d_scratch;
      sa.in_stride = p.in_stride; sa.n_in = p.n;
      sa.L = L; sa.Lw = H + 1024 * n_steps; sa.m0 = g0 - H;
      sa.hl = p.hl; sa.df = plan.df; sa.ch0 = ch0; sa.J = J;
      hipLaunchKernelGGL(polydec_phase_split_s8_kernel, dim3((unsigned)((sa.Lw + J - 1) / J), (unsigned)n_grp), dim3(kSplit8Threads), 0, s, sa);
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
      Dec8Args a;
      a.n_steps = n_steps; a.L = L; a.g0 = g0; a.g_end = g0 + n_slab;
      a.nb = plan.nb; a.df = plan.df; a.ch0 = ch0; a.n_grp = n_grp;
      a.x_xor = p.in_flip ? 0x80808080u : 0u;
      a.corr = d_corr; a.z = (const int8_t *)d_scratch;
      const LongGrid lg = long_grid(n_steps, n_grp, 1);
      a.steps_per_wave = lg.steps_per_wave;
      hipLaunchKernelGGL(polydec_s8_kernel, dim3(lg.gx, lg.gy), dim3(512), kDec8LdsBytes, s, p, (const v4i *)d_frag, a);
      if ((e = hipGetLastError()) != hipSuccess) { return e; }
    }
  }
  return hipSuccess;
}

}  // namespace acdsp
