// fir_s8.hip -- FIRs of 1 .. 16384 taps on 1-byte sample containers (ACDSP_FLAG_IN_BYTES: IN_TYPE of up to 8 bits) on the gfx950 matrix cores,
// exact integer arithmetic.
//
// The formulation is that of fir_long.hip (header comment there): a step is 1024 consecutive outputs of one channel, the 32 MFMA columns are
// 32 consecutive output blocks, K-block b of the [32 x 32 NB] Toeplitz matrix meets "input chunk n + b", the coefficients are split into two
// signed bytes (fragments of fir_mfma_build_fragments_nb, unchanged).  What differs:
//   * ONE sample plane.  A chunk is 32 bytes of the row as it lies in memory: no v_perm split, the window sits in LDS in memory order (lane
//     (column n, half h) reads the 16 bytes at 32 (n + b) + 16 h: the 64 lanes of a ds_read_b128 cover 1 KB back to back).  Signed samples
//     are the B operand as they are; unsigned ones are XOR-ed with 0x80 on the way into LDS (x - 128 as a signed byte) and 128 * sum(c) rides
//     in the correction constant.  A K-block costs one product, and one more inside the high-byte range [hb0, hb1] of the set.
//   * Two accumulator sets per step: V = (hi << 8) + lo + corr.  |plane sum| <= 32 NB 2^14 <= 2^28.01 at NB = 513.
//   * A wave works on a PAIR of steps, 2048 consecutive outputs, at a time: with half the products per K-block the A fragments a wave reads
//     from LDS would otherwise cost as much LDS time as their products cost matrix-pipe time (1 KB per product; a pair: 0.5 KB), and a segment
//     would hold half the matrix-pipe work of fir_long.hip's between two barriers.  The pair's window is one run of 64 + 15 chunks.
//   * Window loads are 16 bytes = 16 samples at a window base that is a multiple of 32 samples, so no load straddles history and row;
//     gfx950 serves vector loads at element-aligned addresses, so a byte row may start anywhere (readable up to the next multiple of 16).
//     They are issued TWO iterations ahead (two register sets, the loop unrolled by two): a wave has 5 KB of reads in flight.
//   * Segment walk as in fir_long.hip (kLongSB = 16 K-blocks per A segment, double-buffered, one __syncthreads() per segment), with one
//     more form: a set of up to kS8OneMax = 33 K-blocks (1025 taps) has its A fragments staged once per workgroup, in front of the step loop,
//     and the loop then runs without a barrier (each wave's window is its own; LDS serves one wave's accesses in order).  The LDS of a launch
//     is sized for its form.
//   * Epilogue: wrap64 / requant64 / store_raw as in fir_long_kernel, or -- where the host proves |V| < 2^30, no wrap of ACC_TYPE, AC_TRN /
//     AC_RND into a 2-byte AC_SAT / signed AC_WRAP output -- the same value from 32-bit arithmetic, stored 16 bytes per lane.  Under
//     ACDSP_FLAG_OUT_BYTES (OUT_TYPE of up to 8 bits in 1-byte containers) the 32-bit epilogue has a 1-byte form (OEB = 1: a step is 1 KB of
//     outputs, 16 bytes per lane in ONE store); the 64-bit one stores through store_raw, which has a 1-byte case.
//   * The K-blocks of a segment run as three loops (below, inside, above the high-byte range): no branch around an LDS read or a product.
//
// Barrier uniformity.  Every loop bound and every branch around a barrier is made of launch arguments and blockIdx only: NSEG (and with it
// the one-segment form), npairs = min(pairs_per_wave, n_pairs - blockIdx.x * pairs_per_wave).  Nothing a wave owns -- its channel (clamped to
// the last one past n_ch), the raggedness of its last pair, the high-byte range -- enters a loop bound or guards a barrier, and no thread
// leaves the kernel before the loop ends.
//
// Speed: profiles/s8_fir_shapes.txt (tools/s8_shapes.py).
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "fir_long_kernels.hpp"

namespace acdsp {

// K-blocks of the largest set whose A fragments stay resident in LDS (the one-segment form): 33 blocks = 1025 taps, 66 KB, beside 48 KB of
// windows.  (16, one segment of the long kernels, left 482 .. 1025 taps to the segmented form with a last segment of ONE block at 1023 taps.)
constexpr int kS8OneMax = 33;
constexpr int kS8NC = 64 + kS8OneMax - 1;           // chunks (32 samples) of a sample window for a pair of steps: 64 + K-blocks of the form - 1
constexpr int kS8NP = 2 * kS8NC;                    // 16-byte loads of the window
constexpr int kS8JN = (kS8NP + 63) / 64;            // ... per lane
constexpr int kS8XBytes = (kS8NP * 16 + 63) / 64 * 64;   // one staged window of a wave
static_assert(kS8JN == 3, "three window loads per lane");
static_assert(kS8OneMax >= kLongSB, "the window of the segmented form fits that of the resident one");
constexpr size_t kS8AWordsMax = (size_t)2 * kS8OneMax * 64 > (size_t)2 * kLongAWords ? (size_t)2 * kS8OneMax * 64 : (size_t)2 * kLongAWords;
constexpr size_t kS8LdsMax = kS8AWordsMax * 16 + (size_t)8 * 2 * kS8XBytes;
static_assert(kS8LdsMax <= 160 * 1024, "LDS of one gfx950 CU");

struct S8Args {
  int64_t pairs_per_wave;   // 2048-sample step pairs per workgroup row
  int64_t n_pairs;          // pairs [s_begin, n_pairs) of the call are this launch's; ceil(n / 2048) is the call's last + 1
  int64_t s_begin;
  int64_t n16;              // n rounded up to a multiple of 16 (rows are readable that far)
  int32_t nb, hb0, hb1;     // K-blocks; the high-plane products of blocks [hb0, hb1] only are issued
  uint32_t x_xor;           // unsigned samples: 0x80808080 turns every byte into x - 128; else 0
  int32_t a_words;          // v4i words of the A region of LDS: 2 nb 64 (one segment, resident) or 2 kLongAWords (double-buffered segments)
  int32_t np;               // window loads per segment: 2 (63 + nb) resident, 2 (63 + kLongSB) segmented
  int32_t fast;             // 32-bit epilogue (launch_fir_s8): y = clamp / wrap((V + half) >> rs) into 2-byte (OEB = 1: 1-byte) containers
  int32_t rs, half, ylo, yhi, wrap_sh, vec;   // wrap_sh: 32 - W_out for a signed AC_WRAP output, else 0; vec: rows take 16-byte stores
  int32_t sat16;            // ... and OUT_TYPE is a signed 16-bit AC_SAT type (the bounds are those of the packing conversion)
  const int64_t *corr;      // [1] 128 * sum(c) for unsigned samples, else 0
};

// FAST: the 32-bit epilogue; else the 64-bit one of fir_long_kernel.
// STREAM (with FAST): the one-segment form on whole pairs and rows that take 16-byte stores.  gfx950 counts loads and stores on ONE counter and
// returns them in order, so the wait in front of a window commit can leave the younger accesses in flight only if the compiler knows how many
// there are: this instantiation has no branch around a global access -- three window loads (clamped, not skipped) and four stores per
// iteration, an even number of iterations per workgroup -- where the general one has the ragged-step and unaligned-row branches.  The rest
// of a call (fewer than 4096 samples per channel) is a second, general launch.
// OEB (with FAST): bytes of an output container of the 32-bit epilogue, 2 or 1 (ACDSP_FLAG_OUT_BYTES); there three window loads and TWO stores
// per iteration of the STREAM form.  The 64-bit epilogue takes the container from p.out_eb.
template <bool FAST, bool STREAM, int OEB>
__global__ void __launch_bounds__(512, 2)
fir_s8_kernel(FirParams p, const v4i *__restrict__ frag, S8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int NB = a.nb;
  const bool one = STREAM || NB <= kS8OneMax;       // (launch argument: uniform over the grid)
  const int NSEG = one ? 1 : (NB + kLongSB - 1) / kLongSB;
  const int pstride = one ? NB * 64 : kLongSB * 64; // v4i words between the two coefficient planes of an A segment
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_col = lane & 31, h = lane >> 5;
  int ch = blockIdx.y * 8 + wave;
  const bool live = ch < p.n_ch;            // a wave past n_ch runs every iteration and barrier on the last channel's rows ...
  if (!live) { ch = p.n_ch - 1; }           // ... and stores nothing (STREAM, which has no branch around a store, repeats that channel's stores)
  // LDS: [A region: a_words v4i][per wave: 2 staged windows of kS8XBytes]
  v4i *ldsA = (v4i *)lds_all;
  unsigned char *ldsX = lds_all + (size_t)a.a_words * 16 + (size_t)wave * 2 * kS8XBytes;

  const unsigned char *xrow = (const unsigned char *)p.x + (int64_t)ch * p.in_stride;
  const unsigned char *hrow = (const unsigned char *)p.hist + (int64_t)ch * p.hl + p.hl;
  // loop bounds: launch arguments and blockIdx only (see "Barrier uniformity" above)
  const int64_t s0 = a.s_begin + (int64_t)blockIdx.x * a.pairs_per_wave;
  const int64_t s1 = (s0 + a.pairs_per_wave < a.n_pairs) ? s0 + a.pairs_per_wave : a.n_pairs;
  const int npairs = (int)(s1 - s0);
  const int total = npairs * NSEG;

  v4i RA[kLongAPerThread], RX0[kS8JN], RX1[kS8JN];
#pragma unroll
  for (int q = 0; q < kLongAPerThread; q++) { RA[q] = (v4i){0, 0, 0, 0}; }
#pragma unroll
  for (int j = 0; j < kS8JN; j++) { RX0[j] = (v4i){0, 0, 0, 0}; RX1[j] = (v4i){0, 0, 0, 0}; }
  // this thread's share of A segment g (segmented form)
  auto load_a = [&](int g) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < kLongAPerThread; q++) {
      const int idx = threadIdx.x + 512 * q, pl = idx / (kLongSB * 64), bl = (idx >> 6) % kLongSB, ln = idx & 63;
      int bg = g * kLongSB + bl;
      if (bg >= NB) { bg = NB - 1; }   // blocks past the set in the last segment: never multiplied, any in-bounds fragment will do
      RA[q] = frag[((size_t)pl * NB + bg) * 64 + ln];
    }
  };
  // this lane's share of the wave's window of (pair s, segment g)
  auto load_x = [&](v4i (&RX)[kS8JN], int s, int g) __attribute__((always_inline)) {
    // window base >= -32 (NB - 1) >= -hl (checked at launch); t is a multiple of 16, so a load never straddles history and row
    const int64_t base = (s0 + s) * 2048 - 32 * (int64_t)(NB - 1) + 32 * kLongSB * (int64_t)g;
#pragma unroll
    for (int j = 0; j < kS8JN; j++) {
      int pc = lane + 64 * j;
      if (STREAM && pc >= a.np) { pc = a.np - 1; }   // (past the window: the last load again, never committed)
      if (pc < a.np) {
        const int64_t t = base + 16 * pc;
        const unsigned char *src = (t < 0) ? hrow + t : xrow + ((t < a.n16) ? t : 0);
        RX[j] = *(const v4i *)src;
      }
    }
  };
  auto advance = [&](int &s, int &g) {
    g++;
    if (g == NSEG) { g = 0; s++; }
  };

  if (one) {
    // the whole set, 2 NB KB, once per workgroup: [plane][block][lane], as the fragments lie in memory
    for (int idx = threadIdx.x; idx < 2 * NB * 64; idx += 512) { ldsA[idx] = frag[idx]; }
    __syncthreads();
  }

  const int64_t corr = a.corr[0];
  v16i hi0 = {0}, lo0 = {0}, hi1 = {0}, lo1 = {0};   // steps 2 s and 2 s + 1 of the pair

  // outputs [T0, T0 + 1024) of the channel from one step's accumulators
  // (ob: the wave's window buffer of this iteration, read to the end by now)
  auto epilogue = [&](const v16i &hi, const v16i &lo, int64_t T0, unsigned char *ob) __attribute__((always_inline)) {
    if constexpr (FAST && OEB == 1) {
      // the 32-bit epilogue into 1-byte containers: lane (n, h) holds outputs 32 n + 8 q + 4 h + rr, so quad q is one dword of the row
      const int c32 = (int)corr;
      unsigned P[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        unsigned w = 0;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int v = (int)(((unsigned)hi[r] << 8) + (unsigned)lo[r] + (unsigned)c32);
          int yy = (v + a.half) >> a.rs;
          yy = yy < a.ylo ? a.ylo : (yy > a.yhi ? a.yhi : yy);                     // AC_SAT (AC_WRAP: the whole int32 range)
          yy = (int)((unsigned)yy << a.wrap_sh) >> a.wrap_sh;                      // signed AC_WRAP: sign-extend from W_out
          w |= ((unsigned)yy & 0xffu) << (8 * rr);
        }
        P[q] = w;
      }
      const int64_t tb = T0 + 32 * n_col;
      unsigned char *yrow = (unsigned char *)p.y + (int64_t)ch * p.out_stride;
      if (STREAM) {
        // the step's 1 KB of outputs through the wave's own window buffer into memory order: the store writes one run of 1 KB, lane = 16-byte
        // chunk of it.  Lane (n, h) holds, per q, the 4 bytes at 32 n + 8 q + 4 h; the 8-byte piece inside a block is XOR-ed with (n >> 3) & 3
        // against bank conflicts of the writes (the 64 lanes of one q then cover 64 different dwords mod 64)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
          *(unsigned *)(ob + 32 * n_col + 8 * (q ^ ((n_col >> 3) & 3)) + 4 * h) = P[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        {
          // chunk `lane` = block lane >> 1, pieces 2 g and 2 g + 1 (g = lane & 1): they sit in granule g ^ (sw >> 1), swapped where sw is odd
          const int blk = lane >> 1, sw = (blk >> 3) & 3;
          const v4i t = *(const v4i *)(ob + 32 * blk + 16 * ((lane & 1) ^ (sw >> 1)));
          const v4i o = (sw & 1) ? (v4i){t.z, t.w, t.x, t.y} : t;
          *(v4i *)(yrow + T0 + 16 * lane) = o;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      } else if (live && a.vec && T0 + 1024 <= p.n) {   // (wave-uniform: whole step inside the call)
        // one exchange of two dwords: h = 0 then owns bytes 32 n .. + 15 (its own quads 0, 1 and the partner's), h = 1 bytes 32 n + 16 .. + 31
        const unsigned R0 = (unsigned)__shfl_xor((int)(h ? P[0] : P[2]), 32);
        const unsigned R1 = (unsigned)__shfl_xor((int)(h ? P[1] : P[3]), 32);
        const v4i o = h ? (v4i){(int)R0, (int)P[2], (int)R1, (int)P[3]} : (v4i){(int)P[0], (int)R0, (int)P[1], (int)R1};
        *(v4i *)(yrow + tb + 16 * h) = o;
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int64_t t0 = tb + 8 * q + 4 * h;
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            if (live && t0 + rr < p.n) { yrow[t0 + rr] = (unsigned char)(P[q] >> (8 * rr)); }
          }
        }
      }
    } else if (FAST) {
      // |V| < 2^30 and ACC_TYPE neither wraps nor rounds (launch_fir_s8): V, the rounding add and the shift in 32 bits
      const int c32 = (int)corr;
      unsigned P[4][2];
      if (a.sat16) {
        // OUT_TYPE is a signed 16-bit AC_SAT type: v_cvt_pk_i16_i32 saturates and packs two outputs at once
        const unsigned k = (unsigned)c32 + (unsigned)a.half;
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
          for (int w = 0; w < 2; w++) {
            const int r = 4 * q + 2 * w;
            const int y0 = (int)(((unsigned)hi[r] << 8) + (unsigned)lo[r] + k) >> a.rs;
            const int y1 = (int)(((unsigned)hi[r + 1] << 8) + (unsigned)lo[r + 1] + k) >> a.rs;
            P[q][w] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(y0, y1));
          }
        }
      } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int y[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int v = (int)(((unsigned)hi[r] << 8) + (unsigned)lo[r] + (unsigned)c32);
          int yy = (v + a.half) >> a.rs;
          yy = yy < a.ylo ? a.ylo : (yy > a.yhi ? a.yhi : yy);                     // AC_SAT (AC_WRAP: the whole int32 range)
          yy = (int)((unsigned)yy << a.wrap_sh) >> a.wrap_sh;                      // signed AC_WRAP: sign-extend from W_out
          y[rr] = yy;
        }
        P[q][0] = ((unsigned)y[0] & 0xffffu) | ((unsigned)y[1] << 16);
        P[q][1] = ((unsigned)y[2] & 0xffffu) | ((unsigned)y[3] << 16);
      }
      }
      const int64_t tb = T0 + 32 * n_col;
      int16_t *yrow = (int16_t *)p.y + (int64_t)ch * p.out_stride;
      if (STREAM) {
        // the step's 2 KB of outputs through the wave's own window buffer into memory order: every store instruction then writes one run of
        // 1 KB, where the exchange below leaves 32-byte halves of 64-byte pieces to two instructions.  Lane (n, h) holds, per q, the 8 bytes
        // at 64 n + 16 q + 8 h; the 16-byte granule inside a block is XOR-ed with (n >> 2) & 3 against bank conflicts of the writes
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
          *(v2u *)(ob + 64 * n_col + 16 * (q ^ ((n_col >> 2) & 3)) + 8 * h) = (v2u){P[q][0], P[q][1]};
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const int blk = 16 * k + (lane >> 2);                       // lane = 16-byte chunk of the run: block, granule lane & 3
          const v4i o = *(const v4i *)(ob + 1024 * k + 64 * (lane >> 2) + 16 * ((lane & 3) ^ ((blk >> 2) & 3)));
          *(v4i *)(yrow + T0 + 512 * k + 8 * lane) = o;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      } else if (live && a.vec && T0 + 1024 <= p.n) {   // (wave-uniform: whole step inside the call)
        // lanes (n, 0) and (n, 1) hold outputs 8 q + 4 h + rr of block n: after one exchange each holds two runs of eight, 16 bytes each
        unsigned R[2][2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
          R[k][0] = (unsigned)__shfl_xor((int)(h ? P[2 * k][0] : P[2 * k + 1][0]), 32);
          R[k][1] = (unsigned)__shfl_xor((int)(h ? P[2 * k][1] : P[2 * k + 1][1]), 32);
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
          // h = 0: outputs 16 k + 0 .. 7 = own quad 2 k, partner's quad 2 k;  h = 1: outputs 16 k + 8 .. 15 = partner's quad 2 k + 1, own quad 2 k + 1
          const v4i o = h ? (v4i){(int)R[k][0], (int)R[k][1], (int)P[2 * k + 1][0], (int)P[2 * k + 1][1]}
                          : (v4i){(int)P[2 * k][0], (int)P[2 * k][1], (int)R[k][0], (int)R[k][1]};
          *(v4i *)(yrow + tb + 16 * k + 8 * h) = o;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int64_t t0 = tb + 8 * q + 4 * h;
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            if (live && t0 + rr < p.n) { yrow[t0 + rr] = (int16_t)(P[q][rr >> 1] >> (16 * (rr & 1))); }
          }
        }
      }
    } else {
      // V = 2^8 hi + lo + corr, exact in 64 bits; then the reference's two conversions (`acc += ...`, `data_out = acc`)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t t0 = T0 + 32 * n_col + 8 * q + 4 * h;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int r = 4 * q + rr;
          const int64_t v = ((int64_t)hi[r] << 8) + (int64_t)lo[r] + corr;
          const int64_t acc = wrap64((int64_t)((uint64_t)v << p.lossless_shift), p.acc.W, p.acc.S);
          const int64_t y = requant64(acc, p.acc.F, p.out);
          if (live && t0 + rr < p.n) { store_raw(p.y, (int64_t)ch * p.out_stride + t0 + rr, p.out_eb, y); }
        }
      }
    }
  };

  // iteration `it` = (pair s, segment g); RX holds its window (loaded two iterations ago) and takes that of iteration it + 2
  auto iteration = [&](v4i (&RX)[kS8JN], const int buf, int it, int s, int g) __attribute__((always_inline)) {
    // registers -> LDS.  Buffer `buf` was last read in iteration it - 2: every wave has passed the barrier of it - 1 since (segmented form);
    // the window is the wave's own, and LDS serves one wave's accesses in order
    if (!one) {
      v4i *dstA = ldsA + buf * kLongAWords;
#pragma unroll
      for (int q = 0; q < kLongAPerThread; q++) { dstA[threadIdx.x + 512 * q] = RA[q]; }
    }
    unsigned char *xb = ldsX + buf * kS8XBytes;
#pragma unroll
    for (int j = 0; j < kS8JN; j++) {
      const int pc = lane + 64 * j;   // (RX[j] is re-read below, so the clamped STREAM loads above stay out of LDS)
      if (pc < a.np) {
        v4i v = RX[j];
        v.x ^= (int)a.x_xor; v.y ^= (int)a.x_xor; v.z ^= (int)a.x_xor; v.w ^= (int)a.x_xor;
        *(v4i *)(xb + 16 * pc) = v;
      }
    }
    // in flight behind this segment's products: the A segment of it + 1 first (it is waited for first), then the window of it + 2
    int s2 = s, g2 = g;
    advance(s2, g2);
    if (!one && it + 1 < total) { load_a(g2); }
    advance(s2, g2);
    if (STREAM) { load_x(RX, s2 < npairs ? s2 : npairs - 1, 0); }   // (past the end: the last window again)
    else if (it + 2 < total) { load_x(RX, s2, g2); }
    if (!one) { __syncthreads(); }
    else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

    if (g == 0) { hi0 = (v16i){0}; lo0 = (v16i){0}; hi1 = (v16i){0}; lo1 = (v16i){0}; }
    const int b0 = g * kLongSB, nbs = one ? NB : ((NB - b0 < kLongSB) ? NB - b0 : kLongSB);
    const v4i *ah = ldsA + (one ? 0 : buf * kLongAWords) + lane, *al = ah + pstride;
    const unsigned char *fx = xb + 32 * n_col + 16 * h;   // step 0: chunk n_col + bl <= 63; step 1: 32 chunks on, <= 95
    // the K-blocks of this segment in three runs -- below, inside and above the high-byte range -- so that no run has a branch around an
    // LDS read or a product: h0 .. h1 - 1 are the blocks with a high-plane product
    int h0 = a.hb0 - b0, h1 = a.hb1 + 1 - b0;
    h0 = h0 < 0 ? 0 : (h0 > nbs ? nbs : h0);
    h1 = h1 < h0 ? h0 : (h1 > nbs ? nbs : h1);
    v4i Alc = al[0], Ahc = ah[(h0 < nbs ? h0 : nbs - 1) * 64], B0c = *(const v4i *)fx, B1c = *(const v4i *)(fx + 1024);
    auto run = [&](int from, int to, auto HI) __attribute__((always_inline)) {
      for (int bl = from; bl < to; bl++) {
        v4i Aln = Alc, Ahn = Ahc, B0n = B0c, B1n = B1c;
        if (bl + 1 < nbs) {   // fragments of the next K-block are in flight while this one multiplies
          Aln = al[(bl + 1) * 64];
          B0n = *(const v4i *)(fx + 32 * (bl + 1));
          B1n = *(const v4i *)(fx + 1024 + 32 * (bl + 1));
        }
        if (decltype(HI)::value) {
          if (bl + 1 < to) { Ahn = ah[(bl + 1) * 64]; }
          hi0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, B0c, hi0, 0, 0, 0);
          hi1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ahc, B1c, hi1, 0, 0, 0);
        }
        lo0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, B0c, lo0, 0, 0, 0);
        lo1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Alc, B1c, lo1, 0, 0, 0);
        Alc = Aln; Ahc = Ahn; B0c = B0n; B1c = B1n;
      }
    };
    run(0, h0, std::false_type());
    run(h0, h1, std::true_type());
    run(h1, nbs, std::false_type());
    if (g == NSEG - 1) {
      const int64_t T0 = (s0 + s) * 2048;
      epilogue(hi0, lo0, T0, xb);
      epilogue(hi1, lo1, T0 + 1024, xb);   // (past the call's end in a ragged last pair: every store is guarded)
    }
  };

  int s = 0, g = 0;
  if (total > 0) {
    if (!one) { load_a(0); }
    load_x(RX0, 0, 0);
    if (STREAM) { load_x(RX1, 1, 0); }   // (STREAM: an even number of pairs per workgroup, launch_fir_s8)
    else if (total > 1) {
      int sb = 0, gb = 0;
      advance(sb, gb);
      load_x(RX1, sb, gb);
    }
  }
  // unrolled by two: the two window register sets alternate (`total` is uniform over the workgroup, so is the branch around the second half)
  int it0 = 0;
  if (STREAM && total > 0) {
    // the first two iterations stand in front of the loop: it is then entered with the same accesses in flight as it is re-entered with, and
    // the counted wait of the first commit is not the (smaller) count of the prologue
    iteration(RX0, 0, 0, s, g);
    advance(s, g);
    iteration(RX1, 1, 1, s, g);
    advance(s, g);
    it0 = 2;
  }
  for (int it = it0; it < total; it += 2) {
    iteration(RX0, 0, it, s, g);
    advance(s, g);
    if (STREAM || it + 1 < total) {
      iteration(RX1, 1, it + 1, s, g);
      advance(s, g);
    }
  }
}

int fir_s8_issued_per_step(const FirLongPlan &plan) {
  return plan.nb + (plan.hb1 >= plan.hb0 ? plan.hb1 - plan.hb0 + 1 : 0);
}

hipError_t launch_fir_s8(const FirParams &p, const FirLongPlan &plan, int64_t sum_abs, const uint32_t *d_frag, const int64_t *d_corr, hipStream_t s) {
  if (p.n <= 0) { return hipSuccess; }
  // the first step reaches 32 (nb - 1) samples back; 513 K-blocks are 16384 taps
  if (plan.nb < 2 || plan.nb > long_blocks(kFirLongMaxTaps) || 32 * (plan.nb - 1) > p.hl || p.in_eb != 1 || p.in.W > 8) { return hipErrorInvalidValue; }
  S8Args a;
  memset(&a, 0, sizeof a);
  a.n_pairs = (p.n + 2047) / 2048;
  a.n16 = (p.n + 15) / 16 * 16;
  // (grids: long_grid with at least 4 pairs = 8 steps per workgroup row, below)
  a.nb = plan.nb; a.hb0 = plan.hb0; a.hb1 = plan.hb1;
  a.x_xor = p.in.S ? 0u : 0x80808080u;
  a.corr = d_corr;
  const bool one = plan.nb <= kS8OneMax;
  a.a_words = one ? 2 * plan.nb * 64 : 2 * kLongAWords;
  a.np = 2 * (63 + (one ? plan.nb : kLongSB));
  // the 32-bit epilogue: |V| <= sum|c| max|x| < 2^30 (so V + half cannot leave int32); V << shift inside a signed ACC_TYPE that wraps (or was
  // proven saturation-free), so ACC_TYPE holds the exact sum and `data_out = acc` rounds V at rs = F_in + F_coeff - F_out bits
  const int rs = p.in.F + p.cf.F - p.out.F;
  const int64_t xmax = p.in.S ? ((int64_t)1 << (p.in.W - 1)) : (((int64_t)1 << p.in.W) - 1);
  const bool small_v = sum_abs >= 0 && sum_abs < ((int64_t)1 << 30) / xmax;
  const int sh = p.lossless_shift;
  const bool acc_exact = p.acc.S && p.acc.O == ACDSP_WRAP && sh >= 0 && p.acc.W >= 2 && p.acc.W <= 64 && 31 + sh <= p.acc.W - 1;
  if (p.out_eb == 1 && p.out.W > 8) { return hipErrorInvalidValue; }
  const bool out_ok = ((p.out_eb == 2 && p.out.W <= 16) || (p.out_eb == 1 && p.out.W <= 8)) && p.out.W >= 2 && (p.out.Q == ACDSP_TRN || p.out.Q == ACDSP_RND) &&
                      (p.out.O == ACDSP_SAT || (p.out.O == ACDSP_WRAP && p.out.S)) && rs >= 1 && rs <= 29;
  if (small_v && acc_exact && out_ok) {
    a.fast = 1;
    a.rs = rs;
    a.half = p.out.Q == ACDSP_RND ? 1 << (rs - 1) : 0;
    const bool sat = p.out.O == ACDSP_SAT;
    a.ylo = sat ? (int32_t)p.out.lo : INT32_MIN;
    a.yhi = sat ? (int32_t)p.out.hi : INT32_MAX;
    a.wrap_sh = sat ? 0 : 32 - p.out.W;
    a.sat16 = (sat && p.out.S && p.out.W == 16) ? 1 : 0;
    a.vec = ((uintptr_t)p.y % 16 == 0 && p.out_stride * p.out_eb % 16 == 0) ? 1 : 0;   // (out_stride in elements: % 8 of 2-byte, % 16 of 1-byte ones)
  }
  const size_t lds = (size_t)a.a_words * 16 + (size_t)8 * 2 * kS8XBytes;
  // one constant limit for every instantiation and form (the larger form's): handles of different forms never lower it under each other
  constexpr int kLdsMax = (int)kS8LdsMax;
  hipError_t e = hipSuccess;
  const int64_t n_all = a.n_pairs, n_full = p.n / 4096 * 2;   // an even number of whole pairs, and an even number per workgroup below
  if (a.fast && a.vec && one && n_full > 0) {
    // whole pairs on the branch-free instantiation, the ragged rest (at most one pair per channel) on the general one behind it
    S8Args f = a;
    f.n_pairs = n_full;
    const LongGrid lf = long_grid(n_full, p.n_ch, 4);
    f.pairs_per_wave = lf.steps_per_wave + (lf.steps_per_wave & 1);
    const unsigned gxf = (unsigned)((n_full + f.pairs_per_wave - 1) / f.pairs_per_wave);
    auto kf = p.out_eb == 1 ? fir_s8_kernel<true, true, 1> : fir_s8_kernel<true, true, 2>;
    if ((e = hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax)) != hipSuccess) { return e; }
    hipLaunchKernelGGL(kf, dim3(gxf, lf.gy), dim3(512), lds, s, p, (const v4i *)d_frag, f);
    if ((e = hipGetLastError()) != hipSuccess || n_full == n_all) { return e; }
    a.s_begin = n_full;
  }
  const LongGrid lr = long_grid(n_all - a.s_begin, p.n_ch, 4);
  a.pairs_per_wave = lr.steps_per_wave;
  auto kern = !a.fast ? fir_s8_kernel<false, false, 2> : (p.out_eb == 1 ? fir_s8_kernel<true, false, 1> : fir_s8_kernel<true, false, 2>);
  if ((e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax)) != hipSuccess) { return e; }
  hipLaunchKernelGGL(kern, dim3(lr.gx, lr.gy), dim3(512), lds, s, p, (const v4i *)d_frag, a);
  return hipGetLastError();
}

}  // namespace acdsp
