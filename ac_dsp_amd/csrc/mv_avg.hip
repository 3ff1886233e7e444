// mv_avg.hip -- ac_mv_avg on many objects (second half).
//
// Replaces the per-sample loop of ac_mv_avg_core::mvAvgCore (reference include/ac_dsp/ac_mv_avg.h:111-123) driven by
// ac_mv_avg::run (:146-190): for every valid window position of a frame
//     acc = 0;  for j = -TAPS/2 .. TAPS/2:  acc = ACC_TYPE(acc + ACC_TYPE(w[j]) * coeffs[j + TAPS/2]);  out = OUT_TYPE(acc)
// with w the ac_window_1d_flag over the frame (AC_WIN: interior positions only; AC_CLIP / AC_MIRROR: every position,
// samples outside the frame replaced by the edge sample / the sample mirrored about it -- include/ac_types/ac_window.h).
//
// Mapping: one thread per output, a 256-thread block per tile of one (object, frame); the block stages the
// 256 + TAPS - 1 window samples -- boundary rule applied, already cast to ACC_TYPE (the cast depends on the sample only) --
// and the coefficients in LDS with coalesced loads, then every thread walks its taps in the reference's order.
// Two arithmetic classes: per-tap requantisation in 128 bits (any Q / O), and, for AC_TRN / AC_RND + AC_WRAP accumulators
// whose products fit 63 bits, the order-free form acc = sum_j ((xq_j * c_j + rnd) >> F_c) mod 2^W_acc in int64.
// Streaming op: 2 + 2 bytes per sample at 16-bit containers; bound by HBM for short windows.
// Host side: launch_mv_avg (at the end) launches what mv_avg_plan.hip decided -- a set plan per coefficient set, a call plan per run (mv_avg_plan.hpp).
#include <cstring>

#include "mv_avg_plan.hpp"

namespace acdsp {

namespace {

constexpr int kTile = kMvTile;

__device__ inline i128 shl128_(i128 v, int s) { return (i128)((u128)v << s); }

// line position of window element `pos` after the boundary rule (n samples per frame)
__device__ inline int64_t fold_pos(int64_t pos, int64_t n, int mode) {
  if (mode == 2) { return pos < 0 ? 0 : (pos > n - 1 ? n - 1 : pos); }
  if (n == 1) { return 0; }
  while (pos < 0 || pos > n - 1) {
    if (pos < 0) { pos = -pos; }
    if (pos > n - 1) { pos = 2 * (n - 1) - pos; }
  }
  return pos;
}

template <bool FAST>
__global__ void __launch_bounds__(kTile) mv_avg_kernel(MvAvgParams p) {
  extern __shared__ int64_t smem[];
  int64_t *win = smem;                       // [kTile + taps - 1]: ACC raw words of line positions m0 - h + j
  int64_t *cf = smem + kTile + p.taps - 1;   // [taps]
  const int tid = threadIdx.x, h = p.taps / 2;
  for (int i = tid; i < p.taps; i += kTile) { cf[i] = p.coeffs[i]; }
  const int64_t pairs = (int64_t)p.n_obj * p.n_frames;
  const int64_t first = p.win_mode == 0 ? h : 0;   // line position of a frame's first output
  for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
    const int64_t obj = pr / p.n_frames, fr = pr % p.n_frames;
    const int64_t xbase = obj * p.in_stride + fr * p.n_sample, ybase = obj * p.out_stride + fr * p.out_per_frame;
    const int64_t m0 = first + (int64_t)blockIdx.x * kTile;   // line position of this tile's first output
    __syncthreads();   // previous pair's readers are done with win[]
    for (int j = tid; j < kTile + p.taps - 1; j += kTile) {
      int64_t pos = m0 - h + j;
      int64_t v = 0;
      if (p.win_mode != 0) { pos = fold_pos(pos, p.n_sample, p.win_mode); }
      if (pos >= 0 && pos < p.n_sample) { v = requant64(load_raw(p.x, xbase + pos, p.in_eb, p.in.S), p.in.F, p.acc); }   // (ACC_TYPE) w[j]
      win[j] = v;
    }
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * kTile + tid;   // output index within the frame
    if (k < p.out_per_frame) {
      const int64_t *w = win + tid;   // w[j + h] = element j of the window centred on this output
      int64_t acc = 0;
      if (FAST) {
        uint64_t s = 0;
        const int sh = p.cf.F;   // >= 0 in this class
        const int64_t rnd = (p.acc.Q == ACDSP_RND && sh > 0) ? (int64_t(1) << (sh - 1)) : 0;
        for (int j = 0; j < p.taps; j++) { s += (uint64_t)((w[j] * cf[j] + rnd) >> sh); }
        acc = wrap64((int64_t)s, p.acc.W, p.acc.S);
      } else {
        const int fp = p.acc.F + p.cf.F, f = fp > p.acc.F ? fp : p.acc.F;
        for (int j = 0; j < p.taps; j++) {
          const i128 sum = shl128_((i128)acc, f - p.acc.F) + shl128_((i128)w[j] * (i128)cf[j], f - fp);
          acc = requant128(sum, f, p.acc);
        }
      }
      store_raw(p.y, ybase + k, p.out_eb, requant64(acc, p.acc.F, p.out));
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// Streaming kernel for the common class: 16-bit samples and 16-bit coefficients whose absolute values sum to < 2^15, a
// wrapping AC_TRN / AC_RND accumulator that holds the cast of a sample exactly (F_acc >= F_in, enough integer bits).  Then
//     acc = wrap( sum_j floor((x_j * 2^d * c_j + rnd) / 2^sh) ),   d = F_acc - F_in,  sh = F_coeff
// and every term fits int32:   d >= sh ("linear"):  x_j * c_j * 2^(d - sh)      -> v_dot2_i32_i16 on sample / coefficient pairs
//                              d <  sh ("per tap"): (x_j * c_j + r) >> (sh - d) -> mad / shift / add per tap.
// A wave owns runs of 512-output tiles of the (object, frame) rows: one coalesced 16-byte load per lane (+ a partial one
// for the window reach) goes to a wave-private LDS image of the tile, the frame-edge positions of AC_CLIP / AC_MIRROR are
// patched in from their source samples, every lane reads its 8 + TAPS - 1 window samples back with (unaligned) 16-byte
// reads, computes 8 consecutive outputs -- coefficients sit in SGPRs -- converts them (32-bit shift / clamp when nothing
// can wrap, else the 64-bit branch-free form) and stores 16 bytes per instruction.  The loads of the next tile are issued
// before the arithmetic of the current one.  No workgroup barrier: waves never share data.  (Argument: MvStreamArgs, mv_avg_plan.hpp.)

typedef short v2s_t __attribute__((ext_vector_type(2)));
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
typedef int v4i_mv __attribute__((ext_vector_type(4)));
// (tile loads keep the plain policy: non-temporal +3 % in time, profiles/r2_copy_probe_ldsdma.txt / DESIGN 5.1)
// 2-byte outputs (the bench row: one 16-byte store per lane) leave with the non-temporal policy; -DACDSP_MV_ST_PLAIN: plain (A/B)
#ifdef ACDSP_MV_ST_PLAIN
#define ACDSP_MV_ST(v, ptr) (*(ptr) = (v))
#else
#define ACDSP_MV_ST(v, ptr) __builtin_nontemporal_store(*reinterpret_cast<const v4u_t *>(&(v)), reinterpret_cast<v4u_t *>(ptr))
#endif

#ifndef ACDSP_MV_AHEAD
#define ACDSP_MV_AHEAD 2   // 4: -3 %, 8: -15 %, 16: -80 % on the bench row (profiles/r4_ab_up_store.txt, last block): more tiles in flight cost occupancy
#endif
// MF > 0 (round 6; windows of 17 taps and more, where the v_dot2 form is bound by VALU issue: 0.46 / 0.29 of the roofline at 33 / 65 taps): the
// window sums of a tile on the matrix cores.  The wave's image is the B operand as it lies -- column j' of v_mfma_i32_16x16x64_i8 is the 64 samples
// from image position 32 j' (+ 64 per further K block), a lane reads 32 aligned bytes and splits them into a low (re-biased by -128) and a high
// byte plane with v_perm_b32 -- and A is the Toeplitz matrix of the coefficients (balanced signed byte digits, built on the host), in TWO row
// orders: row i of fragment set m is output 32 j' + 8 (i >> 2) + (i & 3) + 4 m.  A lane's accumulator rows are then outputs 8 v .. 8 v + 7 of
// the tile, v = 4 (lane & 15) + (lane >> 4): eight consecutive outputs, the same epilogue and 16-byte stores as the v_dot2 form, a whole KB
// per store instruction.  8 MF MFMAs per 512 outputs (4 plane products x 2 row orders), 2 MF 16-byte LDS reads per lane instead of NR.
template <int NR, bool LINEAR, bool CV32, bool EDGE, bool PK = false, int MF = 0, bool RUN = false, int ROW = 0>   // ROW: tiles walk the ROW, frame edges fall inside them (a.row_n; 1: AC_CLIP / AC_MIRROR, 2: AC_WIN; see plan_stream in mv_avg_plan.hip); RUN: output tiles that start off a 16-byte boundary leave as aligned runs (a.run_ok; as a run-time branch it cost the bench row 12 VGPRs and two waves per SIMD: -8 %); PK: packed short frames (MvStreamArgs::pk_*; as run-time branches they cost the bench row 1.4 %)
__global__ void __launch_bounds__(256) mv_avg_stream_kernel(MvStreamArgs a) {
  static_assert(MF == 0 || (LINEAR && !PK), "matrix-core form: linear class, whole-frame tiles");
  static_assert(ROW == 0 || (!PK && MF == 0 && !RUN && EDGE == (ROW == 1)), "row walk: v_dot2 form, aligned outputs");
  constexpr int REGION = 512 + 8 * NR + 8;      // samples of one wave's LDS image (+ 8: the odd-offset window reads one dword further)
  constexpr int NQ = 4 * NR - 3;                // coefficient pairs covering 8 NR - 7 taps (+ a zero)
  // (4- and 8-byte outputs turn their tile around in the same image -- 2 / 4 KB -- before it leaves: IMG)
  constexpr int IMG = REGION > 2048 ? REGION : 2048;
  __shared__ __attribute__((aligned(16))) int16_t sm[4][IMG];   // (exactly 16 KB per workgroup: 16 bytes more -- tried for run_ok tiles of 8-byte outputs -- cost the bench row 9 %, one workgroup per CU less)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  int16_t *img = sm[wave];
  int bx, by_;
  xcd_remap(a.xcd_map, bx, by_);
  const int64_t t0 = ((int64_t)bx * 4 + wave) * a.tiles_per_wave;
  const int64_t t_end = (t0 + a.tiles_per_wave < a.n_tiles) ? t0 + a.tiles_per_wave : a.n_tiles;
  if (t0 >= t_end) { return; }
  const int n_my = (int)(t_end - t0);
  const uint32_t *cp = reinterpret_cast<const uint32_t *>(a.c16), *cpo = reinterpret_cast<const uint32_t *>(a.c16o);
  const int vlane = MF > 0 ? 4 * (lane & 15) + (lane >> 4) : lane;   // whose eight outputs this lane converts and stores
  v4i_mv A[MF > 0 ? 4 * MF : 1];                                        // [m][b][plane]
  if constexpr (MF > 0) {
#pragma unroll
    for (int f = 0; f < 4 * MF; f++) { A[f] = reinterpret_cast<const v4i_mv *>(a.frag)[f * 64 + lane]; }
  }

  // Tiles are fetched two ahead into alternating register sets.  (object, frame, tile) of the tile being fetched: one
  // division per wave, then counted up; past the wave's last tile the fetch repeats that tile (branch-free loop body, so
  // the waits in front of the LDS writes are counted vmcnt's on the older set only).
  struct Tile { uint4 mv, ev; int16_t fxl, fxr; int64_t ti, fr, obj; int bnd; };   // bnd (ROW): image position of the frame edge inside this tile's image, 2^20: none
  const int64_t pair0 = t0 / a.tpf;
  int64_t f_ti = t0 - pair0 * a.tpf, f_obj = pair0 / a.n_frames, f_fr = pair0 - f_obj * a.n_frames;
  int f_left = n_my;   // tiles not fetched yet
  auto fetch = [&](Tile &T) {   // aligned 8-sample groups: whole groups lie inside or outside the frame
    const int16_t *row = a.x + f_obj * a.in_stride + f_fr * a.n_sample;
    // ROW 2 (AC_WIN): the tile's first output o0 = 512 f_ti of the output row belongs to frame fr0 and reads the input row from in0 on; the outputs
    // from the next frame's first one (tile-relative index bnd) read TAPS - 1 samples further on -- the image is the contiguous input
    int64_t in0 = f_ti * 512 - (PK ? 0 : a.hb);
    if constexpr (ROW == 2) {
      const int64_t o0 = f_ti * 512;
      const uint32_t fr0 = (uint32_t)o0 / (uint32_t)a.row_opf;
      in0 = (int64_t)fr0 * a.row_n + (o0 - (int64_t)fr0 * a.row_opf);
      T.bnd = (int)((int64_t)(fr0 + 1) * a.row_opf - o0);
    }
    const int64_t n = a.n_sample, g = in0 + 8 * lane;
    T.ti = f_ti; T.fr = f_fr; T.obj = f_obj;
    // every load is unconditional (addresses clamped into the frame; what the clamped lanes fetch is never used), so
    // the loop body has no load under a branch and the waits stay counted
    const int64_t gc = g < 0 ? 0 : (g < n ? g : n - 8);
    { const v4u_t t_ = *reinterpret_cast<const v4u_t *>(row + gc); T.mv = make_uint4(t_.x, t_.y, t_.z, t_.w); }
    const int64_t g2 = in0 + 512 + 8 * (lane < a.nxg ? lane : 0);
    T.ev = *reinterpret_cast<const uint4 *>(row + (g2 < n ? g2 : n - 8));
#ifndef ACDSP_MV_LDS_EDGE
    if constexpr (ROW == 1) {
      // the one frame edge (a multiple of the frame length, 0 and the row's end included) that can lie inside the image (P0 - hb, P0 + 512 + hb):
      // frames are at least 512 + 2 hb samples long.  Its two halos take the mirrored / clipped samples of the frame they belong to.
      const int64_t P0 = f_ti * 512, c = P0 - a.hb + 1;
      const int64_t B = c <= 0 ? 0 : (int64_t)(((uint32_t)c + (uint32_t)a.row_n - 1u) / (uint32_t)a.row_n) * a.row_n;
      T.bnd = B < P0 + 512 + a.hb ? (int)(B - (P0 - a.hb)) : (1 << 20);
      const int l = lane < a.h ? lane : 0;
      int64_t sl = a.mode == 2 ? B : B + 1 + l, sr = a.mode == 2 ? B - 1 : B - 2 - l;
      sl = sl > n - 1 ? n - 1 : sl;                  // (the row's end: no frame behind it; the row's start: none in front)
      sr = sr < 0 ? 0 : (sr > n - 1 ? n - 1 : sr);
      T.fxl = row[sl];
      T.fxr = row[sr];
    } else if constexpr (EDGE) {   // frame-edge patches of AC_CLIP / AC_MIRROR: the source samples of positions -1 - lane and n + lane
      const int l = lane < a.h ? lane : 0;
      T.fxl = row[a.mode == 2 ? 0 : 1 + l];
      T.fxr = row[a.mode == 2 ? n - 1 : n - 2 - l];
    }
#endif
    if (f_left > 1) {
      f_left--;
      if (++f_ti == a.tpf) {
        f_ti = 0;
        if (++f_fr == a.n_frames) { f_fr = 0; f_obj++; }
      }
    }
  };
  auto process = [&](Tile &T) {
    const int64_t ti = T.ti, fr = T.fr, obj = T.obj, p0 = ti * 512 - a.hb;
    const int bnd = ROW != 0 ? T.bnd : 0;
    // image position of this lane's eight samples: 8 lane, or -- packed short frames -- frame f' = 8 lane / n of the tile at hb + f' (n + 2 hb)
    // (ROW: the samples behind the frame edge sit 2 hb further on -- the gap holds the right halo of the frame that ends and the left halo of the one that begins)
    const int gap = 2 * a.hb;
    const int lb = PK ? a.hb + ((8 * lane) >> a.pk_sh) * a.pk_pitch + ((8 * lane) & (a.pk_n - 1)) : (ROW == 1 ? 8 * lane + (8 * lane >= bnd ? gap : 0) : 8 * lane);
    *reinterpret_cast<uint4 *>(img + lb) = T.mv;
    if (lane < a.nxg) { *reinterpret_cast<uint4 *>(img + 512 + 8 * lane + (ROW == 1 && 512 + 8 * lane >= bnd ? gap : 0)) = T.ev; }
    if constexpr (ROW == 1) {
      if (lane < a.h && bnd < (1 << 20)) {
        img[bnd + lane] = T.fxr;
        img[bnd + gap - 1 - lane] = T.fxl;
      }
    } else if constexpr (EDGE) {   // positions outside [0, n) take the clipped / mirrored source sample
      if constexpr (PK) {
        // every frame of the tile has both its halos inside the image: filled from the staged samples themselves
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int n_patch = (512 >> a.pk_sh) * 2 * a.h;
        for (int e = lane; e < n_patch; e += 64) {
          const int fq = e / (2 * a.h), k2 = e - fq * 2 * a.h, right = k2 >= a.h, k = right ? k2 - a.h : k2;
          const int base = a.hb + fq * a.pk_pitch;
          const int dst = right ? base + a.pk_n + k : base - 1 - k;
          const int src = a.mode == 2 ? (right ? base + a.pk_n - 1 : base) : (right ? base + a.pk_n - 2 - k : base + 1 + k);
          img[dst] = img[src];
        }
      } else {
#ifdef ACDSP_MV_LDS_EDGE
        // A/B variant, off: the sources of a frame's out-of-frame positions lie inside the tile's own image (the first h + 1 / last h + 1 samples of
        // the frame), so the two scattered 2-byte loads per tile (fxl / fxr) could go.  Same box, three passes: 0.7625 ms with them, 0.7638 without.
        const bool left = ti == 0, right = a.n_sample - p0 < REGION;
        if (left || right) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          if (lane < a.h) {
            if (left) { img[a.hb - 1 - lane] = img[a.mode == 2 ? a.hb : a.hb + 1 + lane]; }
            const int64_t idx = a.n_sample + lane - p0;
            if (right && idx < REGION) { img[idx] = img[a.mode == 2 ? a.n_sample - 1 - p0 : a.n_sample - 2 - lane - p0]; }
          }
        }
#else
        if (lane < a.h) {
          if (ti == 0) { img[a.hb - 1 - lane] = T.fxl; }
          const int64_t idx = a.n_sample + lane - p0;
          if (idx < REGION) { img[idx] = T.fxr; }
        }
#endif
      }
    }
    fetch(T);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // The window starts a.off samples into the image: any even byte offset.  A DS read off its natural alignment is replayed lane by lane
    // (~85 instead of ~8 cycles per wave read, profiles/r5_lds_align.txt; rounds 2 - 4 read 16 bytes at 2-byte alignment here -- 8 bytes into
    // a 16-byte granule on the bench row), so the widest reads the offset is aligned for (the offset is wave-uniform: uniform branches).
    int S[8];
    const int s_init = CV32 ? a.r32 : 0;   // the 32-bit epilogue's rounding constant rides in the sum (|sum| < 2^30, r32 <= 2^29)
    if constexpr (MF > 0) {
      const unsigned char *ib = reinterpret_cast<const unsigned char *>(img) + 64 * (lane & 15) + 32 * (lane >> 4);
      const v4i_mv z4 = {0, 0, 0, 0};
      v4i_mv acc[2][3] = {{z4, z4, z4}, {z4, z4, z4}};   // [row order m][weight 1, 2^8, 2^16]
#pragma unroll
      for (int b = 0; b < MF; b++) {
        const uint4 d0 = *reinterpret_cast<const uint4 *>(ib + 128 * b), d1 = *reinterpret_cast<const uint4 *>(ib + 128 * b + 16);
        v4i_mv lo, hi;
        lo.x = (int)(__builtin_amdgcn_perm(d0.y, d0.x, 0x06040200u) ^ 0x80808080u); lo.y = (int)(__builtin_amdgcn_perm(d0.w, d0.z, 0x06040200u) ^ 0x80808080u);
        lo.z = (int)(__builtin_amdgcn_perm(d1.y, d1.x, 0x06040200u) ^ 0x80808080u); lo.w = (int)(__builtin_amdgcn_perm(d1.w, d1.z, 0x06040200u) ^ 0x80808080u);
        hi.x = (int)__builtin_amdgcn_perm(d0.y, d0.x, 0x07050301u); hi.y = (int)__builtin_amdgcn_perm(d0.w, d0.z, 0x07050301u);
        hi.z = (int)__builtin_amdgcn_perm(d1.y, d1.x, 0x07050301u); hi.w = (int)__builtin_amdgcn_perm(d1.w, d1.z, 0x07050301u);
#pragma unroll
        for (int m = 0; m < 2; m++) {
          const v4i_mv cl = A[(m * MF + b) * 2], ch = A[(m * MF + b) * 2 + 1];
          acc[m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cl, lo, acc[m][0], 0, 0, 0);
          acc[m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cl, hi, acc[m][1], 0, 0, 0);
          acc[m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ch, lo, acc[m][1], 0, 0, 0);
          acc[m][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ch, hi, acc[m][2], 0, 0, 0);
        }
      }
      // every partial stays far inside int32; the recombination is modular and the sum itself is inside 2^30 (host-checked)
#pragma unroll
      for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          S[4 * m + r] = (int)((uint32_t)acc[m][0][r] + ((uint32_t)acc[m][1][r] << 8) + ((uint32_t)acc[m][2][r] << 16) + (uint32_t)(s_init + a.kbias));
        }
      }
    } else {
    uint32_t R[4 * NR + 1];
    {
      const unsigned char *wb = reinterpret_cast<const unsigned char *>(img + (PK ? lb - a.hb : (ROW == 1 ? 8 * lane + (8 * lane + a.hb >= bnd ? gap : 0) : (ROW == 2 ? 8 * lane + (8 * lane >= bnd ? 2 * a.h : 0) : lb)))) + 2 * a.off;
      const int bo = 2 * a.off;
      if ((bo & 15) == 0) {
#pragma unroll
        for (int r = 0; r < NR; r++) { const uint4 v = *reinterpret_cast<const uint4 *>(wb + 16 * r); R[4 * r] = v.x; R[4 * r + 1] = v.y; R[4 * r + 2] = v.z; R[4 * r + 3] = v.w; }
      } else if ((bo & 7) == 0) {
#pragma unroll
        for (int r = 0; r < 2 * NR; r++) { const uint2 v = *reinterpret_cast<const uint2 *>(wb + 8 * r); R[2 * r] = v.x; R[2 * r + 1] = v.y; }
      } else if ((bo & 3) == 0) {
#pragma unroll
        for (int r = 0; r < 4 * NR; r++) { R[r] = *reinterpret_cast<const uint32_t *>(wb + 4 * r); }
      } else {   // an odd sample offset: aligned dwords one sample early, shifted down by 16 bits
        uint32_t prev = *reinterpret_cast<const uint32_t *>(wb - 2);
#pragma unroll
        for (int r = 0; r < 4 * NR; r++) {
          const uint32_t nxt = *reinterpret_cast<const uint32_t *>(wb + 2 + 4 * r);
          R[r] = __builtin_amdgcn_alignbit(nxt, prev, 16);
          prev = nxt;
        }
      }
    }
    R[4 * NR] = 0;
    if constexpr (LINEAR) {
      // output i of the lane starts at sample i of its dwords: even outputs pair (x[i+2q], x[i+2q+1]) = dword i/2 + q with
      // (c[2q], c[2q+1]); odd outputs pair the same aligned dwords with the coefficient pairs shifted by one tap,
      // (c[2q-1], c[2q]) with c[-1] = 0 -- no realignment of the samples
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int sum = s_init;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
          sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, R[i / 2 + q]), __builtin_bit_cast(v2s_t, (i & 1) ? cpo[q] : cp[q]), sum, false);
        }
        S[i] = sum;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int sum = s_init;
#pragma unroll
        for (int j = 0; j < 8 * NR - 7; j++) {
          const int k = i + j;
          const int xs = (k & 1) ? ((int)R[k / 2] >> 16) : (int)(int16_t)R[k / 2];
          sum += (xs * (int)a.c16[j] + a.rnd_e) >> a.e;
        }
        S[i] = sum;
      }
    }
    }
    __builtin_amdgcn_wave_barrier();   // every lane has its window: the image may be overwritten
    const int64_t k0 = ti * 512 + 8 * vlane;
    bool done16 = false;
    if constexpr (CV32 && !RUN) {
      // signed 16-bit AC_SAT outputs (the bench row's OUT_TYPE): shift, then v_cvt_pk_i16_i32 saturates and packs two outputs per instruction --
      // 12 instead of 28 VALU instructions per lane and tile on a kernel that is bound by VALU issue
      if (a.pk16) {
        if (k0 < a.opf) {
          typedef short v2s16_ __attribute__((ext_vector_type(2)));
          uint4 v;
          v.x = __builtin_bit_cast(uint32_t, (v2s16_)__builtin_amdgcn_cvt_pk_i16(S[0] >> a.s32, S[1] >> a.s32));
          v.y = __builtin_bit_cast(uint32_t, (v2s16_)__builtin_amdgcn_cvt_pk_i16(S[2] >> a.s32, S[3] >> a.s32));
          v.z = __builtin_bit_cast(uint32_t, (v2s16_)__builtin_amdgcn_cvt_pk_i16(S[4] >> a.s32, S[5] >> a.s32));
          v.w = __builtin_bit_cast(uint32_t, (v2s16_)__builtin_amdgcn_cvt_pk_i16(S[6] >> a.s32, S[7] >> a.s32));
          ACDSP_MV_ST(v, reinterpret_cast<uint4 *>((int16_t *)a.y + (obj * a.out_stride + fr * a.opf + k0)));
        }
        done16 = true;
      }
    }
    if (!done16 && k0 < a.opf) {
      const int64_t yb = obj * a.out_stride + fr * a.opf + k0;
      int64_t ov[8];                                  // OUT raw words (the low out_eb bytes are what leaves)
      if constexpr (CV32) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          int q = S[i] >> a.s32;
          q = q < a.lo32 ? a.lo32 : (q > a.hi32 ? a.hi32 : q);
          if (a.ko32) { q = (int)((uint32_t)q << a.ko32) >> a.ko32; }
          if (a.om != ~uint64_t(0)) { q = (int)((uint32_t)q & (uint32_t)a.om); }
          ov[i] = a.om != ~uint64_t(0) ? (int64_t)(uint32_t)q : (int64_t)q;   // unsigned OUT: the masked word zero-extends; signed: sign-extends
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int64_t acc = (int64_t)(((uint64_t)((int64_t)((uint64_t)(int64_t)S[i] << (a.ls + a.ka)) >> a.ka)) & a.am);   // wrap to ACC_TYPE
          int64_t qv = (int64_t)((uint64_t)((acc + a.rnd) >> a.rs) << a.ls2);
          qv = qv < a.lo ? a.lo : (qv > a.hi ? a.hi : qv);
          ov[i] = (int64_t)(((uint64_t)((int64_t)((uint64_t)qv << a.ko) >> a.ko)) & a.om);
        }
      }
      if (a.vec_ok) {
        if (a.out_eb == 2) {
          uint4 v;
          v.x = __builtin_amdgcn_perm((uint32_t)ov[1], (uint32_t)ov[0], 0x05040100u); v.y = __builtin_amdgcn_perm((uint32_t)ov[3], (uint32_t)ov[2], 0x05040100u);
          v.z = __builtin_amdgcn_perm((uint32_t)ov[5], (uint32_t)ov[4], 0x05040100u); v.w = __builtin_amdgcn_perm((uint32_t)ov[7], (uint32_t)ov[6], 0x05040100u);
          ACDSP_MV_ST(v, reinterpret_cast<uint4 *>((int16_t *)a.y + yb));
        } else {
          // 4- / 8-byte containers: a lane's eight outputs are 32 / 64 contiguous bytes, and stored from the registers every instruction
          // covered its 2 / 4 KB with 16-byte pieces 32 / 64 bytes apart (0.48 / 0.38 of the roofline where the 2-byte row runs 0.69).
          // The tile goes through the wave's LDS image once -- rows of 16 bytes per lane out -- and leaves in whole 1 KB runs.
          unsigned char *ib = reinterpret_cast<unsigned char *>(img);
          if (a.out_eb == 4) {
            uint4 *w = reinterpret_cast<uint4 *>(ib + 32 * vlane);
            w[0] = make_uint4((uint32_t)ov[0], (uint32_t)ov[1], (uint32_t)ov[2], (uint32_t)ov[3]);
            w[1] = make_uint4((uint32_t)ov[4], (uint32_t)ov[5], (uint32_t)ov[6], (uint32_t)ov[7]);
          } else {
            ulonglong2 *w = reinterpret_cast<ulonglong2 *>(ib + 64 * vlane);
#pragma unroll
            for (int i = 0; i < 8; i += 2) { w[i / 2] = make_ulonglong2((uint64_t)ov[i], (uint64_t)ov[i + 1]); }
          }
        }
      } else if (RUN) {
        // output frames that start off a 16-byte boundary (round 6: AC_WIN with TAPS - 1 no multiple of 8 -- 1012 outputs per frame -- ran eight
        // element stores per lane, 0.25 - 0.30 of the roofline): the tile's outputs go to the image at the byte offset their first one has
        // inside its 16-byte granule, and leave below as aligned 16-byte pieces
        // (no guards: what a lane writes past the tile's last output stays in the image)
        const int mis = (int)(((uintptr_t)a.y + (uint64_t)(yb - 8 * vlane) * a.out_eb) & 15);
        unsigned char *ib = reinterpret_cast<unsigned char *>(img) + mis + 8 * vlane * a.out_eb;
        if (a.out_eb == 2) {
          const uint32_t p0_ = __builtin_amdgcn_perm((uint32_t)ov[1], (uint32_t)ov[0], 0x05040100u), p1_ = __builtin_amdgcn_perm((uint32_t)ov[3], (uint32_t)ov[2], 0x05040100u);
          const uint32_t p2_ = __builtin_amdgcn_perm((uint32_t)ov[5], (uint32_t)ov[4], 0x05040100u), p3_ = __builtin_amdgcn_perm((uint32_t)ov[7], (uint32_t)ov[6], 0x05040100u);
          if (!(mis & 2)) {         // wave-uniform: dword-aligned pairs
            uint32_t *w = reinterpret_cast<uint32_t *>(ib);
            w[0] = p0_; w[1] = p1_; w[2] = p2_; w[3] = p3_;
          } else {                  // one element, three straddling pairs, one element
            reinterpret_cast<int16_t *>(ib)[0] = (int16_t)ov[0];
            uint32_t *w = reinterpret_cast<uint32_t *>(ib + 2);
            w[0] = __builtin_amdgcn_alignbit(p1_, p0_, 16); w[1] = __builtin_amdgcn_alignbit(p2_, p1_, 16); w[2] = __builtin_amdgcn_alignbit(p3_, p2_, 16);
            reinterpret_cast<int16_t *>(ib)[7] = (int16_t)ov[7];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++) { reinterpret_cast<int32_t *>(ib)[i] = (int32_t)ov[i]; }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          if (k0 + i < a.opf) { store_raw(a.y, yb + i, a.out_eb, ov[i]); }
        }
      }
    }
    if (RUN && !a.vec_ok) {   // wave-uniform: second half of the unaligned turn-around
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const unsigned char *ib = reinterpret_cast<const unsigned char *>(img);
      const uintptr_t b0 = (uintptr_t)a.y + (uint64_t)(obj * a.out_stride + fr * a.opf + ti * 512) * a.out_eb;
      const int mis = (int)(b0 & 15);
      const int64_t left = a.opf - ti * 512;
      const int total = mis + (int)(left < 512 ? left : 512) * a.out_eb;      // image bytes [mis, total) are this tile's outputs
      unsigned char *g = reinterpret_cast<unsigned char *>(b0 - mis);
#pragma unroll
      for (int k = 0; k < 3; k++) {                                             // 512 x 4 bytes + 15 = 129 pieces at most
        const int o = 16 * (lane + 64 * k);
        if (o >= mis && o + 16 <= total) {
          const uint4 v = *reinterpret_cast<const uint4 *>(ib + o);
          ACDSP_MV_ST(v, reinterpret_cast<uint4 *>(g + o));
        }
      }
      {
        // the first and the last piece of the run hold up to seven 2-byte units each: ONE store instruction for both, a unit per lane (lanes 0 - 7
        // the head, 8 - 15 the tail; as 2-byte stores per piece they were 16 more memory instructions per tile than the aligned form's one)
        const int hf = (mis + 15) & ~15, tf = total & ~15, t0b = tf > hf ? tf : hf;
        const int bb = (lane < 8 ? mis : t0b) + 2 * (lane & 7);
        if (lane < 16 && bb < total && (lane >= 8 || bb < hf)) { *reinterpret_cast<int16_t *>(g + bb) = *reinterpret_cast<const int16_t *>(ib + bb); }
      }
      __builtin_amdgcn_wave_barrier();   // read back before the next tile is staged over it
    }
    {
      if (a.vec_ok && a.out_eb != 2) {   // wave-uniform: the second half of the turn-around above
        __builtin_amdgcn_wave_barrier();
        const unsigned char *ib = reinterpret_cast<const unsigned char *>(img);
        const int64_t rem_b = (a.opf - ti * 512) * a.out_eb;                 // bytes of this tile that exist (a multiple of 32)
        unsigned char *yt = reinterpret_cast<unsigned char *>(a.y) + (obj * a.out_stride + fr * a.opf + ti * 512) * a.out_eb;
        const int nk = a.out_eb == 4 ? 2 : 4;
        for (int k = 0; k < nk; k++) {
          const int off = 1024 * k + 16 * lane;
          if (off < rem_b) {
            const uint4 v = *reinterpret_cast<const uint4 *>(ib + off);
            ACDSP_MV_ST(v, reinterpret_cast<uint4 *>(yt + off));
          }
        }
        __builtin_amdgcn_wave_barrier();   // read back before the next tile is staged over it
      }
    }
  };
  // ACDSP_MV_AHEAD register sets: tiles in flight per wave (A/B knob; 2 = rounds 2 - 3)
  Tile T[ACDSP_MV_AHEAD];
#pragma unroll
  for (int j = 0; j < ACDSP_MV_AHEAD; j++) {
    T[j].mv = T[j].ev = make_uint4(0, 0, 0, 0);
    T[j].fxl = T[j].fxr = 0;
  }
#pragma unroll
  for (int j = 0; j < ACDSP_MV_AHEAD; j++) { fetch(T[j]); }
  for (int it = 0; it < n_my; it += ACDSP_MV_AHEAD) {
#pragma unroll
    for (int j = 0; j < ACDSP_MV_AHEAD; j++) {
      if (j == 0 || it + j < n_my) { process(T[j]); }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 32-bit samples (round 5; the header's usage example declares IN_TYPE ac_fixed<32,16>, ac_mv_avg.h:47): the order-free class on int32
// containers whose cast to ACC_TYPE is exact -- xq = x << d, d = F_acc - F_in >= 0, enough integer bits -- and coefficients inside int32:
//     acc = wrap( sum_j floor((x_j c_j 2^d + rnd) / 2^sh) ),  sh = F_coeff;  x_j c_j is ONE v_mad_i64_i32, host-checked to stay inside 2^62.
// A 256-thread block takes a tile of 1024 outputs of one (object, frame): the 1024 + TAPS - 1 window samples go to LDS as int32 with
// the boundary rule applied (coalesced loads), a thread owns four consecutive outputs and slides an eight-register window over the taps
// -- one aligned 16-byte LDS read per four taps; coefficients are uniform reads -- then converts (requant64: any OUT_TYPE) and
// stores its four outputs as one or two 16-byte vectors.  Before: 128-bit per-tap kernel, 0.034 of the roofline on <32,16> samples.  (Arguments: MvAvgParams and MvW32Args, mv_avg_plan.hpp.)

template <bool LINEAR, bool CONV>   // LINEAR: d >= sh, the products add up unshifted (one v_mad_i64_i32 per tap and output); CONV: TRN / RND into WRAP / SAT
__global__ void __launch_bounds__(256) mv_avg_w32_kernel(MvAvgParams p, MvW32Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char w32_lds[];
  const int h = p.taps / 2, tid = threadIdx.x;
  const int nwin = (1024 + p.taps - 1 + 3 + 4) & ~3;            // window dwords, padded: the last 16-byte read of a thread may reach one group further
  int32_t *win = (int32_t *)w32_lds;
  int32_t *cf = win + nwin;                                       // [taps] coefficients (int32 by the host check)
  for (int i = tid; i < p.taps; i += 256) { cf[i] = (int32_t)p.coeffs[i]; }
  const int64_t pairs = (int64_t)p.n_obj * p.n_frames;
  const int64_t first = p.win_mode == 0 ? h : 0;
  for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
    const int64_t obj = pr / p.n_frames, fr = pr % p.n_frames;
    const int32_t *xrow = (const int32_t *)p.x + obj * p.in_stride + fr * p.n_sample;
    const int64_t ybase = obj * p.out_stride + fr * p.out_per_frame;
    const int64_t m0 = first + (int64_t)blockIdx.x * 1024;
    __syncthreads();
    for (int j = tid; j < nwin; j += 256) {
      int64_t pos = m0 - h + j;
      if (p.win_mode != 0) { pos = fold_pos(pos, p.n_sample, p.win_mode); }
      // (round 6: 16-bit containers as well -- frames that are no multiple of 8 samples, weights beyond the int32 class of the streaming kernel: 0.03 on the int64 kernel)
      win[j] = (pos >= 0 && pos < p.n_sample) ? (p.in_eb == 4 ? xrow[pos] : (int32_t)load_raw(p.x, obj * p.in_stride + fr * p.n_sample + pos, 2, p.in.S)) : 0;
    }
    __syncthreads();
    const int64_t k0 = (int64_t)blockIdx.x * 1024 + 4 * tid;    // first of this thread's four outputs within the frame
    if (k0 < p.out_per_frame) {
      typedef int v4i_ __attribute__((ext_vector_type(4)));
      const v4i_ *wv = (const v4i_ *)(win + 4 * tid);
      v4i_ cur = wv[0];
      uint64_t s[4] = {0, 0, 0, 0};
      for (int jg = 0; 4 * jg < p.taps; jg++) {
        const v4i_ nxt = wv[jg + 1];
        const int w8[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int j = 4 * jg + u;
          if (j < p.taps) {
            const int c = cf[j];
#pragma unroll
            for (int i = 0; i < 4; i++) {
              if (LINEAR) { s[i] = (uint64_t)((int64_t)w8[u + i] * (int64_t)c + (int64_t)s[i]); }
              else { s[i] += (uint64_t)(((int64_t)w8[u + i] * (int64_t)c + a.rnd_e) >> a.e); }
            }
          }
        }
        cur = nxt;
      }
      int64_t o[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (CONV) {
          const int64_t acc = (int64_t)(((uint64_t)((int64_t)(s[i] << (a.ls + a.ka)) >> a.ka)) & a.am);   // (sum << ls) wrapped to ACC_TYPE
          int64_t qv = (int64_t)((uint64_t)((acc + a.rnd) >> a.rs) << a.ls2);
          qv = qv < a.lo ? a.lo : (qv > a.hi ? a.hi : qv);
          o[i] = (int64_t)(((uint64_t)((int64_t)((uint64_t)qv << a.ko) >> a.ko)) & a.om);
        } else {
          o[i] = requant64(wrap64((int64_t)(s[i] << a.ls), p.acc.W, p.acc.S), p.acc.F, p.out);
        }
      }
      if (a.vec_ok && k0 + 4 <= p.out_per_frame) {
        if (p.out_eb == 8) {
          typedef long v2l_ __attribute__((ext_vector_type(2)));
          v2l_ *yp = (v2l_ *)((int64_t *)p.y + ybase + k0);
          yp[0] = (v2l_){o[0], o[1]}; yp[1] = (v2l_){o[2], o[3]};
        } else if (p.out_eb == 4) {
          *(v4i_ *)((int32_t *)p.y + ybase + k0) = (v4i_){(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
        } else {
          typedef short v4s_ __attribute__((ext_vector_type(4)));
          *(v4s_ *)((int16_t *)p.y + ybase + k0) = (v4s_){(short)o[0], (short)o[1], (short)o[2], (short)o[3]};
        }
      } else {
        for (int i = 0; i < 4 && k0 + i < p.out_per_frame; i++) { store_raw(p.y, ybase + k0 + i, p.out_eb, o[i]); }
      }
    }
  }
}

}  // namespace

// The compiled kernels as data, MvCall::inst -> kernel.  mv_avg_stream_kernel: six NR x LINEAR x CV32 x the seven forms of the v_dot2 kernel ...
#define ACDSP_MV_K(NR, LIN, CV, EDGE, PK, MF, RUN, ROW) {{NR, LIN, CV, EDGE, PK, MF, RUN, ROW}, mv_avg_stream_kernel<NR, LIN, CV, EDGE, PK, MF, RUN, ROW>}
#define ACDSP_MV_FORMS(NR, LIN, CV)                                                                                              \
  ACDSP_MV_K(NR, LIN, CV, true, true, 0, false, 0),   /* packed short frames */                                                 \
  ACDSP_MV_K(NR, LIN, CV, false, false, 0, false, 2), /* row walk, AC_WIN */                                                    \
  ACDSP_MV_K(NR, LIN, CV, true, false, 0, false, 1),  /* row walk, frame edges inside the tiles */                              \
  ACDSP_MV_K(NR, LIN, CV, true, false, 0, true, 0), ACDSP_MV_K(NR, LIN, CV, false, false, 0, true, 0), /* aligned runs */     \
  ACDSP_MV_K(NR, LIN, CV, true, false, 0, false, 0), ACDSP_MV_K(NR, LIN, CV, false, false, 0, false, 0)
#define ACDSP_MV_NR(NR) ACDSP_MV_FORMS(NR, true, true), ACDSP_MV_FORMS(NR, true, false), ACDSP_MV_FORMS(NR, false, true), ACDSP_MV_FORMS(NR, false, false)
// ... and on the matrix cores MF x CV32 x EDGE x RUN
#define ACDSP_MV_MF(MF, CV) ACDSP_MV_K(9, true, CV, true, false, MF, true, 0), ACDSP_MV_K(9, true, CV, true, false, MF, false, 0), \
                            ACDSP_MV_K(9, true, CV, false, false, MF, true, 0), ACDSP_MV_K(9, true, CV, false, false, MF, false, 0)
static const MvInst<void (*)(MvStreamArgs)> kStreamKernels[] = {ACDSP_MV_NR(2), ACDSP_MV_NR(3), ACDSP_MV_NR(4), ACDSP_MV_NR(5), ACDSP_MV_NR(7), ACDSP_MV_NR(9),
                                                                ACDSP_MV_MF(1, true), ACDSP_MV_MF(1, false), ACDSP_MV_MF(2, true), ACDSP_MV_MF(2, false)};
#undef ACDSP_MV_MF
#undef ACDSP_MV_NR
#undef ACDSP_MV_FORMS
#undef ACDSP_MV_K
static const MvInst<void (*)(MvAvgParams, MvW32Args)> kW32Kernels[] = {{{true, true}, mv_avg_w32_kernel<true, true>}, {{true, false}, mv_avg_w32_kernel<true, false>},
                                                                        {{false, true}, mv_avg_w32_kernel<false, true>}, {{false, false}, mv_avg_w32_kernel<false, false>}};
static const MvInst<void (*)(MvAvgParams)> kGeneralKernels[] = {{{true}, mv_avg_kernel<true>}, {{false}, mv_avg_kernel<false>}};

hipError_t launch_mv_avg(const MvCall &c, hipStream_t s) {
  switch (c.path) {
    case 0: case 1: return mv_launch(kGeneralKernels, c, s, c.p);
    case 2: case 4: return mv_launch(kStreamKernels, c, s, c.a.st);
    case 3: return mv_launch(kW32Kernels, c, s, c.p, c.a.w32);
    case 5: return launch_mv_avg_s8(c, s);
    default: return hipSuccess;   // nothing to launch
  }
}

}  // namespace acdsp
