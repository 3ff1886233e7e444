// mv_avg_s8.hip -- ac_mv_avg on 1-byte sample rows (ACDSP_FLAG_IN_BYTES; acdsp_mvavg_path 5).
//
// The matrix-core form of mv_avg_stream_kernel (mv_avg.hip, MF instantiations) with the sample side halved.  A byte sample is the B operand of
// v_mfma_i32_16x16x64_i8 as it lies in memory: no split into planes, ONE sample plane, and one product per K block and row order when every
// coefficient is a single signed byte (two when some coefficient carries a high digit).
//
// Class (plan_s8 in mv_avg_plan.hip; the set plan holds the part that depends on the coefficient set): the linear class of plan_stream -- the cast of a sample to ACC_TYPE is exact, d = F_acc - F_in >= sh = F_coeff >= 0, a wrapping
// AC_TRN / AC_RND accumulator (a saturating one that the set plan has proved sat-free arrives here as a wrapping one), coefficients inside int16 with
// sum |c| <= 32767 and none above 32639, AC_TRN / AC_RND into AC_WRAP / AC_SAT outputs -- on windows of 1 .. 65 taps, every window mode,
// n_sample >= TAPS.  Shape: input rows and row pitch aligned to 16 bytes and n_sample % 16 == 0.  Frames of n_sample % 8 == 0 that are no
// multiple of 16 are NOT taken (an 8-byte load form would halve the bytes per load instruction on a kernel that lives on them; they run on the
// order-free int64 kernel, like every other shape outside the class: tests/test_mvavg_bytes_gpu.py pins 24 and 1000).
//
// A wave owns runs of 512-output tiles and a wave-private LDS image of the tile in BYTES; there is no workgroup barrier.  Image position q holds
// the sample at frame position 512 ti - hb + q, hb = the window's half length rounded up to 16 (0 under AC_WIN), so every tile load is one
// aligned 16 bytes per lane (lanes 0 .. 31 the tile, up to four more the window reach); the loads of the tiles ahead are in flight while the
// current one is computed.  The positions outside the frame (AC_CLIP / AC_MIRROR) are patched into the image from their source samples with
// byte writes.  Column j' of the MFMA is the 64 samples from image position 32 j' (+ 64 per further K block): a lane's B fragment is one aligned
// ds_read_b128.  Unsigned samples are re-biased by flipping bit 7; 128 sum(c) rides in a constant.  A is the Toeplitz matrix of the
// coefficients' balanced signed byte digits in two row orders (mv_avg_build_frags with a halo granularity of 16), so that a lane's accumulator
// rows are eight consecutive outputs; the high-digit fragments are neither loaded nor multiplied when every high digit is 0 (HI = false):
// K blocks x 2 MFMAs per 512 outputs.  The accumulator-to-output conversion has the two forms of the 16-bit kernel: 32-bit shift / clamp when
// nothing can wrap, else the 64-bit branch-free form.  Outputs: a lane's eight results leave as one 8-byte store (1-byte containers), one
// 16-byte store (2-byte) or two / four 16-byte stores (4- / 8-byte); rows whose 8-output groups are not aligned take guarded element stores.
#include <cstring>

#include "mv_avg_plan.hpp"

namespace acdsp {

namespace {

typedef int v4i_s8 __attribute__((ext_vector_type(4)));
typedef unsigned v4u_s8 __attribute__((ext_vector_type(4)));
typedef unsigned v2u_s8 __attribute__((ext_vector_type(2)));

constexpr int kS8Img = 1024;     // bytes of one wave's image: 512 + 64 (halos) + what the last column's second K block reads (608), rounded up
constexpr int kS8Ahead = 4;      // tiles in flight per wave: 512 bytes each, the bytes in flight of the 16-bit kernel's two

template <int NB, bool HI, bool CV32, bool EDGE>   // NB: K blocks of 64 samples; HI: some coefficient has a high digit; CV32: 32-bit epilogue; EDGE: AC_CLIP / AC_MIRROR
__global__ void __launch_bounds__(256) mv_avg_s8_kernel(MvS8Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char sm[4][kS8Img];   // 4 KB per workgroup
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  unsigned char *img = sm[wave];
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + wave) * a.tiles_per_wave;
  const int64_t t_end = (t0 + a.tiles_per_wave < a.n_tiles) ? t0 + a.tiles_per_wave : a.n_tiles;
  if (t0 >= t_end) { return; }
  const int n_my = (int)(t_end - t0);
  const int vlane = 4 * (lane & 15) + (lane >> 4);   // whose eight outputs this lane converts and stores
  constexpr int NP = HI ? 2 : 1;
  v4i_s8 A[2 * NB * NP];                             // [m][b][plane]
#pragma unroll
  for (int m = 0; m < 2; m++) {
#pragma unroll
    for (int b = 0; b < NB; b++) {
#pragma unroll
      for (int pl = 0; pl < NP; pl++) { A[(m * NB + b) * NP + pl] = reinterpret_cast<const v4i_s8 *>(a.frag)[((m * NB + b) * 2 + pl) * 64 + lane]; }
    }
  }

  // (object, frame, tile) of the tile being fetched: one division per wave, then counted up; past the wave's last tile the fetch repeats that
  // tile (branch-free loop body, as in mv_avg_stream_kernel)
  struct Tile { uint4 mv; unsigned char fxl, fxr; int64_t ti, fr, obj; };
  const int64_t pair0 = t0 / a.tpf;
  int64_t f_ti = t0 - pair0 * a.tpf, f_obj = pair0 / a.n_frames, f_fr = pair0 - f_obj * a.n_frames;
  int f_left = n_my;
  auto fetch = [&](Tile &T) {   // aligned 16-sample groups: whole groups lie inside or outside the frame
    const unsigned char *row = a.x + f_obj * a.in_stride + f_fr * a.n_sample;
    const int64_t n = a.n_sample, g = f_ti * 512 - a.hb + 16 * (lane < a.nld ? lane : 0);
    T.ti = f_ti; T.fr = f_fr; T.obj = f_obj;
    // unconditional, the address clamped into the frame (what a clamped lane fetches is patched over or belongs to no stored output)
    const int64_t gc = g < 0 ? 0 : (g < n ? g : n - 16);
    { const v4u_s8 t_ = *reinterpret_cast<const v4u_s8 *>(row + gc); T.mv = make_uint4(t_.x, t_.y, t_.z, t_.w); }
    if constexpr (EDGE) {       // the source samples of positions -1 - lane and n + lane (n >= TAPS: one reflection)
      const int l = lane < a.h ? lane : 0;
      T.fxl = row[a.mode == 2 ? 0 : 1 + l];
      T.fxr = row[a.mode == 2 ? n - 1 : n - 2 - l];
    }
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
    if (lane < a.nld) { *reinterpret_cast<uint4 *>(img + 16 * lane) = T.mv; }
    if constexpr (EDGE) {
      if (lane < a.h) {
        if (ti == 0) { img[a.hb - 1 - lane] = T.fxl; }
        const int64_t idx = a.n_sample + lane - p0;
        if (idx < kS8Img) { img[idx] = T.fxr; }
      }
    }
    fetch(T);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned char *ib = img + 32 * (lane & 15) + 16 * (lane >> 4);
    const v4i_s8 z4 = {0, 0, 0, 0};
    v4i_s8 acc[2][2] = {{z4, z4}, {z4, z4}};   // [row order m][weight 1, 2^8]
#pragma unroll
    for (int b = 0; b < NB; b++) {
      const uint4 d = *reinterpret_cast<const uint4 *>(ib + 64 * b);
      const v4i_s8 B = {(int)(d.x ^ a.flip), (int)(d.y ^ a.flip), (int)(d.z ^ a.flip), (int)(d.w ^ a.flip)};
#pragma unroll
      for (int m = 0; m < 2; m++) {
        acc[m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[(m * NB + b) * NP], B, acc[m][0], 0, 0, 0);
        if constexpr (HI) { acc[m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[(m * NB + b) * NP + 1], B, acc[m][1], 0, 0, 0); }
      }
    }
    __builtin_amdgcn_wave_barrier();   // every lane has its fragments: the image may be overwritten
    // |sum c x| < 2^23 and every partial stays far inside int32; the recombination is modular
    int S[8];
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        S[4 * m + r] = (int)((uint32_t)acc[m][0][r] + (HI ? (uint32_t)acc[m][1][r] << 8 : 0u) + (uint32_t)a.kbias);
      }
    }
    const int64_t k0 = ti * 512 + 8 * vlane;
    if (k0 < a.opf) {
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
          const int64_t ac = (int64_t)(((uint64_t)((int64_t)((uint64_t)(int64_t)S[i] << (a.ls + a.ka)) >> a.ka)) & a.am);   // wrap to ACC_TYPE
          int64_t qv = (int64_t)((uint64_t)((ac + a.rnd) >> a.rs) << a.ls2);
          qv = qv < a.lo ? a.lo : (qv > a.hi ? a.hi : qv);
          ov[i] = (int64_t)(((uint64_t)((int64_t)((uint64_t)qv << a.ko) >> a.ko)) & a.om);
        }
      }
      if (a.vec_ok) {
        if (a.out_eb == 1) {
          const uint32_t p01 = __builtin_amdgcn_perm((uint32_t)ov[1], (uint32_t)ov[0], 0x0c0c0400u), p23 = __builtin_amdgcn_perm((uint32_t)ov[3], (uint32_t)ov[2], 0x04000c0cu);
          const uint32_t p45 = __builtin_amdgcn_perm((uint32_t)ov[5], (uint32_t)ov[4], 0x0c0c0400u), p67 = __builtin_amdgcn_perm((uint32_t)ov[7], (uint32_t)ov[6], 0x04000c0cu);
          const v2u_s8 v = {p01 | p23, p45 | p67};
          __builtin_nontemporal_store(v, reinterpret_cast<v2u_s8 *>((unsigned char *)a.y + yb));
        } else if (a.out_eb == 2) {
          const v4u_s8 v = {__builtin_amdgcn_perm((uint32_t)ov[1], (uint32_t)ov[0], 0x05040100u), __builtin_amdgcn_perm((uint32_t)ov[3], (uint32_t)ov[2], 0x05040100u),
                            __builtin_amdgcn_perm((uint32_t)ov[5], (uint32_t)ov[4], 0x05040100u), __builtin_amdgcn_perm((uint32_t)ov[7], (uint32_t)ov[6], 0x05040100u)};
          __builtin_nontemporal_store(v, reinterpret_cast<v4u_s8 *>((int16_t *)a.y + yb));
        } else if (a.out_eb == 4) {
          v4u_s8 *w = reinterpret_cast<v4u_s8 *>((int32_t *)a.y + yb);
          const v4u_s8 v0 = {(uint32_t)ov[0], (uint32_t)ov[1], (uint32_t)ov[2], (uint32_t)ov[3]}, v1 = {(uint32_t)ov[4], (uint32_t)ov[5], (uint32_t)ov[6], (uint32_t)ov[7]};
          __builtin_nontemporal_store(v0, w);
          __builtin_nontemporal_store(v1, w + 1);
        } else {
          v4u_s8 *w = reinterpret_cast<v4u_s8 *>((int64_t *)a.y + yb);
#pragma unroll
          for (int i = 0; i < 8; i += 2) {
            const v4u_s8 v = {(uint32_t)ov[i], (uint32_t)((uint64_t)ov[i] >> 32), (uint32_t)ov[i + 1], (uint32_t)((uint64_t)ov[i + 1] >> 32)};
            __builtin_nontemporal_store(v, w + i / 2);
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          if (k0 + i < a.opf) { store_raw(a.y, yb + i, a.out_eb, ov[i]); }
        }
      }
    }
  };
  Tile T[kS8Ahead];
#pragma unroll
  for (int j = 0; j < kS8Ahead; j++) {
    T[j].mv = make_uint4(0, 0, 0, 0);
    T[j].fxl = T[j].fxr = 0;
  }
#pragma unroll
  for (int j = 0; j < kS8Ahead; j++) { fetch(T[j]); }
  for (int it = 0; it < n_my; it += kS8Ahead) {
#pragma unroll
    for (int j = 0; j < kS8Ahead; j++) {
      if (j == 0 || it + j < n_my) { process(T[j]); }
    }
  }
}

}  // namespace

// NB x HI x CV32 x EDGE (MvCall::inst; plan_s8 in mv_avg_plan.hip decides)
#define ACDSP_MV_S8(NB, HI) {{NB, HI, true, true}, mv_avg_s8_kernel<NB, HI, true, true>}, {{NB, HI, true, false}, mv_avg_s8_kernel<NB, HI, true, false>}, \
                            {{NB, HI, false, true}, mv_avg_s8_kernel<NB, HI, false, true>}, {{NB, HI, false, false}, mv_avg_s8_kernel<NB, HI, false, false>}
static const MvInst<void (*)(MvS8Args)> kS8Kernels[] = {ACDSP_MV_S8(1, true), ACDSP_MV_S8(1, false), ACDSP_MV_S8(2, true), ACDSP_MV_S8(2, false)};
#undef ACDSP_MV_S8

hipError_t launch_mv_avg_s8(const MvCall &c, hipStream_t s) { return mv_launch(kS8Kernels, c, s, c.a.s8); }

}  // namespace acdsp
