// mv_avg_plan.hpp -- the host side of ac_mv_avg in two stages (mv_avg_plan.hip decides; mv_avg.hip / mv_avg_s8.hip own the kernels and launch):
// a set plan per acdsp_mvavg_set_coeffs (what the descriptor and the coefficient set decide) and a call plan per run (set plan + the call's rows +
// the environment knobs -> path, kernel instantiation, grid, arguments).  Neither makes a HIP call; launch_mv_avg launches a call plan.
#pragma once
#include "fir_kernels.hpp"

namespace acdsp {
// The argument structs of the kernels.  Unnamed namespace on purpose: a kernel's symbol name carries its argument type, and the kernels keep the
// names they had when these structs lived in their units.  Every unit that names MvSetPlan / MvCall takes them from THIS header and no unit may
// define or change one of its own: the units' copies are distinct types to the language and have to stay the same bytes.
namespace {
struct MvStreamArgs {   // mv_avg_stream_kernel (mv_avg.hip)
  int16_t c16[66];            // coefficients, zero padded (pairs (c[2q], c[2q+1]) are the v_dot2 operands of even outputs)
  int16_t c16o[66];           // the same behind one zero: pairs (c[2q-1], c[2q]) for odd outputs, whose windows start in a high half
  int32_t taps, h, hb, off, mode, nxg;
  int32_t linear, ls, e, rnd_e;
  int32_t pk16;               // 32-bit epilogue into a signed 16-bit AC_SAT output at aligned frames: saturating packs
  int32_t cv32, s32, r32, lo32, hi32, ko32;   // 32-bit epilogue: q = (S + r32) >> s32, clamp, wrap (ko32 = 32 - W_out or 0)
  int32_t ka, rs, ls2, ko;    // 64-bit epilogue (see IdConv in intg_dump.hip)
  uint64_t am, om;
  int64_t rnd, lo, hi;
  int32_t out_eb, vec_ok, run_ok;   // vec_ok: every lane's eight outputs are an aligned 16 / 32 / 64 bytes; else run_ok: tiles leave through the image as aligned pieces
  int64_t n_sample, n_frames, opf, in_stride, out_stride, tpf, n_tiles, tiles_per_wave;
  const int16_t *x;
  void *y;
  int32_t xcd_map;   // XCD-affine block order (acdsp_dev.hpp: xcd_remap)
  // packed short frames (round 5, PK instantiations): pk_n = samples per frame (64 / 128 / 256; 0 = off), pk_pitch = image samples per frame
  // (n + 2 hb); the tile loads then start at the tile, not hb samples in front of it: every halo is a patch
  int32_t pk_n, pk_pitch, pk_sh;
  int32_t row_n, row_opf;   // ROW instantiations: samples / outputs per frame (the kernel's n_sample / opf are then the ROW's lengths, n_frames = 1); row_n 0: off
  // matrix-core instantiations (MF = K blocks of 64 samples): Toeplitz fragments [m][b][plane][lane] x 16 bytes (mv_avg_build_frags), and
  // 128 sum(c), what the re-biased low sample plane leaves out
  const uint32_t *frag;
  int32_t kbias;
};
struct MvW32Args {   // mv_avg_w32_kernel (mv_avg.hip)
  int32_t d, sh, linear, ls, e; int64_t rnd_e; int32_t vec_ok;
  // branch-free ACC -> OUT (CONV instantiations; IdConv's form in intg_dump.hip): wrap to ACC_TYPE, rounding shift, clamp, wrap to OUT_TYPE
  int32_t ka, rs, ls2, ko; uint64_t am, om; int64_t rnd, lo, hi;
};
struct MvS8Args {   // mv_avg_s8_kernel (mv_avg_s8.hip)
  int32_t h, hb, mode, nld;   // nld: lanes that load (32 for the tile + the 16-byte groups of the window reach)
  uint32_t flip;              // 0x80808080 on unsigned samples
  int32_t kbias;              // 128 sum(c) on unsigned samples (+ the rounding constant of the 32-bit epilogue)
  int32_t ls;                 // d - sh: the sum's weight inside ACC_TYPE
  int32_t s32, lo32, hi32, ko32;              // 32-bit epilogue: q = (S + r32) >> s32, clamp, wrap (ko32 = 32 - W_out or 0)
  int32_t ka, rs, ls2, ko;                    // 64-bit epilogue (see IdConv in intg_dump.hip)
  uint64_t am, om;
  int64_t rnd, lo, hi;
  int32_t out_eb, vec_ok;     // vec_ok: every lane's eight outputs are an aligned 8 (1-byte containers) / 16 / 32 / 64 bytes
  int64_t n_sample, n_frames, opf, in_stride, out_stride, tpf, n_tiles, tiles_per_wave;
  const unsigned char *x;
  void *y;
  const uint32_t *frag;       // [m][b][plane][lane] x 16 bytes
};

}  // namespace

constexpr int kMvTile = 256;   // outputs (and threads) per workgroup of the general kernels
// Where a fact depends on the accumulator wrapping it is the fact for a WRAPPING accumulator; the call combines it with "ACC_TYPE wraps, or
// it is provably saturation-free for this set (sat_free) and ACDSP_NO_SAT_FREE is unset".  No environment knob is read for a set plan.
struct MvSetPlan {
  MvAvgParams p;                    // the general kernels' argument with every field a call does not set (acc.O as the descriptor has it; frag_* = the fragment facts)
  int32_t sat_asks, sat_free;       // a saturating ACC_TYPE of the kind the bound is asked for / no partial sum of this set can reach its range
  int32_t cbits, fast;              // bits of the widest coefficient; order-free int64 sums: products (ACC_TYPE) w[j] * coeffs[j] inside 2^62
  int64_t sum_abs;                  // sum |c|, saturating at INT64_MAX
  int32_t c_int16, c_frag, c_int32; // every coefficient inside int16 / inside -32768 .. 32639 (what mv_avg_build_frags takes) / inside int32
  int32_t s8_ok, stream_ok, w32_ok, cv32, w32_conv;   // the family's class conditions hold (shape and knobs are the call's); CV32 of the streaming / byte kernel, CONV of the w32 kernel
  // argument templates, everything but the call's rows: the exact-cast class (d, sh, linear, ls, e, rnd_e), the ACC -> OUT constants in their 64-bit and
  // 32-bit form, the c16 / c16o tables -- each fact once, where its kernel reads it (kbias and frag of st join on the matrix cores)
  MvStreamArgs st; MvS8Args s8; MvW32Args w32;
};

struct MvCall {
  int32_t path;       // acdsp_mvavg_path, and with it the family: 0 exact order / 1 int64 sums (argument p), 2 streaming kernel / 4 on the matrix cores (a.st), 3 32-bit samples (p, a.w32), 5 byte kernel (a.s8); -1: nothing to launch
  int8_t inst[8];     // the kernel's template arguments in their order, zero padded
  dim3 grid, block;
  uint32_t lds;       // dynamic LDS bytes
  MvAvgParams p;
  union { MvW32Args w32; MvStreamArgs st; MvS8Args s8; } a;
};

// c = the set's raw words, d_coeffs / d_frag = where the handle keeps them on the device, h_frag[kMvAvgFragWords] = the fragments to upload when p.frag_nb > 0;
// rows = sp.p with x, y, the strides, n_sample, n_frames and out_per_frame of the call
MvSetPlan mv_avg_plan_set(const acdsp_mvavg_desc_t &d, int in_eb, int out_eb, const int64_t *c, const int64_t *d_coeffs, const uint32_t *d_frag, uint32_t *h_frag);
MvCall mv_avg_plan_call(const MvSetPlan &sp, const MvAvgParams &rows);
hipError_t launch_mv_avg(const MvCall &c, hipStream_t s);      // mv_avg.hip
hipError_t launch_mv_avg_s8(const MvCall &c, hipStream_t s);   // mv_avg_s8.hip (path 5)

// A family's compiled kernels as data: template arguments -> kernel.  An instantiation that is not in the table is an error, never a fall-back.
template <class K> struct MvInst { int8_t t[8]; K k; };
template <class K, size_t N, class... A>
inline hipError_t mv_launch(const MvInst<K> (&tab)[N], const MvCall &c, hipStream_t s, const A &...args) {
  for (const MvInst<K> &e : tab) {
    if (memcmp(e.t, c.inst, sizeof e.t) == 0) { hipLaunchKernelGGL(e.k, c.grid, c.block, c.lds, s, args...); return hipGetLastError(); }
  }
  return hipErrorNotSupported;
}

}  // namespace acdsp
