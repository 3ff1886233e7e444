// mv_avg_plan.hip -- what ac_mv_avg decides on the host (mv_avg_plan.hpp): set plan, call plan, Toeplitz fragments.  No kernel here, and no HIP call.
#include "engine_common.hpp"
#include "mv_avg_plan.hpp"

namespace acdsp {
namespace {

// The family's environment knobs, read by the call plan where the decision they belong to is reached.  A/B knobs, once per process:
inline bool knob_no_stream() { static const bool v = getenv("ACDSP_NO_MVAVG_STREAM") != nullptr; return v; }
inline bool knob_no_w32() { static const bool v = getenv("ACDSP_NO_MVAVG_W32") != nullptr; return v; }
inline bool knob_no_pk16() { static const bool v = getenv("ACDSP_NO_MVAVG_PK16") != nullptr; return v; }
inline bool knob_no_run() { static const bool v = getenv("ACDSP_NO_MVAVG_RUN") != nullptr; return v; }   // element stores for unaligned output frames
inline bool knob_no_pack() { static const bool v = getenv("ACDSP_NO_MVAVG_PACK") != nullptr; return v; }
inline bool knob_no_row() { static const bool v = getenv("ACDSP_NO_MVAVG_ROW") != nullptr; return v; }
// ... tuning knobs (re-read per launch under ACDSP_TUNE_LIVE; ACDSP_NO_SAT_FREE: engine_common.hpp, ACDSP_XCD_MAP: acdsp_dev.hpp).  The smallest window that takes the matrix cores (0: never)
// (same box, 512 objects x 2^20, frames of 1024: v_dot2 0.68 / MFMA 0.62 of the roofline at 9 taps, 0.57 / 0.62 at 11, 0.46 / 0.61 at 33, 0.29 / 0.53 at
// 65; AC_WIN 0.54 / 0.58 at 9 taps -- profiles/r6_mvavg_mfma.txt)
inline int knob_mfma_min(int win_mode) { ACDSP_TUNE_ENV(e, "ACDSP_MVAVG_MFMA_MIN"); return e ? atoi(e) : (win_mode == 0 ? 9 : 11); }
// the longest window that walks the output row (longer ones: matrix cores, frame-relative)
// (same box, 512 objects x 2^20 in frames of 1024: 9 taps 0.54 frame-relative v_dot2 / 0.59 matrix cores / 0.69 row walk; 17 taps 0.62 / 0.61 / 0.62; 25 taps
// 0.55 / 0.59 / 0.55; 33 taps 0.50 / 0.61 / 0.49 -- the v_dot2 form is VALU-bound from 17 taps on, where the walk buys nothing)
inline int knob_roww_max() { ACDSP_TUNE_ENV(e, "ACDSP_MVAVG_ROWW_MAX"); return e ? atoi(e) : 9; }
// tiles per wave, on the 16-bit and the byte kernel (tests/test_mvavg_bytes_gpu.py walks runs of tiles with it); one once-only read per kernel, as there always was
template <class Args> inline int64_t knob_tpw(int64_t dflt) { ACDSP_TUNE_ENV(e, "ACDSP_MVAVG_TPW"); return e && atoi(e) > 0 ? atoi(e) : dflt; }

inline bool trn_or_rnd(const DFmt &f) { return f.Q == ACDSP_TRN || f.Q == ACDSP_RND; }
// The exact-cast class of the fast kernels, for a wrapping accumulator: the cast of a sample to ACC_TYPE is exact, d = F_acc - F_in >= 0, sh = F_coeff >= 0,
// AC_TRN / AC_RND; d >= sh ("linear"): the products add up unshifted and the sum weighs 2^ls, else every product drops e bits (rnd_e rounds them).
// What differs between the kernels: the linear class only (byte kernel), sums and conversions in 32 / 64-bit words (narrow: W_acc <= 61, ls < W_acc;
// not the 32-bit sliding window), the bits a product may drop
// (k: the class as the w32 kernel's argument spells it -- d, sh, linear, ls, e, rnd_e; false: outside the class, k half filled)
bool cast_class(const MvAvgParams &p, bool linear_only, bool narrow, int e_max, MvW32Args &k) {
  k.d = p.acc.F - p.in.F; k.sh = p.cf.F;
  const int i_in = p.in.W - p.in.F, i_acc = p.acc.W - p.acc.F;
  if (k.d < 0 || k.sh < 0 || (linear_only && k.d < k.sh) || !trn_or_rnd(p.acc)) { return false; }
  if (p.in.S ? (!p.acc.S || i_acc < i_in) : (i_acc < i_in + (p.acc.S ? 1 : 0))) { return false; }   // the cast (ACC_TYPE) w[j] is exact
  k.linear = k.d >= k.sh; k.ls = k.linear ? k.d - k.sh : 0; k.e = k.linear ? 0 : k.sh - k.d;
  if (k.e > e_max || k.ls > 62 || (narrow && (p.acc.W > 61 || k.ls >= p.acc.W))) { return false; }
  k.rnd_e = (!k.linear && p.acc.Q == ACDSP_RND) ? (int64_t(1) << (k.e - 1)) : 0;
  return true;
}

// ACC -> OUT without branches, 64-bit form (IdConv's in intg_dump.hip): wrap to ACC_TYPE, rounding shift, clamp, wrap to OUT_TYPE; into any kernel's argument
template <class Args> void put_conv64(Args &a, const DFmt &acc, const DFmt &out) {
  const int rs = acc.F - out.F;
  a.ka = 64 - acc.W; a.am = acc.S ? ~uint64_t(0) : (~uint64_t(0) >> (64 - acc.W));
  a.rs = rs > 0 ? rs : 0; a.ls2 = rs < 0 ? -rs : 0;
  a.rnd = (out.Q == ACDSP_RND && rs > 0 && rs < 64) ? (int64_t)(uint64_t(1) << (rs - 1)) : 0;   // (rs > 60: no kernel takes the form)
  if (out.O == ACDSP_SAT) { a.lo = out.lo; a.hi = out.hi; a.ko = 0; a.om = ~uint64_t(0); }
  else { a.lo = INT64_MIN; a.hi = INT64_MAX; a.ko = 64 - out.W; a.om = out.S ? ~uint64_t(0) : (~uint64_t(0) >> (64 - out.W)); }
}
// ... 32-bit form, q = (S + r32) >> s32, clamp, wrap: the accumulator cannot wrap (signed, W_acc >= sum bits + 1 + ls) and the output shift swallows ls;
// |sum| <= sum|c| * 2^(W_in - 1) (signed samples) or sum|c| * 2^W_in (unsigned): samples narrower than 16 bits need a narrower accumulator.  Returns CV32 (0: nothing written)
template <class Args> int put_conv32(Args &a, const MvAvgParams &p, int64_t sum_abs, int32_t *r32) {
  int rs = p.acc.F - p.out.F, sum_bits = 0;
  while (sum_bits < 62 && (int64_t(1) << sum_bits) <= sum_abs * (int64_t(1) << (p.in.W - (p.in.S ? 1 : 0)))) { sum_bits++; }   // |sum| < 2^sum_bits
  if (!(p.acc.S && p.acc.W >= sum_bits + 1 + a.ls && rs >= a.ls && rs - a.ls <= 30 && (p.out.S || p.out.W <= 31))) { return 0; }
  a.s32 = rs - a.ls; *r32 = (p.out.Q == ACDSP_RND && a.s32 > 0) ? (1 << (a.s32 - 1)) : 0;
  const bool sat = p.out.O == ACDSP_SAT;
  a.lo32 = sat && p.out.lo > INT32_MIN ? (int32_t)p.out.lo : INT32_MIN; a.hi32 = sat && p.out.hi < INT32_MAX ? (int32_t)p.out.hi : INT32_MAX;
  a.ko32 = !sat && p.out.W < 32 ? 32 - p.out.W : 0;
  return 1;
}
// what the streaming and the byte kernel share of a set: window geometry (halo rounded up to gran samples) and both epilogues; returns CV32
template <class Args> int put_class(Args &a, const MvSetPlan &sp, int ls, int gran, int32_t *r32) {
  a.h = sp.p.taps / 2; a.mode = sp.p.win_mode; a.hb = a.mode == 0 ? 0 : gran * ((a.h + gran - 1) / gran);
  a.ls = ls; a.out_eb = sp.p.out_eb; put_conv64(a, sp.p.acc, sp.p.out);
  return put_conv32(a, sp.p, sp.sum_abs, r32);
}
// the call's rows as the tile walkers take them: frames in 512-output tiles
template <class Args> void put_rows(Args &a, const MvAvgParams &p) {
  a.n_sample = p.n_sample; a.n_frames = p.n_frames; a.opf = p.out_per_frame; a.in_stride = p.in_stride; a.out_stride = p.out_stride;
  a.tpf = (p.out_per_frame + 511) / 512; a.n_tiles = (int64_t)p.n_obj * p.n_frames * a.tpf;
  a.x = (decltype(a.x))p.x; a.y = p.y;
}
// ... and their grid: four waves per workgroup, a.tiles_per_wave tiles each (spans of 16 KB once the call is large enough); false: more workgroups than a grid holds
template <class Args> bool wave_grid(Args &a, int64_t tpw, MvCall &c) {
  for (a.tiles_per_wave = tpw; a.tiles_per_wave > 1 && a.n_tiles / a.tiles_per_wave < 16384;) { a.tiles_per_wave /= 2; }
  a.tiles_per_wave = knob_tpw<Args>(a.tiles_per_wave);
  const int64_t blocks = ((a.n_tiles + a.tiles_per_wave - 1) / a.tiles_per_wave + 3) / 4;
  c.grid = dim3((unsigned)blocks); return blocks <= 0x7FFFFFFF;
}
void set_inst(MvCall &c, int path, std::initializer_list<int> t) {
  c.path = path;
  for (size_t i = 0; i < t.size(); i++) { c.inst[i] = (int8_t)t.begin()[i]; }
}

// Class and shape conditions of mv_avg_s8_kernel (see the header of mv_avg_s8.hip)
bool plan_s8(const MvSetPlan &sp, bool wraps, MvCall &c) {
  const MvAvgParams &p = c.p;
  if (!sp.s8_ok || !wraps) { return false; }
  if (p.n_sample < p.taps || p.n_sample % 16 != 0 || p.in_stride % 16 != 0 || ((uintptr_t)p.x % 16) != 0) { return false; }
  MvS8Args &a = c.a.s8; memcpy(&a, &sp.s8, sizeof a);
  a.vec_ok = p.out_per_frame % 8 == 0 && p.out_stride % 8 == 0 && ((uintptr_t)p.y % (p.out_eb == 1 ? 8 : 16)) == 0 /* what a lane's first store must be aligned to */ &&
             (p.out_eb == 1 || p.out_eb == 2 || p.out_eb == 4 || p.out_eb == 8);
  put_rows(a, p);
  if (!wave_grid(a, 32, c)) { return false; }   // 32 tiles: 16 KB spans, as the 16-bit kernel walks
  set_inst(c, 5, {p.frag_nb, p.frag_hi, sp.cv32, a.mode != 0});   // NB, HI, CV32, EDGE
  return true;
}

// Class and shape conditions of the streaming kernel (see mv_avg.hip)
bool plan_stream(const MvSetPlan &sp, bool wraps, MvCall &c) {
  const MvAvgParams &p = c.p;
  if (knob_no_stream() || !sp.stream_ok || !wraps) { return false; }
  if (p.n_sample < p.taps || p.n_sample % 8 != 0 || p.in_stride % 8 != 0 || ((uintptr_t)p.x % 16) != 0) { return false; }
  MvStreamArgs &a = c.a.st; memcpy(&a, &sp.st, sizeof a);
  a.vec_ok = p.out_per_frame % 8 == 0 && p.out_stride % 8 == 0 && ((uintptr_t)p.y % 16) == 0;
  const bool no_pk16 = knob_no_pk16(), no_run = knob_no_run();
  a.pk16 = !no_pk16 && a.cv32 && a.vec_ok && p.out_eb == 2 && a.lo32 == -32768 && a.hi32 == 32767 && a.ko32 == 0 && a.om == ~uint64_t(0);
  a.run_ok = !a.vec_ok && !no_run && ((uintptr_t)p.y % p.out_eb) == 0 && p.out_eb <= 4;   // (8-byte outputs: 4 KB + the offset would not fit the image; they keep element stores, 64 contiguous bytes per lane)
  put_rows(a, p);
  const auto one_frame = [&](int64_t opf) {   // the ROW is walked as one frame of opf outputs
    a.n_sample = p.n_sample * p.n_frames; a.n_frames = 1; a.opf = opf; a.tpf = (opf + 511) / 512; a.n_tiles = (int64_t)p.n_obj * a.tpf;
  };
  // Frames shorter than a 512-output tile (round 5: 128-sample frames used 16 of a wave's 64 lanes, 0.21 of the roofline): with AC_CLIP /
  // AC_MIRROR every output of a frame depends on that frame's samples only, frames lie back to back in the row, so a tile takes 512 / n whole
  // frames -- each in its own slot of the LDS image, both halos patched from the staged samples -- and the row is walked as ONE frame.
  if (!knob_no_pack() && p.win_mode != 0 && (p.n_sample == 64 || p.n_sample == 128 || p.n_sample == 256) && p.n_frames % (512 / p.n_sample) == 0) {
    a.pk_n = (int32_t)p.n_sample; a.pk_pitch = a.pk_n + 2 * a.hb; a.pk_sh = p.n_sample == 64 ? 6 : (p.n_sample == 128 ? 7 : 8);
    a.nxg = 0; one_frame(p.n_sample * p.n_frames);   // (a multiple of 512)
    a.run_ok = 0;   // (packed tiles keep element stores when the output row is off the boundary)
  }
  const bool no_row = knob_no_row();
  // windows of 17 taps and more: the sums on the matrix cores (fragments built with the set plan: mv_avg_build_frags)
  const int mf_min = knob_mfma_min(p.win_mode);
  const bool mf_wanted = p.frag && p.frag_nb > 0 && a.linear && mf_min > 0 && p.taps >= mf_min;
  const bool row_fits = a.vec_ok && p.n_sample * p.n_frames < (int64_t(1) << 31) - 1024;   // (both row walks: aligned outputs, 32-bit positions)
  // Frames that are no multiple of the 512-output tile (round 6: frames of 1000 samples at 0.57 where 1024 run 0.68).  Frame-relative tiles start wherever
  // their frame starts: every 1 KB store run and load straddles cache lines, and the frame's last tile is partly empty.  With AC_CLIP / AC_MIRROR input
  // and output positions of a row coincide, so the tiles can walk the ROW in aligned 512-output steps and take the frame edges where they fall: at most
  // one edge per tile image (frames of at least 512 + 2 hb samples), the samples behind it shifted by a gap of 2 hb that holds both halos (ROW instantiations).
  if (!no_row && !a.pk_n && !mf_wanted && p.win_mode != 0 && p.n_sample % 512 != 0 && p.n_sample >= 512 + 2 * a.hb && row_fits) {
    a.row_n = (int32_t)p.n_sample;
    one_frame(p.n_sample * p.n_frames);
  }
  // ... and AC_WIN (ROW 2): N - TAPS + 1 outputs per frame lie back to back in the output row while their windows jump TAPS - 1 samples at every frame
  // edge.  Where both are multiples of 8 (TAPS = 9, 17, 25 ...: the windows stay aligned) the tiles walk the OUTPUT row; the image is the contiguous input
  // and the lanes behind the edge start TAPS - 1 samples further on.
  const int roww_max = knob_roww_max();
  if (!no_row && p.win_mode == 0 && p.taps <= roww_max && p.taps > 1 && (p.taps - 1) % 8 == 0 && p.out_per_frame >= 512 && p.out_per_frame % 512 != 0 && row_fits) {
    a.row_n = (int32_t)p.n_sample; a.row_opf = (int32_t)p.out_per_frame;
    one_frame(p.out_per_frame * p.n_frames);
    a.nxg += (p.taps - 1) / 8;
  }
  if (!wave_grid(a, 16, c)) { return false; }   // 16 KB spans (8 / 16 tiles alike, 32: -5 %, 64: -9 %: profiles/r3_span_sweep.txt)
  a.xcd_map = (xcd_map_wanted(false) && c.grid.x % 8 == 0) ? 1 : 0;
  // template arguments NR, LINEAR, CV32, EDGE, PK, MF, RUN, ROW
  if (mf_wanted && !a.pk_n && !a.row_n) {
    a.frag = p.frag;
    a.kbias = (int32_t)(128 * p.frag_csum);
    // (NR = 9: only REGION -- how far the right-edge patches reach into the image -- depends on it here)
    set_inst(c, 4, {9, 1, a.cv32, a.mode != 0, 0, p.frag_nb, a.run_ok, 0});
    return true;
  }
  const int nr = p.taps <= 9 ? 2 : (p.taps <= 17 ? 3 : (p.taps <= 25 ? 4 : (p.taps <= 33 ? 5 : (p.taps <= 49 ? 7 : 9))));   // taps <= 8 NR - 7
  if (a.pk_n) { set_inst(c, 2, {nr, a.linear, a.cv32, 1, 1, 0, 0, 0}); }
  else if (a.row_n) { set_inst(c, 2, {nr, a.linear, a.cv32, a.row_opf ? 0 : 1, 0, 0, 0, a.row_opf ? 2 : 1}); }
  else { set_inst(c, 2, {nr, a.linear, a.cv32, a.mode != 0, 0, 0, a.run_ok, 0}); }
  return true;
}

// mv_avg_w32_kernel's class and shape conditions
bool plan_w32(const MvSetPlan &sp, bool wraps, MvCall &c) {
  const MvAvgParams &p = c.p;
  if (knob_no_w32() || !sp.w32_ok || !wraps) { return false; }
  MvW32Args &a = c.a.w32; memcpy(&a, &sp.w32, sizeof a);
  a.vec_ok = p.out_per_frame % 4 == 0 && p.out_stride % 4 == 0 && ((uintptr_t)p.y % 16) == 0 && (p.out_eb == 2 || p.out_eb == 4 || p.out_eb == 8);
  const int64_t pairs = (int64_t)p.n_obj * p.n_frames;
  c.grid = dim3((unsigned)((p.out_per_frame + 1023) / 1024), (unsigned)(pairs < 65535 ? pairs : 65535));
  c.lds = (uint32_t)((size_t)(((1024 + p.taps - 1 + 3 + 4) & ~3) + p.taps) * sizeof(int32_t));   // the window dwords as the kernel pads them + the coefficients
  set_inst(c, 3, {a.linear, sp.w32_conv});   // LINEAR, CONV
  return true;
}

}  // namespace

MvSetPlan mv_avg_plan_set(const acdsp_mvavg_desc_t &d, int in_eb, int out_eb, const int64_t *c, const int64_t *d_coeffs, const uint32_t *d_frag, uint32_t *h_frag) {
  MvSetPlan sp;
  memset(&sp, 0, sizeof sp);
  MvAvgParams &p = sp.p;
  p.taps = d.taps; p.win_mode = d.win_mode; p.n_obj = d.n_objects; p.in_eb = in_eb; p.out_eb = out_eb; p.coeffs = d_coeffs;
  p.in = make_dfmt(d.in); p.cf = make_dfmt(d.coeff); p.acc = make_dfmt(d.acc); p.out = make_dfmt(d.out);
  p.force_generic = (d.flags & ACDSP_FLAG_FORCE_GENERIC) != 0;
  p.frag_gran = in_eb == 1 ? 16 : 8;   // halo granularity of the fragments: mv_avg_s8_kernel's geometry on byte rows
  int hi = 0;   // (the fragment facts: K blocks, sum of the coefficients, a high digit exists)
  p.frag_nb = mv_avg_build_frags(c, d.taps, d.win_mode, p.frag_gran, h_frag, &p.frag_csum, &hi);
  p.frag_hi = (int16_t)hi; p.frag = p.frag_nb > 0 ? d_frag : nullptr;
  // the coefficient set: range, sum |c|, bits of the widest one
  int64_t cmin = c[0], cmax = c[0];
  for (int i = 1; i < d.taps; i++) { cmin = c[i] < cmin ? c[i] : cmin; cmax = c[i] > cmax ? c[i] : cmax; }
  const uint64_t mmax = (uint64_t)(~cmin > cmax ? ~cmin : cmax);   // cmin >= 0: ~cmin < 0 <= cmax
  for (sp.cbits = 1; sp.cbits < 64 && (mmax >> (sp.cbits - 1)) != 0;) { sp.cbits++; }
  const unsigned __int128 sa = eng::sum_abs(c, (size_t)d.taps);
  sp.sum_abs = sa > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)sa;
  sp.c_int16 = cmin >= -32768 && cmax <= 32767; sp.c_frag = cmin >= -32768 && cmax <= 32639; sp.c_int32 = cmin >= INT32_MIN && cmax <= INT32_MAX;
  // A saturating ACC_TYPE that cannot saturate is a wrapping one (cf. acdsp_fir::sat_free): the cast of a sample is exact, and every partial sum
  // is bounded by sum|c| max|x| 2^d / 2^sh plus one LSB per tap, inside the type's symmetric range.  The kernels then see AC_WRAP.
  const int dc = p.acc.F - p.in.F, sh = p.cf.F;
  sp.sat_asks = d.acc.O != ACDSP_WRAP && d.acc.S && !p.force_generic && trn_or_rnd(p.acc) && d.acc.W <= 64;
  sp.sat_free = sp.sat_asks && dc >= 0 && dc < 40 && sh >= 0 && sh < 64 && d.acc.I >= d.in.I + (d.in.S ? 0 : 1) && eng::sat_free_bound(sa, d.in, d.acc, dc, sh, (size_t)d.taps + 1);
  // order-free class: products (ACC_TYPE) w[j] * coeffs[j] inside 2^62.  The cast sample has at most min(W_acc, W_in + max(F_acc - F_in, 0))
  // bits and the coefficients as many as the set on the handle needs (round 5: the bound by W_acc + W_coeff sent <32,16> samples into a
  // <56,30> accumulator to the 128-bit per-tap kernel)
  const int xbits_in = d.in.W + (d.in.S ? 0 : 1) + (dc > 0 ? dc : 0), xbits_acc = d.acc.W + (d.acc.S ? 0 : 1);
  sp.fast = !p.force_generic && trn_or_rnd(p.acc) && p.cf.F >= 0 && p.cf.F < 62 && (xbits_in < xbits_acc ? xbits_in : xbits_acc) + sp.cbits + (d.coeff.S ? 0 : 1) <= 62;
  const int rs = p.acc.F - p.out.F;
  const bool out_ok = trn_or_rnd(p.out) && (p.out.O == ACDSP_WRAP || p.out.O == ACDSP_SAT);
  const bool cv_ok = out_ok && p.out.W <= 62 && rs <= 60 && p.acc.W + (rs < 0 ? -rs : 0) <= 61;   // the 64-bit form as the streaming and the byte kernel take it
  // the streaming kernel or, on byte rows, the byte kernel: sum |c| <= 32767 keeps every intermediate inside int32 (|sum of products| < 2^30 / 2^23)
  MvW32Args k = {};
  const bool small = cast_class(p, in_eb == 1, true, 30, k) && !p.force_generic && d.taps <= 65 && sp.sum_abs <= 32767 && cv_ok;
  sp.stream_ok = small && in_eb == 2 && (p.in.S || p.in.W <= 15) && sp.c_int16;
  sp.s8_ok = small && in_eb == 1 && p.in.W <= 8 && sp.c_frag && p.frag_nb >= 1;
  if (sp.stream_ok) {
    MvStreamArgs &a = sp.st;
    for (int i = 0; i < d.taps; i++) { a.c16[i] = (int16_t)c[i]; a.c16o[i + 1] = (int16_t)c[i]; }
    a.cv32 = sp.cv32 = put_class(a, sp, k.ls, 8, &a.r32);
    a.taps = d.taps; a.off = a.hb - (d.win_mode == 0 ? 0 : a.h); a.nxg = (a.off + d.taps - 1 + 7) / 8;
    a.linear = k.linear; a.e = k.e; a.rnd_e = (int32_t)k.rnd_e;
  }
  if (sp.s8_ok) {
    MvS8Args &a = sp.s8;
    int32_t r32 = 0;
    sp.cv32 = put_class(a, sp, k.ls, 16, &r32);
    a.nld = 32 + ((d.win_mode == 0 ? 0 : a.hb - a.h) + d.taps - 1 + 15) / 16;
    a.flip = p.in.S ? 0u : 0x80808080u; a.frag = p.frag;
    a.kbias = (p.in.S ? 0 : (int32_t)(128 * p.frag_csum)) + r32;   // the rounding constant rides in the sum (|sum| < 2^24, it is <= 2^29)
  }
  // 32-bit sliding window (16-bit containers as well): coefficients inside int32.  linear: the 32 x 32-bit products add up mod 2^64 and the
  // shift comes once, after the sum; per tap: |x c| + rnd inside int64
  MvW32Args &a = sp.w32;
  sp.w32_ok = cast_class(p, false, false, 62, a) && !p.force_generic && (in_eb == 4 || in_eb == 2) && (p.in.S || p.in.W <= 31) && p.cf.F < 62 && sp.c_int32 && !(a.e > 0 && p.in.W + sp.cbits > 61);
  if (sp.w32_ok) {
    put_conv64(a, p.acc, p.out);
    // ACC -> OUT without branches where the modes and the 64-bit arithmetic allow it (the conditions of intg_dump.hip: make_conv)
    const bool wrap_o = p.out.O == ACDSP_WRAP;
    sp.w32_conv = out_ok && a.rs <= 60 && a.ls + a.ka < 64 && (a.rnd == 0 || p.acc.W <= 61) && (a.ls2 == 0 || p.acc.W + a.ls2 <= 61 || wrap_o) &&
                  (p.acc.S || p.acc.W <= 62 || (rs == 0 && wrap_o)) && (wrap_o || p.out.S ? p.out.W <= 64 : p.out.W <= 62);
  }
  return sp;
}

MvCall mv_avg_plan_call(const MvSetPlan &sp, const MvAvgParams &rows) {
  MvCall c;
  c.path = -1; c.lds = 0; c.block = dim3(256);
  memset(c.inst, 0, sizeof c.inst); memcpy(&c.p, &rows, sizeof c.p);
  MvAvgParams &p = c.p;
  const bool wraps = p.acc.O == ACDSP_WRAP || (sp.sat_asks && !eng::knob_no_sat_free() && sp.sat_free);
  if (wraps) { p.acc.O = ACDSP_WRAP; p.fast = sp.fast; }   // (p.fast is 0 in sp.p)
  if (p.out_per_frame <= 0 || p.n_frames <= 0) { return c; }
  if (p.in_eb == 1 && plan_s8(sp, wraps, c)) { return c; }   // byte rows outside its class: the container-agnostic kernels below
  if (plan_stream(sp, wraps, c) || plan_w32(sp, wraps, c)) { return c; }
  const int64_t pairs = (int64_t)p.n_obj * p.n_frames;
  c.grid = dim3((unsigned)((p.out_per_frame + kMvTile - 1) / kMvTile), (unsigned)(pairs < 65535 ? pairs : 65535)); c.block = dim3(kMvTile);
  c.lds = (uint32_t)((size_t)(kMvTile + 2 * p.taps - 1) * sizeof(int64_t));
  set_inst(c, p.fast ? 1 : 0, {p.fast});   // FAST
  return c;
}

// Toeplitz fragments of the matrix-core forms (mv_avg_stream_kernel, MF instantiations: gran = 8 samples; mv_avg_s8_kernel: gran = 16, the
// samples its 16-byte tile loads are aligned to).  The window's half length is rounded up to `gran` in front of a tile (hb; 0 under AC_WIN) and
// the window starts off = hb - TAPS / 2 samples into the image.  Returns the K blocks (1 / 2; 0: the coefficient set or the window does not
// fit) and fills out[((m nb + b) 2 + plane) 64 + lane][4 dwords]: lane (row i = lane & 15, kg = lane >> 4) holds A[i][16 kg .. 16 kg + 15] of
// K block b, A[i][kk] = digit_plane(c[64 b + kk - sigma_m(i) - off]), sigma_m(i) = 8 (i >> 2) + (i & 3) + 4 m; c = 256 ch + cl with both digits
// signed bytes (balanced: cl = int8(c & 255)), so that every product is a signed i8 x i8 one.  *hi_any: some ch is not 0 (plane 1 is needed).
int mv_avg_build_frags(const int64_t *c, int taps, int win_mode, int gran, uint32_t *out, int64_t *csum, int *hi_any) {
  const int h = taps / 2, hb = win_mode == 0 ? 0 : gran * ((h + gran - 1) / gran), off = win_mode == 0 ? 0 : hb - h;
  if (taps > 65 || 31 + off + taps - 1 >= 128) { return 0; }
  const int nb = (31 + off + taps - 1 < 64) ? 1 : 2;
  int64_t sum = 0;
  int hi = 0;
  for (int t = 0; t < taps; t++) {
    if (c[t] < -32768 || c[t] > 32639) { return 0; }   // the balanced high digit of 32640 .. 32767 is 128
    sum += c[t];
    hi |= (c[t] < -128 || c[t] > 127) ? 1 : 0;
  }
  *csum = sum;
  *hi_any = hi;
  for (int m = 0; m < 2; m++) {
    for (int b = 0; b < nb; b++) {
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 15, kg = lane >> 4, sig = 8 * (i >> 2) + (i & 3) + 4 * m;
        for (int dw = 0; dw < 4; dw++) {
          uint32_t wl = 0, wh = 0;
          for (int bj = 0; bj < 4; bj++) {
            const int t = 64 * b + 16 * kg + 4 * dw + bj - sig - off;
            const int64_t cv = (t >= 0 && t < taps) ? c[t] : 0;
            const int cl = (int)(int8_t)(uint8_t)(cv & 0xFF), ch = (int)((cv - cl) >> 8);
            wl |= (uint32_t)(uint8_t)cl << (8 * bj);
            wh |= (uint32_t)(uint8_t)ch << (8 * bj);
          }
          out[(((size_t)(m * nb + b) * 2 + 0) * 64 + lane) * 4 + dw] = wl;
          out[(((size_t)(m * nb + b) * 2 + 1) * 64 + lane) * 4 + dw] = wh;
        }
      }
    }
  }
  return nb;
}

}  // namespace acdsp
