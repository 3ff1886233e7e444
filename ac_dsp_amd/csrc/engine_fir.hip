// engine_fir.hip -- acdsp_fir_*: the FIR classes (reference ac_fir_{const,load,prog}_coeffs.h, ac_fir_reg_share.h) behind the C ABI
#include "engine_common.hpp"

using namespace acdsp;
using namespace acdsp::eng;

// The handle-constant half of every FirParams of a handle: formats, container bytes, history length, tap order, the handle's buffers.  What a
// call adds: its rows, hist_next, t_begin, in_flip.  ACC_TYPE as the kernels see it: a saturating accumulator that cannot saturate for the
// handle's coefficient set is a wrapping one.  Wider than 64 bits: wide.hip takes ACC_TYPE / OUT_TYPE from FirWideParams, F_acc alone stays
static FirParams fir_params(const acdsp_fir *h) {
  const acdsp_fir_desc_t &d = h->d;
  FirParams k;
  memset(&k, 0, sizeof k);
  k.n_taps = d.n_taps; k.ftype = internal_ftype(d.kind, d.ftype); k.n_ch = d.n_channels; k.coeffs_per_channel = d.coeffs_per_channel;
  k.in = make_dfmt(d.in); k.cf = make_dfmt(d.coeff);
  if (h->wide) { k.acc.F = d.acc.W - d.acc.I; }
  else { k.acc = make_dfmt(d.acc); k.out = make_dfmt(d.out); }
  if (h->sat_free) { k.acc.O = ACDSP_WRAP; }
  k.in_eb = h->in_eb; k.out_eb = h->out_eb; k.hl = h->hl; k.use_rt = (h->use_rt && !h->rt_hybrid) ? 1 : 0;
  k.lossless_shift = k.acc.F - k.in.F - k.cf.F;
  k.hist = h->hist.cur(); k.coeffs = h->d_coeffs.get<int64_t>(); k.rt = fir_rt_cur(h);
  return k;
}
// ... as the int8 MFMA kernel and its class queries see them (epilogue class, register residency, MFMAs issued): the fragments hold the
// coefficients scaled by 2^cshift, so COEFF_TYPE has cshift more fraction bits there (fir_plan_i8)
static FirParams fir_cshifted(FirParams k, int cshift) { k.cf.F += cshift; k.lossless_shift -= cshift; return k; }

static inline bool fir_path_is_mfma(int p) { return p == ACDSP_PATH_MFMA_I8 || p == ACDSP_PATH_MFMA_LONG || p == ACDSP_PATH_MFMA_S8 || p == ACDSP_PATH_MFMA_GEN || p == ACDSP_PATH_MFMA_LOSSY; }
// A/B knob: the exact-order kernel for every per-tap class (no fir_lossy_kernel / fir_satacc_kernel)
static inline bool knob_no_lossy_fast() { static const bool v = getenv("ACDSP_NO_LOSSY_FAST") != nullptr; return v; }

// ---------------------------------------------------------------------------------------------
// FIR
// ---------------------------------------------------------------------------------------------
namespace acdsp {
namespace eng {
// Effective direct-form coefficients of the folded architectures (lossless paths only):
// FOLD_EVEN uses c[0..N/2-1] on both halves (ac_fir_const_coeffs.h:248-251), FOLD_ODD uses
// c[0..mid] with the centre tap alone (:265-273).  Taps the reference never reads become 0.
// ftype: kernel-side value (internal_ftype): the anti-symmetric folds of ac_fir_reg_share negate the mirrored half.
std::vector<int64_t> effective_coeffs(const int64_t *c, int N, int ftype) {
  std::vector<int64_t> e(N, 0);
  if (ftype == ACDSP_FOLD_EVEN || ftype == kRsFoldEven || ftype == kRsFoldEvenAnti) {
    const int64_t sg = ftype == kRsFoldEvenAnti ? -1 : 1;
    for (int i = 0; i < N / 2; i++) { e[i] += c[i]; e[N - 1 - i] += sg * c[i]; }
  } else if (ftype == ACDSP_FOLD_ODD || ftype == kRsFoldOdd || ftype == kRsFoldOddAnti) {
    const int64_t sg = ftype == kRsFoldOddAnti ? -1 : 1;
    int mid = (N - 1) / 2;
    for (int i = 0; i < mid; i++) { e[i] += c[i]; e[N - 1 - i] += sg * c[i]; }
    e[mid] += c[mid];
  } else {
    for (int i = 0; i < N; i++) { e[i] = c[i]; }
  }
  return e;
}

// Kernel-side tap-order code of a (class, FTYPE) pair; -1 where the reference class has no branch for the FTYPE.
int internal_ftype(int kind, int ftype) {
  if (kind != ACDSP_FIR_REG_SHARE) { return (ftype >= ACDSP_SHIFT_REG && ftype <= ACDSP_TRANSPOSED) ? ftype : -1; }
  switch (ftype) {   // ac_fir_reg_share.h:288-306
    case ACDSP_SHIFT_REG: return kRsShiftReg;
    case ACDSP_FOLD_EVEN: return kRsFoldEven;
    case ACDSP_FOLD_EVEN_ANTI: return kRsFoldEvenAnti;
    case ACDSP_FOLD_ODD: return kRsFoldOdd;
    case ACDSP_FOLD_ODD_ANTI: return kRsFoldOddAnti;
    default: return -1;
  }
}
}  // namespace eng
}  // namespace acdsp

namespace {

inline bool is_fold_odd(int ift) { return ift == ACDSP_FOLD_ODD || ift == kRsFoldOdd || ift == kRsFoldOddAnti; }

// the exact-sum shape of a descriptor, the overflow mode of ACC_TYPE left out: `sum << (fa - fi - fc)` in 64 bits, so the shift must be
// 0..63 (formats with I outside [0, W] can ask for more: those stay on the per-tap path)
bool fir_exact_shape(const acdsp_fir_desc_t &d) {
  const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I;
  bool ok = fa >= fi + fc && fa - fi - fc < 64;
  const int ift = internal_ftype(d.kind, d.ftype);
  if (is_fold_odd(ift)) {
    // the ACC_TYPE `fold` must also keep every fraction bit of the pre-add (fc < 0 would let fa >= fi + fc pass with fa < fi)
    ok = ok && fa >= fi;
    // the ACC_TYPE `fold` variable must hold x[i] +/- x[N-1-i] without wrapping (a difference needs a signed type)
    const int need_i = d.in.I + 1 + ((d.acc.S && !d.in.S) ? 1 : 0);
    ok = ok && d.acc.I >= need_i && (d.acc.S || (!d.in.S && ift != kRsFoldOddAnti));
  }
  return ok;
}

// The condition a descriptor fails for the long kernel (kFirLongMinTaps .. kFirLongMaxTaps of 16-bit samples, fir_long.hip) or, under
// ACDSP_FLAG_IN_BYTES, for the byte-sample kernel (1 .. 16384 taps on ACDSP_PATH_MFMA_S8, fir_s8.hip: the same conditions with the sample width
// taken out); nullptr when it is eligible
const char *fir_long_refusal(const acdsp_fir_desc_t &d) {
  if (d.coeffs_per_channel) { return "one coefficient set per channel"; }
  if (d.flags & ACDSP_FLAG_FORCE_GENERIC) { return "ACDSP_FLAG_FORCE_GENERIC (the exact-order kernels end at 2048 taps)"; }
  if (!(d.flags & ACDSP_FLAG_IN_BYTES) && d.in.W > 16) { return "IN_TYPE wider than 16 bits"; }
  if (d.coeff.S ? d.coeff.W > 16 : d.coeff.W > 15) { return "COEFF_TYPE wider than 16 bits signed / 15 bits unsigned"; }
  if (d.acc.W > 64 || d.out.W > 64) { return "ACC_TYPE or OUT_TYPE wider than 64 bits"; }
  if (d.ftype == ACDSP_TRANSPOSED && d.kind != ACDSP_FIR_CONST) { return "TRANSPOSED with loadable coefficients (carried reg_trans partial sums)"; }
  if (!fir_exact_shape(d)) { return "ACC_TYPE is not an exact-sum accumulator (F_acc >= F_in + F_coeff, shift below 64; FOLD_ODD: the pre-add must fit too)"; }
  return nullptr;
}

// (*in_eb / *out_eb: container bytes of the rows under the descriptor's byte flags)
int fir_validate(const acdsp_fir_desc_t &d, int *in_eb, int *out_eb) {
  if (d.kind < ACDSP_FIR_CONST || d.kind > ACDSP_FIR_REG_SHARE) { return fail(ACDSP_EINVAL, "bad FIR class %d", d.kind); }
  if (d.ftype < 0 || d.ftype > ACDSP_FOLD_ODD_ANTI) { return fail(ACDSP_EINVAL, "bad ftype %d", d.ftype); }
  if (internal_ftype(d.kind, d.ftype) < 0) {
    return fail(ACDSP_EUNSUPPORTED, d.kind == ACDSP_FIR_REG_SHARE
                    ? "ac_fir_reg_share::run() has no branch for this FTYPE (output would be an unassigned value)"
                    : "FOLD_*_ANTI: the reference run() has no branch for these (output is an unassigned value)");
  }
  if (d.n_taps < 1 || d.n_taps > kFirLongMaxTaps) { return fail(ACDSP_EUNSUPPORTED, "n_taps=%d outside 1..%d", d.n_taps, kFirLongMaxTaps); }
  if (d.n_channels < 1) { return fail(ACDSP_EINVAL, "n_channels=%d must be positive", d.n_channels); }
  if (d.n_channels > 65535) { return fail(ACDSP_EUNSUPPORTED, "n_channels=%d outside 1..65535", d.n_channels); }
  int rc;
  if ((rc = check_fmt(d.in, "IN_TYPE")) || (rc = check_fmt(d.coeff, "COEFF_TYPE")) || (rc = check_fmt(d.acc, "ACC_TYPE", 128)) ||
      (rc = check_fmt(d.out, "OUT_TYPE", 128))) {
    return rc;
  }
  // exact intermediates must hold: product, aligned sum -- 128 bits on the 64-bit paths, 256 bits on the wide path (wide.hip)
  const bool wide = d.acc.W > 64 || d.out.W > 64;
  const int limit = wide ? 250 : 125;
  int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I, fo = d.out.W - d.out.I;
  int wp = d.in.W + d.coeff.W + 2, fp = fi + fc;
  if (is_fold_odd(internal_ftype(d.kind, d.ftype))) { wp = d.acc.W + d.coeff.W + 1; fp = fa + fc; }
  int f = fp > fa ? fp : fa;
  if (wp + (f - fp) > limit || d.acc.W + (f - fa) > limit || (wide && d.acc.W + (fo > fa ? fo - fa : 0) > limit)) {
    return fail(ACDSP_EUNSUPPORTED, "type combination needs more than %d-bit intermediates", wide ? 256 : 128);
  }
  // FOLD_ODD: the ACC_TYPE `fold` of the pre-add (ac_fir_const_coeffs.h:262-269) is formed from an (in.W + 1)-bit sum shifted to ACC's fraction
  if (wide && is_fold_odd(internal_ftype(d.kind, d.ftype)) && d.in.W + 1 + (fa > fi ? fa - fi : 0) > limit) {
    return fail(ACDSP_EUNSUPPORTED, "type combination needs more than 256-bit intermediates");
  }
  if (wide && d.kind == ACDSP_FIR_REG_SHARE) { return fail(ACDSP_EUNSUPPORTED, "ac_fir_reg_share: ACC / OUT wider than 64 bits not supported"); }
  // (the int16-sample kernels have no 1-byte output tile: byte outputs of an unflagged input are the follow-up)
  if ((rc = byte_rows(nullptr, d.flags, d.in, d.out,
                      "ACDSP_FLAG_OUT_BYTES without ACDSP_FLAG_IN_BYTES: only the byte-sample kernels write 1-byte output rows (the int16-sample kernels are not done yet)",
                      in_eb, out_eb))) {
    return rc;
  }
  const bool in_bytes = (d.flags & ACDSP_FLAG_IN_BYTES) != 0;
  if (in_bytes && wide) { return fail(ACDSP_EUNSUPPORTED, "ACDSP_FLAG_IN_BYTES: ACC_TYPE or OUT_TYPE wider than 64 bits not supported"); }
  // more than 2048 taps: the long (byte samples: the byte-sample) matrix-core kernel or nothing
  const char *const why = d.n_taps > 2048 ? fir_long_refusal(d) : nullptr;
  if (why && in_bytes) { return fail(ACDSP_EUNSUPPORTED, "n_taps=%d: more than 2048 taps of byte samples run on the byte-sample matrix-core kernel only, which does not take %s", d.n_taps, why); }
  if (why) { return fail(ACDSP_EUNSUPPORTED, "n_taps=%d: more than 2048 taps run on the long matrix-core kernel only, which does not take %s", d.n_taps, why); }
  return ACDSP_OK;
}

}  // namespace

extern "C" {

int32_t acdsp_fir_create(const acdsp_fir_desc_t *desc, acdsp_fir_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  int in_eb, out_eb;
  int rc = fir_validate(*desc, &in_eb, &out_eb);
  if (rc) { return rc; }
  if ((rc = check_device(desc->device))) { return rc; }
  std::unique_ptr<acdsp_fir> h(new acdsp_fir());   // (check_device has made the device current: a failure below frees there)
  h->d = *desc;
  const bool in_bytes = (desc->flags & ACDSP_FLAG_IN_BYTES) != 0;
  h->in_eb = in_eb; h->out_eb = out_eb;
  h->wide = desc->acc.W > 64 || desc->out.W > 64;
  h->rt_eb = h->wide ? 16 : 8;
  h->hl = round_up(desc->n_taps + 15, 32);  // >= n_taps-1 for every kernel, >= n_taps+14 for the 16-aligned windows of fir_gen
  // a plan of NB K-blocks reaches 32 (NB - 1) samples back; a padded plan (fir_mfma_plan_blocks: even counts of 10 .. 32 blocks) one block
  // further than the tap count asks for.  Sized from the padded count whatever the ACDSP_NO_MID knob says, and from NB - 1, not NB:
  // round 3 grew the history of UNpadded plans too (240 taps: 288 instead of 256) and let the knob change the state geometry.
  if (h->hl < 32 * (fir_mfma_plan_blocks_padded(desc->n_taps) - 1)) { h->hl = 32 * (fir_mfma_plan_blocks_padded(desc->n_taps) - 1); }
  // reg_trans[] carries partial sums computed with the coefficients of their own time; only
  // the const-coefficient class may trade it for an input history.
  h->use_rt = desc->ftype == ACDSP_TRANSPOSED && desc->kind != ACDSP_FIR_CONST;
  const int fi = desc->in.W - desc->in.I, fc = desc->coeff.W - desc->coeff.I, fa = desc->acc.W - desc->acc.I;
  // exact-dot-product class: the kernels compute `sum << (fa - fi - fc)` in 64 bits, so the shift must be 0..63 (formats
  // with I outside [0, W] can ask for more: those stay on the per-tap path)
  static const bool no_hybrid = getenv("ACDSP_NO_RT_HYBRID") != nullptr;   // A/B knob: reg_trans on the exact-order kernel for every sample
  h->rt_hybrid = h->use_rt && !no_hybrid && !(desc->flags & ACDSP_FLAG_FORCE_GENERIC) && (desc->in.S || desc->in.W <= 15) && desc->acc.O == ACDSP_WRAP && fa >= fi + fc && fa - fi - fc < 64 && !h->wide;
  h->rt_since = desc->n_taps - 1;   // an all-zero state carries no coefficients
  const bool lossless = fir_exact_shape(*desc) && (!h->use_rt || h->rt_hybrid) && !h->wide;   // (the overflow mode: below)
  h->lossless_shape = lossless;
  h->long_shape = !in_bytes && desc->n_taps >= kFirLongMinTaps && fir_long_refusal(*desc) == nullptr;
  h->s8_shape = in_bytes && fir_long_refusal(*desc) == nullptr;
  if (h->s8_shape && h->hl < 32 * (long_blocks(desc->n_taps) - 1)) { return fail(ACDSP_EHIP, "internal: history of %d samples is shorter than the byte-sample kernel's reach", h->hl); }
  // the long kernel's first step reaches 32 (NB - 1) samples back
  if (h->long_shape && h->hl < 32 * (long_blocks(desc->n_taps) - 1)) { return fail(ACDSP_EHIP, "internal: history of %d samples is shorter than the long kernel's reach", h->hl); }
  h->sat_free = false;
  h->lossless = lossless && desc->acc.O == ACDSP_WRAP;
  h->coeffs_set = false;
  h->path = ACDSP_PATH_GENERIC;
  const size_t n_sets = desc->coeffs_per_channel ? (size_t)desc->n_channels : 1;
  int nbk = fir_mfma_plan_blocks(desc->n_taps);
  if (h->s8_shape && nbk < long_blocks(desc->n_taps)) { nbk = long_blocks(desc->n_taps); }   // (one tap: two K-blocks there)
  if ((rc = h->hist.init(desc->n_channels, h->hl, h->in_eb))) { return rc; }
  for (DevBuf &rt : h->d_rt) {
    if (h->use_rt && (rc = rt.alloc_zeroed((size_t)desc->n_channels * desc->n_taps * h->rt_eb))) { return rc; }
  }
  if ((rc = h->d_coeffs.alloc(n_sets * desc->n_taps * sizeof(int64_t))) ||
      (rc = h->d_frag.alloc(n_sets * sizeof(uint32_t) * 2 * (size_t)(nbk > 0 ? nbk : 1) * 64 * 4)) ||
      (rc = h->d_corr.alloc(n_sets * sizeof(int64_t))) ||
      (rc = h->d_gfrag.alloc(kGenFragWords * sizeof(uint32_t))) ||
      (rc = h->d_lzcl.alloc(kLossyTabWords * sizeof(uint32_t))) ||
      (rc = h->tm.init())) {
    return rc;
  }
  *out = h.release();
  if (trace_handles()) { fprintf(stderr, "[acdsp] fir_create kind=%d ftype=%d n_taps=%d n_channels=%d\n", desc->kind, desc->ftype, desc->n_taps, desc->n_channels); }
  return ACDSP_OK;
}

int32_t acdsp_fir_destroy(acdsp_fir_t h) {
  if (!h) { return ACDSP_OK; }
  if (trace_handles()) { fprintf(stderr, "[acdsp] fir_destroy kernel_runs=%lld\n", (long long)h->n_runs); }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

// rt_hybrid: reg_trans[] of every channel from the input history and the coefficients in d_coeffs (the reference's recurrence unrolled
// in time: fir_rt_update_kernel with the history as a call of hl >= n_taps samples, so that no older partial sum enters).  Synchronous.
}  // extern "C" (C++ linkage: the state blobs of engine.hip call it)
namespace acdsp {
namespace eng {
int32_t fir_rt_from_hist(acdsp_fir *h) {
  FirParams k = fir_params(h);   // (rt_hybrid: k.rt = d_rt[cur_rt], and never wide)
  k.use_rt = 1;
  k.x = h->hist.cur(); k.in_stride = h->hl; k.n = h->hl;
  const hipError_t e = launch_fir_rt_update(k, h->d_rt[h->cur_rt ^ 1].get<int64_t>(), nullptr);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "reg_trans rebuild failed: %s", hipGetErrorString(e)); }
  HIP_TRY(hipDeviceSynchronize());
  h->cur_rt ^= 1;
  h->rt_valid = true;
  return ACDSP_OK;
}
}  // namespace eng
}  // namespace acdsp

// ---- acdsp_fir_set_coeffs: the saturation-free proof and one planner per kernel class (their answers: kTaken / kNotThisClass / an error) ----
// The coefficient sets of one set_coeffs call as the planners see them
struct FirSets {
  const int64_t *raw;          // [n][n_taps] raw words as handed in
  size_t n;                    // 1, or one set per channel
  std::vector<int64_t> eff;    // [n][n_taps] effective direct-form taps (effective_coeffs)
  std::vector<int64_t> sum;    // [n] their sums (32768 * sum rides in the correction constant of re-biased unsigned samples)
};

// Saturating accumulators: |every partial sum, in any order| <= sum|c| max|x| (the folds' pre-added pairs included: effective_coeffs lists
// both taps of a pair), plus one LSB per tap where a tap's product is quantised.  Inside the type's SYMMETRIC range the three saturating
// modes never act and equal AC_WRAP.  Signed accumulators, no carried partial sums (reg_trans), at most 64 bits.  ACDSP_NO_SAT_FREE: A/B knob.
static bool fir_sat_free(const acdsp_fir *h, const FirSets &cs) {
  const acdsp_fir_desc_t &d = h->d;
  const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I;
  bool sf = !knob_no_sat_free() && d.acc.O != ACDSP_WRAP && d.acc.S && !h->wide && !h->use_rt && d.acc.W >= 2 && d.acc.W <= 64 &&
            (fa >= fi + fc ? fa - fi - fc < 64 : ((d.acc.Q == ACDSP_TRN || d.acc.Q == ACDSP_RND) && fi + fc - fa < 64));
  if (sf && is_fold_odd(internal_ftype(d.kind, d.ftype))) {   // the `fold` pre-add variable is an ACC_TYPE too
    const int need_i = d.in.I + 1 + (!d.in.S ? 1 : 0);
    sf = fa >= fi && d.acc.I >= need_i;
  }
  for (size_t st = 0; st < cs.n && sf; st++) {
    const unsigned __int128 sa = sum_abs(cs.eff.data() + st * d.n_taps, (size_t)d.n_taps);
    sf = fa >= fi + fc ? sat_free_bound(sa, d.in, d.acc, fa - fi - fc, 0, 0) : sat_free_bound(sa, d.in, d.acc, 0, fi + fc - fa, (size_t)d.n_taps + 1);
  }
  return sf;
}

// unsigned 16-bit samples go through the int8 MFMA and long kernels as x - 32768 (acdsp_fir::in_flip)
static bool fir_flip(const acdsp_fir *h) {
  static const bool no_flip = getenv("ACDSP_NO_UNSIGNED16") != nullptr;   // A/B knob: unsigned 16-bit samples stay on the exact-sum VALU kernel
  return !h->d.in.S && h->d.in.W == 16 && (!no_flip || h->long_shape) && !h->use_rt;   // (the long kernel has no other way to take them)
}

// The shapes the int8 MFMA, gen and lossy classes admit, whatever the taps' values (byte samples and long: s8_shape / long_shape of create)
static bool fir_i8_shape(const acdsp_fir *h) {
  const acdsp_fir_desc_t &d = h->d;
  const bool i16_in = d.in.W <= 15 || (d.in.W == 16 && (d.in.S || fir_flip(h)));
  const bool i16_cf = d.coeff.S ? d.coeff.W <= 16 : d.coeff.W <= 15;
  return h->lossless && !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && i16_in && i16_cf && h->in_eb == 2 && fir_mfma_plan_blocks(d.n_taps) <= fir_mfma_max_blocks();
}
static bool fir_gen_shape(const acdsp_fir *h) {
  const acdsp_fir_desc_t &d = h->d;
  return h->lossless && !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && !d.coeffs_per_channel && !knob_no_gen() &&
         (h->in_eb == 2 || h->in_eb == 4 || h->in_eb == 8) && fits_container(d.in, h->in_eb);
}
// (FOLD_ODD holds the pre-add in an ACC_TYPE variable (ac_fir_prog_coeffs.h:213-227): exact when ACC keeps the sample's fraction bits and
// cannot wrap on the sum of two samples, and the product c * fold then drops the same s bits as an unfolded tap)
static bool fir_lossy_shape(const acdsp_fir *h, const FirParams &kq) {
  const acdsp_fir_desc_t &d = h->d;
  static const bool no_lz = getenv("ACDSP_NO_MFMA_LOSSY") != nullptr;        // A/B knob: class B stays on the VALU kernels
  // 16-bit types: fir_lossy_kernel (int32 VALU, 12 instructions per tap and four outputs) serves them too; the matrix-core kernel needs 6
  // (measured 1.7 - 1.8 x faster at 63 / 127 taps, profiles/r5_shapes.txt) and goes first; ACDSP_LOSSY16_FIRST restores round 4's choice (A/B knob)
  static const bool lz_first = getenv("ACDSP_LOSSY16_FIRST") == nullptr;
  const int fi = kq.in.F, fa = kq.acc.F, sbits = fi + kq.cf.F - fa;
  bool ok = !no_lz && !knob_no_gen() && !h->wide && !h->lossless && !h->use_rt && !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && !d.coeffs_per_channel &&
            (d.acc.O == ACDSP_WRAP || h->sat_free) && (d.acc.Q == ACDSP_TRN || d.acc.Q == ACDSP_RND) && d.acc.S && d.acc.W <= 64 && sbits >= 1 && sbits <= 15 &&
            (h->in_eb == 2 || h->in_eb == 4) && fits_container(d.in, h->in_eb) &&
            (lz_first || !fir_lossy_fast_ok(kq));
  if (ok && is_fold_odd(kq.ftype)) {
    const int need_i = d.in.I + 1 + ((d.acc.S && !d.in.S) ? 1 : 0);
    ok = fa >= fi && d.acc.I >= need_i;
  }
  return ok;
}

// Exclusivity (the comment at acdsp_fir's plan members): does a class BEHIND `path` in the planner order admit the handle's shape as well?  gen
// is not asked against the int8 MFMA and long classes: it is their fall-back and admits their shapes by design.
static bool fir_second_class_admits(const acdsp_fir *h, int path, const FirParams &kq) {
  if (path == ACDSP_PATH_MFMA_LOSSY) { return false; }   // (nothing stands behind it)
  if (path == ACDSP_PATH_MFMA_S8 && (h->long_shape || fir_i8_shape(h) || fir_gen_shape(h))) { return true; }
  if (path == ACDSP_PATH_MFMA_LONG && fir_i8_shape(h)) { return true; }
  return fir_lossy_shape(h, kq);
}

// byte samples (ACDSP_FLAG_IN_BYTES): one sample plane on fir_s8.hip for every tap count; above 2048 taps nothing else exists
static int fir_plan_s8(acdsp_fir *h, const FirSets &cs) {
  if (!h->s8_shape) { return kNotThisClass; }
  const acdsp_fir_desc_t &d = h->d;
  FirLongPlan lp;
  int64_t sa = 0;
  const int r = long_or_nothing("n_taps=", d.n_taps, h->lossless, h->d_frag, h->d_corr, [&](std::vector<uint32_t> *frag, int64_t *corr) {
    if (!long_plan_blocks(cs.eff.data(), d.n_taps, &lp, frag, &sa)) { return false; }
    if (d.in.S) { lp.corr = 0; }   // (128 * sum(c) undoes the x - 128 of UNSIGNED samples; signed ones are the B operand as they are)
    *corr = lp.corr;
    return true;
  });
  if (r == kTaken) { h->lplan = lp; h->s8_sum_abs = sa; }
  return r;
}

// 1026 .. 16384 taps: the split of the int8 class on the long kernel (fir_long.hip), whatever the epilogue class.  Above 2048 taps nothing else
// exists: a set that cannot go there is refused, and the handle stays without a set.
static int fir_plan_long(acdsp_fir *h, const FirSets &cs) {
  if (!h->long_shape) { return kNotThisClass; }
  const acdsp_fir_desc_t &d = h->d;
  const bool flip = fir_flip(h);
  FirLongPlan lp;
  const int r = long_or_nothing("n_taps=", d.n_taps, h->lossless, h->d_frag, h->d_corr, [&](std::vector<uint32_t> *frag, int64_t *corr) {
    if (!fir_long_plan(cs.eff.data(), d.n_taps, &lp, frag)) { return false; }
    if (flip) { lp.corr += 32768 * cs.sum[0]; }   // + 32768 * sum(c): the samples go through the kernel as x - 32768
    *corr = lp.corr;
    return true;
  });
  if (r == kTaken) { h->lplan = lp; h->in_flip = flip; }
  return r;
}

// up to 1025 taps of 16-bit types: the int8 split on fir_mfma.hip, one plan per coefficient set
static int fir_plan_i8(acdsp_fir *h, const FirSets &cs) {
  if (!fir_i8_shape(h)) { return kNotThisClass; }
  const acdsp_fir_desc_t &d = h->d;
  const bool flip = fir_flip(h);
  const size_t per_set = (size_t)2 * fir_mfma_plan_blocks(d.n_taps) * 64 * 4;
  std::vector<uint32_t> frag(cs.n * per_set, 0u);
  std::vector<int64_t> corr(cs.n, 0), sc((size_t)d.n_taps);
  FirMfmaPlan worst;
  bool ok = true;
  // cshift: the sets go through the kernel scaled by 2^cshift (see below); one attempt with the shift the formats ask for, one without
  auto build = [&](int cshift) {
    std::fill(frag.begin(), frag.end(), 0u);
    memset(&worst, 0, sizeof worst);
    ok = true;
    for (size_t st = 0; st < cs.n && ok; st++) {
      for (int i = 0; i < d.n_taps; i++) { sc[i] = (int64_t)((uint64_t)cs.eff[st * d.n_taps + i] << cshift); }
      FirMfmaPlan pl;
      ok = fir_mfma_build_fragments(sc.data(), d.n_taps, &pl, frag.data() + st * per_set);
      if (!ok) { break; }
      if (flip) {   // + 32768 * sum(c): the samples go through the kernel as x - 32768
        pl.corr += 32768 * (int64_t)((uint64_t)cs.sum[st] << cshift);
        // the kernel sees signed 16-bit samples (|x| <= 2^15) but the recombined sum is the UNSIGNED dot product, |y| <= 65535 * sum|c|:
        // the no-wrap proof of the fast epilogues (fir_mfma_epilogue_class: sum_abs * x_max against ACC's range) must use that bound
        pl.sum_abs *= 2;
      }
      corr[st] = pl.corr;
      worst.nb = pl.nb;
      worst.hi_mask |= pl.hi_mask; worst.lo_mask |= pl.lo_mask;
      if (pl.sum_abs > worst.sum_abs) { worst.sum_abs = pl.sum_abs; }
      if (pl.sum_abs_hi > worst.sum_abs_hi) { worst.sum_abs_hi = pl.sum_abs_hi; }
      if (pl.sum_abs_lo > worst.sum_abs_lo) { worst.sum_abs_lo = pl.sum_abs_lo; }
      const int64_t ca = pl.corr < 0 ? -pl.corr : pl.corr, wa = worst.corr < 0 ? -worst.corr : worst.corr;
      if (st == 0 || ca > wa) { worst.corr = pl.corr; }
    }
  };
  // Narrow types (<8,1> samples and coefficients into an <8,1> output: 7 dropped bits) leave the 32-bit epilogue classes less than one bit
  // to shift by once the 16 - W_out bits of the packed finish are taken off (fir_mfma_epilogue_class: rse >= 1), and ran the generic
  // epilogue with element-wise stores (0.18 of the roofline).  The sum is linear in the set: the fragments are built from c << cshift and the
  // kernel is told F_coeff + cshift -- every bound scales with it, and the classes are asked again with the scaled plan.
  h->mfma_cshift = 0;
  const int nar_d = (h->out_eb == 2 && d.out.W >= 2 && d.out.W < 16) ? 16 - d.out.W : 0;
  const int rse = (d.in.W - d.in.I) + (d.coeff.W - d.coeff.I) - (d.out.W - d.out.I) - nar_d;
  static const bool no_cshift = getenv("ACDSP_NO_CSHIFT") != nullptr;   // A/B knob
  const int want = (h->out_eb == 2 && rse < 1 && rse > -14 && !no_cshift) ? 1 - rse : 0;
  if (want > 0) {
    build(want);
    const int epi = ok ? fir_mfma_epilogue_class(fir_cshifted(fir_params(h), want), worst) : 0;
    if (epi == 1 || epi == 2) { h->mfma_cshift = want; }
  }
  if (!h->mfma_cshift) { build(0); }
  if (ok && d.coeffs_per_channel && worst.nb > fir_mfma_max_reg_blocks()) {
    // a set per channel needs the register-resident kernels: beyond 9 K-blocks only band-limited sets with the fast int16 epilogue
    ok = fir_mfma_register_resident(fir_cshifted(fir_params(h), h->mfma_cshift), worst);
  }
  if (!ok) { return kNotThisClass; }
  int rc;
  if ((rc = h->d_frag.upload(frag.data(), frag.size() * sizeof(uint32_t))) || (rc = h->d_corr.upload(corr.data(), corr.size() * sizeof(int64_t)))) { return rc; }
  h->plan = worst;
  h->in_flip = flip;
  return kTaken;
}

// wide inputs (more than 16 bits) / other misses of the int8 and long classes: generalised multi-plane MFMA kernel
static int fir_plan_gen(acdsp_fir *h, const FirSets &cs) {
  if (!fir_gen_shape(h)) { return kNotThisClass; }
  std::vector<uint32_t> gfrag;
  if (!fir_gen_plan(cs.eff.data(), h->d.n_taps, 1, 0, &h->gplan, &gfrag)) { return kNotThisClass; }
  const int rc = h->d_gfrag.upload(gfrag.data(), gfrag.size() * sizeof(uint32_t));
  return rc ? rc : kTaken;
}

// Class B (lossy accumulator, AC_TRN / AC_RND into AC_WRAP) on the matrix cores: sum_k Q(p_k) = (sum_k p_k + N h - sum_k ((p_k + h) mod 2^s)) >> s.
// The exact sum is class A on the effective taps; the residues need the low s bits of every (folded) sample and coefficient (fir_gen_kernels.hpp: fir_gen_ring_kernel, LZ).
static int fir_plan_lossy(acdsp_fir *h, const FirSets &cs, const FirParams &kq) {
  if (!fir_lossy_shape(h, kq)) { return kNotThisClass; }
  const acdsp_fir_desc_t &d = h->d;
  const int ift = kq.ftype, sbits = kq.in.F + kq.cf.F - kq.acc.F;
  const bool fold_odd = is_fold_odd(ift), fold_even = ift == ACDSP_FOLD_EVEN || ift == kRsFoldEven || ift == kRsFoldEvenAnti;
  const bool anti = ift == kRsFoldEvenAnti || ift == kRsFoldOddAnti;
  const int n_pair = fold_odd ? (d.n_taps - 1) / 2 : (fold_even ? d.n_taps / 2 : 0);
  const int n_single = fold_odd ? 1 : (fold_even ? 0 : d.n_taps);
  std::vector<uint32_t> gfrag, tab;
  if (n_pair + n_single < 1 || !fir_gen_plan(cs.eff.data(), d.n_taps, 1, 0, &h->gplan, &gfrag)) { return kNotThisClass; }
  // the exact sum must not leave int64 (the shift by s follows it), unless ACC_TYPE only keeps bits that survive a wrap of 2^64
  const int xb = d.in.W - (d.in.S ? 1 : 0);
  const bool bounded = h->gplan.sum_abs_h < (int64_t(1) << 61) && xb <= 61 && h->gplan.sum_abs_h <= ((int64_t(1) << 61) >> xb);
  int acc_bits = d.acc.W;       // |acc| <= sum|c| 2^xb / 2^s + 1 when the sum is bounded: lets a 64-bit ACC_TYPE round into OUT_TYPE in int64
  if (bounded) {
    int sb = 0;
    while (sb < 62 && (int64_t(1) << sb) <= h->gplan.sum_abs_h) { sb++; }
    const int vb = sb + xb - sbits + 2;
    if (vb < acc_bits) { acc_bits = vb < 2 ? 2 : vb; }
  }
  const int single0 = fold_odd ? (d.n_taps - 1) / 2 : 0;
  if (!(d.acc.W + sbits <= 64 || bounded) || !fir_gen_lossy_shape_ok(kq, h->gplan, acc_bits) ||
      !fir_gen_lossy_table(h->gplan, cs.raw, d.n_taps, n_pair, n_single, single0, anti ? 1 : 0, sbits, d.acc.Q == ACDSP_RND, &h->lzp, &tab)) {
    return kNotThisClass;
  }
  h->lzp.d_tab = h->d_lzcl.get<uint32_t>(); h->lzp.acc_bits = acc_bits;
  int rc;
  if ((rc = h->d_gfrag.upload(gfrag.data(), gfrag.size() * sizeof(uint32_t))) || (rc = h->d_lzcl.upload(tab.data(), tab.size() * sizeof(uint32_t)))) { return rc; }
  return kTaken;
}

extern "C" {

int32_t acdsp_fir_set_coeffs(acdsp_fir_t h, const int64_t *coeffs) {
  if (!h || !coeffs) { return fail(ACDSP_EINVAL, "null argument"); }
  const acdsp_fir_desc_t &d = h->d;
  if (d.kind == ACDSP_FIR_CONST && h->coeffs_set && d.ftype == ACDSP_TRANSPOSED) { return fail(ACDSP_ESTATE, "const-coefficient TRANSPOSED filter: coefficients are bound once"); }
  int rc = check_device(d.device);
  if (rc) { return rc; }
  const size_t n_sets = d.coeffs_per_channel ? (size_t)d.n_channels : 1;
  const acdsp::DFmt cf = make_dfmt(d.coeff);
  for (size_t i = 0; i < n_sets * d.n_taps; i++) {
    if (coeffs[i] < cf.lo || coeffs[i] > cf.hi) { return fail(ACDSP_EINVAL, "coefficient %zu = %lld is not a COEFF_TYPE raw word", i, (long long)coeffs[i]); }
  }
  // the same set again (ac_fir_prog_coeffs hands its coefficients to every one-sample call): nothing changes, no state event
  if (h->coeffs_set && h->h_coeffs.size() == n_sets * d.n_taps && memcmp(h->h_coeffs.data(), coeffs, n_sets * d.n_taps * sizeof(int64_t)) == 0) { return ACDSP_OK; }
  // Kernels of earlier run() calls may still be reading d_coeffs / d_frag.
  HIP_TRY(hipDeviceSynchronize());
  if (h->rt_hybrid && h->coeffs_set) {
    // a change mid-stream: the partial sums of the next n_taps - 1 outputs keep the OLD coefficients' products (ac_fir_load_coeffs.h:265-278)
    if (!h->rt_valid && (rc = fir_rt_from_hist(h))) { return rc; }
    h->rt_since = 0;
  }
  // from here on the device side changes: a failure below must not leave the OLD set looking current (the early return above compares
  // against h_coeffs), so the handle is without a set until the call succeeds
  h->coeffs_set = false;
  h->h_coeffs.clear();
  if ((rc = h->d_coeffs.upload(coeffs, n_sets * d.n_taps * sizeof(int64_t)))) { return rc; }
  h->in_flip = false;
  FirSets cs = {coeffs, n_sets, {}, {}};
  for (size_t st = 0; st < n_sets; st++) {
    const std::vector<int64_t> e = effective_coeffs(coeffs + st * d.n_taps, d.n_taps, internal_ftype(d.kind, d.ftype));
    cs.eff.insert(cs.eff.end(), e.begin(), e.end());
    cs.sum.push_back(0);
    for (int64_t v : e) { cs.sum[st] += v; }
  }
  h->sat_free = fir_sat_free(h, cs);
  h->lossless = h->lossless_shape && (d.acc.O == ACDSP_WRAP || h->sat_free);
  const FirParams kq = fir_params(h);   // (behind sat_free: ACC_TYPE as the kernels see it)
  // the planners in priority order; the first that takes the set names the path
  int path = ACDSP_PATH_MFMA_S8, r = fir_plan_s8(h, cs);
  if (r == kNotThisClass) { path = ACDSP_PATH_MFMA_LONG; r = fir_plan_long(h, cs); }
  if (r == kNotThisClass) { path = ACDSP_PATH_MFMA_I8; r = fir_plan_i8(h, cs); }
  if (r == kNotThisClass) { path = ACDSP_PATH_MFMA_GEN; r = fir_plan_gen(h, cs); }
  if (r == kNotThisClass) { path = ACDSP_PATH_MFMA_LOSSY; r = fir_plan_lossy(h, cs, kq); }
  if (r > 0) { return r; }
  if (r == kTaken && fir_second_class_admits(h, path, kq)) { return fail(ACDSP_EHIP, "internal: a second kernel class admits the coefficient set that path %d took", path); }
  h->path = h->wide ? ACDSP_PATH_WIDE
            : r == kTaken ? path
                          : ((h->lossless && !(d.flags & ACDSP_FLAG_FORCE_GENERIC)) ? ACDSP_PATH_LOSSLESS64 : ACDSP_PATH_GENERIC);
  h->kclass = h->path;
  if (h->path == ACDSP_PATH_GENERIC && !knob_no_lossy_fast() && !(d.flags & ACDSP_FLAG_FORCE_GENERIC)) {
    h->kclass = fir_lossy_fast_ok(kq) ? ACDSP_KCLASS_LOSSY16 : (fir_satacc_fast_ok(kq) ? ACDSP_KCLASS_SATACC16 : ACDSP_PATH_GENERIC);
  }
  h->coeffs_set = true;
  h->h_coeffs.assign(coeffs, coeffs + n_sets * d.n_taps);
  return ACDSP_OK;
}

int32_t acdsp_fir_clone(acdsp_fir_t h, acdsp_fir_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_fir_t c = nullptr;
  int rc = acdsp_fir_create(&h->d, &c);
  if (rc) { return rc; }
  if (h->coeffs_set && (rc = acdsp_fir_set_coeffs(c, h->h_coeffs.data()))) { acdsp_fir_destroy(c); return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = c->hist.copy_from(h->hist))) { return rc; }
  if (h->use_rt) {
    HIP_TRY(hipMemcpy(c->d_rt[0].get(), fir_rt_cur(h), (size_t)h->d.n_channels * h->d.n_taps * h->rt_eb, hipMemcpyDeviceToDevice));
  }
  c->cur_rt = 0; c->rt_valid = h->rt_valid; c->rt_since = h->rt_since;
  *out = c;
  return ACDSP_OK;
}

int32_t acdsp_fir_path(acdsp_fir_t h) { return h ? h->path : -1; }
int32_t acdsp_fir_kernel_class(acdsp_fir_t h) { return (h && h->coeffs_set) ? h->kclass : -1; }

}  // extern "C"

// Do the matrix-core kernels take the caller's rows as they are (acdsp_fir_run: else fir_gen reads an aligned staging image of them)?
static bool fir_rows_aligned(const acdsp_fir *h, const void *d_in, int64_t in_stride, int64_t n) {
  static const bool aligned_only = getenv("ACDSP_ALIGNED_ONLY") != nullptr;   // A/B knob: the round-2 behaviour
  const int path = h->path;
  // byte rows (fir_s8.hip) may start anywhere: a row must be readable up to the next multiple of 16 samples = 16 bytes
  if (path == ACDSP_PATH_MFMA_S8) { return in_stride >= (n + 15) / 16 * 16; }
  // the int8 and long kernels take any element-aligned row that is readable up to the next multiple of 8 samples; fir_gen wants whole slots
  if (path == ACDSP_PATH_MFMA_I8 || path == ACDSP_PATH_MFMA_LONG) { return rows_vec_aligned(d_in, in_stride, h->in_eb) || (!aligned_only && in_stride >= (n + 7) / 8 * 8); }
  return rows_in_slots(d_in, in_stride, h->in_eb, n);
}

// What acdsp_fir_run refuses while its stream is capturing, decided before the call touches the stream or the handle
int acdsp::eng::fir_capture_check(const acdsp_fir *h, const void *d_in, int64_t in_stride, int64_t n) {
  if (h->rt_hybrid) {
    const int64_t m_rt = (int64_t)h->d.n_taps - 1 - h->rt_since;
    if (m_rt > 0 && n > 0) {
      return fail(ACDSP_ESTATE, "fir_run under graph capture: a TRANSPOSED filter within n_taps - 1 samples of a coefficient change keeps host-side state; run %lld more samples before capturing", (long long)m_rt);
    }
  }
  if (fir_path_is_mfma(h->path) && !fir_rows_aligned(h, d_in, in_stride, n)) {
    // rows the matrix-core kernels do not take as they are go through the aligned staging image, which is allocated on growth
    const size_t need = (size_t)h->d.n_channels * ((n + 15) / 16 * 16) * h->in_eb;
    if (need > h->st.cap_in) {
      return fail(ACDSP_ESTATE, "fir_run under graph capture: these rows need the aligned staging image (%zu bytes, %zu allocated) and a captured call "
                  "cannot allocate; run one eager call of this shape before capturing, or lay the rows out on 16-byte boundaries", need, h->st.cap_in);
    }
  }
  return ACDSP_OK;
}

extern "C" {

int32_t acdsp_fir_run(acdsp_fir_t h, const void *d_in, int64_t in_stride, int64_t n, void *d_out, int64_t out_stride,
                      void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n < 0 || (n > 0 && (!d_in || !d_out || in_stride < n || out_stride < n))) {
    return fail(ACDSP_EINVAL, "fir_run: bad buffer arguments");
  }
  if (!h->coeffs_set) { return fail(ACDSP_ESTATE, "fir_run before acdsp_fir_set_coeffs"); }
  if (n == 0) { return ACDSP_OK; }
  const acdsp_fir_desc_t &d = h->d;
  int rc = check_device(d.device);
  if (rc) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  const bool capturing = stream_is_capturing(s);
  if (capturing && (rc = fir_capture_check(h, d_in, in_stride, n))) { return rc; }
  FirParams k = fir_params(h);
  const bool hyb = h->rt_hybrid;
  k.in_stride = in_stride; k.out_stride = out_stride; k.n = n; k.x = d_in; k.y = d_out;
  // rt_hybrid: the first m outputs still carry partial sums of the previous coefficient set
  int64_t m_rt = 0;
  if (hyb) {
    m_rt = (int64_t)d.n_taps - 1 - h->rt_since;
    m_rt = m_rt < 0 ? 0 : (m_rt > n ? n : m_rt);
  }

  int path = h->path;
  if (h->wide) {
    FirWideParams kw;
    kw.p = k; kw.acc = make_wfmt(d.acc); kw.out = make_wfmt(d.out); kw.rt = h->d_rt[h->hist.index()].get();
    HIP_TRY(hipEventRecord(h->tm.start(), s));
    hipError_t ew = launch_fir_wide(kw, s);
    if (ew != hipSuccess) { return fail(ACDSP_EHIP, "wide FIR kernel launch failed: %s", hipGetErrorString(ew)); }
    HIP_TRY(hipEventRecord(h->tm.stop(), s));
    h->tm.commit();
    const int nxw = h->hist.next(!h->use_rt && k.n >= k.hl);
    ew = h->use_rt ? launch_fir_wide_rt_update(kw, h->d_rt[nxw].get(), s) : launch_fir_hist_update(k, h->hist.at(nxw), s);
    if (ew != hipSuccess) { return fail(ACDSP_EHIP, "wide FIR state kernel launch failed: %s", hipGetErrorString(ew)); }
    h->hist.commit(nxw);
    return ACDSP_OK;
  }
  FirParams kraw = k;   // the state kernels always see the caller's samples
  const bool flipped = h->in_flip;   // (set by the planners of ACDSP_PATH_MFMA_I8 and ACDSP_PATH_MFMA_LONG alone)
  if (flipped) {
    // unsigned 16-bit samples: the kernel flips the top bit of every sample as it splits the rows and the history into byte planes
    // (FirParams::in_flip; round 4 and the first half of round 5 wrote a flipped image of both first: a second pass over the call's input,
    // 0.21 - 0.33 of the roofline where the signed types run at 0.55)
    k.in_flip = 1;
    k.in.S = 1; k.in.lo = -32768; k.in.hi = 32767;
  }
  if (fir_path_is_mfma(path)) {
    // The matrix-core kernels read rows with 16-byte vector loads (fir_gen: in whole 16-sample slots).  gfx950 serves a vector
    // access at any ELEMENT-aligned address, so the int8 kernel takes unaligned rows as they are (round 3: a row stride of 2^20 + 3
    // samples costs +12 %, profiles/r3_unaligned.txt; the staging copy below -- hipMemcpy2DAsync of misaligned rows -- cost 6.4 ms
    // per 2 GB, 7 x the filter itself) as long as a row is readable up to the next multiple of 8 samples.  fir_gen still wants
    // whole aligned slots: rows that are not laid out that way are first copied, on the device, into an aligned staging image.
    const bool aligned = fir_rows_aligned(h, d_in, in_stride, n);
    if (!aligned) {
      const int64_t si = (n + 15) / 16 * 16;
      if ((rc = h->st.ensure((size_t)d.n_channels * si * h->in_eb, 0))) { return rc; }   // (under capture: large enough already, fir_capture_check)
      if (capturing) { h->st.captured = true; }
      HIP_TRY(hipMemcpy2DAsync(h->st.d_in.get(), (size_t)si * h->in_eb, d_in, (size_t)in_stride * h->in_eb, (size_t)n * h->in_eb,
                               (size_t)d.n_channels, hipMemcpyDeviceToDevice, s));
      k.x = h->st.d_in.get(); k.in_stride = si;
    }
  }
  // Small calls (the drop-in run() of one channel; ac_fir_prog_coeffs is ONE sample per call, reference ac_fir_prog_coeffs.h:281)
  // are launch-bound: no timing events, and the exact-order kernels write the next history themselves -- one launch per call.
  const bool small = h->small_call;
  const bool fuse_hist = small && !flipped && (!h->use_rt || hyb) && (path == ACDSP_PATH_LOSSLESS64 || path == ACDSP_PATH_GENERIC ||
                                                (path == ACDSP_PATH_MFMA_I8 && !h->mfma_cshift && fir_mfma_register_resident(k, h->plan)));   // single-wave workgroups
  const int nxt_fused = h->hist.next(false);
  if (fuse_hist) { k.hist_next = h->hist.at(nxt_fused); }
  if (!small) { HIP_TRY(hipEventRecord(h->tm.start(), s)); }
  hipError_t e;
  if (path == ACDSP_PATH_MFMA_I8) {
    // (the fragments hold c << mfma_cshift: the kernel's shifts follow; the state kernels below keep the handle's formats)
    e = launch_fir_mfma(fir_cshifted(k, h->mfma_cshift), h->plan, d.coeffs_per_channel, h->d_frag.get<uint32_t>(), h->d_corr.get<int64_t>(), s);
  }
  else if (path == ACDSP_PATH_MFMA_LONG) { e = launch_fir_long(k, h->lplan, h->d_frag.get<uint32_t>(), h->d_corr.get<int64_t>(), s); }
  else if (path == ACDSP_PATH_MFMA_S8) { e = launch_fir_s8(k, h->lplan, h->s8_sum_abs, h->d_frag.get<uint32_t>(), h->d_corr.get<int64_t>(), s); }
  else if (path == ACDSP_PATH_MFMA_GEN) { e = launch_fir_gen(k, h->gplan, h->d_gfrag.get<uint32_t>(), 0, 0, 0, n, s); }
  else if (path == ACDSP_PATH_MFMA_LOSSY) {
    // complete chunks on the matrix cores, the ragged rest (and calls shorter than a chunk) on the exact-order kernel
    int64_t cov = 0;
    e = launch_fir_gen(k, h->gplan, h->d_gfrag.get<uint32_t>(), 0, 0, 0, n, s, &h->lzp, &cov);
    if (e == hipSuccess && cov < n) { FirParams kt = k; kt.t_begin = cov; e = launch_fir_generic(kt, s); }
  }
  else if (path == ACDSP_PATH_LOSSLESS64) { e = launch_fir_lossless64(k, s); }
  else {
    const bool no_lossy = knob_no_lossy_fast();
    e = (!no_lossy && fir_lossy_fast_ok(k)) ? launch_fir_lossy(k, s) : ((!no_lossy && fir_satacc_fast_ok(k)) ? launch_fir_satacc(k, s) : launch_fir_generic(k, s));
  }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "FIR kernel launch failed: %s", hipGetErrorString(e)); }
  h->n_runs++;
  if (!small) {
    HIP_TRY(hipEventRecord(h->tm.stop(), s));
    h->tm.commit();
  }
  if (hyb) {
    if (m_rt > 0) {
      // exact-order pass over the call's first m samples, on reg_trans, behind the main kernel (it overwrites those outputs)
      FirParams kt = k;
      kt.use_rt = 1; kt.n = m_rt; kt.hist_next = nullptr;
      e = launch_fir_generic(kt, s);
      if (e == hipSuccess && m_rt == n) { e = launch_fir_rt_update(kt, h->d_rt[h->cur_rt ^ 1].get<int64_t>(), s); }
      if (e != hipSuccess) { return fail(ACDSP_EHIP, "FIR reg_trans kernel launch failed: %s", hipGetErrorString(e)); }
      if (m_rt == n) { h->cur_rt ^= 1; h->rt_valid = true; } else { h->rt_valid = false; }   // past the transition reg_trans is rebuilt on demand
    } else {
      h->rt_valid = false;
    }
    h->rt_since = h->rt_since + n >= (int64_t)d.n_taps - 1 ? (int64_t)d.n_taps - 1 : h->rt_since + n;
  }
  if (fuse_hist) { h->hist.commit(nxt_fused); return ACDSP_OK; }
  // state carry.  A call of at least hl samples takes the new history from its input alone: written in place behind the
  // main kernel (same stream), no buffer flip -- the handle's host-side state is then the same after every call, which is what
  // lets any schedule of such calls be captured into a HIP graph.  Shorter calls (and reg_trans, which reads its old value)
  // go into the other buffer, then flip.
  const int nxt = h->hist.next((!h->use_rt || hyb) && k.n >= k.hl);
  if (h->use_rt && !hyb) {
    e = launch_fir_rt_update(k, h->d_rt[nxt].get<int64_t>(), s);
  } else {
    e = launch_fir_hist_update(flipped ? kraw : k, h->hist.at(nxt), s);
  }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "FIR state kernel launch failed: %s", hipGetErrorString(e)); }
  h->hist.commit(nxt);
  return ACDSP_OK;
}

int32_t acdsp_fir_run_host(acdsp_fir_t h, const void *h_in, int64_t n, void *h_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n < 0 || (n > 0 && (!h_in || !h_out))) { return fail(ACDSP_EINVAL, "fir_run_host: bad arguments"); }
  if (n == 0) { return ACDSP_OK; }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  const int64_t stride = (n + 15) / 16 * 16;  // rows 16-byte aligned and readable in whole 16-sample slots
  const HostRows r = {h->d.n_channels, h_in, n, stride, h->in_eb, h_out, n, stride, n, h->out_eb};
  return run_host_staged(h->st, r, true, [&](const void *d_in, void *d_out, bool pinned) {
    h->small_call = pinned;
    const int rc_run = acdsp_fir_run(h, d_in, stride, n, d_out, stride, nullptr);
    h->small_call = false;
    return rc_run;
  });
}

int32_t acdsp_fir_reset(acdsp_fir_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->hist.zero())) { return rc; }
  for (DevBuf &rt : h->d_rt) {
    if (rt && (rc = rt.zero((size_t)h->d.n_channels * h->d.n_taps * h->rt_eb))) { return rc; }
  }
  h->rt_valid = true; h->rt_since = h->d.n_taps - 1;
  return ACDSP_OK;
}

int32_t acdsp_fir_last_kernel_ms(acdsp_fir_t h, float *ms) {
  if (!h || !ms) { return fail(ACDSP_EINVAL, "null argument"); }
  return h->tm.stats(1, ms, nullptr);
}

int32_t acdsp_fir_kernel_stats(acdsp_fir_t h, int32_t last_k, float *avg_ms, float *min_ms) {
  if (!h) { return fail(ACDSP_EINVAL, "null argument"); }
  return h->tm.stats(last_k, avg_ms, min_ms);
}

int32_t acdsp_fir_mfma_epilogue(acdsp_fir_t h) {
  if (!h || !h->coeffs_set || h->path != ACDSP_PATH_MFMA_I8) { return -1; }
  return fir_mfma_epilogue_class(fir_cshifted(fir_params(h), h->mfma_cshift), h->plan) | (h->mfma_cshift << 8) | (h->in_flip ? 1 << 16 : 0);
}

int32_t acdsp_fir_mfma_issued(acdsp_fir_t h, int32_t *per_1024_samples) {
  if (!h || !per_1024_samples) { return fail(ACDSP_EINVAL, "null argument"); }
  if (!h->coeffs_set) { return fail(ACDSP_ESTATE, "acdsp_fir_mfma_issued before acdsp_fir_set_coeffs"); }
  *per_1024_samples = 0;
  if (h->path == ACDSP_PATH_MFMA_I8) {
    *per_1024_samples = fir_mfma_issued_per_step(fir_cshifted(fir_params(h), h->mfma_cshift), h->plan);
  } else if (h->path == ACDSP_PATH_MFMA_LONG) {
    *per_1024_samples = fir_long_issued_per_step(h->lplan);
  } else if (h->path == ACDSP_PATH_MFMA_S8) {
    *per_1024_samples = fir_s8_issued_per_step(h->lplan);
  }
  return ACDSP_OK;
}

int32_t acdsp_fir_in_elem_bytes(acdsp_fir_t h) { return h ? h->in_eb : -1; }
int32_t acdsp_fir_out_elem_bytes(acdsp_fir_t h) { return h ? h->out_eb : -1; }

}  // extern "C"

