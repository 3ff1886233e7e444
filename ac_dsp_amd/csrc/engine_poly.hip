// engine_poly.hip -- acdsp_polydec_* / acdsp_polyintr_*: ac_poly_dec and ac_poly_intr behind the C ABI
#include "engine_common.hpp"

using namespace acdsp;
using namespace acdsp::eng;

// acdsp_poly{dec,intr}_set_scratch_cap / _long_geometry: the LongScratch of a long-eligible handle (long_shape)
template <typename H>
static int poly_set_scratch_cap(H *h, uint64_t bytes) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (!h->long_shape) { return ACDSP_OK; }
  if (const int rc = check_device(h->d.device)) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  return h->scratch.size(bytes);
}
template <typename H>
static int poly_long_geometry(H *h, int64_t *slab, int32_t *group_channels, uint64_t *scratch_bytes) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  h->scratch.geometry(h->long_shape, slab, group_channels, scratch_bytes);
  return ACDSP_OK;
}

// ---------------------------------------------------------------------------------------------
// polyphase decimator
// ---------------------------------------------------------------------------------------------
// (struct acdsp_polydec: engine_common.hpp -- the polydec cascade of engine_ddc.hip reads it)

namespace {

// Long prototypes (polydec_long.hip): the condition a descriptor fails, or nullptr when it is long-eligible
const char *polydec_long_refusal(const acdsp_polydec_desc_t &d) {
  if (d.df < 1 || d.df > kPolyDecLongMaxDf) { return "DF outside 1..256"; }
  if (d.n_taps < 1 || (int64_t)d.n_taps * d.df > kPolyDecLongMaxTaps) { return "NTAPS*DF above 16384"; }
  if (d.flags & ACDSP_FLAG_FORCE_GENERIC) { return "ACDSP_FLAG_FORCE_GENERIC (the exact-order kernel ends at NTAPS*DF = 2048)"; }
  if (d.in.W > 16) { return "IN_TYPE wider than 16 bits"; }
  if (d.coeff.S ? d.coeff.W > 16 : d.coeff.W > 15) { return "COEFF_TYPE wider than 16 bits signed / 15 bits unsigned"; }
  // (ACC_TYPE / OUT_TYPE of more than 64 bits never get here: check_fmt refuses them for every ac_poly_dec shape)
  const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I;
  if (fa < fi + fc || fa - fi - fc >= 64) { return "ACC_TYPE is not an exact-sum accumulator (F_acc >= F_in + F_coeff, shift below 64)"; }
  return nullptr;
}

}  // namespace

extern "C" {

int32_t acdsp_polydec_create(const acdsp_polydec_desc_t *desc, acdsp_polydec_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  if (desc->n_taps < 1 || desc->df < 1 || (int64_t)desc->n_taps * desc->df > kPolyDecLongMaxTaps) {
    return fail(ACDSP_EUNSUPPORTED, "poly_dec: NTAPS*DF = %lld outside 1..%d", (long long)desc->n_taps * desc->df, kPolyDecLongMaxTaps);
  }
  if (desc->n_channels < 1) { return fail(ACDSP_EINVAL, "n_channels=%d must be positive", desc->n_channels); }
  if (desc->n_channels > 65535) { return fail(ACDSP_EUNSUPPORTED, "n_channels=%d outside 1..65535", desc->n_channels); }
  int rc;
  if ((rc = check_fmt(desc->in, "IN_TYPE")) || (rc = check_fmt(desc->coeff, "COEFF_TYPE")) || (rc = check_fmt(desc->acc, "ACC_TYPE")) ||
      (rc = check_fmt(desc->out, "OUT_TYPE"))) {
    return rc;
  }
  int in_eb, out_eb;
  if ((rc = byte_rows("poly_dec", desc->flags, desc->in, desc->out, nullptr, &in_eb, &out_eb))) { return rc; }
  const bool in_bytes = in_eb == 1;
  const int fi = desc->in.W - desc->in.I, fc = desc->coeff.W - desc->coeff.I, fa = desc->acc.W - desc->acc.I;
  const int f = fi + fc > fa ? fi + fc : fa;
  if (desc->in.W + desc->coeff.W + 2 + (f - fi - fc) > 125 || desc->acc.W + (f - fa) > 125) {
    return fail(ACDSP_EUNSUPPORTED, "type combination needs more than 128-bit intermediates");
  }
  // NTAPS*DF above 2048: the long matrix-core kernel or nothing
  const char *const long_why = polydec_long_refusal(*desc);
  if ((int64_t)desc->n_taps * desc->df > 2048 && long_why) {
    return fail(ACDSP_EUNSUPPORTED, "poly_dec: NTAPS*DF = %lld: more than 2048 taps run on the long matrix-core kernel only, which does not take %s",
                (long long)desc->n_taps * desc->df, long_why);
  }
  if ((rc = check_device(desc->device))) { return rc; }
  std::unique_ptr<acdsp_polydec> h(new acdsp_polydec());   // (check_device has made the device current: a failure below frees there)
  h->d = *desc;
  h->in_eb = in_eb; h->out_eb = out_eb;
  h->hl = round_up(desc->n_taps * desc->df + 15, 32);
  h->lossless_shape = fa >= fi + fc && fa - fi - fc < 64;
  h->lossless = h->lossless_shape && desc->acc.O == ACDSP_WRAP;
  if ((rc = h->hist.init(desc->n_channels, h->hl, h->in_eb)) || (rc = h->d_coeffs.alloc((size_t)desc->n_taps * desc->df * sizeof(int64_t))) ||
      (rc = h->d_gfrag.alloc(kGenFragWords * sizeof(uint32_t)))) {
    return rc;
  }
  // the long kernel takes the eligible shapes the ring kernel has no plan for (DF > 64, more than 8 K blocks): a test of the shape alone
  int g_off, g_nb;
  h->long_shape = !long_why && !fir_gen_window(desc->n_taps * desc->df, desc->df, (desc->df - 1) % 16, &g_off, &g_nb);
  if (h->long_shape) {
    // unsigned 16-bit samples: read as x - 32768, 32768 * sum(c) rides in the correction constant; unsigned bytes (ACDSP_FLAG_IN_BYTES,
    // polydec_s8.hip): read as x - 128, 128 * sum(c)
    h->in_flip = !desc->in.S && (in_bytes || desc->in.W == 16);
    // scratch: phase rows of IN containers (int16, or bytes under ACDSP_FLAG_IN_BYTES), df * in_eb bytes per slab output, in front of them the
    // reach of 32 (nb - 1) samples
    if ((rc = h->d_lfrag.alloc((size_t)2 * desc->df * long_blocks(desc->n_taps) * 64 * 4 * sizeof(uint32_t))) || (rc = h->d_lcorr.alloc(sizeof(int64_t))) ||
        (rc = h->scratch.init((uint64_t)desc->df * (uint64_t)in_eb, 32 * (uint64_t)(long_blocks(desc->n_taps) - 1), desc->n_channels))) {
      return rc;
    }
  }
  *out = h.release();
  return ACDSP_OK;
}

int32_t acdsp_polydec_destroy(acdsp_polydec_t h) {
  if (!h) { return ACDSP_OK; }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

int32_t acdsp_polydec_set_coeffs(acdsp_polydec_t h, const int64_t *coeffs) {
  if (!h || !coeffs) { return fail(ACDSP_EINVAL, "null argument"); }
  const acdsp_polydec_desc_t &d = h->d;
  int rc = check_device(d.device);
  if (rc) { return rc; }
  const int n = d.n_taps * d.df;
  const acdsp::DFmt cf = make_dfmt(d.coeff);
  for (int i = 0; i < n; i++) {
    if (coeffs[i] < cf.lo || coeffs[i] > cf.hi) { return fail(ACDSP_EINVAL, "coefficient %d = %lld is not a COEFF_TYPE raw word", i, (long long)coeffs[i]); }
  }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->d_coeffs.upload(coeffs, (size_t)n * sizeof(int64_t)))) { return rc; }
  h->gen_ok = false;
  {
    // |every partial sum of an output| <= sum|c| max|x| over all NTAPS * DF coefficients: inside the symmetric range of a signed saturating
    // ACC_TYPE the saturation never acts (ACDSP_NO_SAT_FREE: A/B knob)
    const bool sf = !knob_no_sat_free() && d.acc.O != ACDSP_WRAP && d.acc.S && h->lossless_shape && d.acc.W >= 2 && d.acc.W <= 64 &&
                    sat_free_bound(sum_abs(coeffs, (size_t)n), d.in, d.acc, (d.acc.W - d.acc.I) - (d.in.W - d.in.I) - (d.coeff.W - d.coeff.I), 0, 0);
    h->sat_free = sf;
    h->lossless = h->lossless_shape && (d.acc.O == ACDSP_WRAP || sf);
  }
  const bool in_bytes = (d.flags & ACDSP_FLAG_IN_BYTES) != 0;   // (a byte container holds every IN_TYPE the flag admits, unsigned ones re-biased)
  if (h->lossless && !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && !knob_no_gen() &&(in_bytes || fits_container(d.in, h->in_eb))) {
    // decimating FIR  y[g] = sum_k hh[k] x[g*DF + DF-1 - k],  hh[df + tp*DF] = c[tp + NTAPS*df]
    std::vector<int64_t> hh((size_t)n, 0);
    for (int df = 0; df < d.df; df++) { for (int tp = 0; tp < d.n_taps; tp++) { hh[df + tp * d.df] = coeffs[tp + d.n_taps * df]; } }
    std::vector<uint32_t> fr;
    // (unsigned bytes: the GenArgs kernels take the non-zero correction 128 * sum(c) as the sign of the re-bias -- a set whose sum is 0 mod 2^57
    // keeps the exact-order kernel)
    if (fir_gen_plan(hh.data(), n, d.df, (d.df - 1) % 16, &h->gplan, &fr) && !(in_bytes && !d.in.S && (uint64_t)h->gplan.sum_h * 128 == 0)) {
      if ((rc = h->d_gfrag.upload(fr.data(), fr.size() * sizeof(uint32_t)))) { return rc; }
      h->gen_ok = true;
    }
  }
  // Long shapes: the int8 split of polydec_long.hip.  Above 2048 taps nothing else exists: a set that cannot go there is refused, and the
  // handle stays without a set.
  h->long_ok = false;
  if (h->long_shape) {
    rc = long_or_nothing("poly_dec: NTAPS*DF = ", n, h->lossless, h->d_lfrag, h->d_lcorr, [&](std::vector<uint32_t> *fr, int64_t *corr) {
      if (!polydec_long_plan(coeffs, d.n_taps, d.df, &h->lplan, fr)) { return false; }
      int64_t sc = 0;
      for (int i = 0; i < n; i++) { sc += coeffs[i]; }
      if (in_bytes) { h->lplan.corr = h->in_flip ? 128 * sc : 0; }   // one sample plane: no low plane to re-bias
      else if (h->in_flip) { h->lplan.corr += 32768 * sc; }
      *corr = h->lplan.corr;
      return true;
    });
    h->long_ok = rc == kTaken;
    if (rc == ACDSP_EUNSUPPORTED) { h->coeffs_set = false; }   // (a refusal: the handle stays without a set)
    if (rc > 0) { return rc; }
  }
  h->coeffs_set = true;
  return ACDSP_OK;
}

int32_t acdsp_polydec_path(acdsp_polydec_t h) { return h ? h->last_path : -1; }
int32_t acdsp_polydec_in_elem_bytes(acdsp_polydec_t h) { return h ? h->in_eb : -1; }
int32_t acdsp_polydec_ring_shape(acdsp_polydec_t h) { return h ? h->last_ring : -1; }

int32_t acdsp_polydec_set_scratch_cap(acdsp_polydec_t h, uint64_t bytes) { return poly_set_scratch_cap(h, bytes); }
int32_t acdsp_polydec_long_geometry(acdsp_polydec_t h, int64_t *slab_outputs, int32_t *group_channels, uint64_t *scratch_bytes) {
  return poly_long_geometry(h, slab_outputs, group_channels, scratch_bytes);
}

int32_t acdsp_polydec_run(acdsp_polydec_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                          void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  const acdsp_polydec_desc_t &d = h->d;
  if (n_in < 0 || n_in % d.df != 0) { return fail(ACDSP_EINVAL, "poly_dec: n_in = %lld is not a multiple of DF = %d", (long long)n_in, d.df); }
  const int64_t n_out = n_in / d.df;
  if (n_in > 0 && (!d_in || !d_out || in_stride < n_in || out_stride < n_out)) { return fail(ACDSP_EINVAL, "poly_dec: bad buffer arguments"); }
  if (!h->coeffs_set) { return fail(ACDSP_ESTATE, "poly_dec run before set_coeffs"); }
  if (n_in == 0) { return ACDSP_OK; }
  int rc = check_device(d.device);
  if (rc) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  FirParams k = fir_params_of(make_dfmt(d.in), make_dfmt(d.coeff), make_dfmt(d.acc), make_dfmt(d.out), h->in_eb, h->out_eb, h->hl, d.n_channels,
                              {d_in, in_stride, n_in, d_out, out_stride});
  k.n_taps = d.n_taps * d.df; k.ftype = ACDSP_SHIFT_REG;
  if (h->sat_free) { k.acc.O = ACDSP_WRAP; }
  k.lossless_shift = k.acc.F - k.in.F - k.cf.F;
  k.hist = h->hist.cur(); k.coeffs = h->d_coeffs.get<int64_t>();
  const bool aligned = rows_in_slots(d_in, in_stride, h->in_eb, n_in);
  hipError_t e;
  h->last_ring = 0;
  if (h->long_ok) {   // every call, whatever its length or alignment
    k.in_flip = h->in_flip;
    if (h->in_eb == 1) {
      h->last_path = ACDSP_PATH_MFMA_S8;
      e = launch_polydec_s8(k, h->lplan, h->scratch.geo, h->d_lfrag.get<uint32_t>(), h->d_lcorr.get<int64_t>(), h->scratch.buf.get(), n_out, s);
    } else {
      h->last_path = ACDSP_PATH_MFMA_LONG;
      e = launch_polydec_long(k, h->lplan, h->scratch.geo, h->d_lfrag.get<uint32_t>(), h->d_lcorr.get<int64_t>(), h->scratch.buf.get(), n_out, s);
    }
  } else if (h->gen_ok && aligned) {
    h->last_path = ACDSP_PATH_MFMA_GEN;
    e = launch_fir_gen(k, h->gplan, h->d_gfrag.get<uint32_t>(), 0, 0, d.df - 1, n_out, s, nullptr, nullptr, &h->last_ring);
  } else {
    h->last_path = ACDSP_PATH_GENERIC;
    e = launch_polydec_generic(k, d.n_taps, d.df, n_out, s);
  }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "poly_dec kernel launch failed: %s", hipGetErrorString(e)); }
  const int nxt = h->hist.next(k.n >= k.hl);
  e = launch_fir_hist_update(k, h->hist.at(nxt), s);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "poly_dec state kernel launch failed: %s", hipGetErrorString(e)); }
  h->hist.commit(nxt);
  return ACDSP_OK;
}

int32_t acdsp_polydec_run_host(acdsp_polydec_t h, const void *h_in, int64_t n_in, void *h_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n_in < 0 || n_in % h->d.df != 0 || (n_in > 0 && (!h_in || !h_out))) { return fail(ACDSP_EINVAL, "poly_dec run_host: bad arguments"); }
  if (n_in == 0) { return ACDSP_OK; }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  const int64_t n_out = n_in / h->d.df;
  const HostRows r = {h->d.n_channels, h_in, n_in, (n_in + 15) / 16 * 16, h->in_eb, h_out, n_out, (n_out + 7) / 8 * 8, n_out, h->out_eb};
  return run_host_staged(h->st, r, false, [&](const void *d_in, void *d_out, bool) { return acdsp_polydec_run(h, d_in, r.si, n_in, d_out, r.so, nullptr); });
}

int32_t acdsp_polydec_reset(acdsp_polydec_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  return h->hist.zero();
}

// Deep copy (the reference object is a plain aggregate: taps[], acc, acc1[] and coeffs_t go with it, ac_poly_dec.h:132-135): descriptor,
// scratch cap, coefficients when set, input history.  Scratch and staging are the clone's own.
int32_t acdsp_polydec_clone(acdsp_polydec_t h, acdsp_polydec_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_polydec_t c = nullptr;
  int rc = acdsp_polydec_create(&h->d, &c);
  if (rc) { return rc; }
  std::unique_ptr<acdsp_polydec, int32_t (*)(acdsp_polydec_t)> guard(c, acdsp_polydec_destroy);
  if (c->long_shape && h->scratch.cap != c->scratch.cap && (rc = c->scratch.size(h->scratch.cap))) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if (h->coeffs_set) {
    std::vector<int64_t> cf((size_t)h->d.n_taps * h->d.df);
    HIP_TRY(hipMemcpy(cf.data(), h->d_coeffs.get(), cf.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if ((rc = acdsp_polydec_set_coeffs(c, cf.data()))) { return rc; }
  }
  if ((rc = c->hist.copy_from(h->hist))) { return rc; }
  c->last_path = h->last_path;
  c->last_ring = h->last_ring;
  *out = guard.release();
  return ACDSP_OK;
}

// State blob, kind 6: the newest `hl` input samples of every channel, oldest first, in IN containers (1-byte ones under ACDSP_FLAG_IN_BYTES:
// elem_bytes 1, so a flagged blob and an unflagged handle refuse each other; the reference's taps[NTAPS*DF]; acc and
// acc1[] are rebuilt by every group).  A call consumes whole groups of DF, so there is no phase to carry.
static StateHdr polydec_state_hdr(const acdsp_polydec *h) {
  StateHdr s = state_hdr(6, (uint32_t)h->d.n_channels, (uint32_t)h->in_eb, (uint64_t)h->hl);
  s.p0 = (uint32_t)h->d.n_taps; s.p1 = (uint32_t)h->d.df;
  return s;
}

int64_t acdsp_polydec_state_size(acdsp_polydec_t h) { return h ? (int64_t)(sizeof(StateHdr) + state_payload(polydec_state_hdr(h))) : -1; }

int32_t acdsp_polydec_state_get(acdsp_polydec_t h, void *buf, uint64_t cap_bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  const StateHdr s = polydec_state_hdr(h);
  return state_blob_get("polydec", h->d.device, s, {{h->hist.cur(), state_payload(s)}}, buf, cap_bytes);
}

int32_t acdsp_polydec_state_set(acdsp_polydec_t h, const void *buf, uint64_t bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  // every kernel path of a descriptor keeps the same history today; a blob of another length (another build) is taken as long as it covers
  // the NTAPS*DF - 1 samples an output reaches back
  StateHdr s;
  return history_state_set("polydec", "blob does not belong to an ac_poly_dec of this NTAPS / DF / channel count", h->d.device, polydec_state_hdr(h),
                           h->hist.cur(), buf, bytes, 0, (uint64_t)h->d.n_taps * h->d.df - 1, uint64_t(1) << 20, false, &s);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// polyphase interpolator (second half): ac_poly_intr
// ---------------------------------------------------------------------------------------------
struct acdsp_polyintr {
  acdsp_polyintr_desc_t d;
  int in_eb, out_eb, hl;
  bool ctrl_set = false;
  History hist;            // (flips on every call: the saved sums flip with it)
  DevBuf d_saved[2];       // sums of the last sample, emitted by the next call (folded cores); indexed like the history
  SideStream side;         // head / tail kernels of a call beside its matrix-core kernel (fir_kernels.hpp)
  int64_t t_total = 0;
  DevBuf d_coeffs, d_sign, d_corr;
  ~acdsp_polyintr() { side.destroy(); }
  // exact-accumulation class on the matrix cores (fir_up.hip): folded per-phase taps of the current control words
  bool up_ok = false;
  bool acc64_ok = false;        // a 64-bit ACC_TYPE whose sums the current control words keep inside 62 bits: the exact-accumulation class applies
  int up_px = 2;                // input byte planes of the matrix-core kernel (= container bytes; 1 under ACDSP_FLAG_IN_BYTES)
  FirUpPlan up_plan;
  uint32_t up_shmask = 0;
  int64_t up_max_abs = -1;      // bound on |z| of the folded taps (enables the 32-bit epilogue)
  DevBuf d_upfrag, d_upcorr;
  // long sub-filters (polyintr_long.hip): long_shape = the descriptor is long-capable (create); long_ok = the current control words run
  // there.  scratch: the phase rows
  bool long_shape = false, long_ok = false;
  PolyIntrLongPlan lplan;
  LongScratch scratch;
  DevBuf d_lfrag, d_lcorr, d_lhalve;
  int last_path = ACDSP_PATH_GENERIC;
  Staging st;
};

namespace {

inline int polyintr_lag(const acdsp_polyintr_desc_t &d) { return d.ftype == ACDSP_POLY_FOLD_ANTI ? 0 : 1; }

// the exact-accumulation class of ac_poly_intr as far as the descriptor decides it (a 64-bit ACC_TYPE needs the bound of the control words too)
inline bool polyintr_lossless_desc(const acdsp_polyintr_desc_t &d) {
  const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I, ls = fa - fi - fc;
  return d.in.S && d.acc.S && d.acc.O == ACDSP_WRAP && ls >= 0 && ls < 64 && fa >= fi && d.acc.I >= d.in.I + 1 && d.acc.W <= 64;
}

// Long sub-filters (polyintr_long.hip): the condition a descriptor fails, or nullptr when it is long-capable
const char *polyintr_long_refusal(const acdsp_polyintr_desc_t &d) {
  const int nt = d.n_taps + polyintr_lag(d);
  if (nt < kPolyIntrLongMinTaps) { return "fewer than 65 taps per phase"; }
  if (nt > kPolyIntrLongMaxTaps) { return "more than 16384 taps per phase"; }
  if (d.flags & ACDSP_FLAG_FORCE_GENERIC) { return "ACDSP_FLAG_FORCE_GENERIC (the exact-order kernels end at NTAPS = 2048)"; }
  if (!d.in.S || d.in.W > 16) { return "an IN_TYPE that is unsigned or wider than 16 bits"; }
  if (d.flags & ACDSP_FLAG_IN_BYTES) { return "ACDSP_FLAG_IN_BYTES (the long kernels read int16 rows; byte rows end at NTAPS = 2048, on the exact kernels)"; }
  if (d.coeff.S ? d.coeff.W > 16 : d.coeff.W > 15) { return "a COEFF_TYPE wider than 16 bits signed / 15 bits unsigned"; }
  if (!polyintr_lossless_desc(d)) {
    return "an ACC_TYPE that is not an exact accumulator (signed AC_WRAP, F_acc >= F_in + F_coeff, I_acc >= I_in + 1, W_acc <= 64)";
  }
  if ((int64_t)d.ifac * long_blocks(nt) > kPolyIntrLongMaxBlocks) { return "IF * K-blocks per phase above the K-block budget of 1024"; }
  return nullptr;
}

// Per-phase taps of ac_poly_intr as one linear filter of the input (host side; see fir_up.hip).  E[j][k] multiplies
// x[n - k] in the output group of input sample n.  Returns false when the control words make the cores non-linear in the
// input (a phase with sign[j] = 0 negates samples in IN_TYPE: -min(IN_TYPE) is not representable).
bool polyintr_linear_taps(const acdsp_polyintr_desc_t &d, const int64_t *coeffs, const uint8_t *sign, const uint8_t *corr,
                          std::vector<int64_t> *E, int *nt, uint32_t *sh_mask, __int128 *max_abs_sum, std::vector<uint8_t> *halve = nullptr) {
  const int N = d.n_taps, L = d.ifac;
  std::vector<std::vector<__int128>> sub((size_t)L, std::vector<__int128>((size_t)N, 0));   // sub-filter sums acc_n[j] = sum_k sub[j][k] x[n-k]
  for (int j = 0; j < L; j++) {
    if (d.ftype == ACDSP_POLY_FOLD_ANTI) {
      for (int i = 0; i < N; i++) { sub[j][i] = coeffs[i + N * j]; }                           // ac_poly_intr.h:246-256
      continue;
    }
    if (!sign[j]) { return false; }
    if (d.ftype == ACDSP_POLY_FOLD_EVEN) {                                                      // :141-151
      for (int i = 0; i < N / 2; i++) { const int64_t c = coeffs[i + j * N / 2]; sub[j][i] += c; sub[j][N - 1 - i] += c; }
    } else {                                                                                    // :194-209
      const int mid = (N - 1) / 2;
      for (int i = 0; i <= mid; i++) {
        const int64_t c = coeffs[i + (N / 2 + 1) * j];
        sub[j][i] += c;
        if (i != mid) { sub[j][N - 1 - i] += c; }
      }
    }
  }
  *max_abs_sum = 0;
  for (int j = 0; j < L; j++) {
    __int128 sa = 0;
    for (int k = 0; k < N; k++) { sa += sub[j][k] < 0 ? -sub[j][k] : sub[j][k]; }
    if (sa > *max_abs_sum) { *max_abs_sum = sa; }
  }
  const int lag = polyintr_lag(d);   // banks: the sums of sample n-1 leave with sample n (:153-175)
  *nt = N + lag;
  *sh_mask = 0;   // (phases 0 .. 31, all fir_up.hip takes; `halve` holds every phase)
  if (halve) { halve->assign((size_t)L, 0); }
  E->assign((size_t)L * (size_t)*nt, 0);
  for (int j = 0; j < L; j++) {
    const int cj = d.ftype == ACDSP_POLY_FOLD_ANTI ? j : corr[j];
    for (int k = 0; k < N; k++) {
      __int128 g = sub[j][k];
      if (cj != j) { g -= sub[cj][k]; }                      // (t1 + ACC(-t2)) >> 1 with sign[j] set (:164-172)
      if (g < INT64_MIN / 4 || g > INT64_MAX / 4) { return false; }
      (*E)[(size_t)j * *nt + k + lag] = (int64_t)g;
    }
    if (cj != j) {
      if (j < 32) { *sh_mask |= 1u << j; }
      if (halve) { (*halve)[(size_t)j] = 1; }
    }
  }
  return true;
}

}  // namespace

extern "C" {

int32_t acdsp_polyintr_destroy(acdsp_polyintr_t h) {
  if (!h) { return ACDSP_OK; }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

int32_t acdsp_polyintr_path(acdsp_polyintr_t h) { return h ? h->last_path : -1; }
int32_t acdsp_polyintr_in_elem_bytes(acdsp_polyintr_t h) { return h ? h->in_eb : -1; }
int32_t acdsp_polyintr_out_elem_bytes(acdsp_polyintr_t h) { return h ? h->out_eb : -1; }

int32_t acdsp_polyintr_create(const acdsp_polyintr_desc_t *desc, acdsp_polyintr_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  const acdsp_polyintr_desc_t &d = *desc;
  if (d.ftype < ACDSP_POLY_FOLD_EVEN || d.ftype > ACDSP_POLY_FOLD_ANTI) { return fail(ACDSP_EINVAL, "bad poly_intr ftype %d", d.ftype); }
  if (d.n_taps < 1 || d.n_taps > kPolyIntrLongMaxTaps - polyintr_lag(d)) {
    return fail(ACDSP_EUNSUPPORTED, "NTAPS=%d outside 1..%d", d.n_taps, kPolyIntrLongMaxTaps - polyintr_lag(d));
  }
  if (d.ifac < 1 || d.ifac > 255) { return fail(ACDSP_EUNSUPPORTED, "IF=%d outside 1..255 (corr[] is ac_int<8,false>)", d.ifac); }
  if (d.coeff_sz < 1 || d.coeff_sz > (1 << 20)) { return fail(ACDSP_EUNSUPPORTED, "COEFFSZ=%d outside 1..2^20", d.coeff_sz); }
  if (d.n_channels < 1) { return fail(ACDSP_EINVAL, "n_channels=%d must be positive", d.n_channels); }
  if (d.n_channels > 65535) { return fail(ACDSP_EUNSUPPORTED, "n_channels=%d outside 1..65535", d.n_channels); }
  int rc;
  if ((rc = check_fmt(d.in, "IN_TYPE")) || (rc = check_fmt(d.coeff, "COEFF_TYPE")) || (rc = check_fmt(d.acc, "ACC_TYPE")) ||
      (rc = check_fmt(d.out, "OUT_TYPE"))) {
    return rc;
  }
  {  // 128-bit exact intermediates: product coeff * fold (ACC_TYPE) or taps * coeff, aligned with the accumulator
    const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I;
    const int wp = d.ftype == ACDSP_POLY_FOLD_ANTI ? d.in.W + d.coeff.W + 2 : d.acc.W + d.coeff.W + 1;
    const int fp = d.ftype == ACDSP_POLY_FOLD_ANTI ? fi + fc : fa + fc;
    const int f = fp > fa ? fp : fa;
    if (wp + (f - fp) > 125 || d.acc.W + (f - fa) > 125) { return fail(ACDSP_EUNSUPPORTED, "type combination needs more than 128-bit intermediates"); }
  }
  // byte rows (ACDSP_FLAG_IN_BYTES, ACDSP_FLAG_OUT_BYTES with it): the common order of refusals, before the family's own
  int in_eb, out_eb;
  if ((rc = byte_rows("poly_intr", d.flags, d.in, d.out, "ACDSP_FLAG_OUT_BYTES needs ACDSP_FLAG_IN_BYTES (1-byte output rows exist on the byte-sample kernels only)",
                      &in_eb, &out_eb))) {
    return rc;
  }
  // NTAPS above 2048: the long matrix-core kernels or nothing
  const char *const long_why = polyintr_long_refusal(d);
  if (d.n_taps > 2048 && long_why) {
    return fail(ACDSP_EUNSUPPORTED, "poly_intr: NTAPS=%d: more than 2048 taps run on the long matrix-core kernels only, which do not take %s", d.n_taps, long_why);
  }
  if ((rc = check_device(d.device))) { return rc; }
  std::unique_ptr<acdsp_polyintr> h(new acdsp_polyintr());   // (check_device has made the device current: a failure below frees there)
  h->d = d;
  h->in_eb = in_eb; h->out_eb = out_eb;
  h->hl = round_up(d.n_taps + 15, 32);
  if ((rc = h->hist.init(d.n_channels, h->hl, h->in_eb))) { return rc; }
  for (DevBuf &sv : h->d_saved) {
    if ((rc = sv.alloc_zeroed((size_t)d.n_channels * d.ifac * sizeof(int64_t)))) { return rc; }   // acc_a / acc_b start at 0 (ac_poly_intr.h:117-118)
  }
  if ((rc = h->d_coeffs.alloc((size_t)d.coeff_sz * sizeof(int64_t))) || (rc = h->d_sign.alloc((size_t)d.ifac)) || (rc = h->d_corr.alloc((size_t)d.ifac))) { return rc; }
  h->long_shape = long_why == nullptr;
  if (h->long_shape) {
    const int nb = long_blocks(d.n_taps + polyintr_lag(d));
    // a step reaches 32 (nb - 1) samples back: inside the history as far as real taps go (nt - 1 <= NTAPS), beyond it over zero-padded taps only
    if (h->hl < d.n_taps || h->hl % 32 || 32 * (nb - 1) > h->hl) { return fail(ACDSP_EHIP, "internal: history of %d samples is shorter than the long kernel's reach", h->hl); }
    // scratch: phase rows of OUT containers, ifac * out_eb bytes per slab input sample, no head
    if ((rc = h->d_lfrag.alloc((size_t)2 * d.ifac * nb * 64 * 4 * sizeof(uint32_t))) || (rc = h->d_lcorr.alloc((size_t)d.ifac * sizeof(int64_t))) ||
        (rc = h->d_lhalve.alloc((size_t)d.ifac)) || (rc = h->scratch.init((uint64_t)d.ifac * out_eb, 0, d.n_channels))) {
      if (d.n_taps > 2048) { return rc; }
      // up to 2048 taps the handle existed without these buffers: it stays what it was, on the exact kernels
      h->long_shape = false;
      h->d_lfrag = DevBuf(); h->d_lcorr = DevBuf(); h->d_lhalve = DevBuf(); h->scratch = LongScratch();
      (void)hipGetLastError();
    }
  }
  *out = h.release();
  return ACDSP_OK;
}

int32_t acdsp_polyintr_set_ctrl(acdsp_polyintr_t h, const int64_t *coeffs, const uint8_t *sign, const uint8_t *corr) {
  if (!h || !coeffs || !sign || !corr) { return fail(ACDSP_EINVAL, "null argument"); }
  const acdsp_polyintr_desc_t &d = h->d;
  int rc = check_device(d.device);
  if (rc) { return rc; }
  const acdsp::DFmt cf = make_dfmt(d.coeff);
  for (int i = 0; i < d.coeff_sz; i++) {
    if (coeffs[i] < cf.lo || coeffs[i] > cf.hi) { return fail(ACDSP_EINVAL, "coefficient %d = %lld is not a COEFF_TYPE raw word", i, (long long)coeffs[i]); }
  }
  const int N = d.n_taps, J = d.ifac - 1;
  const int max_ci = d.ftype == ACDSP_POLY_FOLD_EVEN ? (N / 2 - 1) + J * N / 2
                     : d.ftype == ACDSP_POLY_FOLD_ODD ? (N - 1) / 2 + (N / 2 + 1) * J : (N - 1) + N * J;
  if (max_ci >= d.coeff_sz) { return fail(ACDSP_EINVAL, "the reference would read coeffs[%d] of coeffs[COEFFSZ = %d]", max_ci, d.coeff_sz); }
  for (int j = 0; j < d.ifac; j++) {
    if (d.ftype != ACDSP_POLY_FOLD_ANTI && corr[j] >= d.ifac) { return fail(ACDSP_EINVAL, "corr[%d] = %d indexes outside the IF = %d accumulator banks", j, corr[j], d.ifac); }
  }
  // The cores as IF linear filters of the input, folded once for every decision below (an O(IF * NTAPS) fold: exact-accumulation descriptors only)
  const int fi = d.in.W - d.in.I, fc = d.coeff.W - d.coeff.I, fa = d.acc.W - d.acc.I, ls = fa - fi - fc;
  const bool lossless = polyintr_lossless_desc(d);
  std::vector<int64_t> E;
  std::vector<uint8_t> hv;
  int nt = 0;
  uint32_t shm = 0;
  __int128 sa = 0;
  const bool linear = lossless && polyintr_linear_taps(d, coeffs, sign, corr, &E, &nt, &shm, &sa, &hv);
  // |acc| <= sum|taps| * 2^(W_in - 1) << ls must stay inside ACC_TYPE (62 bits of a 64-bit one); a pair sum then fits one more bit
  const bool no_wrap = linear && d.in.W - 1 + ls < 100 && (sa << (d.in.W - 1 + ls)) < ((__int128)1 << ((d.acc.W < 64 ? d.acc.W : 63) - 1));
  // Long sub-filters (polyintr_long.hip): decided on the host before anything is uploaded.  The control words must keep the cores linear
  // (every sign[j] set on the folded cores), no sum may wrap ACC_TYPE (the pair halving does not commute with a wrap) and every folded tap
  // must split into two signed bytes.  Above 2048 taps nothing else exists: a set that cannot go there is refused and the handle keeps
  // the state it had.
  bool long_ok = false;
  std::vector<uint32_t> lfrag;
  std::vector<int64_t> lcorr;
  std::vector<uint8_t> lhalve;
  PolyIntrLongPlan lpl;
  if (h->long_shape) {
    const char *why = nullptr;
    if (!linear) { why = "a phase with sign[j] = 0 (it negates samples in IN_TYPE)"; }
    else if (!no_wrap) { why = "sub-filter sums that may wrap ACC_TYPE"; }
    else if (!polyintr_long_plan(E.data(), d.ifac, nt, hv.data(), &lpl, &lfrag, &lcorr, &lhalve)) { why = "a folded tap outside -32768..32639 (it cannot be split into two signed bytes)"; }
    long_ok = why == nullptr;
    if (!long_ok && d.n_taps > 2048) {
      return fail(ACDSP_EUNSUPPORTED, "poly_intr: NTAPS=%d: more than 2048 taps run on the long matrix-core kernels only, which do not take %s", d.n_taps, why);
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->d_coeffs.upload(coeffs, (size_t)d.coeff_sz * sizeof(int64_t))) || (rc = h->d_sign.upload(sign, (size_t)d.ifac)) ||
      (rc = h->d_corr.upload(corr, (size_t)d.ifac))) {
    return rc;
  }
  h->ctrl_set = true;
  h->long_ok = false;
  if (long_ok) {
    if ((rc = h->d_lfrag.upload(lfrag.data(), lfrag.size() * sizeof(uint32_t))) || (rc = h->d_lcorr.upload(lcorr.data(), lcorr.size() * sizeof(int64_t))) ||
        (rc = h->d_lhalve.upload(lhalve.data(), lhalve.size()))) {
      return rc;
    }
    h->lplan = lpl;
    h->long_ok = true;
  }
  // matrix-core path: exact-accumulation class, int16 / int32 samples or int8 rows (ACDSP_FLAG_IN_BYTES: one plane), control words that keep the cores linear, and an
  // accumulator that cannot wrap (the symmetric-pair halving (t1 -/+ t2) >> 1 does not commute with a wrap)
  h->up_ok = false;
  // (a 64-bit ACC_TYPE -- the header's own usage example, ac_poly_intr.h:45-48: <32,16> samples and coefficients into <64,32> -- belongs to
  // the class when the control words bound every sub-filter sum to 62 bits: nothing can wrap and the pair sum t1 -/+ t2 stays inside int64)
  h->acc64_ok = lossless && d.acc.W == 64 && no_wrap;
  const int upx = h->in_eb;
  // (a long-capable handle has nt >= 65 taps per phase: fir_up_plan has no plan there)
  if (!h->long_shape && no_wrap && !knob_no_gen() && !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && (h->in_eb == 1 || h->in_eb == 2 || h->in_eb == 4) && d.ifac <= 32) {
    std::vector<uint32_t> frag;
    std::vector<int64_t> ucorr;
    FirUpPlan pl;
    if (fir_up_plan(E.data(), d.ifac, nt, upx, &pl, &frag, &ucorr) && fir_up_shape_ok(h->in_eb, upx, pl.nb, d.ifac, h->out_eb)) {
      if ((rc = h->d_upfrag.alloc_upload(frag)) || (rc = h->d_upcorr.alloc_upload(ucorr))) { return rc; }
      h->up_plan = pl; h->up_shmask = shm; h->up_ok = true; h->up_px = upx;
      {  // |z| <= max_j sum_k |E_j[k]| * 2^(W_in - 1)
        __int128 worst = 0;
        for (int j = 0; j < d.ifac; j++) {
          __int128 sj = 0;
          for (int k = 0; k < nt; k++) { const int64_t v = E[(size_t)j * nt + k]; sj += v < 0 ? -(__int128)v : (__int128)v; }
          if (sj > worst) { worst = sj; }
        }
        worst <<= (d.in.W - 1);
        h->up_max_abs = worst < ((__int128)1 << 62) ? (int64_t)worst : -1;
      }
    }
  }
  return ACDSP_OK;
}

int32_t acdsp_polyintr_set_scratch_cap(acdsp_polyintr_t h, uint64_t bytes) { return poly_set_scratch_cap(h, bytes); }
int32_t acdsp_polyintr_long_geometry(acdsp_polyintr_t h, int64_t *slab_inputs, int32_t *group_channels, uint64_t *scratch_bytes) {
  return poly_long_geometry(h, slab_inputs, group_channels, scratch_bytes);
}

int64_t acdsp_polyintr_out_count(acdsp_polyintr_t h, int64_t n_in) {
  if (!h || n_in < 0) { return -1; }
  if (n_in == 0) { return 0; }
  const int64_t groups = (h->d.ftype != ACDSP_POLY_FOLD_ANTI && h->t_total == 0) ? n_in - 1 : n_in;   // `init` (:175)
  return groups * h->d.ifac;
}

int32_t acdsp_polyintr_run(acdsp_polyintr_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                           int64_t *n_out, void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (!h->ctrl_set) { return fail(ACDSP_ESTATE, "poly_intr run before acdsp_polyintr_set_ctrl (the reference reads uninitialised structs)"); }
  if (n_in < 0 || (n_in > 0 && (!d_in || in_stride < n_in))) { return fail(ACDSP_EINVAL, "poly_intr run: bad input arguments"); }
  const int64_t no = acdsp_polyintr_out_count(h, n_in);
  if (n_out) { *n_out = no; }
  if (n_in == 0) { return ACDSP_OK; }
  if (no > 0 && (!d_out || out_stride < no)) { return fail(ACDSP_EINVAL, "poly_intr run: output buffer too small for %lld outputs", (long long)no); }
  if (stream_is_capturing((hipStream_t)stream) && h->d.ftype != ACDSP_POLY_FOLD_ANTI && h->t_total == 0) {
    return fail(ACDSP_ESTATE, "poly_intr run under graph capture: the stream's first call emits one group less and cannot be replayed; run it before capturing");
  }
  const acdsp_polyintr_desc_t &d = h->d;
  int rc = check_device(d.device);
  if (rc) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  PolyIntrParams p;
  memset(&p, 0, sizeof p);
  p.n_taps = d.n_taps; p.coeff_sz = d.coeff_sz; p.ifac = d.ifac; p.ftype = d.ftype; p.n_ch = d.n_channels;
  p.in = make_dfmt(d.in); p.cf = make_dfmt(d.coeff); p.acc = make_dfmt(d.acc); p.out = make_dfmt(d.out);
  p.in_eb = h->in_eb; p.out_eb = h->out_eb; p.hl = h->hl;
  p.skip = (d.ftype != ACDSP_POLY_FOLD_ANTI && h->t_total == 0) ? 1 : 0;
  {  // exact-accumulation class (see polyintr_acc_fast): the `fold` needs one more integer bit than IN_TYPE
    const int fi = p.in.F, fc = p.cf.F, fa = p.acc.F;
    p.lossless_shift = fa - fi - fc;
    p.lossless = !(d.flags & ACDSP_FLAG_FORCE_GENERIC) && d.in.S && d.acc.S && d.acc.O == ACDSP_WRAP && p.lossless_shift >= 0 && p.lossless_shift < 64 && fa >= fi &&
                 d.acc.I >= d.in.I + 1 && (d.acc.W <= 63 || h->acc64_ok) && (d.in.O == ACDSP_WRAP || d.in.O == ACDSP_SAT || d.in.O == ACDSP_SAT_SYM || d.in.O == ACDSP_SAT_ZERO);
  }
  p.in_stride = in_stride; p.out_stride = out_stride; p.n = n_in; p.n_out = no;
  const CallRows rows = {d_in, in_stride, n_in, d_out, out_stride};
  const int nxt = h->hist.next(false);   // (always the other buffer: the saved sums flip with it)
  int64_t *const saved_next = h->d_saved[nxt].get<int64_t>();
  p.x = d_in; p.y = d_out; p.hist = h->hist.cur();
  p.coeffs = h->d_coeffs.get<int64_t>(); p.sign = h->d_sign.get<uint8_t>(); p.corr = h->d_corr.get<uint8_t>(); p.saved = h->d_saved[h->hist.index()].get<int64_t>();
  p.o_begin = 0; p.o_end = no;
  hipError_t e = hipSuccess;
  // Complete steps of 32 input slots go to the matrix-core kernel; the head (history, the saved sums of the previous call)
  // and the ragged tail stay on the VALU kernels.
  int64_t o_a = 0, o_b = 0;   // outputs [o_a, o_b) are produced by fir_up
  bool forked = false;
  h->last_path = p.lossless ? ACDSP_PATH_LOSSLESS64 : ACDSP_PATH_GENERIC;
  if (h->long_ok) {
    // Long sub-filters, every call whatever its length and alignment.  Two things stay on the exact kernels below, beside the long kernels on
    // the side stream: the first group of a call on the folded cores (it carries the sums saved by the previous call, formed with the
    // coefficients of their own time) and the sums of the call's last sample -- so the stream continues bit for bit on the exact kernels
    // when later control words leave the long path.
    h->last_path = ACDSP_PATH_MFMA_LONG;
    const int64_t o_lo = (d.ftype != ACDSP_POLY_FOLD_ANTI && h->t_total > 0) ? d.ifac : 0;
    if (SideStream::enabled()) {
      const hipError_t ef = h->side.fork(s);
      if (ef != hipSuccess) { return fail(ACDSP_EHIP, "poly_intr side stream: %s", hipGetErrorString(ef)); }
      forked = true;
    }
    FirParams k = fir_params_of(p.in, p.cf, p.acc, p.out, h->in_eb, h->out_eb, h->hl, d.n_channels, rows);
    k.lossless_shift = p.lossless_shift; k.hist = p.hist;
    e = launch_polyintr_long(k, h->lplan, h->scratch.geo, h->d_lfrag.get<uint32_t>(), h->d_lcorr.get<int64_t>(), h->d_lhalve.get<uint8_t>(), h->scratch.buf.get(),
                             p.skip, o_lo, no, s);
    if (e != hipSuccess) {
      if (forked) { (void)h->side.join(s); }
      return fail(ACDSP_EHIP, "poly_intr long kernel launch failed: %s", hipGetErrorString(e));
    }
    o_a = o_lo; o_b = no;   // (a call that ends with its first group runs that group and the save kernel in one launch below)
  } else if (h->up_ok && p.lossless) {
    const int L = d.ifac;
    const int64_t out_off = -(int64_t)p.skip * L, slot_a = h->up_plan.hs;
    const int64_t n_steps = (n_in / 16 - slot_a) / 32;
    // the tile stores need dword alignment only (gfx950 serves dword-aligned multi-dword stores): IF = 2 into 2-byte containers starts its
    // first call one input's outputs = 4 bytes into the 8-byte grid.  1-byte rows: the first call of a folded core starts IF bytes in front
    // of the row, so a factor that is no multiple of 4 leaves THAT call on the VALU kernels (later calls have out_off = 0)
    const int64_t oal = h->out_eb >= 8 ? 8 : 4;
    const bool aligned = rows_vec_aligned(d_in, in_stride, h->in_eb) && ((uintptr_t)d_out % oal == 0) &&
                         ((out_stride * h->out_eb) % oal == 0) && ((out_off * h->out_eb) % oal == 0);
    if (aligned && n_steps > 0) {
      // the head and the tail of the call (two launches of a few thousand waves, 16 us each, + the saved sums) neither feed nor follow the
      // matrix-core kernel: forked here, they overlap it on the handle's side stream (4.7 % of the bench row when they queued behind it)
      if (SideStream::enabled()) {
        const hipError_t ef = h->side.fork(s);
        if (ef != hipSuccess) { return fail(ACDSP_EHIP, "poly_intr side stream: %s", hipGetErrorString(ef)); }
        forked = true;
      }
      FirParams k = fir_params_of(p.in, p.cf, p.acc, p.out, h->in_eb, h->out_eb, 0, d.n_channels, rows);   // (no history: whole steps inside the call)
      k.lossless_shift = p.lossless_shift;
      e = launch_fir_up(k, h->up_plan, h->up_px, h->d_upfrag.get<uint32_t>(), h->d_upcorr.get<int64_t>(), 0, 0, 0, h->up_shmask, h->up_max_abs, slot_a, n_steps, out_off, s);
      if (e == hipSuccess) {
        o_a = 16 * slot_a * L + out_off; o_b = 16 * (slot_a + 32 * n_steps) * L + out_off;
        h->last_path = ACDSP_PATH_MFMA_GEN;
      } else if (e != hipErrorNotSupported) {
        if (forked) { (void)h->side.join(s); }   // (an unjoined fork invalidates a stream capture and leaves the side stream waiting: advisor, round 5)
        return fail(ACDSP_EHIP, "poly_intr matrix-core kernel launch failed: %s", hipGetErrorString(e));
      }
    }
  }
  hipStream_t vs = (forked && o_b > o_a) ? h->side.s : s;
  if (o_b > o_a) {
    p.o_begin = 0; p.o_end = o_a;
    // (the head of a long call is the one group that reads `saved`: no window or coefficient table to stage)
    e = h->long_ok ? launch_polyintr_saved_group(p, vs) : launch_polyintr(p, nullptr, vs);
    if (e == hipSuccess) { p.o_begin = o_b; p.o_end = no; e = launch_polyintr(p, saved_next, vs); }
  } else {
    e = launch_polyintr(p, saved_next, s);
  }
  hipError_t eh = hipSuccess;
  if (e == hipSuccess) {
    FirParams k = fir_params_of(p.in, DFmt(), DFmt(), DFmt(), h->in_eb, 0, h->hl, d.n_channels, {d_in, in_stride, n_in, nullptr, 0});   // (input side only)
    k.hist = p.hist;
    eh = launch_fir_hist_update(k, h->hist.at(nxt), vs);   // (never in place -- so it may run beside the main kernel too)
  }
  if (forked) {   // (always joined, used or not: an unjoined fork is an error under stream capture)
    const hipError_t ej = h->side.join(s);
    if (e == hipSuccess && ej != hipSuccess) { e = ej; }
  }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "poly_intr kernel launch failed: %s", hipGetErrorString(e)); }
  if (eh != hipSuccess) { return fail(ACDSP_EHIP, "poly_intr state kernel launch failed: %s", hipGetErrorString(eh)); }
  h->hist.commit(nxt);
  h->t_total += n_in;
  return ACDSP_OK;
}

int32_t acdsp_polyintr_run_host(acdsp_polyintr_t h, const void *h_in, int64_t n_in, void *h_out, int64_t out_cap, int64_t *n_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n_in < 0 || (n_in > 0 && !h_in)) { return fail(ACDSP_EINVAL, "poly_intr run_host: bad arguments"); }
  const int64_t no = acdsp_polyintr_out_count(h, n_in);
  if (n_out) { *n_out = no; }
  if (n_in == 0) { return ACDSP_OK; }
  if (no > 0 && (!h_out || out_cap < no)) { return fail(ACDSP_EINVAL, "poly_intr run_host: output buffer too small"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  const HostRows r = {h->d.n_channels, h_in, n_in, (n_in + 15) / 16 * 16, h->in_eb, h_out, no, (no + 15) / 16 * 16 + 16, out_cap, h->out_eb};
  return run_host_staged(h->st, r, false, [&](const void *d_in, void *d_out, bool) { return acdsp_polyintr_run(h, d_in, r.si, n_in, d_out, r.so, nullptr, nullptr); });
}

int32_t acdsp_polyintr_reset(acdsp_polyintr_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->hist.zero())) { return rc; }
  for (DevBuf &sv : h->d_saved) {
    if ((rc = sv.zero((size_t)h->d.n_channels * h->d.ifac * sizeof(int64_t)))) { return rc; }
  }
  h->t_total = 0;
  return ACDSP_OK;
}

// Deep copy (the reference core is a plain aggregate: taps[], acc_a[], acc_b[] and the control structs go with it, ac_poly_intr.h:106-109):
// descriptor, scratch cap, control words when set, input history, saved sums, input count.  Scratch, side stream and staging are the clone's own.
int32_t acdsp_polyintr_clone(acdsp_polyintr_t h, acdsp_polyintr_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_polyintr_t c = nullptr;
  int rc = acdsp_polyintr_create(&h->d, &c);
  if (rc) { return rc; }
  std::unique_ptr<acdsp_polyintr, int32_t (*)(acdsp_polyintr_t)> guard(c, acdsp_polyintr_destroy);
  if (c->long_shape != h->long_shape) { return fail(ACDSP_EHIP, "polyintr_clone: the buffers of the long kernels could not be allocated a second time"); }
  if (c->long_shape && h->scratch.cap != c->scratch.cap && (rc = c->scratch.size(h->scratch.cap))) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if (h->ctrl_set) {
    std::vector<int64_t> cf((size_t)h->d.coeff_sz);
    std::vector<uint8_t> sg((size_t)h->d.ifac), cr((size_t)h->d.ifac);
    HIP_TRY(hipMemcpy(cf.data(), h->d_coeffs.get(), cf.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sg.data(), h->d_sign.get(), sg.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cr.data(), h->d_corr.get(), cr.size(), hipMemcpyDeviceToHost));
    if ((rc = acdsp_polyintr_set_ctrl(c, cf.data(), sg.data(), cr.data()))) { return rc; }
  }
  if ((rc = c->hist.copy_from(h->hist))) { return rc; }   // (the clone's current index is 0: so is that of its saved sums)
  HIP_TRY(hipMemcpy(c->d_saved[0].get(), h->d_saved[h->hist.index()].get(), (size_t)h->d.n_channels * h->d.ifac * sizeof(int64_t), hipMemcpyDeviceToDevice));
  c->t_total = h->t_total;
  c->last_path = h->last_path;
  *out = guard.release();
  return ACDSP_OK;
}

// State blob, kind 7: the newest `hl` input samples of every channel, oldest first, in IN containers (taps[]; 1-byte ones under
// ACDSP_FLAG_IN_BYTES: elem_bytes 1, so a flagged blob and an unflagged handle refuse each other, while ACDSP_FLAG_OUT_BYTES changes nothing --
// the saved sums are ACC words -- and blobs move both ways between handles with and without it), the input count in t_total
// (the folded cores emit nothing for the first sample of a stream) and, behind the histories, the sub-filter sums of the last sample
// [channel][IF] as int64 ACC raw words (the bank of acc_a / acc_b that the next sample emits: formed with the control words of their own
// time, so carried, not recomputed; all zero on FOLD_ANTI, which emits at once).
static StateHdr polyintr_state_hdr(const acdsp_polyintr *h) {
  StateHdr s = state_hdr(7, (uint32_t)h->d.n_channels, (uint32_t)h->in_eb, (uint64_t)h->hl);
  s.t_total = h->t_total;
  s.p0 = (uint32_t)h->d.n_taps; s.p1 = (uint32_t)h->d.ifac; s.p2 = (uint32_t)h->d.ftype; s.p3 = (uint32_t)h->d.coeff_sz;
  return s;
}
static uint64_t polyintr_saved_bytes(const acdsp_polyintr *h) { return (uint64_t)h->d.n_channels * h->d.ifac * sizeof(int64_t); }

int64_t acdsp_polyintr_state_size(acdsp_polyintr_t h) {
  return h ? (int64_t)(sizeof(StateHdr) + state_payload(polyintr_state_hdr(h)) + polyintr_saved_bytes(h)) : -1;
}

int32_t acdsp_polyintr_state_get(acdsp_polyintr_t h, void *buf, uint64_t cap_bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  const StateHdr s = polyintr_state_hdr(h);   // (run() is asynchronous on two streams: the getter drains the device)
  return state_blob_get("polyintr", h->d.device, s, {{h->hist.cur(), state_payload(s)}, {h->d_saved[h->hist.index()].get(), polyintr_saved_bytes(h)}}, buf, cap_bytes);
}

int32_t acdsp_polyintr_state_set(acdsp_polyintr_t h, const void *buf, uint64_t bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  // every kernel path of a descriptor keeps the same history today; a blob of another length (another build) is taken as long as it covers
  // the NTAPS samples the sums of a call's first group reach back
  const uint64_t sv = polyintr_saved_bytes(h);
  StateHdr s;
  const int rc = history_state_set("polyintr", "blob does not belong to an ac_poly_intr of this NTAPS / IF / ftype / COEFFSZ / channel count", h->d.device,
                                   polyintr_state_hdr(h), h->hist.cur(), buf, bytes, sv, (uint64_t)h->d.n_taps, uint64_t(1) << 20, true, &s);
  if (rc) { return rc; }
  // the saved sums are indexed like the history: they go beside the buffer just written
  HIP_TRY(hipMemcpy(h->d_saved[h->hist.index()].get(), (const char *)buf + sizeof s + state_payload(s), sv, hipMemcpyHostToDevice));
  h->t_total = s.t_total;
  return ACDSP_OK;
}

}  // extern "C"

