// engine_ddc.hip -- acdsp_ddc_*: the decimator -> FIR cascade and the decimator -> ac_poly_dec cascade (acdsp_ddc_create_polydec) behind the C ABI
#include "engine_common.hpp"

using namespace acdsp;
using namespace acdsp::eng;

// ---------------------------------------------------------------------------------------------
// DDC cascade: ac_cic_dec_full -> ac_fir_* on the decimator's lossless INT_TYPE words
// ---------------------------------------------------------------------------------------------
namespace acdsp {
// (b_flags / b_name: stage B's descriptor flags and its name in the messages)
static int ddc_flag_refusals_of(const acdsp_cic_desc_t &cic, int32_t b_flags, const char *b_name, int32_t ddc_flags) {
  if (ddc_flags & ~ACDSP_DDC_IN_BYTES) { return fail(ACDSP_EINVAL, "ddc: unknown bits 0x%x in ddc_flags", (unsigned)(ddc_flags & ~ACDSP_DDC_IN_BYTES)); }
  if (b_flags & ACDSP_FLAG_IN_BYTES) { return fail(ACDSP_EUNSUPPORTED, "ddc: ACDSP_FLAG_IN_BYTES on the cascade's %s (it reads the decimator's INT_TYPE words)", b_name); }
  if (cic.flags & ACDSP_FLAG_IN_BYTES) { return fail(ACDSP_EUNSUPPORTED, "ddc: ACDSP_FLAG_IN_BYTES on the cascade's CIC decimator (the cascade kernel reads int16 rows)"); }
  if ((b_flags | cic.flags) & ACDSP_FLAG_OUT_BYTES) { return fail(ACDSP_EUNSUPPORTED, "ddc: ACDSP_FLAG_OUT_BYTES on a stage of the cascade (1-byte output rows: the FIR under both byte flags only)"); }
  if ((ddc_flags & ACDSP_DDC_IN_BYTES) && cic.in.W > 8) { return fail(ACDSP_EINVAL, "ddc: ACDSP_DDC_IN_BYTES: IN_TYPE W=%d does not fit a 1-byte container", cic.in.W); }
  return ACDSP_OK;
}
int ddc_flag_refusals(const acdsp_cic_desc_t &cic, const acdsp_fir_desc_t &fir, int32_t ddc_flags) { return ddc_flag_refusals_of(cic, fir.flags, "FIR", ddc_flags); }
int ddc_flag_refusals(const acdsp_cic_desc_t &cic, const acdsp_polydec_desc_t &pd, int32_t ddc_flags) { return ddc_flag_refusals_of(cic, pd.flags, "ac_poly_dec", ddc_flags); }
}  // namespace acdsp

namespace {
// The format part of both stages' kernel arguments (the per-call fields stay zero): what launch_cascade and cascade_shape_ok read
void ddc_stage_params(const acdsp_ddc *h, FirParams *pa_out, FirParams *pb_out) {
  const acdsp_cic_desc_t &cd = h->cic->d;
  FirParams &pa = *pa_out, &pb = *pb_out;
  memset(&pa, 0, sizeof pa); memset(&pb, 0, sizeof pb);
  pa.n_ch = cd.n_channels; pa.in = make_dfmt(cd.in); pa.out = make_dfmt(cd.out); pa.acc = pa.out; pa.cf = pa.in;
  pa.in_eb = h->cic->in_eb; pa.out_eb = h->cic->out_eb; pa.hl = h->hl;
  if (h->pd) {   // (a saturating ACC_TYPE gets here only when the coefficient set cannot reach its bounds: acdsp_polydec::sat_free)
    const acdsp_polydec_desc_t &dd = h->pd->d;
    pb.n_ch = dd.n_channels; pb.in = make_dfmt(dd.in); pb.cf = make_dfmt(dd.coeff); pb.acc = make_dfmt(dd.acc); pb.out = make_dfmt(dd.out);
    pb.acc.O = ACDSP_WRAP;
    pb.in_eb = h->pd->in_eb; pb.out_eb = h->pd->out_eb;
  } else {
    const acdsp_fir_desc_t &fd = h->fir->d;
    pb.n_ch = fd.n_channels; pb.in = make_dfmt(fd.in); pb.cf = make_dfmt(fd.coeff); pb.acc = make_dfmt(fd.acc); pb.out = make_dfmt(fd.out);
    pb.in_eb = h->fir->in_eb; pb.out_eb = h->fir->out_eb;
  }
  pb.lossless_shift = pb.acc.F - pb.in.F - pb.cf.F;
}

// Does the fused kernel take this decimator and these formats at every window phase?  Asked at creation: a descriptor outside the compiled
// families -- 8-bit samples in int16 rows, whose INT_TYPE has fewer than 33 bits, as much as a byte cascade at another rate -- runs the two
// kernels instead of resolving to a fused handle whose every run() then fails with "shape outside the compiled cascade kernel".
bool ddc_stage_a_ok(const acdsp_ddc *h) {
  FirParams pa, pb;
  ddc_stage_params(h, &pa, &pb);
  const std::vector<int64_t> &taps = h->cic->h_taps;
  for (int fm = 0; fm < 16; fm++) {
    FirGenPlan pl;
    std::vector<uint32_t> fr;
    if (!fir_gen_plan(taps.data(), (int)taps.size(), h->cic->d.R, fm, &pl, &fr) || fr.size() > kGenFragWords ||
        !(h->pd ? cascade_dec_shape_ok(pa, pl, h->cic->it.W, pb, nullptr, h->df, 0) : cascade_shape_ok(pa, pl, h->cic->it.W, pb, nullptr))) { return false; }
  }
  return true;
}

// Two-kernel polydec cascade: the q < DF words behind the last whole group of a call move to the front of the intermediate rows, where the next
// call's decimator output lands behind them.  (A kernel, not a 2-D copy: a few bytes per row, and it records into a graph like any launch.)
__global__ void ddc_queue_move_kernel(unsigned char *mid, int64_t row_bytes, int64_t src_off, int n_bytes, int n_ch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_ch * n_bytes) { return; }
  const int64_t ch = i / n_bytes, k = i % n_bytes;
  mid[ch * row_bytes + k] = mid[ch * row_bytes + src_off + k];
}

// words of the stream that wait in front of the next call of a polydec cascade
int64_t ddc_queued(const acdsp_ddc *h) {
  if (!h->fused) { return h->n_q; }
  const int R = h->cic->d.R;
  return ((h->t_total + R - 1) / R) % h->df;   // the decimator has emitted ceil(t_total / R) words
}
}  // namespace

// The intermediate rows of the two-kernel mode hold at least `cap` words each (the stream `s` is drained before they are replaced).  The queued
// words of a polydec cascade move with them.  A captured graph has the old buffer's address in its kernel arguments: it stays allocated,
// unused, until the handle goes.
int acdsp::eng::ddc_mid_reserve(acdsp_ddc *h, int64_t cap, hipStream_t s) {
  if (cap <= h->mid_cap) { return ACDSP_OK; }
  HIP_TRY(hipStreamSynchronize(s));
  const size_t eb = (size_t)h->cic->out_eb, n_ch = (size_t)h->cic->d.n_channels;
  DevBuf fresh;
  int rc = fresh.alloc(n_ch * (size_t)cap * eb);
  if (rc) { return rc; }
  if (h->n_q > 0) {
    HIP_TRY(hipMemcpy2D(fresh.get(), (size_t)cap * eb, h->d_mid.get(), (size_t)h->mid_cap * eb, (size_t)h->n_q * eb, n_ch, hipMemcpyDeviceToDevice));
  }
  if (h->captured && h->d_mid) { h->retired.push_back(std::move(h->d_mid)); }
  h->d_mid = std::move(fresh);
  h->mid_cap = cap;
  return ACDSP_OK;
}

extern "C" {

int32_t acdsp_ddc_destroy(acdsp_ddc_t h) {
  if (!h) { return ACDSP_OK; }
  if (h->cic) { (void)hipSetDevice(h->cic->d.device); }
  const acdsp_cic_t cic = h->cic;
  const acdsp_fir_t fir = h->fir;
  const acdsp_polydec_t pd = h->pd;
  delete h;   // the cascade's own buffers first, then the stages
  acdsp_cic_destroy(cic);
  acdsp_fir_destroy(fir);
  acdsp_polydec_destroy(pd);
  return ACDSP_OK;
}

int32_t acdsp_ddc_create(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, acdsp_ddc_t *out) { return acdsp_ddc_create_ex(cic, fir, 0, out); }

int32_t acdsp_ddc_create_ex(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, int32_t ddc_flags, acdsp_ddc_t *out) {
  if (!cic || !fir || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  int rc;
  if ((rc = ddc_flag_refusals(*cic, *fir, ddc_flags))) { return rc; }
  if (cic->interp) { return fail(ACDSP_EINVAL, "ddc: stage A must be the decimator"); }
  if (cic->n_channels != fir->n_channels || cic->device != fir->device) { return fail(ACDSP_EINVAL, "ddc: both stages must cover the same channels on one device"); }
  if (fir->coeffs_per_channel) { return fail(ACDSP_EUNSUPPORTED, "ddc: one shared coefficient set"); }
  const bool in_bytes = (ddc_flags & ACDSP_DDC_IN_BYTES) != 0;
  std::unique_ptr<acdsp_ddc, int32_t (*)(acdsp_ddc_t)> h(new acdsp_ddc(), acdsp_ddc_destroy);
  h->cic_desc = *cic; h->fir_desc = *fir; h->ddc_flags = ddc_flags;
  // the container flag belongs to the composite; its decimator stage is the byte-row decimator
  acdsp_cic_desc_t stage_a = *cic;
  if (in_bytes) { stage_a.flags |= ACDSP_FLAG_IN_BYTES; }
  if ((rc = acdsp_cic_create(&stage_a, &h->cic)) || (rc = acdsp_fir_create(fir, &h->fir))) { return rc; }
  // the cascade is lossless in the middle: the decimator writes its INT_TYPE and the FIR reads exactly that type
  const acdsp_fmt_t &it = h->cic->it;
  const bool same = [&](const acdsp_fmt_t &f) { return f.W == it.W && f.I == it.I && f.S == it.S; }(cic->out) && fir->in.W == it.W &&
                    fir->in.I == it.I && fir->in.S == it.S;
  if (!same) {
    return fail(ACDSP_EINVAL, "ddc: the decimator's OUT_TYPE and the FIR's IN_TYPE must both be the INT_TYPE <%d,%d>", it.W, it.I);
  }
  static const bool no_fuse = getenv("ACDSP_NO_FUSE") != nullptr;
  h->fused = !no_fuse && h->fir->lossless && !(fir->flags & ACDSP_FLAG_FORCE_GENERIC) && !(cic->flags & ACDSP_FLAG_FORCE_GENERIC) && h->fir->out_eb == 4 &&
             (in_bytes ? h->cic->gen_plan_ok : (h->cic->gen_ok && h->cic->in_eb == 2)) && ddc_stage_a_ok(h.get());
  if (h->fused) {
    h->hl = round_up(256 * cic->R + (int)h->cic->h_taps.size() + 48, 64);
    if ((rc = h->hist.init(cic->n_channels, h->hl, h->cic->in_eb)) || (rc = h->plansA.init()) ||
        (rc = h->d_fragB.alloc(kGenFragWords * sizeof(uint32_t)))) {
      return rc;
    }
  }
  if ((rc = h->tm.init())) { return rc; }
  *out = h.release();
  return ACDSP_OK;
}

// The cascade with a decimating second stage: ac_cic_dec_full -> ac_poly_dec on the INT_TYPE words.  Same handle type, same refusals in the
// same order; `fir` stays null and every acdsp_ddc_* call branches on `pd`.
int32_t acdsp_ddc_create_polydec(const acdsp_cic_desc_t *cic, const acdsp_polydec_desc_t *pd, int32_t ddc_flags, acdsp_ddc_t *out) {
  if (!cic || !pd || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  int rc;
  if ((rc = ddc_flag_refusals(*cic, *pd, ddc_flags))) { return rc; }
  if (cic->interp) { return fail(ACDSP_EINVAL, "ddc: stage A must be the decimator"); }
  if (cic->n_channels != pd->n_channels || cic->device != pd->device) { return fail(ACDSP_EINVAL, "ddc: both stages must cover the same channels on one device"); }
  acdsp_fmt_t it;
  if ((rc = acdsp_cic_int_type(cic, &it))) { return rc; }   // (host arithmetic: a decimator without an INT_TYPE is refused here, as its create would)
  const auto is_it = [&](const acdsp_fmt_t &f) { return f.W == it.W && f.I == it.I && f.S == it.S; };
  if (!is_it(cic->out) || !is_it(pd->in)) {
    return fail(ACDSP_EINVAL, "ddc: the decimator's OUT_TYPE and the ac_poly_dec's IN_TYPE must both be the INT_TYPE <%d,%d>", it.W, it.I);
  }
  const bool in_bytes = (ddc_flags & ACDSP_DDC_IN_BYTES) != 0;
  std::unique_ptr<acdsp_ddc, int32_t (*)(acdsp_ddc_t)> h(new acdsp_ddc(), acdsp_ddc_destroy);
  h->cic_desc = *cic; h->pd_desc = *pd; h->ddc_flags = ddc_flags; h->df = pd->df;
  memset(&h->fir_desc, 0, sizeof h->fir_desc);
  acdsp_cic_desc_t stage_a = *cic;
  if (in_bytes) { stage_a.flags |= ACDSP_FLAG_IN_BYTES; }
  if ((rc = acdsp_cic_create(&stage_a, &h->cic)) || (rc = acdsp_polydec_create(pd, &h->pd))) { return rc; }
  if (h->cic->out_eb != h->pd->in_eb) { return fail(ACDSP_EHIP, "internal: the stages disagree about the INT_TYPE container"); }
  // the fused class: int16 rows, DF = 2, a prototype of at most 128 taps, an exact-sum accumulator, int32 output containers
  static const bool no_fuse = getenv("ACDSP_NO_FUSE") != nullptr;
  h->fused = !no_fuse && !in_bytes && pd->df >= 2 && pd->df <= kDdcMaxFusedDf && (int64_t)pd->n_taps * pd->df <= 128 && h->pd->lossless_shape &&
             !(pd->flags & ACDSP_FLAG_FORCE_GENERIC) && !(cic->flags & ACDSP_FLAG_FORCE_GENERIC) && h->pd->out_eb == 4 && h->cic->gen_ok &&
             h->cic->in_eb == 2 && ddc_stage_a_ok(h.get());
  if (h->fused) {
    h->hl = round_up(256 * cic->R + (int)h->cic->h_taps.size() + 48, 64);   // the warm-up is ONE stage-A sub-step, as in the FIR cascade
    if ((rc = h->hist.init(cic->n_channels, h->hl, h->cic->in_eb)) || (rc = h->plansA.init()) ||
        (rc = h->d_fragB.alloc(kDdcMaxFusedDf * kGenFragWords * sizeof(uint32_t)))) {
      return rc;
    }
  }
  if ((rc = h->tm.init())) { return rc; }
  *out = h.release();
  return ACDSP_OK;
}

// acdsp_ddc_set_coeffs of a polydec cascade: the [NTAPS*DF] set of acdsp_polydec_set_coeffs; fused mode plans the prototype at every window
// phase first_b = DF - 1 - q and uploads all of them here, so that a capture finds the plan of whatever phase the stream stands in
static int32_t ddc_polydec_set_coeffs(acdsp_ddc_t h, const int64_t *coeffs) {
  int rc = acdsp_polydec_set_coeffs(h->pd, coeffs);   // validation + the two-kernel path's own plan
  if (rc) { return rc; }
  const acdsp_polydec_desc_t &d = h->pd->d;
  const int n = d.n_taps * d.df;
  if (h->fused) {
    std::vector<int64_t> hh((size_t)n, 0);
    for (int df = 0; df < d.df; df++) { for (int tp = 0; tp < d.n_taps; tp++) { hh[df + tp * d.df] = coeffs[tp + d.n_taps * df]; } }
    std::vector<uint32_t> fr[kDdcMaxFusedDf];
    bool ok = h->pd->lossless;
    for (int q = 0; ok && q < d.df; q++) {
      ok = fir_gen_plan(hh.data(), n, d.df, d.df - 1 - q, &h->planBq[q], &fr[q]) && fr[q].size() <= kGenFragWords && cascade_dec_plan_ok(h->planBq[q], d.df, d.df - 1 - q);
    }
    if (!ok) {
      if (h->t_total != 0) { return fail(ACDSP_EUNSUPPORTED, "ddc: this coefficient set does not fit the fused kernel and the stream has started"); }
      h->fused = false;   // before the first sample: the two kernels for the handle's lifetime
    } else {
      HIP_TRY(hipDeviceSynchronize());
      for (int q = 0; q < d.df; q++) {
        HIP_TRY(hipMemcpy(h->d_fragB.get<uint32_t>() + (size_t)q * kGenFragWords, fr[q].data(), fr[q].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      }
    }
  }
  h->h_pd_coeffs.assign(coeffs, coeffs + n);
  h->coeffs_set = true;
  return ACDSP_OK;
}

int32_t acdsp_ddc_set_coeffs(acdsp_ddc_t h, const int64_t *coeffs) {
  if (!h || !coeffs) { return fail(ACDSP_EINVAL, "null argument"); }
  if (h->pd) { return ddc_polydec_set_coeffs(h, coeffs); }
  int rc = acdsp_fir_set_coeffs(h->fir, coeffs);   // validation + the two-kernel path's own fragments
  if (rc) { return rc; }
  if (h->fused) {
    const acdsp_fir_desc_t &d = h->fir->d;
    std::vector<int64_t> eff = effective_coeffs(coeffs, d.n_taps, internal_ftype(d.kind, d.ftype));
    std::vector<uint32_t> fr;
    if (!fir_gen_plan(eff.data(), d.n_taps, 1, 0, &h->planB, &fr) || fr.size() > kGenFragWords || h->planB.nb > 3 ||
        h->planB.pc > 2 || h->planB.off != 128) {   // (byte rows: stage B's plan class is the int16 cascade's, on four planes)
      if (h->t_total != 0) { return fail(ACDSP_EUNSUPPORTED, "ddc: this coefficient set does not fit the fused kernel and the stream has started"); }
      h->fused = false;   // before the first sample: the two kernels for the handle's lifetime
    } else {
      HIP_TRY(hipDeviceSynchronize());
      if ((rc = h->d_fragB.upload(fr.data(), fr.size() * sizeof(uint32_t)))) { return rc; }
    }
  }
  h->coeffs_set = true;
  return ACDSP_OK;
}

// Deep copy: both stage descriptors, the coefficients when set, and the stream state of the mode the handle runs in -- the input history and
// input count of the fused kernel, or clones of the two stage handles.  Plans, the intermediate buffer and the timers are the clone's own.
int32_t acdsp_ddc_clone(acdsp_ddc_t h, acdsp_ddc_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_ddc_t c = nullptr;
  int rc = h->pd ? acdsp_ddc_create_polydec(&h->cic_desc, &h->pd_desc, h->ddc_flags, &c) : acdsp_ddc_create_ex(&h->cic_desc, &h->fir_desc, h->ddc_flags, &c);
  if (rc) { return rc; }
  std::unique_ptr<acdsp_ddc, int32_t (*)(acdsp_ddc_t)> guard(c, acdsp_ddc_destroy);
  // (the clone's stream has not started: a set that does not fit the fused kernel moves it to the two kernels, as it moved the original)
  if (h->coeffs_set && (rc = acdsp_ddc_set_coeffs(c, h->pd ? h->h_pd_coeffs.data() : h->fir->h_coeffs.data()))) { return rc; }
  if (c->fused != h->fused) { return fail(ACDSP_EHIP, "internal: ddc_clone resolved to another kernel mode than its original"); }
  HIP_TRY(hipDeviceSynchronize());
  if (h->fused) {
    if ((rc = c->hist.copy_from(h->hist))) { return rc; }
    c->t_total = h->t_total;
  } else {
    acdsp_cic_t cic = nullptr;
    acdsp_fir_t fir = nullptr;
    if ((rc = acdsp_cic_clone(h->cic, &cic))) { return rc; }
    acdsp_cic_destroy(c->cic);
    c->cic = cic;
    if (h->pd) {   // ... and the queued words, at the front of the clone's own intermediate rows
      acdsp_polydec_t pd = nullptr;
      if ((rc = acdsp_polydec_clone(h->pd, &pd))) { return rc; }
      acdsp_polydec_destroy(c->pd);
      c->pd = pd;
      if (h->n_q > 0) {
        if ((rc = ddc_mid_reserve(c, ddc_queue_cap(h->df), nullptr))) { return rc; }
        const size_t eb = (size_t)h->cic->out_eb;
        HIP_TRY(hipMemcpy2D(c->d_mid.get(), (size_t)c->mid_cap * eb, h->d_mid.get(), (size_t)h->mid_cap * eb, (size_t)h->n_q * eb, (size_t)h->cic->d.n_channels,
                            hipMemcpyDeviceToDevice));
        c->n_q = h->n_q;
      }
    } else {
      if ((rc = acdsp_fir_clone(h->fir, &fir))) { return rc; }
      acdsp_fir_destroy(c->fir);
      c->fir = fir;
    }
  }
  *out = guard.release();
  return ACDSP_OK;
}

int64_t acdsp_ddc_out_count(acdsp_ddc_t h, int64_t n_in) {
  if (!h || n_in < 0) { return -1; }
  int64_t n_mid;   // words the decimator emits
  if (!h->fused) { n_mid = acdsp_cic_out_count(h->cic, n_in); }
  else {
    const int R = h->cic->d.R;
    const int64_t first = (R - h->t_total % R) % R;
    n_mid = n_in > first ? (n_in - first + R - 1) / R : 0;
  }
  return h->pd ? (ddc_queued(h) + n_mid) / h->df : n_mid;   // whole groups of DF, the waiting words included
}

int32_t acdsp_ddc_path(acdsp_ddc_t h) { return h ? (h->fused ? 1 : 0) : -1; }

int32_t acdsp_ddc_in_elem_bytes(acdsp_ddc_t h) { return h ? h->cic->in_eb : -1; }

int32_t acdsp_ddc_reset(acdsp_ddc_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = acdsp_cic_reset(h->cic);
  if (!rc) { rc = h->pd ? acdsp_polydec_reset(h->pd) : acdsp_fir_reset(h->fir); }
  if (rc) { return rc; }
  h->n_q = 0;
  if ((rc = h->hist.zero())) { return rc; }   // (fused mode only: otherwise there is none)
  h->t_total = 0;
  return ACDSP_OK;
}

int32_t acdsp_ddc_run(acdsp_ddc_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                      int64_t *n_out, void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (!h->coeffs_set) { return fail(ACDSP_ESTATE, "ddc_run before acdsp_ddc_set_coeffs"); }
  if (n_in < 0 || (n_in > 0 && (!d_in || in_stride < n_in))) { return fail(ACDSP_EINVAL, "ddc_run: bad input arguments"); }
  const int64_t no = acdsp_ddc_out_count(h, n_in);
  if (n_out) { *n_out = no; }
  if (n_in == 0) { return ACDSP_OK; }
  if (no > 0 && (!d_out || out_stride < no)) { return fail(ACDSP_EINVAL, "ddc_run: output buffer too small for %lld outputs", (long long)no); }
  const acdsp_cic_desc_t &cd = h->cic->d;
  int rc = check_device(cd.device);
  if (rc) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  const bool capturing = stream_is_capturing(s);
  if (!h->fused) {
    // two kernels with the INT_TYPE stream in HBM between them.  Polydec cascade: the n_q words that wait from earlier calls stand at the
    // front of every row, the decimator writes behind them, ac_poly_dec takes the whole groups and the rest moves to the front
    const int df = h->pd ? h->df : 1;
    const int64_t n_mid = acdsp_cic_out_count(h->cic, n_in), tot = h->n_q + n_mid, rem = tot % df;
    const int64_t cap = (tot + 15) / 16 * 16 + 16;
    if (capturing) {
      // everything either stage would refuse, and a buffer that had to grow, before the first stream operation of the call
      if (cap > h->mid_cap) {
        return fail(ACDSP_ESTATE, "ddc_run under graph capture: the intermediate buffer holds %lld samples per channel and this call needs %lld; "
                    "run one eager call of at least this length before capturing", (long long)h->mid_cap, (long long)cap);
      }
      if ((rc = cic_capture_check(h->cic, d_in, in_stride, n_in))) { return rc; }
      if (h->pd && n_mid % df != 0) {
        return fail(ACDSP_ESTATE, "ddc_run under graph capture: the decimator emits %lld words, not a multiple of DF = %d (a replay would repeat the captured queue length)",
                    (long long)n_mid, df);
      }
      if (!h->pd && (rc = fir_capture_check(h->fir, h->d_mid.get(), h->mid_cap, no))) { return rc; }
      h->captured = true;
    }
    if ((rc = ddc_mid_reserve(h, cap, s))) { return rc; }
    const size_t eb = (size_t)h->cic->out_eb;
    unsigned char *mid = h->d_mid.get<unsigned char>();
    int64_t nn = 0;
    HIP_TRY(hipEventRecord(h->tm.start(), s));
    rc = acdsp_cic_run(h->cic, d_in, in_stride, n_in, mid + (size_t)h->n_q * eb, h->mid_cap, &nn, stream);
    if (!rc && nn != n_mid) { rc = fail(ACDSP_EHIP, "internal: the decimator emitted another word count than it announced"); }
    if (!rc && no > 0) {
      rc = h->pd ? acdsp_polydec_run(h->pd, mid, h->mid_cap, no * df, d_out, out_stride, stream) : acdsp_fir_run(h->fir, mid, h->mid_cap, nn, d_out, out_stride, stream);
    }
    HIP_TRY(hipEventRecord(h->tm.stop(), s));
    h->tm.commit();
    if (!rc && h->pd) {
      if (rem > 0 && no > 0) {   // (no == 0: every word of the row waits where it stands)
        const int nb = (int)(rem * (int64_t)eb), n_ch = h->cic->d.n_channels;
        const int64_t total = (int64_t)n_ch * nb;
        hipLaunchKernelGGL(ddc_queue_move_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mid, (int64_t)h->mid_cap * (int64_t)eb,
                           no * df * (int64_t)eb, nb, n_ch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { return fail(ACDSP_EHIP, "ddc queue kernel launch failed: %s", hipGetErrorString(e)); }
      }
      h->n_q = rem;
    }
    return rc;
  }
  // fused: alignment is the only per-call requirement
  if (!rows_in_slots(d_in, in_stride, h->cic->in_eb, n_in) || !rows_vec_aligned(d_out, out_stride, 4)) {
    return fail(ACDSP_EUNSUPPORTED, "ddc_run (fused): rows must be 16-byte aligned and readable up to a multiple of 16 samples");
  }
  const int R = cd.R;
  if (capturing && n_in % R != 0) {
    return fail(ACDSP_ESTATE, "ddc_run under graph capture: n_in = %lld is not a multiple of R = %d (a replay would repeat the captured decimation phase)",
                (long long)n_in, R);
  }
  if (capturing && h->pd && n_in % ((int64_t)R * h->df) != 0) {
    return fail(ACDSP_ESTATE, "ddc_run under graph capture: n_in = %lld is not a multiple of R * DF = %lld (a replay would repeat the captured queue length)",
                (long long)n_in, (long long)R * h->df);
  }
  const int64_t first = (R - h->t_total % R) % R;
  const int fm = (int)(first % 16);
  if (capturing && h->plansA.state(fm) == 0) {
    return fail(ACDSP_ESTATE, "ddc_run under graph capture: the stage-A plan of window phase %d (t_total %% R = %lld) is not on the device yet and its upload "
                "synchronises the stream; one eager call at that phase unlocks it (so does the eager call in front of the capture)", fm, (long long)(h->t_total % R));
  }
  if (!capturing) {
    int fms[3];
    decimator_phases(R, h->t_total, n_in, fms);
    if ((rc = h->plansA.prepare(h->cic->h_taps, R, fms, 3, s))) { return rc; }
  }
  const FirGenPlan *planA = nullptr;
  const uint32_t *fragA = nullptr;
  h->plansA.get(fm, &planA, &fragA);
  if (!planA) { return fail(ACDSP_EUNSUPPORTED, "ddc_run (fused): decimator shape outside the fused kernel"); }
  FirParams pa, pb;
  ddc_stage_params(h, &pa, &pb);
  pa.in_stride = in_stride; pa.n = n_in; pa.x = d_in; pa.hist = h->hist.cur();
  pb.y = d_out; pb.out_stride = out_stride; pb.n = no;
  HIP_TRY(hipEventRecord(h->tm.start(), s));
  hipError_t e;
  if (h->pd) {
    // stage B's window phase: output 0 of the call leaves with local word DF - 1 - q.  (no == 0: nothing to launch, the history moves on)
    const int q = (int)ddc_queued(h);
    e = launch_cascade_dec(pa, *planA, fragA, h->cic->it.W, first, pb, h->planBq[q], h->d_fragB.get<uint32_t>() + (size_t)q * kGenFragWords, h->df,
                           h->df - 1 - q, no, s);
  } else {
    e = launch_cascade(pa, *planA, fragA, h->cic->it.W, first, pb, h->planB, h->d_fragB.get<uint32_t>(), no, s);
  }
  if (e == hipErrorNotSupported) { return fail(ACDSP_EUNSUPPORTED, "ddc_run (fused): shape outside the compiled cascade kernel"); }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "cascade kernel launch failed: %s", hipGetErrorString(e)); }
  HIP_TRY(hipEventRecord(h->tm.stop(), s));
  h->tm.commit();
  const int nxt = h->hist.next(pa.n >= pa.hl);
  e = launch_fir_hist_update(pa, h->hist.at(nxt), s);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "ddc state kernel launch failed: %s", hipGetErrorString(e)); }
  h->hist.commit(nxt);
  h->t_total += n_in;
  return ACDSP_OK;
}

int32_t acdsp_ddc_kernel_stats(acdsp_ddc_t h, int32_t last_k, float *avg_ms, float *min_ms) {
  if (!h) { return fail(ACDSP_EINVAL, "null argument"); }
  return h->tm.stats(last_k, avg_ms, min_ms);
}

}  // extern "C"

