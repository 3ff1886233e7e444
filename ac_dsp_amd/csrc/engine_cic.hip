// engine_cic.hip -- acdsp_cic_*: ac_cic_dec_full / ac_cic_intr_full behind the C ABI
#include "engine_common.hpp"

using namespace acdsp;
using namespace acdsp::eng;

// ---------------------------------------------------------------------------------------------
// CIC
// ---------------------------------------------------------------------------------------------
namespace {

int log2_ceil_u64(uint64_t x) {
  int lf = 63;
  while (lf > 0 && !((x >> lf) & 1)) { lf--; }
  return (x == (1ull << lf)) ? lf : lf + 1;
}

// find_inter_type_cic_dec / _intr: reference ac_cic_dec_full.h:116-137, ac_cic_intr_full.h:107-127.
// power<> is an `int` enum there, so parameter sets whose product reaches 2^31 do not compile in
// the reference; they are rejected here.
int cic_int_type(const acdsp_cic_desc_t &d, acdsp_fmt_t *it) {
  if (d.R < 1 || d.M < 1 || d.N < 1) { return fail(ACDSP_EINVAL, "CIC: R, M, N must be >= 1"); }
  uint64_t pr = 1, pm = 1;
  const int er = d.interp ? d.N - 1 : d.N;
  for (int i = 0; i < er; i++) { pr *= (uint64_t)d.R; if (pr >= (1ull << 31)) { return fail(ACDSP_EUNSUPPORTED, "CIC: R^N overflows the reference's int power<>"); } }
  for (int i = 0; i < d.N; i++) { pm *= (uint64_t)d.M; if (pm >= (1ull << 31)) { return fail(ACDSP_EUNSUPPORTED, "CIC: M^N overflows the reference's int power<>"); } }
  if (pr * pm >= (1ull << 31)) { return fail(ACDSP_EUNSUPPORTED, "CIC: (R*M)^N overflows the reference's int power<>"); }
  const int outF = d.in.W - d.in.I;
  const int outW = log2_ceil_u64(pr * pm) + d.in.W + (d.in.S ? 0 : 1);
  it->W = outW; it->I = outW - outF; it->S = 1; it->Q = ACDSP_TRN; it->O = ACDSP_WRAP;
  return ACDSP_OK;
}

// The byte-container flags of a CIC descriptor (`flags`: the descriptor's, or those of them the caller looks at): *in_eb, or what is refused
// before any device use
int cic_byte_rows(const acdsp_cic_desc_t &d, int flags, int *in_eb) {
  int out_eb;
  const int rc = byte_rows("CIC", flags, d.in, d.out, nullptr, in_eb, &out_eb);
  if (rc || *in_eb != 1) { return rc; }
  if (d.interp) { return fail(ACDSP_EUNSUPPORTED, "CIC: ACDSP_FLAG_IN_BYTES on an interpolator (interp == 1) is not supported: its input stream is the thin one"); }
  if (d.out.W > 64) { return fail(ACDSP_EUNSUPPORTED, "CIC: ACDSP_FLAG_IN_BYTES with an OUT_TYPE wider than 64 bits (W=%d) is not supported", d.out.W); }
  return ACDSP_OK;
}

}  // namespace

extern "C" {

int32_t acdsp_cic_int_type(const acdsp_cic_desc_t *desc, acdsp_fmt_t *it) {
  if (!desc || !it) { return fail(ACDSP_EINVAL, "null argument"); }
  return cic_int_type(*desc, it);
}

int32_t acdsp_cic_create(const acdsp_cic_desc_t *desc, acdsp_cic_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  int rc;
  if ((rc = check_fmt(desc->in, "IN_TYPE")) || (rc = check_fmt(desc->out, "OUT_TYPE", 128))) { return rc; }
  acdsp_fmt_t it;
  if ((rc = cic_int_type(*desc, &it))) { return rc; }
  // INT_TYPE (reference ac_cic_dec_full.h:116-137, ac_cic_intr_full.h:107-127) of up to 128 bits; more than 64 -> wide.hip
  if (it.W > 128) { return fail(ACDSP_EUNSUPPORTED, "CIC: intermediate type needs %d bits (> 128)", it.W); }
  {
    const int fo = desc->out.W - desc->out.I, fi = desc->in.W - desc->in.I;
    if (it.W + (fo > fi ? fo - fi : 0) > 250) { return fail(ACDSP_EUNSUPPORTED, "CIC: OUT_TYPE conversion needs more than 256-bit intermediates"); }
  }
  if (desc->N > kCicMaxN) { return fail(ACDSP_EUNSUPPORTED, "CIC: N=%d > %d", desc->N, kCicMaxN); }
  // rate counters are ac_int<8,false> in the reference (ac_cic_full_core.h:72-73)
  if (desc->R > 256) { return fail(ACDSP_EUNSUPPORTED, "CIC: R=%d > 256 (8-bit rate counter in the reference)", desc->R); }
  if (desc->interp && desc->R < 2) { return fail(ACDSP_EUNSUPPORTED, "CIC interpolator: R=1 never re-arms in the reference (ac_cic_full_core.h:146-158)"); }
  if (desc->interp && desc->N > 255) { return fail(ACDSP_EUNSUPPORTED, "CIC: N too large"); }
  if (desc->n_channels < 1) { return fail(ACDSP_EINVAL, "CIC: n_channels=%d must be positive", desc->n_channels); }
  if (desc->n_channels > 65535) { return fail(ACDSP_EUNSUPPORTED, "CIC: n_channels=%d outside 1..65535", desc->n_channels); }
  int in_eb;
  if ((rc = cic_byte_rows(*desc, desc->flags, &in_eb))) { return rc; }
  const bool in_bytes = in_eb == 1;
  if ((rc = check_device(desc->device))) { return rc; }
  std::unique_ptr<acdsp_cic> h(new acdsp_cic());   // (check_device has made the device current: a failure below frees there)
  h->d = *desc;
  h->it = it;
  h->in_eb = in_eb;
  h->out_eb = elem_bytes(desc->out.W);
  h->me = desc->M < 2 ? desc->M : 2;  // effective comb delay of the reference's delay line, see cic.hip
  h->wide = it.W > 64 || desc->out.W > 64;
  const int64_t mem = desc->interp ? (int64_t)desc->N * h->me + 1 : (int64_t)desc->N * desc->R * h->me - 1;
  h->hl = round_up((int)(mem > 1 ? mem : 1) + 16, kCicTile);   // + 16: the 16-aligned input windows of fir_gen
  h->warm = h->hl;
  // FIR identity of both directions: h = z^-(N-1) * boxcar(R*M')^N, all arithmetic mod 2^64 (then mod 2^outW)
  cic2_stage1_taps(desc->R * h->me, desc->N, &h->h_taps);
  const bool no_gen = knob_no_gen();
  FirGenPlan probe;
  std::vector<uint32_t> fr;
  // decimator on the matrix cores through that identity (fir_gen.hip): where the taps have a plan at both ends of the window offsets
  // (byte rows: fir_gen.hip has no 1-byte shape -- every rate with a byte stage-1 shape goes to the two-stage kernel, the rest to the recurrence kernel)
  h->gen_plan_ok = !desc->interp && !h->wide && !no_gen &&
                   fir_gen_plan(h->h_taps.data(), (int)h->h_taps.size(), desc->R, 15, &probe, &fr) &&   // worst-case window offset
                   fir_gen_plan(h->h_taps.data(), (int)h->h_taps.size(), desc->R, 0, &probe, &fr);
  h->gen_ok = !in_bytes && fits_container(desc->in, h->in_eb) && h->gen_plan_ok;
  {
    // two-stage decimator (cic2.hip) where R = R1 R2 with a compiled stage-1 rate: its chunk 0 starts `wu` steps of 256 R1 inputs early,
    // so the handle keeps that much input history (the samples beyond the filter memory only ever feed warm-up values the combs cancel)
    // (below R = 32 the one-stage FIR identity serves the rates it has a plan for; where it has none -- R M N too many taps, e.g. R 24 M 2 N 4 -- the
    // two-stage kernel takes over there as well instead of the recurrence kernel)
    const bool one_stage = h->gen_ok && desc->R < 32;
    static const bool no_c2 = getenv("ACDSP_NO_CIC2") != nullptr;         // A/B knob: recurrence kernel as before
    // (ACDSP_NO_GEN: the two-stage kernel is a multi-plane matrix-core kernel too -- without the check a handle whose one-stage identity the knob
    // switched off came here instead of to the recurrence kernel, with the longer history of this kernel)
    static const bool c2_all = getenv("ACDSP_CIC2_ALL") != nullptr;       // A/B knob: also where the one-stage FIR identity fits (R < 32)
    if (!desc->interp && !h->wide && !no_c2 && !no_gen && (desc->R >= 32 || c2_all || !one_stage) && (in_bytes || fits_container(desc->in, h->in_eb)) && !(desc->flags & ACDSP_FLAG_FORCE_GENERIC) &&
        cic2_factor(h->in_eb, desc->R, h->me, desc->N, &h->c2_R1, &h->c2_R2, &h->c2_wu)) {
      cic2_stage1_taps(h->c2_R1, desc->N, &h->c2_taps);
      h->c2_ok = fir_gen_plan(h->c2_taps.data(), (int)h->c2_taps.size(), h->c2_R1, 15, &probe, &fr) &&
                 fir_gen_plan(h->c2_taps.data(), (int)h->c2_taps.size(), h->c2_R1, 0, &probe, &fr);
      if (h->c2_ok) {
        const int need = round_up(cic2_hist_len(h->in_eb, h->c2_R1, desc->N, h->c2_wu), kCicTile);
        if (need > h->hl) { h->hl = need; }
        h->c2_first = c2_all && one_stage;   // (acdsp_cic_run gives the one-stage kernel the first refusal otherwise: the knob chose nothing)
      }
    }
  }
  if ((rc = h->hist.init(desc->n_channels, h->hl, h->in_eb))) { return rc; }
  if ((desc->interp && !no_gen) || h->wide) {   // interpolator (and wide.hip): polyphase FIR kernel reads the taps themselves
    if ((rc = h->d_taps.alloc_upload(h->h_taps))) { return rc; }
    // ... and, where the shape is compiled in, the same identity phase by phase on the matrix cores
    const int R = desc->R, n_taps = (int)h->h_taps.size(), kmax = (n_taps + R - 1) / R;
    if (desc->interp && !h->wide && !(desc->flags & ACDSP_FLAG_FORCE_GENERIC) && fits_container(desc->in, h->in_eb) && (h->in_eb == 2 || h->in_eb == 4) && R <= 32) {
      std::vector<int64_t> E((size_t)R * kmax, 0);
      for (int r = 0; r < R; r++) { for (int k = 0; k < kmax; k++) { if (r + R * k < n_taps) { E[(size_t)r * kmax + k] = h->h_taps[(size_t)(r + R * k)]; } } }
      std::vector<uint32_t> frag;
      std::vector<int64_t> ucorr;
      FirUpPlan pl;
      if (fir_up_plan(E.data(), R, kmax, h->in_eb, &pl, &frag, &ucorr) && pl.pc <= 3 && pl.nb == 1 && fir_up_shape_ok(h->in_eb, h->in_eb, pl.nb, R, h->out_eb)) {
        if ((rc = h->d_upfrag.alloc_upload(frag)) || (rc = h->d_upcorr.alloc_upload(ucorr))) { return rc; }
        h->up_plan = pl; h->up_px = h->in_eb; h->up_ok = true;
      }
    }
  }
  if (h->gen_ok && (rc = h->gen.init())) { return rc; }
  if (h->c2_ok && (rc = h->c2.init())) { return rc; }
  if ((rc = h->tm.init())) { return rc; }
  *out = h.release();
  if (trace_handles()) { fprintf(stderr, "[acdsp] cic_create interp=%d R=%d M=%d N=%d n_channels=%d\n", desc->interp, desc->R, desc->M, desc->N, desc->n_channels); }
  return ACDSP_OK;
}

int32_t acdsp_cic_destroy(acdsp_cic_t h) {
  if (!h) { return ACDSP_OK; }
  if (trace_handles()) { fprintf(stderr, "[acdsp] cic_destroy kernel_runs=%lld\n", (long long)h->tm.count); }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

int32_t acdsp_cic_clone(acdsp_cic_t h, acdsp_cic_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_cic_t c = nullptr;
  int rc = acdsp_cic_create(&h->d, &c);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = c->hist.copy_from(h->hist))) { return rc; }
  c->t_total = h->t_total;
  *out = c;
  return ACDSP_OK;
}

int32_t acdsp_cic_path(acdsp_cic_t h) { return h ? h->last_path : -1; }

int32_t acdsp_cic_in_elem_bytes(acdsp_cic_t h) { return h ? h->in_eb : -1; }

int32_t acdsp_cic_two_stage_rates(const acdsp_cic_desc_t *desc, int32_t *R1, int32_t *R2) {
  if (!desc || !R1 || !R2) { return fail(ACDSP_EINVAL, "null argument"); }
  *R1 = *R2 = 0;
  int rc;
  if ((rc = check_fmt(desc->in, "IN_TYPE")) || (rc = check_fmt(desc->out, "OUT_TYPE", 128))) { return rc; }
  acdsp_fmt_t it;
  if ((rc = cic_int_type(*desc, &it))) { return rc; }
  int in_eb;
  if ((rc = cic_byte_rows(*desc, desc->flags & ~ACDSP_FLAG_OUT_BYTES, &in_eb))) { return rc; }   // (the rates do not depend on the OUT rows)
  const bool in_bytes = in_eb == 1;
  if (desc->interp || it.W > 64 || desc->out.W > 64 || desc->N > kCicMaxN || desc->R > 256) { return ACDSP_OK; }
  if ((desc->flags & ACDSP_FLAG_FORCE_GENERIC) || !(in_bytes || fits_container(desc->in, in_eb))) { return ACDSP_OK; }
  int r1 = 0, r2 = 0, wu = 0;
  if (cic2_factor(in_eb, desc->R, desc->M < 2 ? desc->M : 2, desc->N, &r1, &r2, &wu)) { *R1 = r1; *R2 = r2; }
  return ACDSP_OK;
}

int32_t acdsp_cic_reset(acdsp_cic_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->hist.zero())) { return rc; }
  h->t_total = 0;
  return ACDSP_OK;
}

static void cic_window(const acdsp_cic *h, int64_t n_in, CicParams *p) {
  const int R = h->d.R;
  p->t_prev = h->t_total;
  if (!h->d.interp) {
    // decIntgCore emits when rate_cnt == 0, i.e. at global input indices 0, R, 2R, ... (ac_cic_full_core.h:116-133)
    p->phase0 = (int)(h->t_total % R);
    p->first = (R - p->phase0) % R;
    p->q_begin = p->q_end = p->q_skip = 0;
  } else {
    // intrIntg: the call that consumes inputs T..T+K-1 runs iterations [(T-1)R+1, (T+K-1)R+1)
    // (first call starts at 0); the first N-1 iterations ever are dropped (ac_cic_intr_full.h:200-213)
    p->phase0 = 0; p->first = 0;
    p->q_begin = h->t_total == 0 ? 0 : (h->t_total - 1) * R + 1;
    p->q_end = n_in > 0 ? (h->t_total + n_in - 1) * R + 1 : p->q_begin;
    p->q_skip = h->d.N - 1;
  }
}

int64_t acdsp_cic_out_count(acdsp_cic_t h, int64_t n_in) {
  if (!h || n_in < 0) { return -1; }
  if (n_in == 0) { return 0; }
  CicParams p;
  cic_window(h, n_in, &p);
  if (!h->d.interp) { return n_in > p.first ? (n_in - p.first + h->d.R - 1) / h->d.R : 0; }
  int64_t lo = p.q_begin > p.q_skip ? p.q_begin : p.q_skip;
  return p.q_end > lo ? p.q_end - lo : 0;
}

}  // extern "C"

// What acdsp_cic_run refuses while its stream is capturing, decided before the call touches the stream or the handle (the two-kernel DDC asks
// before its own first stream operation): calls whose host-side phase a replay would repeat, and decimator calls whose window phase has no
// uploaded fir_gen plan yet -- the upload synchronises the stream.
int acdsp::eng::cic_capture_check(const acdsp_cic *h, const void *d_in, int64_t in_stride, int64_t n_in) {
  const acdsp_cic_desc_t &d = h->d;
  if (d.interp) {
    if (h->t_total == 0) {
      return fail(ACDSP_ESTATE, "cic_run under graph capture: the interpolator's first call drops its start-up outputs and cannot be replayed; run it before capturing");
    }
    return ACDSP_OK;
  }
  if (n_in % d.R != 0) {
    return fail(ACDSP_ESTATE, "cic_run under graph capture: n_in = %lld is not a multiple of R = %d (a replay would repeat the captured decimation phase)",
                (long long)n_in, d.R);
  }
  if (!rows_in_slots(d_in, in_stride, h->in_eb, n_in)) { return ACDSP_OK; }   // the recurrence kernel: no plan
  const int fm = (int)(((d.R - h->t_total % d.R) % d.R) % 16);
  int st = -1;
  if (h->gen_ok && !h->c2_first) { st = h->gen.state(fm); }
  if (st < 0 && h->c2_ok) { st = h->c2.state(fm); }
  if (st == 0) {
    return fail(ACDSP_ESTATE, "cic_run under graph capture: the matrix-core plan of window phase %d (t_total %% R = %lld) is not on the device yet and its upload "
                "synchronises the stream; one eager call at that phase unlocks it (so does the eager call in front of the capture)", fm, (long long)(h->t_total % d.R));
  }
  return ACDSP_OK;
}

extern "C" {

int32_t acdsp_cic_run(acdsp_cic_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                      int64_t *n_out, void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n_in < 0 || (n_in > 0 && (!d_in || in_stride < n_in))) { return fail(ACDSP_EINVAL, "cic_run: bad input arguments"); }
  const int64_t no = acdsp_cic_out_count(h, n_in);
  if (n_out) { *n_out = no; }
  if (n_in == 0) { return ACDSP_OK; }
  if (no > 0 && (!d_out || out_stride < no)) { return fail(ACDSP_EINVAL, "cic_run: output buffer too small for %lld outputs", (long long)no); }
  const acdsp_cic_desc_t &d = h->d;
  int rc = check_device(d.device);
  if (rc) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  const bool capturing = stream_is_capturing(s);
  if (capturing && (rc = cic_capture_check(h, d_in, in_stride, n_in))) { return rc; }
  CicParams p;
  cic_window(h, n_in, &p);
  p.q_from = p.q_to = 0;
  p.interp = d.interp; p.R = d.R; p.me = h->me; p.N = d.N; p.n_ch = d.n_channels;
  p.w_int = h->it.W;
  p.in = make_dfmt(d.in);
  if (h->wide) { memset(&p.out, 0, sizeof p.out); } else { p.out = make_dfmt(d.out); }
  p.in_eb = h->in_eb; p.out_eb = h->out_eb;
  p.hl = h->hl; p.warm_tiles = h->warm / kCicTile;
  p.t_from = 0; p.emit_from = 0;
  p.vec_ok = rows_vec_aligned(d_in, in_stride, h->in_eb);
  const bool slots = rows_in_slots(d_in, in_stride, h->in_eb, n_in);
  p.out_simple = (p.out.F == p.in.F && p.out.O == ACDSP_WRAP) ? ((p.out.S && p.out.W >= h->it.W) ? 2 : 1) : 0;
  p.in_stride = in_stride; p.out_stride = out_stride; p.n_in = n_in;
  p.x = d_in; p.y = d_out; p.hist = h->hist.cur();
  // chunking: aim at >= 4096 waves, keep the warm-up below ~6 % of a chunk
  const int64_t groups = (d.n_channels + 63) / 64;
  int64_t chunk = (n_in * groups + 4095) / 4096;
  const int64_t floor_chunk = (int64_t)16 * h->warm > 1024 ? (int64_t)16 * h->warm : 1024;
  if (chunk < floor_chunk) { chunk = floor_chunk; }
  p.chunk = (chunk + kCicTile - 1) / kCicTile * kCicTile;
  // decimator on the matrix cores when the FIR identity fits and the rows are slot-aligned
  bool use_gen = h->gen_ok && !h->c2_first && !d.interp && slots;
  const uint32_t *gfrag = nullptr, *c2frag = nullptr;
  const FirGenPlan *gpl = nullptr, *c2pl = nullptr;
  const int fm = (int)(p.first % 16);
  if (!capturing && (use_gen || (h->c2_ok && slots))) {
    // plans of this call's window phase, of the next call's and of phase 0: a capture that follows finds them uploaded (cic_capture_check)
    int fms[3];
    decimator_phases(d.R, h->t_total, n_in, fms);
    if (use_gen && (rc = h->gen.prepare(h->h_taps, d.R, fms, 3, s))) { return rc; }
    const bool gen_all = use_gen && h->gen.state(fms[0]) == 1 && h->gen.state(fms[1]) == 1 && h->gen.state(fms[2]) == 1;
    if (h->c2_ok && !gen_all && (rc = h->c2.prepare(h->c2_taps, h->c2_R1, fms, 3, s))) { return rc; }
  }
  if (use_gen) {
    h->gen.get(fm, &gpl, &gfrag);
    use_gen = gpl != nullptr;
  }
  // ... or in two stages (R = R1 R2, cic2.hip) where the one-stage window does not fit: complete chunks there, the ragged end on the recurrence kernel
  bool use_c2 = h->c2_ok && !use_gen && slots;
  if (use_c2) {
    h->c2.get(fm, &c2pl, &c2frag);
    use_c2 = c2pl != nullptr;
  }
  const bool use_intr_fir = d.interp && h->d_taps && !h->wide;
  h->last_path = h->wide ? ACDSP_PATH_WIDE : (use_gen ? ACDSP_PATH_MFMA_GEN : (use_intr_fir ? ACDSP_PATH_LOSSLESS64 : 0));
  HIP_TRY(hipEventRecord(h->tm.start(), s));
  hipError_t e;
  if (h->wide) {
    CicWideParams pw;
    pw.p = p; pw.out = make_wfmt(d.out);
    e = launch_cic_wide(pw, h->d_taps.get<int64_t>(), (int)h->h_taps.size(), no, s);
  } else if (use_gen) {
    FirParams k = fir_params_of(p.in, p.in, p.out, p.out, h->in_eb, h->out_eb, h->hl, d.n_channels, {d_in, in_stride, n_in, d_out, out_stride});
    k.hist = h->hist.cur();
    e = launch_fir_gen(k, *gpl, gfrag, 1, h->it.W, p.first, no, s);
  } else if (use_intr_fir) {
    // whole steps of 32 input slots on the matrix cores; the head (history, earlier-call phase) and the tail (the call's
    // last input emits only its first iteration, ac_cic_intr_full.h:200-205) on the polyphase VALU kernel
    int64_t q_a = 0, q_b = 0;
    const int64_t lo = p.q_begin > p.q_skip ? p.q_begin : p.q_skip;
    p.q_from = p.q_to = 0;
    static const bool no_up = getenv("ACDSP_NO_CIC_UP") != nullptr;   // A/B knob: polyphase VALU kernel only
    if (h->up_ok && p.vec_ok && !no_up) {
      const int64_t slot_a = h->up_plan.hs, n_steps = ((n_in - 1) / 16 - slot_a) / 32;
      const int64_t out_off = (int64_t)d.R * p.t_prev - lo;
      // 8-byte stores: 4-byte containers may start on odd elements (a continuing call starts R - 1 outputs into a phase group, a first
      // call N - 1): gfx950 serves dword-aligned multi-dword stores
      const int64_t oal = h->out_eb == 4 ? 4 : 8;
      const bool out_ok = ((uintptr_t)d_out % oal == 0) && ((out_stride * h->out_eb) % oal == 0) && ((out_off * h->out_eb) % oal == 0);
      if (n_steps > 0 && out_ok && (int64_t)d.R * (p.t_prev + 16 * slot_a) >= lo) {
        const FirParams k = fir_params_of(p.in, p.in, p.out, p.out, h->in_eb, h->out_eb, 0, d.n_channels, {d_in, in_stride, n_in, d_out, out_stride});
        e = launch_fir_up(k, h->up_plan, h->up_px, h->d_upfrag.get<uint32_t>(), h->d_upcorr.get<int64_t>(), 1, h->it.W, p.out_simple, 0, -1, slot_a, n_steps, out_off, s);
        if (e == hipSuccess) {
          q_a = (int64_t)d.R * (p.t_prev + 16 * slot_a); q_b = (int64_t)d.R * (p.t_prev + 16 * (slot_a + 32 * n_steps));
          h->last_path = ACDSP_PATH_MFMA_GEN;
        } else if (e != hipErrorNotSupported) {
          return fail(ACDSP_EHIP, "CIC interpolator matrix-core kernel launch failed: %s", hipGetErrorString(e));
        }
      }
    }
    if (q_b > q_a) {
      e = hipSuccess;
      if (q_a > lo) { p.q_from = lo; p.q_to = q_a; e = launch_cic_intr_fir(p, h->d_taps.get<int64_t>(), (int)h->h_taps.size(), s); }
      if (e == hipSuccess && p.q_end > q_b) { p.q_from = q_b; p.q_to = p.q_end; e = launch_cic_intr_fir(p, h->d_taps.get<int64_t>(), (int)h->h_taps.size(), s); }
      p.q_from = p.q_to = 0;
    } else {
      e = launch_cic_intr_fir(p, h->d_taps.get<int64_t>(), (int)h->h_taps.size(), s);
    }
  } else {
    int64_t covered = 0;
    e = hipSuccess;
    if (use_c2) { e = launch_cic2(p, *c2pl, c2frag, h->c2_R1, h->c2_R2, h->c2_wu, no, s, &covered); }
    if (e == hipSuccess && covered < no) {
      if (covered > 0) {            // the ragged end of the call: outputs from `covered` on, i.e. emitting samples from first + covered R on
        p.emit_from = p.first + covered * d.R;
        p.t_from = p.emit_from / kCicTile * kCicTile;
        p.chunk = (floor_chunk + kCicTile - 1) / kCicTile * kCicTile;      // a short rest: many short chunks
      }
      e = launch_cic(p, s);
      p.t_from = 0; p.emit_from = 0;
    }
    if (covered > 0) { h->last_path = ACDSP_PATH_CIC_2STAGE; }
  }
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "CIC kernel launch failed: %s", hipGetErrorString(e)); }
  HIP_TRY(hipEventRecord(h->tm.stop(), s));
  h->tm.commit();
  const int nxt = h->hist.next(p.n_in >= p.hl);
  e = launch_cic_hist_update(p, h->hist.at(nxt), s);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "CIC state kernel launch failed: %s", hipGetErrorString(e)); }
  h->hist.commit(nxt);
  h->t_total += n_in;
  return ACDSP_OK;
}

int32_t acdsp_cic_run_host(acdsp_cic_t h, const void *h_in, int64_t n_in, void *h_out, int64_t out_cap, int64_t *n_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (n_in < 0 || (n_in > 0 && !h_in)) { return fail(ACDSP_EINVAL, "cic_run_host: bad arguments"); }
  const int64_t no = acdsp_cic_out_count(h, n_in);
  if (n_out) { *n_out = no; }
  if (n_in == 0) { return ACDSP_OK; }
  if (no > out_cap || (no > 0 && !h_out)) { return fail(ACDSP_EINVAL, "cic_run_host: output capacity %lld < %lld", (long long)out_cap, (long long)no); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  const HostRows r = {h->d.n_channels, h_in, n_in, (n_in + 15) / 16 * 16, h->in_eb, h_out, no, (no + 7) / 8 * 8 + 8, no, h->out_eb};
  return run_host_staged(h->st, r, true, [&](const void *d_in, void *d_out, bool) { return acdsp_cic_run(h, d_in, r.si, n_in, d_out, r.so, nullptr, nullptr); });
}

int32_t acdsp_cic_last_kernel_ms(acdsp_cic_t h, float *ms) {
  if (!h || !ms) { return fail(ACDSP_EINVAL, "null argument"); }
  return h->tm.stats(1, ms, nullptr);
}

int32_t acdsp_cic_kernel_stats(acdsp_cic_t h, int32_t last_k, float *avg_ms, float *min_ms) {
  if (!h) { return fail(ACDSP_EINVAL, "null argument"); }
  return h->tm.stats(last_k, avg_ms, min_ms);
}

}  // extern "C"

