// engine_misc.hip -- acdsp_intgdump_* / acdsp_mvavg_*: ac_intg_dump and ac_mv_avg behind the C ABI
#include "engine_common.hpp"
#include "mv_avg_plan.hpp"

using namespace acdsp;
using namespace acdsp::eng;

// ---------------------------------------------------------------------------------------------
// integrate-and-dump: ac_intg_dump
// ---------------------------------------------------------------------------------------------
struct acdsp_intgdump {
  acdsp_intgdump_desc_t d;
  int in_eb, out_eb;
  History temp;                 // temp[]: n_objects x CHN ACC raw words (int64), ping-pong like an input history
  DevBuf d_blk;                 // int64 [3][cap] off / rounds / out
  DevBuf d_chain;               // int32 [cap]
  int64_t blk_cap = 0;
  bool captured = false;        // a call of this handle has been recorded into a graph, which holds d_blk / d_chain: a later (eager) call with
  std::vector<DevBuf> retired;  // another table keeps the old arrays here instead of freeing or overwriting them
  bool pending = false;         // the last call ended on a block that did not dump: temp[] is non-zero
  bool temp_zero = true;        // temp.cur() is known to be all zero (create / reset / zeroed behind a general-kernel call that dumped everything):
                                // what the tile / stream kernels rely on when they leave temp[] alone (advisor, round 5)
  int last_path = 0;            // acdsp_intgdump_path
  // block table of the last call: a stream that dumps on a fixed schedule passes the same n_sample[] every call, and then
  // neither the table is rebuilt nor uploaded and run() stays asynchronous (no stream synchronisation)
  std::vector<int64_t> last_ns;
  void *last_stream = nullptr;
  int64_t tbl_grp = 0, tbl_uni_rounds = 0, tbl_max_rounds = 0;
  int32_t tbl_start = 0;
  Staging st;
};

namespace {
// per block: rounds consumed and whether it dumps (ac_intg_dump.h:138-146)
inline int64_t intg_rounds(int64_t n_sample, int ns, bool *dumps) {
  *dumps = n_sample >= 1 && n_sample <= ns;
  return *dumps ? n_sample : ns;
}
}  // namespace

extern "C" {

int32_t acdsp_intgdump_destroy(acdsp_intgdump_t h) {
  if (!h) { return ACDSP_OK; }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

int32_t acdsp_intgdump_create(const acdsp_intgdump_desc_t *desc, acdsp_intgdump_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  const acdsp_intgdump_desc_t &d = *desc;
  if (d.ns < 1 || d.ns > (1 << 24)) { return fail(ACDSP_EUNSUPPORTED, "NS=%d outside 1..2^24", d.ns); }
  if (d.chn < 1 || d.chn > 4096) { return fail(ACDSP_EUNSUPPORTED, "CHN=%d outside 1..4096", d.chn); }
  if (d.n_objects < 1) { return fail(ACDSP_EINVAL, "n_objects=%d must be positive", d.n_objects); }
  if (d.n_objects > 65535) { return fail(ACDSP_EUNSUPPORTED, "n_objects=%d outside 1..65535", d.n_objects); }
  int rc;
  if ((rc = check_fmt(d.in, "IN_TYPE")) || (rc = check_fmt(d.acc, "ACC_TYPE")) || (rc = check_fmt(d.out, "OUT_TYPE"))) { return rc; }
  int in_eb, out_eb;
  if ((rc = byte_rows("intg_dump", d.flags, d.in, d.out, nullptr, &in_eb, &out_eb))) { return rc; }
  if ((rc = check_device(d.device))) { return rc; }
  std::unique_ptr<acdsp_intgdump> h(new acdsp_intgdump());   // (check_device has made the device current: a failure below frees there)
  h->d = d;
  h->in_eb = in_eb; h->out_eb = out_eb;
  if ((rc = h->temp.init(d.n_objects, d.chn, sizeof(int64_t)))) { return rc; }   // temp[i] = 0.0 (ac_intg_dump.h:86-89)
  *out = h.release();
  return ACDSP_OK;
}

int32_t acdsp_intgdump_counts(acdsp_intgdump_t h, const int64_t *n_sample, int64_t n_blocks, int64_t *n_in, int64_t *n_out) {
  if (!h || (n_blocks > 0 && !n_sample) || n_blocks < 0) { return fail(ACDSP_EINVAL, "intg_dump counts: bad arguments"); }
  int64_t rounds = 0, groups = 0;
  for (int64_t b = 0; b < n_blocks; b++) {
    bool dumps;
    rounds += intg_rounds(n_sample[b], h->d.ns, &dumps);
    groups += dumps ? 1 : 0;
  }
  if (n_in) { *n_in = rounds * h->d.chn; }
  if (n_out) { *n_out = groups * h->d.chn; }
  return ACDSP_OK;
}

int32_t acdsp_intgdump_run(acdsp_intgdump_t h, const void *d_in, int64_t in_stride, const int64_t *n_sample, int64_t n_blocks,
                           void *d_out, int64_t out_stride, int64_t *n_out, void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int64_t ni = 0, no = 0;
  int rc = acdsp_intgdump_counts(h, n_sample, n_blocks, &ni, &no);
  if (rc) { return rc; }
  if (n_out) { *n_out = no; }
  if (n_blocks == 0) { return ACDSP_OK; }
  if (n_blocks > (1 << 24)) { return fail(ACDSP_EUNSUPPORTED, "intg_dump run: more than 2^24 blocks in one call"); }
  if ((ni > 0 && (!d_in || in_stride < ni)) || (no > 0 && (!d_out || out_stride < no))) { return fail(ACDSP_EINVAL, "intg_dump run: buffers too small"); }
  const acdsp_intgdump_desc_t &d = h->d;
  if ((rc = check_device(d.device))) { return rc; }
  hipStream_t s = (hipStream_t)stream;
  if (stream_is_capturing(s)) {
    // A captured call only enqueues kernels: its block table is the one the preceding eager call on this stream uploaded, and it neither finds
    // nor leaves sums in temp[] (pending / temp_zero and the temp[] ping-pong are host-side state that a replay would not repeat)
    const bool same = n_blocks <= h->blk_cap && h->last_stream == stream && (int64_t)h->last_ns.size() == n_blocks &&
                      memcmp(h->last_ns.data(), n_sample, (size_t)n_blocks * sizeof(int64_t)) == 0;
    if (!same) {
      return fail(ACDSP_ESTATE, "intg_dump run under graph capture: the n_sample table differs from that of the last call on this stream and its upload "
                  "synchronises the stream; run one eager call with this table on the capture stream first");
    }
    if (h->pending) {
      return fail(ACDSP_ESTATE, "intg_dump run under graph capture: sums of blocks that did not dump are pending in temp[], host-side state a replay "
                  "would not repeat; capture from a call boundary behind a dump");
    }
    if (h->tbl_grp != n_blocks) {
      return fail(ACDSP_ESTATE, "intg_dump run under graph capture: the call holds blocks that do not dump, whose sums a replay would not carry "
                  "(host-side state); every block of a captured call must dump");
    }
    h->captured = true;
  }
  const bool same_table = n_blocks <= h->blk_cap && h->last_stream == stream && (int64_t)h->last_ns.size() == n_blocks &&
                          memcmp(h->last_ns.data(), n_sample, (size_t)n_blocks * sizeof(int64_t)) == 0;
  // A captured graph has the tables' addresses in its kernel arguments and replays with their contents: once a call of the handle has been
  // captured, an (eager) call with another table gets device arrays of its own and the old ones stay allocated, untouched, until the handle goes
  if (n_blocks > h->blk_cap || (h->captured && !same_table)) {
    HIP_TRY(hipStreamSynchronize(s));
    h->blk_cap = 0;
    if (h->captured && h->d_blk) { h->retired.push_back(std::move(h->d_blk)); h->retired.push_back(std::move(h->d_chain)); }
    h->captured = false;
    if ((rc = h->d_blk.alloc((size_t)3 * n_blocks * sizeof(int64_t))) || (rc = h->d_chain.alloc((size_t)n_blocks * sizeof(int32_t)))) { return rc; }
    h->blk_cap = n_blocks;
    h->last_ns.clear();   // new device arrays: the table has to be uploaded again
  }
  if (!same_table) {
    std::vector<int64_t> blk((size_t)3 * n_blocks);
    std::vector<int32_t> chain((size_t)n_blocks);
    int64_t off = 0, grp = 0;
    int32_t start = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
      bool dumps;
      const int64_t r = intg_rounds(n_sample[b], d.ns, &dumps);
      blk[(size_t)b] = off; blk[(size_t)(n_blocks + b)] = r; blk[(size_t)(2 * n_blocks + b)] = dumps ? grp : -1;
      chain[(size_t)b] = start;
      off += r;
      if (dumps) { grp++; start = (int32_t)(b + 1); }
    }
    h->last_ns.clear();                 // (stays empty if the upload fails)
    // the previous table may still be read by a kernel on another stream: drain the device before overwriting it
    if (h->last_stream != stream) { HIP_TRY(hipDeviceSynchronize()); }
    HIP_TRY(hipMemcpyAsync(h->d_blk.get(), blk.data(), blk.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->d_chain.get(), chain.data(), chain.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // blk / chain are stack vectors
    h->tbl_grp = grp; h->tbl_start = start;
    h->tbl_uni_rounds = blk[(size_t)n_blocks];
    h->tbl_max_rounds = 0;
    for (int64_t b = 0; b < n_blocks; b++) { if (blk[(size_t)(n_blocks + b)] > h->tbl_max_rounds) { h->tbl_max_rounds = blk[(size_t)(n_blocks + b)]; } }
    for (int64_t b = 1; b < n_blocks && h->tbl_uni_rounds > 0; b++) { if (blk[(size_t)(n_blocks + b)] != h->tbl_uni_rounds) { h->tbl_uni_rounds = 0; } }
    h->last_ns.assign(n_sample, n_sample + n_blocks);
    h->last_stream = stream;
  }
  const int64_t grp = h->tbl_grp;
  const int32_t start = h->tbl_start;
  IntgDumpParams p;
  memset(&p, 0, sizeof p);
  p.chn = d.chn; p.n_obj = d.n_objects; p.n_blocks = (int32_t)n_blocks;
  p.in = make_dfmt(d.in); p.acc = make_dfmt(d.acc); p.out = make_dfmt(d.out);
  p.in_eb = h->in_eb; p.out_eb = h->out_eb; p.in_stride = in_stride; p.out_stride = out_stride;
  // A saturating ACC_TYPE whose bounds no block sum of this call can reach is a wrapping one (round 5; cf. acdsp_fir::sat_free): every block
  // dumps and nothing is carried in, so a sum has at most max-rounds terms of at most max|x| each.
  bool sat_free = false;
  if (d.acc.O != ACDSP_WRAP && !h->pending && grp == n_blocks && p.acc.F >= p.in.F && p.acc.F - p.in.F < 64 - d.in.W && (d.acc.S || !d.in.S)) {
    sat_free = !knob_no_sat_free() && sat_free_bound((unsigned __int128)h->tbl_max_rounds, d.in, d.acc, p.acc.F - p.in.F, 0, 0);
  }
  p.lossless = (d.acc.O == ACDSP_WRAP || sat_free) && p.acc.F >= p.in.F && p.acc.F - p.in.F < 64 - d.in.W;
  p.tile_ok = p.lossless && !h->pending && h->temp_zero && grp == n_blocks;
  if (p.tile_ok) { p.uni_rounds = h->tbl_uni_rounds; }
  int64_t *const d_blk = h->d_blk.get<int64_t>();
  p.x = d_in; p.y = d_out; p.temp = static_cast<const int64_t *>(h->temp.cur());
  p.blk_off = d_blk; p.blk_rounds = d_blk + n_blocks; p.blk_out = d_blk + 2 * n_blocks; p.blk_chain = h->d_chain.get<int32_t>();
  bool temp_written = true;
  const int nxt = h->temp.next(false);
  hipError_t e = launch_intg_dump(p, static_cast<int64_t *>(h->temp.at(nxt)), s, &temp_written, &h->last_path);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "intg_dump kernel launch failed: %s", hipGetErrorString(e)); }
  if (temp_written) { h->temp.commit(nxt); }   // (else: nothing carried in, every block dumped -- the all-zero temp[] of this side stays the state)
  h->pending = start != (int32_t)n_blocks;   // the call ended on blocks that did not dump: their sums sit in temp[]
  if (temp_written) {
    // the general kernel wrote the next temp[]: non-zero while sums are pending; when every chain dumped it is zeroed HERE rather than trusted
    h->temp_zero = false;
    if (!h->pending) {
      HIP_TRY(hipMemsetAsync(h->temp.cur(), 0, h->temp.bytes(), s));
      h->temp_zero = true;
    }
  }
  return ACDSP_OK;
}

int32_t acdsp_intgdump_path(acdsp_intgdump_t h) { return h ? h->last_path : -1; }
int32_t acdsp_intgdump_in_elem_bytes(acdsp_intgdump_t h) { return h ? h->in_eb : -1; }

int32_t acdsp_intgdump_run_host(acdsp_intgdump_t h, const void *h_in, const int64_t *n_sample, int64_t n_blocks, void *h_out,
                                int64_t out_cap, int64_t *n_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int64_t ni = 0, no = 0;
  int rc = acdsp_intgdump_counts(h, n_sample, n_blocks, &ni, &no);
  if (rc) { return rc; }
  if (n_out) { *n_out = no; }
  if (n_blocks == 0) { return ACDSP_OK; }
  if ((ni > 0 && !h_in) || (no > 0 && (!h_out || out_cap < no))) { return fail(ACDSP_EINVAL, "intg_dump run_host: bad buffers"); }
  if ((rc = check_device(h->d.device))) { return rc; }
  const HostRows r = {h->d.n_objects, h_in, ni, ni > 0 ? ni : 1, h->in_eb, h_out, no, no > 0 ? no : 1, out_cap, h->out_eb};
  return run_host_staged(h->st, r, false, [&](const void *d_in, void *d_out, bool) { return acdsp_intgdump_run(h, d_in, r.si, n_sample, n_blocks, d_out, r.so, nullptr, nullptr); });
}

int32_t acdsp_intgdump_reset(acdsp_intgdump_t h) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->temp.zero())) { return rc; }
  h->pending = false;
  h->temp_zero = true;
  return ACDSP_OK;
}

// Deep copy (the reference core is a plain aggregate: temp[CHN] goes with it, ac_intg_dump.h:96-103): descriptor, temp[] and what the host
// knows about it.  Block table and staging are the clone's own: its first call uploads a table.
int32_t acdsp_intgdump_clone(acdsp_intgdump_t h, acdsp_intgdump_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_intgdump_t c = nullptr;
  int rc = acdsp_intgdump_create(&h->d, &c);
  if (rc) { return rc; }
  std::unique_ptr<acdsp_intgdump, int32_t (*)(acdsp_intgdump_t)> guard(c, acdsp_intgdump_destroy);
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = c->temp.copy_from(h->temp))) { return rc; }
  c->pending = h->pending;
  c->temp_zero = h->temp_zero;
  c->last_path = h->last_path;
  *out = guard.release();
  return ACDSP_OK;
}

// State blob, kind 8: temp[] of every object, [n_objects][CHN] int64 ACC raw words; bit 0 of the header's `reserved` = the stream stands
// behind a block that did not dump (its sums sit in temp[]).  Nothing in it depends on the input container: a blob moves both ways between a
// handle with ACDSP_FLAG_IN_BYTES and one without.
static StateHdr intgdump_state_hdr(const acdsp_intgdump *h) {
  StateHdr s = state_hdr(8, (uint32_t)h->d.n_objects, (uint32_t)sizeof(int64_t), (uint64_t)h->d.chn);
  s.p0 = (uint32_t)h->d.ns; s.p1 = (uint32_t)h->d.chn;
  s.reserved = h->pending ? 1 : 0;
  return s;
}

int64_t acdsp_intgdump_state_size(acdsp_intgdump_t h) { return h ? (int64_t)(sizeof(StateHdr) + state_payload(intgdump_state_hdr(h))) : -1; }

int32_t acdsp_intgdump_state_get(acdsp_intgdump_t h, void *buf, uint64_t cap_bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  const StateHdr s = intgdump_state_hdr(h);
  return state_blob_get("intgdump", h->d.device, s, {{h->temp.cur(), state_payload(s)}}, buf, cap_bytes);
}

int32_t acdsp_intgdump_state_set(acdsp_intgdump_t h, const void *buf, uint64_t bytes) {
  if (!h || !buf) { return fail(ACDSP_EINVAL, "null argument"); }
  const StateHdr mine = intgdump_state_hdr(h);
  StateHdr s;
  int rc = state_blob_hdr("intgdump", buf, bytes, &s);
  if (rc) { return rc; }
  if (!state_compatible(s, mine) || bytes != sizeof s + state_payload(mine) || (s.reserved & ~(uint64_t)1)) {
    return fail(ACDSP_EINVAL, "intgdump_state_set: blob does not belong to an ac_intg_dump of this NS / CHN / object count");
  }
  const acdsp::DFmt af = make_dfmt(h->d.acc);
  const unsigned char *pay = (const unsigned char *)buf + sizeof s;
  bool all_zero = true;
  for (uint64_t i = 0; i < state_payload(mine) / sizeof(int64_t); i++) {
    int64_t w;
    memcpy(&w, pay + i * sizeof(int64_t), sizeof w);
    if (w < af.lo || w > af.hi) { return fail(ACDSP_EINVAL, "intgdump_state_set: word %llu = %lld is not an ACC_TYPE raw word", (unsigned long long)i, (long long)w); }
    all_zero = all_zero && w == 0;
  }
  if ((rc = check_device(h->d.device))) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->temp.cur(), pay, state_payload(mine), hipMemcpyHostToDevice));
  // what run() derives from temp[]: the tile / stream kernels leave temp[] alone only when it is known to be zero, and sums that are carried
  // keep a call on the exact-order kernel.  Sums in temp[] are pending whatever the flag of a hand-made blob says.
  h->temp_zero = all_zero;
  h->pending = (s.reserved & 1) != 0 || !all_zero;
  h->last_ns.clear();   // the block table of the last call is rebuilt and uploaded by the next one, not trusted across a state load
  return ACDSP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// moving average (second half)
// ---------------------------------------------------------------------------------------------
struct acdsp_mvavg {
  acdsp_mvavg_desc_t d;
  int in_eb, out_eb;
  bool coeffs_set = false;
  DevBuf d_coeffs;
  std::vector<int64_t> h_coeffs;
  DevBuf d_frag;                // matrix-core form of the streaming kernel: fragments of the coefficient set (mv_avg_build_frags)
  MvSetPlan plan;               // what the descriptor and the coefficient set decide (mv_avg_plan.hpp); rebuilt by every set_coeffs
  int last_path = 0;
  Staging st;
};

extern "C" {

int32_t acdsp_mvavg_create(const acdsp_mvavg_desc_t *desc, acdsp_mvavg_t *out) {
  if (!desc || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  int rc;
  if ((rc = check_fmt(desc->in, "IN_TYPE")) || (rc = check_fmt(desc->coeff, "COEFF_TYPE")) || (rc = check_fmt(desc->acc, "ACC_TYPE")) ||
      (rc = check_fmt(desc->out, "OUT_TYPE"))) {
    return rc;
  }
  if (desc->taps < 1 || desc->taps > 1025) { return fail(ACDSP_EUNSUPPORTED, "mv_avg: TAPS=%d outside 1..1025", desc->taps); }
  if (!(desc->taps & 1)) { return fail(ACDSP_EUNSUPPORTED, "mv_avg: even TAPS: the reference's MAC loop reads coeffs[TAPS] (ac_mv_avg.h:117-119)"); }
  if (desc->win_mode < ACDSP_WIN_PLAIN || desc->win_mode > ACDSP_WIN_CLIP) { return fail(ACDSP_EINVAL, "mv_avg: bad window mode %d", desc->win_mode); }
  if (desc->max_sample < 1) { return fail(ACDSP_EINVAL, "mv_avg: MAX_SAMPLE must be >= 1"); }
  if (desc->n_objects < 1) { return fail(ACDSP_EINVAL, "mv_avg: n_objects must be >= 1"); }
  // 128-bit exact intermediates: ACC x COEFF product aligned with the accumulator
  const int fc = desc->coeff.W - desc->coeff.I;
  if (desc->acc.W + desc->coeff.W + 2 + (fc < 0 ? -fc : 0) > 125) { return fail(ACDSP_EUNSUPPORTED, "mv_avg: type combination needs more than 128-bit intermediates"); }
  int in_eb, out_eb;
  if ((rc = byte_rows("mv_avg", desc->flags, desc->in, desc->out, "ACDSP_FLAG_OUT_BYTES needs ACDSP_FLAG_IN_BYTES (1-byte output rows exist on the byte-sample kernels only)",
                      &in_eb, &out_eb))) {
    return rc;
  }
  if ((rc = check_device(desc->device))) { return rc; }
  std::unique_ptr<acdsp_mvavg> h(new acdsp_mvavg());   // (check_device has made the device current: a failure below frees there)
  h->d = *desc;
  h->in_eb = in_eb; h->out_eb = out_eb;
  if ((rc = h->d_coeffs.alloc((size_t)desc->taps * sizeof(int64_t))) || (rc = h->d_frag.alloc((size_t)kMvAvgFragWords * sizeof(uint32_t)))) { return rc; }
  *out = h.release();
  return ACDSP_OK;
}

int32_t acdsp_mvavg_destroy(acdsp_mvavg_t h) {
  if (!h) { return ACDSP_OK; }
  (void)hipSetDevice(h->d.device);
  delete h;
  return ACDSP_OK;
}

// Deep copy: descriptor and the coefficient set, when bound.  The reference builds its core inside run() (ac_mv_avg.h:154): there is no stream
// state to carry, and staging is the clone's own.
int32_t acdsp_mvavg_clone(acdsp_mvavg_t h, acdsp_mvavg_t *out) {
  if (!h || !out) { return fail(ACDSP_EINVAL, "null argument"); }
  acdsp_mvavg_t c = nullptr;
  int rc = acdsp_mvavg_create(&h->d, &c);
  if (rc) { return rc; }
  if (h->coeffs_set && (rc = acdsp_mvavg_set_coeffs(c, h->h_coeffs.data()))) { acdsp_mvavg_destroy(c); return rc; }
  c->last_path = h->last_path;
  *out = c;
  return ACDSP_OK;
}

int32_t acdsp_mvavg_set_coeffs(acdsp_mvavg_t h, const int64_t *coeffs) {
  if (!h || !coeffs) { return fail(ACDSP_EINVAL, "null argument"); }
  const DFmt cf = make_dfmt(h->d.coeff);
  for (int i = 0; i < h->d.taps; i++) {
    if (coeffs[i] < cf.lo || coeffs[i] > cf.hi) { return fail(ACDSP_EINVAL, "coefficient %d = %lld is not a COEFF_TYPE raw word", i, (long long)coeffs[i]); }
  }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = h->d_coeffs.upload(coeffs, (size_t)h->d.taps * sizeof(int64_t)))) { return rc; }
  h->h_coeffs.assign(coeffs, coeffs + h->d.taps);
  std::vector<uint32_t> fr((size_t)kMvAvgFragWords, 0u);
  h->plan = mv_avg_plan_set(h->d, h->in_eb, h->out_eb, coeffs, h->d_coeffs.get<int64_t>(), h->d_frag.get<uint32_t>(), fr.data());
  if (h->plan.p.frag_nb > 0 && (rc = h->d_frag.upload(fr.data(), fr.size() * sizeof(uint32_t)))) { return rc; }
  h->coeffs_set = true;
  return ACDSP_OK;
}

int32_t acdsp_mvavg_path(acdsp_mvavg_t h) { return h ? h->last_path : -1; }
int32_t acdsp_mvavg_in_elem_bytes(acdsp_mvavg_t h) { return h ? h->in_eb : -1; }
int32_t acdsp_mvavg_out_elem_bytes(acdsp_mvavg_t h) { return h ? h->out_eb : -1; }

// Host only (no device, no handle): the Toeplitz fragments acdsp_mvavg_set_coeffs would upload for this coefficient set -- in_bytes != 0: in the
// geometry of the byte-plane kernel -- into out[ACDSP_MVAVG_FRAG_WORDS].  Returns the K blocks (0: the set stays off the matrix cores).
int32_t acdsp_mvavg_frags_host(const int64_t *coeffs, int32_t taps, int32_t win_mode, int32_t in_bytes, uint32_t *out, int64_t *csum, int32_t *hi_any) {
  if (!coeffs || !out || !csum || !hi_any || taps < 1 || !(taps & 1) || win_mode < ACDSP_WIN_PLAIN || win_mode > ACDSP_WIN_CLIP) { (void)fail(ACDSP_EINVAL, "mvavg_frags_host: bad arguments"); return -1; }
  static_assert(ACDSP_MVAVG_FRAG_WORDS == kMvAvgFragWords, "the header's fragment size");
  memset(out, 0, (size_t)kMvAvgFragWords * sizeof(uint32_t));
  *csum = 0; *hi_any = 0;
  return mv_avg_build_frags(coeffs, taps, win_mode, in_bytes ? 16 : 8, out, csum, hi_any);
}

int64_t acdsp_mvavg_out_per_frame(acdsp_mvavg_t h, int64_t n_sample) {
  if (!h || n_sample < 1 || n_sample > h->d.max_sample) { return -1; }
  if (h->d.win_mode == ACDSP_WIN_PLAIN) { return n_sample >= h->d.taps ? n_sample - h->d.taps + 1 : 0; }
  return n_sample;
}

int32_t acdsp_mvavg_run(acdsp_mvavg_t h, const void *d_in, int64_t in_stride, int64_t n_sample, int64_t n_frames, void *d_out,
                        int64_t out_stride, int64_t *n_out, void *stream) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  if (!h->coeffs_set) { return fail(ACDSP_ESTATE, "mvavg_run before acdsp_mvavg_set_coeffs"); }
  const int64_t opf = acdsp_mvavg_out_per_frame(h, n_sample);
  if (opf < 0) { return fail(ACDSP_EINVAL, "mv_avg: n_sample=%lld outside 1..MAX_SAMPLE=%d (the reference's frame loop would lose alignment)", (long long)n_sample, h->d.max_sample); }
  if (n_frames < 0 || n_frames > (int64_t(1) << 40) / n_sample) { return fail(ACDSP_EINVAL, "mv_avg: bad frame count"); }
  const int64_t no = opf * n_frames;
  if (n_out) { *n_out = no; }
  if (n_frames == 0) { return ACDSP_OK; }
  if (!d_in || in_stride < n_sample * n_frames) { return fail(ACDSP_EINVAL, "mv_avg run: bad input arguments"); }
  if (no > 0 && (!d_out || out_stride < no)) { return fail(ACDSP_EINVAL, "mv_avg run: output buffer too small for %lld outputs", (long long)no); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  MvAvgParams p = h->plan.p;   // the general kernels' argument: the set plan's fields and this call's rows
  p.n_sample = n_sample; p.n_frames = n_frames; p.out_per_frame = opf; p.in_stride = in_stride; p.out_stride = out_stride; p.x = d_in; p.y = d_out;
  const MvCall c = mv_avg_plan_call(h->plan, p);
  if (c.path >= 0) { h->last_path = c.path; }
  hipError_t e = launch_mv_avg(c, (hipStream_t)stream);
  if (e != hipSuccess) { return fail(ACDSP_EHIP, "mv_avg kernel launch failed: %s", hipGetErrorString(e)); }
  return ACDSP_OK;
}

int32_t acdsp_mvavg_run_host(acdsp_mvavg_t h, const void *h_in, int64_t n_sample, int64_t n_frames, void *h_out, int64_t out_cap,
                             int64_t *n_out) {
  if (!h) { return fail(ACDSP_EINVAL, "null handle"); }
  const int64_t opf = acdsp_mvavg_out_per_frame(h, n_sample);
  if (opf < 0 || n_frames < 0) { return fail(ACDSP_EINVAL, "mv_avg run_host: bad n_sample / n_frames"); }
  const int64_t ni = n_sample * n_frames, no = opf * n_frames;
  if (n_out) { *n_out = no; }
  if (n_frames == 0) { return ACDSP_OK; }
  if (!h_in || (no > 0 && (!h_out || out_cap < no))) { return fail(ACDSP_EINVAL, "mv_avg run_host: bad buffers"); }
  int rc = check_device(h->d.device);
  if (rc) { return rc; }
  const HostRows r = {h->d.n_objects, h_in, ni, ni, h->in_eb, h_out, no, no > 0 ? no : 1, out_cap, h->out_eb};   // (rows stay packed on the device)
  return run_host_staged(h->st, r, false, [&](const void *d_in, void *d_out, bool) { return acdsp_mvavg_run(h, d_in, r.si, n_sample, n_frames, d_out, r.so, nullptr, nullptr); });
}

}  // extern "C"

