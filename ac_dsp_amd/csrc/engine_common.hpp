// engine_common.hpp -- what the translation units of the C-ABI layer share: engine.hip (entry points common to all + diagnostics + state
// blobs + stream files) and one file per operator family, engine_fir.hip, engine_cic.hip, engine_ddc.hip, engine_poly.hip, engine_misc.hip.
// Host-side object model: one handle = n independent reference filter objects whose state lives in HBM and carries across run() calls.
// There is no CPU compute path: every run() launches HIP kernels.
// Building blocks of the handles, each the single owner of what the families used to spell out one by one: DevBuf (one device allocation),
// History (the ping-pong input history), PhasePlans (per first % 16 fir_gen plans with their fragments), Staging + run_host_staged (the
// host-buffer calls), sat_free_bound / fits_container (arithmetic of the path decisions), Timer (event ring), byte_rows (the byte-container
// flags of a descriptor), rows_in_slots / rows_vec_aligned (the row layout of the matrix-core kernels), fir_params_of (the FirParams of a
// family that borrows a FIR kernel), long_or_nothing (a set on a long class: plan, upload or the refusal above 2048 taps), LongScratch (the
// phase-row scratch of the long poly kernels), knob_no_gen / knob_no_sat_free (the shared A/B knobs), and for the state blobs StateHdr with history_blob_fits (THE re-length rule), state_blob_get (every _state_get) and
// history_state_set (the _state_set of every input-history family).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "wide_kernels.hpp"
#include "cic_kernels.hpp"
#include "fir_kernels.hpp"

namespace acdsp {
namespace eng {

// sets the calling thread's acdsp_last_error() message and returns `code` (engine.hip)
int fail(int code, const char *fmt, ...);
// Device check of every entry point (engine.hip)
int check_device(int device);

// Is `s` recording a HIP graph?  A replayed graph re-runs the kernels with the HOST-side bookkeeping of capture time baked into
// their arguments (decimation / interpolation phase, "first call of the stream" special cases), so calls whose bookkeeping would
// not return to the captured value are refused while capturing instead of replaying the wrong phase silently.
inline bool stream_is_capturing(hipStream_t s) {
  // The legacy NULL stream cannot be captured, and asking about it while ANOTHER stream is in a global-mode capture returns an
  // error that may invalidate that capture and stays behind as the thread's last error (the next launch's hipGetLastError would
  // report it as a kernel failure): the host-buffer paths, which run on the NULL stream, never ask.
  if (s == nullptr) { return false; }
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(s, &st);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) { return fail(ACDSP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } \
  } while (0)

// max_w: 64 for IN / COEFF and every class without a wide path; 128 for ACC / OUT of the FIR classes and OUT of the CIC classes
// (wide.hip).  Unsigned types of the full container width are not representable in the signed raw words and are refused.
inline int check_fmt(const acdsp_fmt_t &f, const char *name, int max_w = 64) {
  if (f.W < 1 || f.W > max_w) { return fail(ACDSP_EUNSUPPORTED, "%s: W=%d outside 1..%d", name, f.W, max_w); }
  if (!f.S && (f.W == 64 || f.W == 128)) { return fail(ACDSP_EUNSUPPORTED, "%s: unsigned W=%d not supported", name, f.W); }
  if (f.Q < 0 || f.Q > ACDSP_RND_CONV_ODD) { return fail(ACDSP_EINVAL, "%s: bad Q mode %d", name, f.Q); }
  if (f.O < 0 || f.O > ACDSP_SAT_SYM) { return fail(ACDSP_EINVAL, "%s: bad O mode %d", name, f.O); }
  if (f.S != 0 && f.S != 1) { return fail(ACDSP_EINVAL, "%s: S must be 0 or 1", name); }
  return ACDSP_OK;
}

// ACDSP_TRACE=1: one stderr line per handle created and destroyed (with the number of run() calls it launched kernels for) -- how
// tests/test_cpp_gpu.py tells a testbench that reached the HIP kernels from one the header's host loop served (include/ac_dsp/acdsp_engine.h)
inline bool trace_handles() {
  static const bool t = getenv("ACDSP_TRACE") != nullptr;
  return t;
}
// A/B knobs more than one family reads, each read once per process.  ACDSP_NO_GEN: no multi-plane matrix-core kernels (fir_gen, fir_up, cic2);
// ACDSP_NO_SAT_FREE: a saturating accumulator keeps its saturation whatever the coefficient set (sat_free_bound is never asked)
inline bool knob_no_gen() { static const bool v = getenv("ACDSP_NO_GEN") != nullptr; return v; }
inline bool knob_no_sat_free() { static const bool v = getenv("ACDSP_NO_SAT_FREE") != nullptr; return v; }

inline int elem_bytes(int W) { return W <= 16 ? 2 : (W <= 32 ? 4 : (W <= 64 ? 8 : 16)); }
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// The one sample-width predicate of the matrix-core paths: do the value bits of `f` (an unsigned type needs one more) fit `eb` byte planes?
inline bool fits_container(const acdsp_fmt_t &f, int eb) { return (f.W + (f.S ? 0 : 1) + 7) / 8 <= eb; }

// sum of |c[i]|
inline unsigned __int128 sum_abs(const int64_t *c, size_t n) {
  unsigned __int128 sa = 0;
  for (size_t i = 0; i < n; i++) { sa += (unsigned __int128)(c[i] < 0 ? -(__int128)c[i] : (__int128)c[i]); }
  return sa;
}

// "A saturating accumulator that cannot saturate is a wrapping one": is  ((sa * max|x|) << lshift >> rshift) + lsb_slack  inside the top value
// of ACC_TYPE `acc` (the SYMMETRIC range of a signed type, so that none of the three saturating modes acts)?  sa = sum|c| over every term of a
// partial sum (or the number of unit-weight terms); lshift / rshift move the products to the accumulator's fraction (0 <= rshift < 64);
// lsb_slack = one LSB per term whose product is quantised on the way, + 1 (0 where nothing is dropped).  The callers keep their own
// preconditions (signedness, Q modes, pre-add widths); the answer decides whether a handle drops saturation, so a wrong "yes" is a silent
// parity error: every step that could leave 128 bits answers "no".
inline bool sat_free_bound(unsigned __int128 sa, const acdsp_fmt_t &in, const acdsp_fmt_t &acc, int lshift, int rshift, size_t lsb_slack) {
  const unsigned __int128 xmax = in.S ? ((unsigned __int128)1 << (in.W - 1)) : (((unsigned __int128)1 << in.W) - 1);
  const unsigned __int128 top = ((unsigned __int128)1 << (acc.W - (acc.S ? 1 : 0))) - 1;
  unsigned __int128 b = sa * xmax;                       // W_in, W_coeff <= 64, but sums of 2^10 taps (sa < 2^74) times 2^64 may overflow
  if (sa != 0 && b / sa != xmax) { return false; }
  if (lshift > 0 && (b >> (127 - lshift)) != 0) { return false; }
  b = ((b << lshift) >> rshift) + (unsigned __int128)lsb_slack;
  return b <= top;
}

// HIP-event timing of the main kernel of each run(), recorded on the launch stream.
// A ring of event pairs so that a whole timed region can be read back afterwards.
struct Timer {
  static const int kRing = 64;
  hipEvent_t e0[kRing] = {}, e1[kRing] = {};
  int64_t count = 0;  // runs recorded so far
  Timer() = default;
  Timer(const Timer &) = delete;
  Timer &operator=(const Timer &) = delete;
  ~Timer() {
    for (int i = 0; i < kRing; i++) {
      if (e0[i]) { (void)hipEventDestroy(e0[i]); }
      if (e1[i]) { (void)hipEventDestroy(e1[i]); }
    }
  }
  int init() {
    for (int i = 0; i < kRing; i++) {
      HIP_TRY(hipEventCreate(&e0[i]));
      HIP_TRY(hipEventCreate(&e1[i]));
    }
    return ACDSP_OK;
  }
  hipEvent_t start() { return e0[count % kRing]; }
  hipEvent_t stop() { return e1[count % kRing]; }
  void commit() { count++; }
  // average / minimum over the last k runs
  int stats(int k, float *avg, float *mn) {
    if (count == 0) { return fail(ACDSP_ESTATE, "no run() recorded yet"); }
    if (k < 1) { k = 1; }
    if (k > kRing) { k = kRing; }
    if (k > count) { k = (int)count; }
    double sum = 0;
    float lo = 1e30f;
    for (int i = 0; i < k; i++) {
      const int64_t idx = (count - 1 - i) % kRing;
      float ms = 0;
      HIP_TRY(hipEventSynchronize(e1[idx]));
      HIP_TRY(hipEventElapsedTime(&ms, e0[idx], e1[idx]));
      sum += ms;
      if (ms < lo) { lo = ms; }
    }
    if (avg) { *avg = (float)(sum / k); }
    if (mn) { *mn = lo; }
    return ACDSP_OK;
  }
};

// Move-only owner of one device allocation.  The destructor frees on the calling thread's current device: acdsp_*_destroy makes the
// handle's device current before it deletes the handle.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }
  ~DevBuf() { release(); }
  void release() {
    if (p_) { (void)hipFree(p_); p_ = nullptr; }
  }
  // (a live buffer is freed first: the caller has made sure that no kernel still reads it)
  int alloc(size_t bytes) {
    release();
    HIP_TRY(hipMalloc(&p_, bytes));
    return ACDSP_OK;
  }
  int alloc_zeroed(size_t bytes) {
    const int rc = alloc(bytes);
    return rc ? rc : zero(bytes);
  }
  int zero(size_t bytes) {
    HIP_TRY(hipMemset(p_, 0, bytes));
    return ACDSP_OK;
  }
  int upload(const void *host, size_t bytes) {   // synchronous
    HIP_TRY(hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice));
    return ACDSP_OK;
  }
  template <typename T>
  int alloc_upload(const std::vector<T> &v) {
    const int rc = alloc(v.size() * sizeof(T));
    return rc ? rc : upload(v.data(), v.size() * sizeof(T));
  }
  template <typename T = void>
  T *get() const { return static_cast<T *>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void *p_ = nullptr;
};

// The ping-pong input history of a handle: rows x hl containers, all zero at creation.  A captured HIP graph has both buffers' addresses
// baked into its kernel arguments, so the two allocations live exactly as long as the handle.
class History {
 public:
  int init(int rows, int hl, int elem_bytes) {
    bytes_ = (size_t)rows * hl * elem_bytes;
    for (DevBuf &b : buf_) {
      const int rc = b.alloc_zeroed(bytes_);
      if (rc) { return rc; }
    }
    return ACDSP_OK;
  }
  size_t bytes() const { return bytes_; }   // of one buffer
  int index() const { return cur_; }
  void *cur() const { return buf_[cur_].get(); }
  // index of the buffer the state kernel of a call writes: the current one (in place) when the call's input alone defines the new
  // history, else the other one ...
  int next(bool in_place) const { return in_place ? cur_ : (cur_ ^ 1); }
  void *at(int i) const { return buf_[i].get(); }
  // ... which becomes the current one once that kernel is enqueued
  void commit(int next) { cur_ = next; }
  int zero() {   // (the caller has drained the device)
    for (DevBuf &b : buf_) {
      if (b) { const int rc = b.zero(bytes_); if (rc) { return rc; } }
    }
    return ACDSP_OK;
  }
  // clone: this (fresh) history takes the current state of `o` (same geometry)
  int copy_from(const History &o) {
    HIP_TRY(hipMemcpy(buf_[0].get(), o.cur(), bytes_, hipMemcpyDeviceToDevice));
    cur_ = 0;
    return ACDSP_OK;
  }

 private:
  DevBuf buf_[2];
  size_t bytes_ = 0;
  int cur_ = 0;
};

// words of one fir_gen fragment slab: fir_gen_plan gives at most 3 coefficient byte planes x 8 K-blocks, each [64 lanes][4] dwords
constexpr int kGenMaxPlanes = 3, kGenMaxBlocks = 8;
constexpr size_t kGenFragWords = (size_t)kGenMaxPlanes * kGenMaxBlocks * 64 * 4;

// fir_gen plans of one tap set for each window offset first % 16 (a decimator's calls start at any phase), built and uploaded by prepare();
// the fragments share one device slab of 16.  The upload copies from pageable memory and synchronises the stream, which a capturing stream does
// not allow: an eager call prepares its own phase, the phase of the call that follows it and phase 0 (where reset() leads), so that a capture
// behind any eager call finds its plan, and get() itself never touches the stream.
class PhasePlans {
 public:
  int init() { return frag_.alloc(16 * kGenFragWords * sizeof(uint32_t)); }
  // 1: the plan of phase `fm` is on the device; -1: the taps have no plan at that phase; 0: not built yet
  int state(int fm) const { return ((have_ >> fm) & 1) ? 1 : (((none_ >> fm) & 1) ? -1 : 0); }
  // builds and uploads whichever of the phases fms[0..n) are still missing: copies on `s` and one synchronisation -- never under capture
  int prepare(const std::vector<int64_t> &taps, int R, const int *fms, int n, hipStream_t s) {
    std::vector<uint32_t> fr[3];   // (stack vectors: alive until the synchronisation below)
    int n_up = 0;
    uint32_t up = 0;
    for (int i = 0; i < n && n_up < 3; i++) {
      const int fm = fms[i];
      if (state(fm) != 0 || ((up >> fm) & 1)) { continue; }
      if (!fir_gen_plan(taps.data(), (int)taps.size(), R, fm, &plan_[fm], &fr[n_up]) || fr[n_up].size() > kGenFragWords) { none_ |= 1u << fm; continue; }
      HIP_TRY(hipMemcpyAsync(frag_.get<uint32_t>() + (size_t)fm * kGenFragWords, fr[n_up].data(), fr[n_up].size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      up |= 1u << fm;
      n_up++;
    }
    if (up) {
      HIP_TRY(hipStreamSynchronize(s));
      have_ |= up;
    }
    return ACDSP_OK;
  }
  // *plan = the prepared plan of phase `fm` and *frag its device fragments, or *plan = nullptr where there is none (state(fm) != 1)
  void get(int fm, const FirGenPlan **plan, const uint32_t **frag) const {
    const bool ok = state(fm) == 1;
    *plan = ok ? &plan_[fm] : nullptr;
    *frag = ok ? frag_.get<uint32_t>() + (size_t)fm * kGenFragWords : nullptr;
  }

 private:
  FirGenPlan plan_[16];
  uint32_t have_ = 0, none_ = 0;
  DevBuf frag_;   // [16][kGenFragWords]
};

// Window phases first % 16 an eager decimator call at input count `t_total` of `n_in` samples prepares (PhasePlans::prepare): its own, that of
// the call behind it -- which may be the first one of a graph capture -- and phase 0
inline void decimator_phases(int R, int64_t t_total, int64_t n_in, int fms[3]) {
  fms[0] = (int)(((R - t_total % R) % R) % 16);
  fms[1] = (int)(((R - (t_total + n_in) % R) % R) % 16);
  fms[2] = 0;
}

// Buffers of the host-side calls (run_host_staged)
struct Staging {
  DevBuf d_in, d_out;
  size_t cap_in = 0, cap_out = 0;
  // Small calls (the drop-in run() of one channel, ac_fir_prog_coeffs: ONE sample per call, reference ac_fir_prog_coeffs.h:281):
  // a pinned, device-mapped host buffer the kernels read and write directly -- no H2D / D2H copy calls, one synchronisation.
  static const size_t kPinBytes = 64 * 1024;
  void *pin_in = nullptr, *pin_out = nullptr;
  static bool pinned_enabled() { static const bool off = getenv("ACDSP_NO_PINNED") != nullptr; return !off; }   // A/B knob: always the device staging buffers
  Staging() = default;
  Staging(const Staging &) = delete;
  Staging &operator=(const Staging &) = delete;
  ~Staging() {
    if (pin_in) { (void)hipHostFree(pin_in); }
    if (pin_out) { (void)hipHostFree(pin_out); }
  }
  int ensure_pinned() {
    if (!pin_in) { HIP_TRY(hipHostMalloc(&pin_in, kPinBytes, hipHostMallocMapped)); }
    if (!pin_out) { HIP_TRY(hipHostMalloc(&pin_out, kPinBytes, hipHostMallocMapped)); }
    return ACDSP_OK;
  }
  // acdsp_fir_run has used d_in under graph capture: the graph holds its address, so growing the image later keeps the old one in `retired`
  // (allocated, unused, until the handle goes) instead of freeing it
  bool captured = false;
  std::vector<DevBuf> retired;
  int ensure(size_t bin, size_t bout) {
    int rc;
    if (bin > cap_in) {
      cap_in = 0;
      if (captured && d_in) { retired.push_back(std::move(d_in)); }
      captured = false;
      if ((rc = d_in.alloc(bin))) { return rc; }
      cap_in = bin;
    }
    if (bout > cap_out) {
      cap_out = 0;
      if ((rc = d_out.alloc(bout))) { return rc; }
      cap_out = bout;
    }
    return ACDSP_OK;
  }
};

// One host-buffer call: `rows` rows of n_in containers of in_eb bytes, packed in h_in, go into device rows of `si` containers; `run(d_in,
// d_out, pinned)` performs the family's device run() on the NULL stream (rows of si / so containers) and returns its status; after one
// synchronisation n_out containers of out_eb bytes per row come back into h_out, whose rows are out_pitch containers apart.
// pin_small: calls whose padded images both fit Staging::kPinBytes go through the pinned buffers instead.
struct HostRows {
  int rows;
  const void *h_in; int64_t n_in, si; int in_eb;
  void *h_out; int64_t n_out, so, out_pitch; int out_eb;
};
template <typename Run>
int run_host_staged(Staging &st, const HostRows &r, bool pin_small, Run run) {
  const size_t rows = (size_t)r.rows, bin = rows * r.si * r.in_eb, bout = rows * r.so * r.out_eb;
  const size_t in_row = (size_t)r.n_in * r.in_eb, out_row = (size_t)r.n_out * r.out_eb;
  int rc;
  if (pin_small && bin <= Staging::kPinBytes && bout <= Staging::kPinBytes && Staging::pinned_enabled()) {
    if ((rc = st.ensure_pinned())) { return rc; }
    for (size_t c = 0; c < rows; c++) { memcpy((char *)st.pin_in + c * r.si * r.in_eb, (const char *)r.h_in + c * in_row, in_row); }
    if ((rc = run(st.pin_in, st.pin_out, true))) { return rc; }
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (size_t c = 0; c < rows; c++) { memcpy((char *)r.h_out + c * r.out_pitch * r.out_eb, (const char *)st.pin_out + c * r.so * r.out_eb, out_row); }
    return ACDSP_OK;
  }
  if ((rc = st.ensure(bin, bout))) { return rc; }
  if (in_row > 0) { HIP_TRY(hipMemcpy2D(st.d_in.get(), (size_t)r.si * r.in_eb, r.h_in, in_row, in_row, rows, hipMemcpyHostToDevice)); }
  if ((rc = run(st.d_in.get(), st.d_out.get(), false))) { return rc; }
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (out_row > 0) {
    HIP_TRY(hipMemcpy2D(r.h_out, (size_t)r.out_pitch * r.out_eb, st.d_out.get(), (size_t)r.so * r.out_eb, out_row, rows, hipMemcpyDeviceToHost));
  }
  return ACDSP_OK;
}

// ---- state blobs (acdsp_*_state_get / _set): what engine.hip (FIR, CIC, DDC) and the family files (poly_dec, poly_intr, intg_dump) share ----
// 64-byte little-endian header in front of the raw state words.
struct StateHdr {
  char magic[8];            // "ACDSPST1"
  uint32_t version;         // 1
  uint32_t kind;            // 1: FIR input history, 2: FIR reg_trans partial sums, 3: CIC input history + input count,
                            // 4: fused DDC input history + input count, 5: two-kernel DDC (CIC blob + FIR blob follow),
                            // 6: ac_poly_dec input history, 7: ac_poly_intr input history + input count + saved sums, 8: ac_intg_dump temp[],
                            // 9: fused polydec DDC input history + input count, 10: two-kernel polydec DDC (CIC blob + ac_poly_dec blob + queued words)
  uint32_t n_channels;
  uint32_t elem_bytes;      // bytes per state word (IN container; reg_trans: 8, or 16 for an ACC_TYPE wider than 64 bits; temp[]: 8)
  uint64_t per_channel;     // state words per channel
  int64_t t_total;          // (two-kernel polydec DDC: queued words per channel)  CIC, poly_intr: inputs consumed so far (decimation / interpolation phase, "first sample" of the folded cores); else 0
  uint32_t p0, p1, p2, p3;  // FIR: n_taps, ftype, class, 0;  CIC: R, M, N, interp;  poly_dec: NTAPS, DF;  poly_intr: NTAPS, IF, ftype, COEFFSZ;  intg_dump: NS, CHN
  uint64_t reserved;        // two-kernel DDC: channel count;  polydec DDC: DF in the high half;  intg_dump: bit 0 = pending (the stream stands behind a block that did not dump)
};
static_assert(sizeof(StateHdr) == 64, "state header is 64 bytes");

inline StateHdr state_hdr(uint32_t kind, uint32_t n_channels, uint32_t elem_bytes, uint64_t per_channel) {
  StateHdr s;
  memset(&s, 0, sizeof s);
  memcpy(s.magic, "ACDSPST1", 8);
  s.version = 1;
  s.kind = kind; s.n_channels = n_channels; s.elem_bytes = elem_bytes; s.per_channel = per_channel;
  return s;
}
inline uint64_t state_payload(const StateHdr &s) { return (uint64_t)s.n_channels * s.per_channel * s.elem_bytes; }

// everything but t_total must agree between the blob and the handle it is loaded into
inline bool state_compatible(const StateHdr &blob, const StateHdr &mine) {
  return memcmp(blob.magic, "ACDSPST1", 8) == 0 && blob.version == 1 && blob.kind == mine.kind && blob.n_channels == mine.n_channels &&
         blob.elem_bytes == mine.elem_bytes && blob.per_channel == mine.per_channel && blob.p0 == mine.p0 && blob.p1 == mine.p1 &&
         blob.p2 == mine.p2 && blob.p3 == mine.p3;
}

// device image of an input-history blob `s` (payload `src`) of another history length than the handle's (`mine`): the newest
// min(blob, mine) samples of every channel are kept, older ones zero
inline std::vector<unsigned char> relen_image(const StateHdr &s, const StateHdr &mine, const unsigned char *src) {
  const size_t eb = mine.elem_bytes, pm = (size_t)mine.per_channel, pb = (size_t)s.per_channel, keep = pm < pb ? pm : pb;
  std::vector<unsigned char> img((size_t)mine.n_channels * pm * eb, 0);
  for (size_t c = 0; c < mine.n_channels; c++) { memcpy(&img[(c * pm + (pm - keep)) * eb], src + (c * pb + (pb - keep)) * eb, keep * eb); }
  return img;
}

// An input-history blob `s` of `bytes` bytes (header, history, `extra` bytes behind it) against the header `mine` of the handle it is meant for:
// 0 = not this handle's, 1 = the handle's own layout, 2 = another history LENGTH, of at most max_len samples, that still covers the filter
// memory of `mem` samples.  THE re-length rule of every input-history family: a handle's length is its filter memory rounded up for the kernels'
// windows -- it differs between kernel paths and between builds -- and the samples beyond the memory only ever meet zero coefficients (or feed
// warm-up values the combs cancel), so relen_image keeps the newest min(blob, mine) samples and zeroes older ones.
constexpr uint64_t kNoOtherLength = ~uint64_t(0);   // `mem` of a state that is not an input history (FIR reg_trans sums) or whose length never varies
inline int history_blob_fits(const StateHdr &s, const StateHdr &mine, uint64_t bytes, uint64_t extra, uint64_t mem, uint64_t max_len) {
  if (state_compatible(s, mine)) { return bytes == sizeof s + state_payload(mine) + extra ? 1 : 0; }
  StateHdr same_len = s;
  same_len.per_channel = mine.per_channel;
  const bool relen = s.per_channel != mine.per_channel && s.per_channel >= mem && s.per_channel <= max_len && state_compatible(same_len, mine) &&
                     bytes == sizeof s + state_payload(s) + extra;
  return relen ? 2 : 0;
}

// The header of a blob handed to acdsp_<name>_state_set
inline int state_blob_hdr(const char *name, const void *buf, uint64_t bytes, StateHdr *s) {
  if (bytes < sizeof *s) { return fail(ACDSP_EINVAL, "%s_state_set: blob shorter than its header", name); }
  memcpy(s, buf, sizeof *s);
  return ACDSP_OK;
}

// acdsp_<name>_state_get: the header `s`, then the device blocks `parts` in order, into buf[cap]; a part without a pointer is counted and left
// for the caller to fill.  `pre` runs on the drained device in front of the copies; the parts' pointers are read after it (FIR: reg_trans[] may
// have to be rebuilt first, into the other buffer).
struct StatePart { const void *dev; uint64_t bytes; };
template <typename Pre>
int state_blob_get(const char *name, int device, const StateHdr &s, const StatePart *parts, int n_parts, void *buf, uint64_t cap, Pre pre) {
  uint64_t need = sizeof s;
  for (int i = 0; i < n_parts; i++) { need += parts[i].bytes; }
  if (cap < need) { return fail(ACDSP_EINVAL, "%s_state_get: buffer of %llu bytes, state needs %llu", name, (unsigned long long)cap, (unsigned long long)need); }
  int rc = check_device(device);
  if (rc) { return rc; }
  HIP_TRY(hipDeviceSynchronize());   // run() is asynchronous: the state of the last call must have landed
  if ((rc = pre())) { return rc; }
  memcpy(buf, &s, sizeof s);
  char *dst = (char *)buf + sizeof s;
  for (int i = 0; i < n_parts; i++) {
    if (parts[i].dev) { HIP_TRY(hipMemcpy(dst, parts[i].dev, parts[i].bytes, hipMemcpyDeviceToHost)); }
    dst += parts[i].bytes;
  }
  return ACDSP_OK;
}
inline int state_blob_get(const char *name, int device, const StateHdr &s, std::initializer_list<StatePart> parts, void *buf, uint64_t cap) {
  return state_blob_get(name, device, s, parts.begin(), (int)parts.size(), buf, cap, [] { return (int)ACDSP_OK; });
}

// acdsp_<name>_state_set of the input-history families: the blob buf[bytes] -- header, history, `extra` bytes behind it -- goes into the history
// at d_hist if history_blob_fits() says it is the state of the handle with header `mine`, re-lengthed where it has to be; anything else, and a
// negative input count where the family carries a phase in t_total (`phased`), is refused with "<name>_state_set: <refusal>" before the device
// is touched.  *s_out = the blob's header: the caller takes t_total and whatever follows the history from it.
inline int history_state_set(const char *name, const char *refusal, int device, const StateHdr &mine, void *d_hist, const void *buf, uint64_t bytes,
                             uint64_t extra, uint64_t mem, uint64_t max_len, bool phased, StateHdr *s_out) {
  StateHdr &s = *s_out;
  int rc = state_blob_hdr(name, buf, bytes, &s);
  if (rc) { return rc; }
  const int fit = history_blob_fits(s, mine, bytes, extra, mem, max_len);
  if (!fit || (phased && s.t_total < 0)) { return fail(ACDSP_EINVAL, "%s_state_set: %s", name, refusal); }
  if ((rc = check_device(device))) { return rc; }
  HIP_TRY(hipDeviceSynchronize());
  const unsigned char *pay = (const unsigned char *)buf + sizeof s;
  if (fit == 2) {
    const std::vector<unsigned char> img = relen_image(s, mine, pay);
    HIP_TRY(hipMemcpy(d_hist, img.data(), img.size(), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(d_hist, pay, state_payload(mine), hipMemcpyHostToDevice));
  }
  return ACDSP_OK;
}

// The byte-container flags of a descriptor (ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES): container bytes of the IN and OUT rows, or the refusal.
// One order of checks for every family; `prefix` = the family's name in its messages (nullptr: none); out_needs_in = the family's sentence for
// OUT_BYTES without IN_BYTES where it has 1-byte output rows, nullptr where it has none.  Family-specific refusals follow in the family.
inline int byte_rows(const char *prefix, int flags, const acdsp_fmt_t &in, const acdsp_fmt_t &out, const char *out_needs_in, int *in_eb, int *out_eb) {
  const bool in_bytes = (flags & ACDSP_FLAG_IN_BYTES) != 0, out_bytes = (flags & ACDSP_FLAG_OUT_BYTES) != 0;
  const std::string p = prefix ? std::string(prefix) + ": " : std::string();
  if (in_bytes && in.W > 8) { return fail(ACDSP_EINVAL, "%sACDSP_FLAG_IN_BYTES: IN_TYPE W=%d does not fit a 1-byte container", p.c_str(), in.W); }
  if (out_bytes && !out_needs_in) {
    return fail(ACDSP_EUNSUPPORTED, "%sACDSP_FLAG_OUT_BYTES is not supported (1-byte output rows: the FIR under both byte flags only)", p.c_str());
  }
  if (out_bytes && !in_bytes) { return fail(ACDSP_EUNSUPPORTED, "%s%s", p.c_str(), out_needs_in); }
  if (out_bytes && out.W > 8) { return fail(ACDSP_EINVAL, "%sACDSP_FLAG_OUT_BYTES: OUT_TYPE W=%d does not fit a 1-byte container", p.c_str(), out.W); }
  *in_eb = in_bytes ? 1 : elem_bytes(in.W);
  *out_eb = out_bytes ? 1 : elem_bytes(out.W);
  return ACDSP_OK;
}

// The row layout the vector loads of the matrix-core kernels want: a 16-byte aligned base and row pitch ...
inline bool rows_vec_aligned(const void *d_in, int64_t in_stride, int in_eb) { return (uintptr_t)d_in % 16 == 0 && (in_stride * in_eb) % 16 == 0; }
// ... and rows that lie in whole 16-sample slots: readable up to the next multiple of 16 samples
inline bool rows_in_slots(const void *d_in, int64_t in_stride, int in_eb, int64_t n) { return rows_vec_aligned(d_in, in_stride, in_eb) && in_stride >= (n + 15) / 16 * 16; }

// The rows of one call, and a zeroed FirParams filled from formats, container bytes, history length, channel count and those rows: what the
// families that borrow a FIR kernel hand to it (poly_dec, poly_intr, CIC).  Everything else stays zero until the caller sets it.
struct CallRows { const void *x; int64_t in_stride, n; void *y; int64_t out_stride; };
inline FirParams fir_params_of(const DFmt &in, const DFmt &cf, const DFmt &acc, const DFmt &out, int in_eb, int out_eb, int hl, int n_ch, const CallRows &r) {
  FirParams k;
  memset(&k, 0, sizeof k);
  k.n_ch = n_ch; k.in = in; k.cf = cf; k.acc = acc; k.out = out; k.in_eb = in_eb; k.out_eb = out_eb; k.hl = hl;
  k.in_stride = r.in_stride; k.out_stride = r.out_stride; k.n = r.n; k.x = r.x; k.y = r.y;
  return k;
}

// A planner of set_coeffs answers kTaken (the set runs on its kernel class, plan and device tables in place), kNotThisClass or an ACDSP_E* code (all positive)
enum { kNotThisClass = 0, kTaken = -1 };

// A coefficient set on a long matrix-core class (FIR long, FIR byte samples, poly_dec long) -- above 2048 taps the only class there is, so a
// set that cannot go there is refused ("<what><n>: ...") where up to 2048 taps it is left to the other classes.  A set whose saturating
// ACC_TYPE is not provably saturation-free (!lossless) cannot; plan(&frag, &corr) builds the family's plan and fragments and its correction
// constant, with the family's own rule for re-biased samples, and answers false for a tap that does not split into two signed bytes.
template <typename Plan>
int long_or_nothing(const char *what, int n, bool lossless, DevBuf &d_frag, DevBuf &d_corr, Plan plan) {
  if (!lossless) {
    if (n <= 2048) { return kNotThisClass; }
    return fail(ACDSP_EUNSUPPORTED, "%s%d: the saturating ACC_TYPE cannot be proven saturation-free for this coefficient set, and more than 2048 taps have no exact-order kernel", what, n);
  }
  std::vector<uint32_t> frag;
  int64_t corr = 0;
  if (!plan(&frag, &corr)) {
    if (n <= 2048) { return kNotThisClass; }
    return fail(ACDSP_EUNSUPPORTED, "%s%d: a coefficient of 32640 or more cannot be split into two signed bytes, and more than 2048 taps run on the matrix cores only", what, n);
  }
  int rc;
  if ((rc = d_frag.upload(frag.data(), frag.size() * sizeof(uint32_t))) || (rc = d_corr.upload(&corr, sizeof corr))) { return rc; }
  return kTaken;
}

// The scratch of the phase rows of a long poly_dec / poly_intr handle: cap, geometry and buffer, sized at create / set_scratch_cap / clone,
// never in run().  init(): rows of `sample_bytes` per slab sample behind a head of `head` samples, n_ch channels, under the default cap.
struct LongScratch {
  uint64_t cap = (uint64_t)128 << 20;
  LongGeom geo = {0, 0, 0};
  DevBuf buf;
  uint64_t sample_bytes = 0, head = 0;   // the rows (init)
  int n_ch = 0;
  int init(uint64_t sample_bytes_, uint64_t head_, int n_ch_) {
    sample_bytes = sample_bytes_; head = head_; n_ch = n_ch_;
    return size(cap);
  }
  // under `new_cap` (the caller has drained the device when a buffer is live).  The new buffer is allocated first: a failure leaves cap,
  // geometry and scratch as they were
  int size(uint64_t new_cap) {
    const LongGeom g = long_geometry(sample_bytes, head, n_ch, new_cap);
    DevBuf fresh;
    const int rc = fresh.alloc(g.bytes);
    if (rc) { return rc; }
    buf = std::move(fresh);   // (the old buffer goes with `fresh`)
    geo = g; cap = new_cap;
    return ACDSP_OK;
  }
  // the out-parameters of acdsp_*_long_geometry (null ones skipped); zeros for a handle that is not long
  void geometry(bool is_long, int64_t *slab, int32_t *group, uint64_t *bytes) const {
    if (slab) { *slab = is_long ? geo.slab : 0; }
    if (group) { *group = is_long ? geo.group : 0; }
    if (bytes) { *bytes = is_long ? geo.bytes : 0; }
  }
};

}  // namespace eng
}  // namespace acdsp

using namespace acdsp;   // (the handle structs live in the global namespace: they are the opaque types of include/acdsp.h)
using acdsp::eng::Timer;
using acdsp::eng::Staging;
using acdsp::eng::DevBuf;
using acdsp::eng::History;
using acdsp::eng::PhasePlans;
using acdsp::eng::LongScratch;

struct acdsp_fir {
  acdsp_fir_desc_t d;
  int in_eb, out_eb, hl;
  bool use_rt, lossless, coeffs_set;
  // AC_SAT / AC_SAT_SYM / AC_SAT_ZERO accumulators (round 5): lossless_shape = the exact-sum conditions with the overflow mode left out (create);
  // sat_free = no partial sum of the CURRENT coefficient set can reach the type's bounds, so the saturation is dead code and the handle
  // runs the classes of a wrapping accumulator (set_coeffs; every FirParams of the handle then carries AC_WRAP: fir_params)
  bool lossless_shape = false, sat_free = false;
  bool wide = false;   // ACC_TYPE or OUT_TYPE wider than 64 bits: wide.hip (reg_trans words are then 16 bytes)
  bool small_call = false;   // set by run_host around a call that fits the pinned buffers (launch-bound: see acdsp_fir_run)
  int rt_eb = 8;
  int path;
  History hist;
  DevBuf d_rt[2];               // reg_trans[] (use_rt), ping-pong: indexed by the history's index, or by cur_rt (rt_hybrid)
  // TRANSPOSED with loadable coefficients, exact-sum class (rt_hybrid): reg_trans[] differs from an input history only while partial sums
  // of an EARLIER coefficient set are still in it -- for the n_taps - 1 samples behind a coefficient change (or a loaded state blob).  Those
  // samples run the exact-order kernel on reg_trans; everything else is the same dot product as SHIFT_REG and runs the matrix-core kernels
  // on the input history, which is kept up to date by every call.  reg_trans is rebuilt from the history (rt_from_hist) when it is asked for.
  // unsigned 16-bit samples on the int8 MFMA kernel: x_u = (x_u ^ 0x8000 as int16) + 32768 -- the kernel flips the top bit as it splits
  // the samples into byte planes (FirParams::in_flip) and 32768 * sum(c) rides in the correction constant; rows and state stay raw
  bool in_flip = false;
  bool rt_hybrid = false, rt_valid = true;
  int64_t rt_since = 0;         // samples since the last coefficient change / state load, saturating at n_taps - 1
  int cur_rt = 0;               // rt_hybrid: index of the current reg_trans buffer (the history has its own)
  DevBuf d_coeffs;
  // The selected plan.  `path` names the kernel class that took the current coefficient set (the planners of set_coeffs, engine_fir.hip, tried
  // in the order below; the first that takes the set ends the sequence), and the plan data of that class is the only plan data that is valid:
  //   ACDSP_PATH_MFMA_S8     lplan, s8_sum_abs, d_frag, d_corr   (ACDSP_FLAG_IN_BYTES, fir_s8.hip)
  //   ACDSP_PATH_MFMA_LONG   lplan, d_frag, d_corr, in_flip      (1026 .. 16384 taps, fir_long.hip)
  //   ACDSP_PATH_MFMA_I8     plan, mfma_cshift, d_frag [n_sets][2][nb][64][4] Toeplitz byte-plane fragments, d_corr [n_sets] 128 * sum(c), in_flip
  //   ACDSP_PATH_MFMA_GEN    gplan, d_gfrag                      (the generalised multi-plane kernel, fir_gen.hip)
  //   ACDSP_PATH_MFMA_LOSSY  gplan, d_gfrag, lzp, d_lzcl         (class B, fir_gen_ring.hip: plan of the effective taps + residue table)
  // At most one class can take a set, by the shapes they admit: byte samples need 1-byte rows, long at least 1026 taps of rows that are not
  // bytes, int8 MFMA 2-byte rows and at most 33 K-blocks (1025 taps), gen rows of at least 2 bytes, and lossy an accumulator that is NOT
  // lossless where the other four need a lossless one.  gen admits the shapes of long and int8 MFMA too: it is their fall-back, reached only
  // when their two-byte split fails.  set_coeffs checks the other pairs on every call ("internal: ...": fir_second_class_admits).
  DevBuf d_frag, d_corr;
  FirMfmaPlan plan;             // worst case over the coefficient sets (bounds for the epilogue choice)
  int mfma_cshift = 0;          // the fragments hold the coefficients scaled by 2^mfma_cshift (narrow types: engine_fir.hip, fir_plan_i8)
  bool long_shape = false;      // the descriptor is long-eligible (create)
  FirLongPlan lplan;
  bool s8_shape = false;        // the descriptor is byte-eligible (create): in_eb == 1
  int64_t s8_sum_abs = 0;       // sum |c| of the effective taps (the 32-bit epilogue's bound)
  DevBuf d_gfrag;
  FirGenPlan gplan;
  FirLossyPlan lzp;
  DevBuf d_lzcl;
  int64_t n_runs = 0;             // run() calls that launched kernels (ACDSP_TRACE)
  int kclass = 0;                 // acdsp_fir_kernel_class
  std::vector<int64_t> h_coeffs;  // last coefficient set (for clone)
  Timer tm;
  Staging st;
};

struct acdsp_cic {
  acdsp_cic_desc_t d;
  acdsp_fmt_t it;
  int in_eb, out_eb, hl, me;
  // decimator through its FIR identity on the matrix cores (fir_gen.hip): taps, and per (first mod 16) plans / fragments
  std::vector<int64_t> h_taps;
  bool gen_ok = false;
  bool gen_plan_ok = false;      // ... its plan class alone, whatever the row containers (the byte cascade stands on it: engine_ddc.hip)
  PhasePlans gen;
  // decimator in two stages (cic2.hip): R = c2_R1 * c2_R2, stage-1 taps z^-(N-1) boxcar(R1)^N with their per (first mod 16) plans / fragments
  bool c2_ok = false;
  bool c2_first = false;   // ACDSP_CIC2_ALL: the two-stage kernel goes first where the one-stage identity (gen_ok) would serve the handle too
  int c2_R1 = 0, c2_R2 = 0, c2_wu = 0;
  std::vector<int64_t> c2_taps;
  PhasePlans c2;
  int warm = 0;                  // inputs the recurrence kernel simulates in front of a chunk (the filter memory; hl may be longer: cic2.hip)
  DevBuf d_taps;                 // interpolator: the identity's taps for the polyphase kernel
  // interpolator on the matrix cores (fir_up.hip): per-phase taps E_r[k] = h[r + R k]
  bool up_ok = false;
  int up_px = 0;
  FirUpPlan up_plan;
  DevBuf d_upfrag, d_upcorr;
  int last_path = 0;
  bool wide = false;    // INT_TYPE or OUT_TYPE wider than 64 bits: both directions through cic_wide_kernel (wide.hip)
  int64_t t_total = 0;  // inputs consumed so far (all calls)
  History hist;
  Timer tm;
  Staging st;
};

// ac_poly_dec handle (engine_poly.hip; stage B of the polydec cascade: engine_ddc.hip)
struct acdsp_polydec {
  acdsp_polydec_desc_t d;
  int in_eb, out_eb, hl;
  bool lossless = false, coeffs_set = false, gen_ok = false;
  bool lossless_shape = false, sat_free = false;   // a saturating ACC_TYPE no partial sum of the current set can reach is a wrapping one (cf. acdsp_fir::sat_free)
  History hist;
  DevBuf d_coeffs, d_gfrag;
  FirGenPlan gplan;
  // long prototypes (polydec_long.hip): long_shape = the descriptor is long-eligible and the ring kernel has no plan for its shape (create);
  // long_ok = the current set runs there.  scratch: the phase streams
  bool long_shape = false, long_ok = false, in_flip = false;
  PolyDecLongPlan lplan;
  LongScratch scratch;
  DevBuf d_lfrag, d_lcorr;
  int last_path = ACDSP_PATH_GENERIC;
  int32_t last_ring = 0;   // ring-shape id of the last run(), 0 when no ring row ran
  Staging st;
};

// DDC cascade handle (engine_ddc.hip; the state blobs of engine.hip read it)
constexpr int kDdcMaxFusedDf = 2;   // decimation of the fused polydec cascade's stage B (fir_gen_cascade_dec.hip)
struct acdsp_ddc {
  acdsp_cic_t cic = nullptr;     // stage A: parameter checks, INT_TYPE, FIR-identity taps; runs the stage in two-kernel mode
  acdsp_fir_t fir = nullptr;     // stage B: coefficient checks; runs the stage in two-kernel mode
  // what the caller handed to acdsp_ddc_create_ex: clone recreates from these -- under ACDSP_DDC_IN_BYTES the decimator stage itself was created
  // from a copy carrying ACDSP_FLAG_IN_BYTES (cic->d), which the cascade's own entry point refuses
  acdsp_cic_desc_t cic_desc;
  acdsp_fir_desc_t fir_desc;
  int32_t ddc_flags = 0;
  bool fused = false;           // decided at creation / coefficient load; a handle never switches modes mid-stream
  // fused mode: the only state is the input history (stage B's window is recomputed from it) and the input count
  int hl = 0;
  History hist;
  int64_t t_total = 0;
  PhasePlans plansA;
  FirGenPlan planB;
  DevBuf d_fragB;
  bool coeffs_set = false;
  // two-kernel mode: intermediate stream
  DevBuf d_mid;
  int64_t mid_cap = 0;
  bool captured = false;         // a call of this handle has been recorded into a graph, which holds d_mid's address: growing the buffer
  std::vector<DevBuf> retired;   // later (eager) keeps the old one here instead of freeing it
  Timer tm;
  // polydec cascade (acdsp_ddc_create_polydec): stage B is the decimating ac_poly_dec `pd` and `fir` stays null.  df = its DF (0: FIR cascade).
  // A call consumes whole groups of DF intermediate words; the q < DF words behind the last whole group wait for the next call.  Fused mode
  // recomputes them from the input history (q = ceil(t_total / R) % DF); two-kernel mode keeps them at the front of d_mid (n_q of them).
  acdsp_polydec_t pd = nullptr;
  acdsp_polydec_desc_t pd_desc;
  int df = 0;
  int64_t n_q = 0;
  FirGenPlan planBq[kDdcMaxFusedDf];   // fused: the prototype's plan at window phase first = DF - 1 - q; fragments in d_fragB, kGenFragWords apart
  std::vector<int64_t> h_pd_coeffs;     // last [NTAPS*DF] set (for clone)
};

namespace acdsp {
namespace eng {
// current reg_trans[] buffer of a use_rt handle
inline int64_t *fir_rt_cur(const acdsp_fir *h) { return h->d_rt[h->rt_hybrid ? h->cur_rt : h->hist.index()].get<int64_t>(); }
// refusals of acdsp_cic_run / acdsp_fir_run while the stream is capturing (ACDSP_ESTATE with the message set), else ACDSP_OK: no side effects
int cic_capture_check(const acdsp_cic *h, const void *d_in, int64_t in_stride, int64_t n_in);
int fir_capture_check(const acdsp_fir *h, const void *d_in, int64_t in_stride, int64_t n);
// two-kernel DDC: intermediate rows of at least `cap` words, the queued words of a polydec cascade kept (engine_ddc.hip; the state blobs load into them)
int ddc_mid_reserve(acdsp_ddc *h, int64_t cap, hipStream_t s);
// ... and the capacity that holds every word that can wait between two calls of a polydec cascade (DF - 1), as run() would round it: what a
// clone and a loaded blob reserve before they copy the queue in
inline int64_t ddc_queue_cap(int df) { return ((int64_t)df + 15) / 16 * 16 + 16; }
// FIR helpers other families use (engine_fir.hip)
std::vector<int64_t> effective_coeffs(const int64_t *c, int N, int ftype);
int internal_ftype(int kind, int ftype);
// rt_hybrid: rebuild reg_trans[] from the input history (engine_fir.hip; the state blobs need it)
int32_t fir_rt_from_hist(acdsp_fir *h);
}  // namespace eng
}  // namespace acdsp
