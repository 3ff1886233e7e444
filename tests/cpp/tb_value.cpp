// tb_value.cpp -- value semantics of the drop-in ac_poly_dec, ac_poly_intr, ac_intg_dump and ac_mv_avg classes (own code).
// The reference blocks are plain C++ objects whose streaming state lives in data members, so copying one copies its stream.
// For every class: an object is fed half a stream and copied; the original and the copy get DIFFERENT second halves and each must
// equal, value for value, an uncopied object fed the same whole sequence.  Also: copy-assignment onto an object that has already
// run, copies of a never-run object, self-assignment, and an object inside a std::vector that reallocates.
// Then the batched engines behind the classes (acdsp::polydec_engine, polyintr_engine, intgdump_engine, ddc_engine): calls on device
// rows, state() / set_state() into a fresh engine, copies at half time, reset(), each against an uninterrupted engine.
#include <ac_dsp/ac_poly_intr.h>   // (its FTYPE enum: this translation unit cannot take the FIR headers)
#include <ac_dsp/ac_poly_dec.h>
#include <ac_dsp/ac_intg_dump.h>
#include <ac_dsp/ac_mv_avg.h>

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned lcg(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
template <class T> static T rnd_word(unsigned &s) {
  T v;
  v.set_slc(0, ac_int<T::width, true>((int)(lcg(s) % (1u << T::width)) - (1 << (T::width - 1))));
  return v;
}

typedef ac_fixed<16, 2, true> IN_T;
typedef ac_fixed<16, 2, true> CF_T;
typedef ac_fixed<40, 12, true> ACC_T;
typedef ac_fixed<16, 3, true, AC_RND, AC_SAT> OUT_T;
typedef std::vector<OUT_T> outs;

// Chunks of a stream: 0 = the first half, 1 and 2 = two different second halves, 3 = an unrelated stream (what an object ran before it
// is assigned to).  Every adaptor D has: dut_t, make(), feed(dut, which, out) -- feed appends the outputs the chunk produced.

struct dec_d {   // ac_poly_dec: the coefficient struct travels with chunk 0 only, so a copy must carry coeffs_t / have_coeffs_ as well
  enum { NTAPS = 6, DF = 4 };
  struct STR_CF { CF_T coeffs[NTAPS * DF]; };
  typedef ac_poly_dec<IN_T, CF_T, STR_CF, ACC_T, OUT_T, NTAPS, DF> dut_t;
  static const char *name() { return "ac_poly_dec"; }
  static dut_t make() { return dut_t(); }
  static void feed(dut_t &d, int which, outs &y) {
    ac_channel<IN_T> in;
    ac_channel<OUT_T> out;
    ac_channel<STR_CF> cch;
    unsigned s = 1000u + (unsigned)which;
    if (which == 0 || which == 3) {
      STR_CF c;
      for (int i = 0; i < NTAPS * DF; i++) { c.coeffs[i] = rnd_word<CF_T>(s); }
      cch.write(c);
    }
    const int n = (which == 0 ? 37 : 23) * DF;   // whole groups: nothing stays queued
    for (int i = 0; i < n; i++) { in.write(rnd_word<IN_T>(s)); }
    d.run(in, out, cch);
    while (out.available(1)) { y.push_back(out.read()); }
  }
};

template <FTYPE ft, int HEAD> struct intr_d {   // ac_poly_intr: HEAD = 1 leaves the folded cores with saved sums only, nothing emitted yet
  enum { N = ft == FOLD_ODD ? 9 : 8, IFAC = 3, CSZ = N * IFAC };
  struct ctrl_s { bool sign[IFAC]; ac_int<8, false> corr[IFAC]; };
  struct coef_s { CF_T coeffs[CSZ]; };
  typedef ac_poly_intr<IN_T, CF_T, ACC_T, OUT_T, ctrl_s, coef_s, N, CSZ, IFAC, ft> dut_t;
  static const char *name() { return ft == FOLD_EVEN ? "ac_poly_intr FOLD_EVEN" : (ft == FOLD_ODD ? "ac_poly_intr FOLD_ODD" : "ac_poly_intr FOLD_ANTI"); }
  static dut_t make() { return dut_t(); }
  static void feed(dut_t &d, int which, outs &y) {
    ac_channel<IN_T> in;
    ac_channel<OUT_T> out;
    ac_channel<ctrl_s> cch;
    ac_channel<coef_s> kch;
    ac_channel<bool> flag;
    unsigned s = 2000u + (unsigned)which;
    if (which == 0 || which == 3) {
      ctrl_s ct;
      coef_s co;
      for (int j = 0; j < IFAC; j++) { ct.sign[j] = true; ct.corr[j] = IFAC - 1 - j; }
      for (int i = 0; i < CSZ; i++) { co.coeffs[i].set_slc(0, ac_int<CF_T::width, true>((int)(lcg(s) % 2000) - 1000)); }
      cch.write(ct); kch.write(co); flag.write(true);
      d.run(in, out, cch, kch, flag);
    }
    const int n = which == 0 ? HEAD : 11;
    for (int i = 0; i < n; i++) {
      in.write(rnd_word<IN_T>(s)); flag.write(false);
      d.run(in, out, cch, kch, flag);
    }
    while (out.available(1)) { y.push_back(out.read()); }
  }
};

struct dump_d {   // ac_intg_dump: chunk 0 ends on a block with n_sample = 0 -- NS rounds, no dump, its sums carry into the second half
  enum { NS = 8, CHN = 3 };
  typedef ac_int<8, false> N_T;
  typedef ac_intg_dump<IN_T, ACC_T, OUT_T, N_T, NS, CHN> dut_t;
  static const char *name() { return "ac_intg_dump"; }
  static dut_t make() { return dut_t(); }
  static void feed(dut_t &d, int which, outs &y) {
    static const int blocks[4][4] = {{5, 8, 3, 0}, {2, 7, 0, 4}, {6, 1, 8, 8}, {4, 0, 0, 2}};
    ac_channel<IN_T> in;
    ac_channel<OUT_T> out;
    ac_channel<N_T> nch;
    unsigned s = 3000u + (unsigned)which;
    for (int b = 0; b < 4; b++) {
      const int n = blocks[which][b], rounds = (n >= 1 && n <= NS) ? n : NS;
      nch.write(N_T(n));
      for (int k = 0; k < rounds * CHN; k++) { in.write(rnd_word<IN_T>(s)); }
    }
    d.run(in, out, nch);
    while (out.available(1)) { y.push_back(out.read()); }
  }
};

struct avg_d {   // ac_mv_avg: nothing crosses calls; a copy borrows the same coefficient array and must give the same frames
  enum { MAX_SAMPLE = 64, TAPS = 5 };
  typedef ac_int<8, false> S_T;
  typedef ac_mv_avg<MAX_SAMPLE, TAPS, AC_MIRROR, IN_T, OUT_T, ACC_T, CF_T, S_T> dut_t;
  static const char *name() { return "ac_mv_avg"; }
  static const CF_T *coeffs() {
    static CF_T c[TAPS];
    static bool init = false;
    if (!init) { unsigned s = 4000u; for (int i = 0; i < TAPS; i++) { c[i] = rnd_word<CF_T>(s); } init = true; }
    return c;
  }
  static dut_t make() { return dut_t(coeffs()); }
  static void feed(dut_t &d, int which, outs &y) {
    ac_channel<IN_T> in;
    ac_channel<OUT_T> out;
    ac_channel<S_T> nch;
    unsigned s = 4100u + (unsigned)which;
    const int n = 20 + which;
    nch.write(S_T(n));
    for (int i = 0; i < 2 * n; i++) { in.write(rnd_word<IN_T>(s)); }   // two frames
    d.run(in, out, nch);
    while (out.available(1)) { y.push_back(out.read()); }
  }
};

static int differs(const char *what, const char *cls, const outs &got, const outs &want) {
  int bad = got.size() != want.size() ? 1 : 0;
  for (size_t i = 0; i < got.size() && i < want.size(); i++) { if (!(got[i] == want[i])) { bad++; } }
  if (bad) { printf("  %s: %s: %d mismatches (%zu outputs, %zu expected)\n", cls, what, bad, got.size(), want.size()); }
  return bad;
}

template <class D> static int scenario() {
  typedef typename D::dut_t T;
  int bad = 0;
  // uncopied objects fed the whole sequences 0+1 and 0+2
  outs want_a, want_b;
  { T r = D::make(); D::feed(r, 0, want_a); D::feed(r, 1, want_a); }
  { T r = D::make(); D::feed(r, 0, want_b); D::feed(r, 2, want_b); }
  if (want_a.empty() || want_b.empty()) { printf("  %s: the reference sequences produced no output\n", D::name()); bad++; }
  {
    // copy construction at half time; copy-assignment onto an object that has already run another stream; self-assignment
    outs ya, yb, yc, junk;
    T a = D::make();
    D::feed(a, 0, ya);
    yb = ya; yc = ya;
    T b(a);
    T c = D::make();
    D::feed(c, 3, junk);
    c = a;
    T &self = a;
    a = self;
    D::feed(b, 2, yb);   // the copy first, then the original: neither disturbs the other
    D::feed(a, 1, ya);
    D::feed(c, 2, yc);
    bad += differs("original after being copied", D::name(), ya, want_a);
    bad += differs("copy-constructed object", D::name(), yb, want_b);
    bad += differs("object assigned to after it had run", D::name(), yc, want_b);
  }
  {
    // a never-run object: its copy starts a fresh stream, and assigning it replaces the stream of an object that has run
    outs ye, yf, yg, junk;
    T e = D::make();
    T f(e);
    T g = D::make();
    D::feed(g, 3, junk);
    g = e;
    D::feed(f, 0, yf); D::feed(f, 1, yf);
    D::feed(g, 0, yg); D::feed(g, 2, yg);
    D::feed(e, 0, ye); D::feed(e, 1, ye);
    bad += differs("copy of a never-run object", D::name(), yf, want_a);
    bad += differs("object assigned a never-run one", D::name(), yg, want_b);
    bad += differs("never-run object after being copied", D::name(), ye, want_a);
  }
  {
    // inside a std::vector that reallocates between the halves
    outs yv;
    std::vector<T> v;
    v.push_back(D::make());
    D::feed(v[0], 0, yv);
    const T *before = &v[0];
    while (&v[0] == before) { v.push_back(D::make()); }
    D::feed(v[0], 1, yv);
    bad += differs("element of a vector that reallocated", D::name(), yv, want_a);
  }
  printf("%-28s %s\n", D::name(), bad ? "FAILED" : "ok");
  return bad;
}

// ---- the batched engines behind the classes: device rows, checkpoint blobs, copies ----------------------------------------------------
typedef std::vector<int16_t> words;   // every type of this file lives in 2-byte containers

static words rnd_rows(unsigned seed, size_t n) {
  words w(n);
  for (size_t i = 0; i < n; i++) { w[i] = (int16_t)((int)(lcg(seed) % 65536u) - 32768); }
  return w;
}
static words part(const words &rows, int n_ch, size_t n, size_t lo, size_t hi) {   // columns [lo, hi) of dense [n_ch][n] rows
  words p;
  for (int c = 0; c < n_ch; c++) { p.insert(p.end(), rows.begin() + c * n + lo, rows.begin() + c * n + hi); }
  return p;
}
static int rows_differ(const char *what, const words &head, size_t nh, const words &tail, size_t nt, const words &whole, int n_ch) {
  int bad = 0;
  for (int c = 0; c < n_ch; c++) {
    for (size_t i = 0; i < nh + nt; i++) {
      const int16_t got = i < nh ? head[c * nh + i] : tail[c * nt + (i - nh)];
      if (got != whole[c * (nh + nt) + i]) { bad++; }
    }
  }
  if (bad) { printf("  %s: %d words differ from the uninterrupted run\n", what, bad); }
  return bad;
}
// dense host rows <-> device rows of `stride` containers, through the C ABI's own memory helpers
struct dev_rows {
  void *p;
  int n_ch, eb;
  size_t stride;
  dev_rows(int n_ch_, size_t n, int eb_) : p(0), n_ch(n_ch_), eb(eb_), stride((n + 63) / 64 * 64) {
    acdsp::check(acdsp_dev_alloc(acdsp::default_device(), (uint64_t)n_ch * stride * eb, &p), "acdsp_dev_alloc");
  }
  ~dev_rows() { acdsp_dev_free(acdsp::default_device(), p); }
  void put(const void *rows, size_t n) {
    std::vector<unsigned char> img((size_t)n_ch * stride * eb, 0);
    for (int c = 0; c < n_ch; c++) { memcpy(&img[c * stride * eb], (const unsigned char *)rows + c * n * eb, n * eb); }
    acdsp::check(acdsp_copy_h2d(acdsp::default_device(), p, img.data(), img.size()), "acdsp_copy_h2d");
  }
  void get(void *rows, size_t n) {
    std::vector<unsigned char> img((size_t)n_ch * stride * eb);
    acdsp::check(acdsp_sync(acdsp::default_device(), 0), "acdsp_sync");
    acdsp::check(acdsp_copy_d2h(acdsp::default_device(), img.data(), p, img.size()), "acdsp_copy_d2h");
    for (int c = 0; c < n_ch; c++) { memcpy((unsigned char *)rows + c * n * eb, &img[c * stride * eb], n * eb); }
  }
private:
  dev_rows(const dev_rows &);
  dev_rows &operator=(const dev_rows &);
};

template <class E> static words polydec_on_device(E &e, const words &x, int n_ch, size_t n_in, int df) {
  dev_rows in(n_ch, n_in, 2), out(n_ch, n_in / df, 2);
  in.put(x.data(), n_in);
  e.run(in.p, (int64_t)in.stride, (int64_t)n_in, out.p, (int64_t)out.stride);
  words y((size_t)n_ch * (n_in / df));
  out.get(y.data(), n_in / df);
  return y;
}

static int batched_polydec() {
  const int NT = 8, DF = 4, CH = 3;
  const size_t G = 300, GH = 133;                    // groups in all / before the cut
  typedef acdsp::polydec_engine<IN_T, CF_T, ACC_T, OUT_T> E;
  unsigned s = 5000u;
  std::vector<int64_t> c((size_t)NT * DF);
  for (size_t i = 0; i < c.size(); i++) { c[i] = (int)(lcg(s) % 65536u) - 32768; }
  const words x = rnd_rows(5001u, CH * G * DF);
  const words xh = part(x, CH, G * DF, 0, GH * DF), xt = part(x, CH, G * DF, GH * DF, G * DF);
  int bad = 0;
  E whole(NT, DF, CH);
  whole.set_coeffs_raw(c);
  words y_all(CH * G);
  whole.run_host(x.data(), (int64_t)(G * DF), y_all.data());
  // head on device rows, blob, a fresh engine takes the blob and the tail from host rows
  E a(NT, DF, CH);
  a.set_coeffs_raw(c);
  const words yh = polydec_on_device(a, xh, CH, GH * DF, DF);
  const std::vector<unsigned char> blob = a.state();
  E b(a);                                            // ... and a copy at the same point
  E r(NT, DF, CH);
  r.set_coeffs_raw(c);
  r.set_state(blob);
  words yt(CH * (G - GH)), ytb(CH * (G - GH));
  r.run_host(xt.data(), (int64_t)((G - GH) * DF), yt.data());
  b.run_host(xt.data(), (int64_t)((G - GH) * DF), ytb.data());
  bad += rows_differ("polydec_engine: head on device rows + restored tail", yh, GH, yt, G - GH, y_all, CH);
  bad += rows_differ("polydec_engine: copied engine's tail", yh, GH, ytb, G - GH, y_all, CH);
  if (r.path() != b.path() || a.state() != blob) { printf("  polydec_engine: path / state of the source changed\n"); bad++; }
  r.reset();                                         // back to a fresh stream
  words y2(CH * G);
  r.run_host(x.data(), (int64_t)(G * DF), y2.data());
  if (y2 != y_all) { printf("  polydec_engine: reset() did not start the stream anew\n"); bad++; }
  printf("%-28s %s\n", "polydec_engine", bad ? "FAILED" : "ok");
  return bad;
}

static int batched_polyintr() {
  const int N = 8, IFAC = 3, CH = 3, CSZ = N * IFAC;
  const size_t n = 200, nh = 77;
  typedef acdsp::polyintr_engine<IN_T, CF_T, ACC_T, OUT_T> E;
  unsigned s = 6000u;
  std::vector<int64_t> c((size_t)CSZ);
  for (size_t i = 0; i < c.size(); i++) { c[i] = (int)(lcg(s) % 2000u) - 1000; }
  std::vector<unsigned char> sg(IFAC, 1), cr(IFAC);
  for (int j = 0; j < IFAC; j++) { cr[j] = (unsigned char)(IFAC - 1 - j); }
  const words x = rnd_rows(6001u, CH * n);
  const words xh = part(x, CH, n, 0, nh), xt = part(x, CH, n, nh, n);
  int bad = 0;
  int64_t no = 0;
  E whole(N, CSZ, IFAC, ACDSP_POLY_FOLD_EVEN, CH);
  whole.set_ctrl_raw(c, sg, cr);
  const size_t o_all = (n - 1) * IFAC, o_h = (nh - 1) * IFAC, o_t = (n - nh) * IFAC;   // the first sample of a stream emits nothing
  words y_all(CH * o_all);
  whole.run_host(x.data(), (int64_t)n, y_all.data(), (int64_t)o_all, &no);
  if ((size_t)no != o_all) { bad++; }
  E a(N, CSZ, IFAC, ACDSP_POLY_FOLD_EVEN, CH);
  a.set_ctrl_raw(c, sg, cr);
  words yh(CH * o_h), yt(CH * o_t), ytb(CH * o_t);
  a.run_host(xh.data(), (int64_t)nh, yh.data(), (int64_t)o_h, &no);
  const std::vector<unsigned char> blob = a.state();
  E b = a;
  E r(N, CSZ, IFAC, ACDSP_POLY_FOLD_EVEN, CH);
  r.set_ctrl_raw(c, sg, cr);
  r.set_state(blob);
  if (r.out_count(5) != 5 * IFAC) { printf("  polyintr_engine: the restored engine counts like a fresh stream\n"); bad++; }
  r.run_host(xt.data(), (int64_t)(n - nh), yt.data(), (int64_t)o_t, &no);
  b.run_host(xt.data(), (int64_t)(n - nh), ytb.data(), (int64_t)o_t, &no);
  bad += rows_differ("polyintr_engine: head + restored tail", yh, o_h, yt, o_t, y_all, CH);
  bad += rows_differ("polyintr_engine: copied engine's tail", yh, o_h, ytb, o_t, y_all, CH);
  printf("%-28s %s\n", "polyintr_engine", bad ? "FAILED" : "ok");
  return bad;
}

static int batched_intgdump() {
  const int NS = 8, CHN = 3, OBJ = 4;
  typedef acdsp::intgdump_engine<IN_T, ACC_T, OUT_T> E;
  const int64_t th[4] = {5, 8, 3, 0}, tt[4] = {2, 7, 4, 1}, tw[8] = {5, 8, 3, 0, 2, 7, 4, 1};   // the head ends on a block that does not dump
  int bad = 0;
  E whole(NS, CHN, OBJ), a(NS, CHN, OBJ), r(NS, CHN, OBJ);
  int64_t ih = 0, oh = 0, it = 0, ot = 0, no = 0;
  a.counts(th, 4, &ih, &oh);
  a.counts(tt, 4, &it, &ot);
  const words x = rnd_rows(7001u, (size_t)OBJ * (ih + it));
  const words xh = part(x, OBJ, ih + it, 0, ih), xt = part(x, OBJ, ih + it, ih, ih + it);
  words y_all(OBJ * (oh + ot)), yh(OBJ * oh), yt(OBJ * ot), ytb(OBJ * ot);
  whole.run_host(x.data(), tw, 8, y_all.data(), oh + ot, &no);
  a.run_host(xh.data(), th, 4, yh.data(), oh, &no);
  const std::vector<unsigned char> blob = a.state();
  E b(a);
  r.set_state(blob);
  r.run_host(xt.data(), tt, 4, yt.data(), ot, &no);
  b.run_host(xt.data(), tt, 4, ytb.data(), ot, &no);
  bad += rows_differ("intgdump_engine: head + restored tail", yh, oh, yt, ot, y_all, OBJ);
  bad += rows_differ("intgdump_engine: copied engine's tail", yh, oh, ytb, ot, y_all, OBJ);
  printf("%-28s %s\n", "intgdump_engine", bad ? "FAILED" : "ok");
  return bad;
}

// the DDC cascade lives on device rows only: a copy taken inside a decimation period carries the phase and both stages
template <class E> static std::vector<int32_t> ddc_call(E &e, const words &x, int n_ch, size_t n_in) {
  const int64_t no = e.out_count((int64_t)n_in);
  dev_rows in(n_ch, n_in, 2), out(n_ch, (size_t)no, 4);
  in.put(x.data(), n_in);
  int64_t got = 0;
  e.run_device(in.p, (int64_t)in.stride, (int64_t)n_in, out.p, (int64_t)out.stride, &got);
  std::vector<int32_t> y((size_t)n_ch * (size_t)no);
  out.get(y.data(), (size_t)no);
  if (got != no) { y.clear(); }
  return y;
}

static int batched_ddc() {
  const int CH = 2, TAPS = 127, R = 16;
  typedef ac_fixed<16, 1, true> DIN;
  typedef ac_fixed<36, 21, true> DINT;
  typedef ac_fixed<24, 9, true, AC_RND, AC_SAT> DOUT;
  typedef ac_fixed<16, 1, true> DCF;
  typedef ac_fixed<60, 30, true> DACC;
  typedef acdsp::ddc_engine<DIN, DINT, DOUT, DCF, DACC> E;
  DCF c[TAPS];
  unsigned s = 8000u;
  for (int i = 0; i < TAPS; i++) { c[i].set_slc(0, ac_int<16, true>((int)(lcg(s) % 600u) - 300)); }
  const size_t nh = R * 100 + 5, nt = R * 60 + 3;
  const words xh = rnd_rows(8001u, CH * nh), xt = rnd_rows(8002u, CH * nt);
  int bad = 0;
  E ref(R, 1, 5, ACDSP_FIR_CONST, ACDSP_SHIFT_REG, TAPS, CH), a(R, 1, 5, ACDSP_FIR_CONST, ACDSP_SHIFT_REG, TAPS, CH);
  ref.set_coeffs(c);
  a.set_coeffs(c);
  const std::vector<int32_t> wh = ddc_call(ref, xh, CH, nh), wt = ddc_call(ref, xt, CH, nt);
  const std::vector<int32_t> yh = ddc_call(a, xh, CH, nh);
  E b(a);
  E d(R, 1, 5, ACDSP_FIR_CONST, ACDSP_SHIFT_REG, TAPS, CH);
  d = a;
  const std::vector<int32_t> yb = ddc_call(b, xt, CH, nt), ya = ddc_call(a, xt, CH, nt), yd = ddc_call(d, xt, CH, nt);
  if (wt.empty() || yh != wh || ya != wt || yb != wt || yd != wt || b.fused() != a.fused()) { printf("  ddc_engine: a copy does not continue the stream of its original\n"); bad++; }
  printf("%-28s %s\n", "ddc_engine", bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int fails = 0;
  fails += batched_ddc();
  fails += batched_polydec();
  fails += batched_polyintr();
  fails += batched_intgdump();
  fails += scenario<dec_d>();
  fails += scenario<intr_d<FOLD_EVEN, 1> >();
  fails += scenario<intr_d<FOLD_ODD, 9> >();
  fails += scenario<intr_d<FOLD_ANTI, 9> >();
  fails += scenario<dump_d>();
  fails += scenario<avg_d>();
  printf(fails ? "Test FAILED.\n" : "Test PASSED.\n");
  return fails ? 1 : 0;
}
