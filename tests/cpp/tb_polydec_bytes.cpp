// tb_polydec_bytes.cpp -- acdsp::polydec_engine with ACDSP_FLAG_IN_BYTES: 1-byte input containers through the C++ layer.  A flagged decimator
// and an unflagged one (int16 containers) are fed the same 8-bit samples in two calls; every output must agree.  Between the calls the
// state of the flagged engine crosses into a second flagged engine through state() / set_state() (the 1-byte state blob), which must then
// continue the stream like the first.  Unsigned samples likewise; a ring shape (16 x 8) and a long one (16 x 32).
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

template <class IN, class ACC>
static int run_case(const char *name, int nt, int df, int want_path) {
  typedef ac_fixed<16, 2, true> COEFF;
  typedef ac_fixed<24, 12, true, AC_RND, AC_SAT> OUT;
  acdsp::polydec_engine<IN, COEFF, ACC, OUT> bytes(nt, df, 1, -1, ACDSP_FLAG_IN_BYTES), moved(nt, df, 1, -1, ACDSP_FLAG_IN_BYTES), words(nt, df);
  int fails = 0;
  if (bytes.in_bytes() != 1 || words.in_bytes() != 2) { std::cout << name << ": in_bytes() " << bytes.in_bytes() << " / " << words.in_bytes() << "\n"; fails++; }
  uint32_t lcg = 2463534242u;
  std::vector<int64_t> c((size_t)nt * df);
  for (size_t i = 0; i < c.size(); i++) {
    lcg = lcg * 1664525u + 1013904223u;
    c[i] = (int64_t)((lcg >> 12) % 65408u) - 32768;           // -32768 .. 32639: splits into two signed bytes
  }
  bytes.set_coeffs_raw(c); moved.set_coeffs_raw(c); words.set_coeffs_raw(c);
  const int groups[] = {5003, 2048};
  long total = 0;
  for (unsigned k = 0; k < 2; k++) {
    std::vector<IN> x((size_t)groups[k] * df);
    for (size_t i = 0; i < x.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));     // every raw word of the 8-bit type
      x[i] = v;
    }
    const std::vector<OUT> yb = bytes.run_host(x), yw = words.run_host(x);
    const std::vector<OUT> ym = k == 1 ? moved.run_host(x) : yb;
    if (yb.size() != yw.size() || ym.size() != yw.size() || yw.size() != (size_t)groups[k]) { std::cout << name << ": call " << k << " output counts " << yb.size() << " / " << yw.size() << " / " << ym.size() << "\n"; fails++; continue; }
    for (size_t i = 0; i < yw.size(); i++) {
      if (yb[i] != yw[i] || ym[i] != yw[i]) {
        if (fails < 5) { std::cout << name << ": call " << k << " output " << i << ": " << yb[i].to_double() << " / " << ym[i].to_double() << " != " << yw[i].to_double() << "\n"; }
        fails++;
      }
    }
    if (k == 0) {
      const std::vector<unsigned char> blob = bytes.state();
      if (blob.size() == words.state().size()) { std::cout << name << ": the byte blob is as long as the int16 blob\n"; fails++; }
      moved.set_state(blob);
    }
    total += (long)groups[k] * df;
  }
  if (acdsp_polydec_in_elem_bytes(bytes.handle()) != 1 || acdsp_polydec_in_elem_bytes(words.handle()) != 2) { std::cout << name << ": acdsp_polydec_in_elem_bytes\n"; fails++; }
  if (bytes.path() != want_path) { std::cout << name << ": path " << bytes.path() << ", expected " << want_path << "\n"; fails++; }
  std::cout << name << ": " << total << " samples in 2 calls, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 2, true>, ac_fixed<40, 20, true> >("signed <8,2>, 16 x 8", 16, 8, ACDSP_PATH_MFMA_GEN);
  fails += run_case<ac_fixed<8, 0, false>, ac_fixed<48, 26, true> >("unsigned <8,0>, 16 x 8", 16, 8, ACDSP_PATH_MFMA_GEN);
  fails += run_case<ac_fixed<8, 2, true>, ac_fixed<40, 20, true> >("signed <8,2>, 16 x 32", 16, 32, ACDSP_PATH_MFMA_S8);
  fails += run_case<ac_fixed<8, 0, false>, ac_fixed<48, 26, true> >("unsigned <8,0>, 16 x 32", 16, 32, ACDSP_PATH_MFMA_S8);
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
