// tb_fir_outbytes.cpp -- acdsp::fir_engine with ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES: 1-byte containers on both sides of the C++ layer.
// A doubly flagged engine of 255 taps takes typed ac_fixed values in and gives typed values out (run_values: container_io packs the samples
// into 1-byte containers and unpacks the 1-byte outputs); every output is compared with the same filter written as a loop on the ac_fixed
// templates (`acc += x * c` into ACC_TYPE, `out = acc` into OUT_TYPE).  Calls of several lengths continue one stream, one of them long enough
// for the branch-free kernel instantiation.  Signed and unsigned types.
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

typedef ac_fixed<16, 2, true> C16;
typedef ac_fixed<48, 28, true> ACC;

template <class IN, class OUT>
static int run_case(const char *name, double gain) {
  const int TAPS = 255;
  std::vector<C16> c(TAPS);
  for (int i = 0; i < TAPS; i++) { c[i] = C16(gain * ((((i * 37) % 19) - 9) / 8.0 + 0.31)); }
  acdsp::fir_engine<IN, OUT, C16, ACC> eng(ACDSP_FIR_LOAD, ACDSP_SHIFT_REG, TAPS, 1, false, -1, ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES);
  int fails = 0;
  if (eng.in_bytes() != 1 || eng.out_bytes() != 1) { std::cout << name << ": in_bytes() " << eng.in_bytes() << ", out_bytes() " << eng.out_bytes() << "\n"; fails++; }
  eng.set_coeffs(c.data());
  const int calls[] = {300, 5, 4096 + 1024 + 77, 1, 2049};
  std::vector<IN> hist((size_t)TAPS, IN(0));   // hist[k] = x[n - 1 - k]
  uint32_t lcg = 2463534242u;
  long total = 0, on_bound = 0;
  OUT top, bottom;
  top.template set_val<AC_VAL_MAX>();
  bottom.template set_val<AC_VAL_MIN>();
  for (unsigned k = 0; k < sizeof calls / sizeof calls[0]; k++) {
    std::vector<IN> x((size_t)calls[k]);
    for (size_t i = 0; i < x.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
      x[i] = v;
    }
    std::vector<OUT> y;
    eng.run_values(x, y);
    if (y.size() != x.size()) { std::cout << name << ": call " << k << ": " << y.size() << " outputs\n"; fails++; continue; }
    for (size_t i = 0; i < x.size(); i++) {
      hist.insert(hist.begin(), x[i]);
      hist.pop_back();
      ACC acc = 0;
      for (int t = 0; t < TAPS; t++) { acc += hist[(size_t)t] * c[(size_t)t]; }
      const OUT want = acc;
      on_bound += (want == top || want == bottom) ? 1 : 0;
      if (y[i] != want) {
        if (fails < 5) { std::cout << name << ": call " << k << " sample " << i << ": " << y[i].to_double() << " != " << want.to_double() << "\n"; }
        fails++;
      }
    }
    total += calls[k];
  }
  if (acdsp_fir_out_elem_bytes(eng.handle()) != 1 || acdsp_fir_in_elem_bytes(eng.handle()) != 1) { std::cout << name << ": acdsp_fir_*_elem_bytes\n"; fails++; }
  if (acdsp_fir_path(eng.handle()) != ACDSP_PATH_MFMA_S8) { std::cout << name << ": path " << acdsp_fir_path(eng.handle()) << "\n"; fails++; }
  if (5 * on_bound > total) { std::cout << name << ": " << on_bound << " of " << total << " expected outputs sit on a bound of OUT_TYPE (more than 20 %)\n"; fails++; }
  std::cout << name << ": " << total << " samples in " << sizeof calls / sizeof calls[0] << " calls, " << on_bound << " on a bound, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 2, true>, ac_fixed<8, 6, true, AC_RND, AC_SAT> >("signed <8,2> into <8,6,RND,SAT>", 0.9);
  fails += run_case<ac_fixed<8, 3, false>, ac_fixed<8, 8, false, AC_RND, AC_SAT> >("unsigned <8,3> into unsigned <8,8,RND,SAT>", 0.4);
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
