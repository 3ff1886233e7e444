// tb_bytes.cpp -- acdsp::fir_engine with ACDSP_FLAG_IN_BYTES: 1-byte input containers through the C++ layer.  A flagged engine and an
// unflagged one (int16 containers) are fed the same ac_fixed<8,2> samples, in calls small enough for the header's host loop and large
// enough for the GPU in turn, so that the filter state moves both ways through the engine's 1-byte state blob (container_io with eb == 1);
// every output must agree.  Unsigned samples likewise.
#include <ac_dsp/ac_fir_load_coeffs.h>

#include <iostream>
#include <vector>

typedef ac_fixed<16, 2, true> C16;
typedef ac_fixed<48, 28, true> ACC;
typedef ac_fixed<16, 8, true, AC_RND, AC_SAT> OUT16;

template <class IN>
static int run_case(const char *name) {
  const int TAPS = 63;
  std::vector<C16> c(TAPS);
  for (int i = 0; i < TAPS; i++) { c[i] = C16(0.9 * (((i * 37) % 19) - 9) / 8.0); }
  acdsp::fir_engine<IN, OUT16, C16, ACC> bytes(ACDSP_FIR_LOAD, SHIFT_REG, TAPS, 1, false, -1, ACDSP_FLAG_IN_BYTES);
  acdsp::fir_engine<IN, OUT16, C16, ACC> words(ACDSP_FIR_LOAD, SHIFT_REG, TAPS);
  int fails = 0;
  if (bytes.in_bytes() != 1 || words.in_bytes() != 2) { std::cout << name << ": in_bytes() " << bytes.in_bytes() << " / " << words.in_bytes() << "\n"; fails++; }
  const int calls[] = {5, 300, 7, 1, 500, 64, 3};
  uint32_t lcg = 12345u;
  long total = 0;
  for (unsigned k = 0; k < sizeof calls / sizeof calls[0]; k++) {
    std::vector<IN> x((size_t)calls[k]);
    for (size_t i = 0; i < x.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
      x[i] = v;
    }
    std::vector<OUT16> yb, yw;
    bytes.run_values_c(x, yb, c.data());
    words.run_values_c(x, yw, c.data());
    for (size_t i = 0; i < x.size(); i++) {
      if (yb[i] != yw[i]) {
        if (fails < 5) { std::cout << name << ": call " << k << " sample " << i << ": " << yb[i].to_double() << " != " << yw[i].to_double() << "\n"; }
        fails++;
      }
    }
    total += calls[k];
  }
  if (acdsp_fir_in_elem_bytes(bytes.handle()) != 1 || acdsp_fir_in_elem_bytes(words.handle()) != 2) { std::cout << name << ": acdsp_fir_in_elem_bytes\n"; fails++; }
  std::cout << name << ": " << total << " samples in " << sizeof calls / sizeof calls[0] << " calls, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 2, true> >("signed <8,2>");
  fails += run_case<ac_fixed<8, 3, false> >("unsigned <8,3>");
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
