// tb_cic_bytes.cpp -- acdsp::cic_engine with ACDSP_FLAG_IN_BYTES: 1-byte input containers through the C++ layer.  A flagged decimator and an
// unflagged one (int16 containers) are fed the same ac_fixed<8,1> samples in two calls; every output must agree.  Between the calls the state
// of the flagged engine crosses into a second flagged engine through state() / set_state() (the 1-byte state blob), which must then
// continue the stream like the first.  Unsigned samples likewise.
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

template <class IN, class OUT>
static int run_case(const char *name) {
  const unsigned R = 64, M = 1, N = 4;
  acdsp::cic_engine<IN, OUT> bytes(false, R, M, N, 1, -1, ACDSP_FLAG_IN_BYTES), moved(false, R, M, N, 1, -1, ACDSP_FLAG_IN_BYTES);
  acdsp::cic_engine<IN, OUT> words(false, R, M, N);
  int fails = 0;
  if (bytes.in_bytes() != 1 || words.in_bytes() != 2) { std::cout << name << ": in_bytes() " << bytes.in_bytes() << " / " << words.in_bytes() << "\n"; fails++; }
  const int calls[] = {70001, 41003};
  uint32_t lcg = 12345u;
  long total = 0;
  for (unsigned k = 0; k < 2; k++) {
    std::vector<IN> x((size_t)calls[k]);
    for (size_t i = 0; i < x.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
      x[i] = v;
    }
    std::vector<OUT> yb, yw, ym;
    bytes.run_values(x, yb);
    words.run_values(x, yw);
    if (k == 1) { moved.run_values(x, ym); } else { ym = yb; }
    if (yb.size() != yw.size() || ym.size() != yw.size() || yw.empty()) { std::cout << name << ": call " << k << " output counts " << yb.size() << " / " << yw.size() << " / " << ym.size() << "\n"; fails++; continue; }
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
    total += calls[k];
  }
  if (acdsp_cic_in_elem_bytes(bytes.handle()) != 1 || acdsp_cic_in_elem_bytes(words.handle()) != 2) { std::cout << name << ": acdsp_cic_in_elem_bytes\n"; fails++; }
  if (acdsp_cic_path(bytes.handle()) != ACDSP_PATH_CIC_2STAGE) { std::cout << name << ": path " << acdsp_cic_path(bytes.handle()) << "\n"; fails++; }
  std::cout << name << ": " << total << " samples in 2 calls, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 1, true>, ac_fixed<32, 25, true> >("signed <8,1>");
  fails += run_case<ac_fixed<8, 8, false>, ac_fixed<33, 33, true> >("unsigned <8,8>");
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
