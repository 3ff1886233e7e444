// tb_polyintr_bytes.cpp -- acdsp::polyintr_engine with ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES: 1-byte input and output containers through
// the C++ layer.  A doubly flagged engine, one with the input flag alone and an unflagged one (int16 containers) are fed the same 8-bit samples
// through run_host, call by call (the folded cores emit nothing for the first sample of a stream); the raw output words must agree, whatever
// their container.  A folded core with symmetric pairs and the plain core, calls long enough for the matrix-core kernel and short ones.
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

template <class IN, class COEFF, class ACC, class OUT>
static int run_case(const char *name, int n_taps, int ifac, int ftype, bool pairs) {
  const int N_CH = 3;
  typedef acdsp::polyintr_engine<IN, COEFF, ACC, OUT> engine_t;
  const int csz = n_taps * ifac;   // (covers what every core reads)
  engine_t both(n_taps, csz, ifac, ftype, N_CH, -1, ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES), in_only(n_taps, csz, ifac, ftype, N_CH, -1, ACDSP_FLAG_IN_BYTES),
      words(n_taps, csz, ifac, ftype, N_CH);
  int fails = 0;
  if (both.in_bytes() != 1 || both.out_bytes() != 1 || in_only.in_bytes() != 1 || in_only.out_bytes() != 2 || words.in_bytes() != 2 || words.out_bytes() != 2) {
    std::cout << name << ": in_bytes() / out_bytes() of the three engines\n";
    fails++;
  }
  uint32_t lcg = 2463534242u;
  std::vector<int64_t> c((size_t)csz);
  for (int i = 0; i < csz; i++) {
    lcg = lcg * 1664525u + 1013904223u;
    c[(size_t)i] = (int64_t)((lcg >> 12) & 0xffff) - 32768;   // every raw word of a 16-bit COEFF_TYPE
  }
  std::vector<unsigned char> sign((size_t)ifac, 1), corr((size_t)ifac);
  for (int j = 0; j < ifac; j++) { corr[(size_t)j] = (unsigned char)(pairs ? ifac - 1 - j : j); }
  both.set_ctrl_raw(c, sign, corr); in_only.set_ctrl_raw(c, sign, corr); words.set_ctrl_raw(c, sign, corr);
  if (acdsp_polyintr_in_elem_bytes(both.handle()) != 1 || acdsp_polyintr_out_elem_bytes(both.handle()) != 1 || acdsp_polyintr_out_elem_bytes(in_only.handle()) != 2 ||
      acdsp_polyintr_in_elem_bytes(words.handle()) != 2) {
    std::cout << name << ": acdsp_polyintr_in_elem_bytes / acdsp_polyintr_out_elem_bytes\n";
    fails++;
  }
  const int calls[4] = {1, 700, 37, 1056};
  long total = 0;
  engine_t copy(both);   // a copy carries the flags (acdsp_polyintr_clone recreates the handle from its descriptor)
  for (int k = 0; k < 4; k++) {
    const int n = calls[k];
    std::vector<int64_t> raw((size_t)(N_CH * n));
    for (size_t i = 0; i < raw.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
      raw[i] = acdsp::raw_of(v);
    }
    std::vector<unsigned char> xb, xw;
    acdsp::pack(raw, 1, xb);
    acdsp::pack(raw, 2, xw);
    const int64_t no = both.out_count(n), cap = no > 0 ? no : 1;
    std::vector<unsigned char> y1((size_t)(N_CH * cap)), y2((size_t)(N_CH * cap) * 2), yw(y2.size());
    int64_t n1 = -1, n2 = -1, nw = -1;
    both.run_host(xb.data(), n, y1.data(), cap, &n1);
    in_only.run_host(xb.data(), n, y2.data(), cap, &n2);
    words.run_host(xw.data(), n, yw.data(), cap, &nw);
    if (n1 != no || n2 != no || nw != no) { std::cout << name << ": call " << k << ": output counts " << n1 << " / " << n2 << " / " << nw << " / " << no << "\n"; fails++; }
    if (no == 0) { continue; }
    if (y2 != yw) { std::cout << name << ": call " << k << ": the engine with byte inputs differs from the int16 engine\n"; fails++; }
    long bad = 0;
    for (size_t i = 0; i < y1.size(); i++) {
      // the 8-bit OUT raw word sits in the low byte of the little-endian int16 container, sign- or zero-extended above it
      const unsigned char ext = (OUT::sign && (yw[2 * i] & 0x80)) ? 0xff : 0x00;
      if (y1[i] != yw[2 * i] || yw[2 * i + 1] != ext) { bad++; }
    }
    if (bad) { std::cout << name << ": call " << k << ": " << bad << " byte outputs differ from the int16 engine's words\n"; fails++; }
    total += (long)raw.size();
  }
  if (copy.in_bytes() != 1 || copy.out_bytes() != 1) { std::cout << name << ": a copied engine lost its flags\n"; fails++; }
  std::cout << name << ": " << total << " samples, " << fails << " mismatches\n";
  return fails;
}

int main() {
  typedef ac_fixed<8, 2, true> I8;
  typedef ac_fixed<16, 2, true> C16;
  typedef ac_fixed<32, 12, true> A32;
  int fails = run_case<I8, C16, A32, ac_fixed<8, 2, true, AC_RND, AC_SAT> >("FOLD_EVEN 16 taps x IF 4, pairs", 16, 4, ACDSP_POLY_FOLD_EVEN, true);
  fails += run_case<I8, C16, A32, ac_fixed<8, 3, false, AC_RND, AC_SAT> >("FOLD_ANTI 12 taps x IF 7, unsigned outputs", 12, 7, ACDSP_POLY_FOLD_ANTI, false);
  fails += run_case<ac_fixed<8, 8, false>, C16, ac_fixed<40, 26, true>, ac_fixed<8, 8, false, AC_TRN, AC_WRAP> >("FOLD_ODD 15 taps x IF 3, unsigned samples", 15, 3,
                                                                                                           ACDSP_POLY_FOLD_ODD, true);
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
