// tb_mvavg_bytes.cpp -- acdsp::mvavg_engine with ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES: 1-byte input and output containers through the
// C++ layer.  A doubly flagged engine, one with the input flag alone and an unflagged one (int16 containers) are fed the same 8-bit samples
// through run_host; the raw output words must agree, whatever their container.  Signed and unsigned samples, AC_MIRROR and AC_WIN.
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

template <class IN, class COEFF, class ACC, class OUT>
static int run_case(const char *name, int win_mode) {
  const int TAPS = 9, N = 512, FRAMES = 3, N_OBJ = 3;
  typedef acdsp::mvavg_engine<IN, COEFF, ACC, OUT> engine_t;
  engine_t both(N, TAPS, win_mode, N_OBJ, -1, ACDSP_FLAG_IN_BYTES | ACDSP_FLAG_OUT_BYTES), in_only(N, TAPS, win_mode, N_OBJ, -1, ACDSP_FLAG_IN_BYTES),
      words(N, TAPS, win_mode, N_OBJ);
  int fails = 0;
  if (both.in_bytes() != 1 || both.out_bytes() != 1 || in_only.in_bytes() != 1 || in_only.out_bytes() != 2 || words.in_bytes() != 2 || words.out_bytes() != 2) {
    std::cout << name << ": in_bytes() / out_bytes() of the three engines\n";
    fails++;
  }
  std::vector<int64_t> c((size_t)TAPS);
  for (int i = 0; i < TAPS; i++) { c[(size_t)i] = 3 + 2 * i; }   // raw COEFF words, sum 99
  both.set_coeffs_raw(c); in_only.set_coeffs_raw(c); words.set_coeffs_raw(c);
  uint32_t lcg = 2463534242u;
  std::vector<int64_t> raw((size_t)(N_OBJ * N * FRAMES));
  for (size_t i = 0; i < raw.size(); i++) {
    lcg = lcg * 1664525u + 1013904223u;
    IN v;
    v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
    raw[i] = acdsp::raw_of(v);
  }
  std::vector<unsigned char> xb, xw;
  acdsp::pack(raw, 1, xb);
  acdsp::pack(raw, 2, xw);
  const int64_t no = both.out_per_frame(N) * FRAMES;
  std::vector<unsigned char> y1((size_t)(N_OBJ * no)), y2((size_t)(N_OBJ * no) * 2), yw(y2.size());
  int64_t n1 = -1, n2 = -1, nw = -1;
  both.run_host(xb.data(), N, FRAMES, y1.data(), no, &n1);
  in_only.run_host(xb.data(), N, FRAMES, y2.data(), no, &n2);
  words.run_host(xw.data(), N, FRAMES, yw.data(), no, &nw);
  if (n1 != no || n2 != no || nw != no || no <= 0) { std::cout << name << ": output counts " << n1 << " / " << n2 << " / " << nw << " / " << no << "\n"; fails++; }
  if (y2 != yw) { std::cout << name << ": the engine with byte inputs differs from the int16 engine\n"; fails++; }
  long bad = 0;
  for (size_t i = 0; i < y1.size(); i++) {
    // the 8-bit OUT raw word sits in the low byte of the little-endian int16 container, sign- or zero-extended above it
    const unsigned char ext = (OUT::sign && (yw[2 * i] & 0x80)) ? 0xff : 0x00;
    if (y1[i] != yw[2 * i] || yw[2 * i + 1] != ext) { bad++; }
  }
  if (bad) { std::cout << name << ": " << bad << " byte outputs differ from the int16 engine's words\n"; fails++; }
  if (acdsp_mvavg_in_elem_bytes(both.handle()) != 1 || acdsp_mvavg_out_elem_bytes(both.handle()) != 1 || acdsp_mvavg_out_elem_bytes(in_only.handle()) != 2 ||
      acdsp_mvavg_in_elem_bytes(words.handle()) != 2) {
    std::cout << name << ": acdsp_mvavg_in_elem_bytes / acdsp_mvavg_out_elem_bytes\n";
    fails++;
  }
  engine_t copy(both);   // a copy carries the flags and the coefficients
  std::vector<unsigned char> y3(y1.size());
  int64_t n3 = -1;
  copy.set_coeffs_raw(c);
  copy.run_host(xb.data(), N, FRAMES, y3.data(), no, &n3);
  if (n3 != no || y3 != y1 || copy.out_bytes() != 1) { std::cout << name << ": a copied engine differs\n"; fails++; }
  std::cout << name << ": " << (long)raw.size() << " samples, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 4, true>, ac_fixed<8, 1, true>, ac_fixed<24, 12, true>, ac_fixed<8, 4, true, AC_RND, AC_SAT> >("signed <8,4> AC_MIRROR", ACDSP_WIN_MIRROR);
  fails += run_case<ac_fixed<8, 8, false>, ac_fixed<8, 1, true>, ac_fixed<24, 17, true>, ac_fixed<8, 8, false, AC_RND, AC_SAT> >("unsigned <8,8> AC_WIN", ACDSP_WIN_PLAIN);
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
