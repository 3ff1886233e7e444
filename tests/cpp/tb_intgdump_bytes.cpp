// tb_intgdump_bytes.cpp -- acdsp::intgdump_engine with ACDSP_FLAG_IN_BYTES: 1-byte input containers through the C++ layer.  A flagged engine
// and an unflagged one (int16 containers) are fed the same 8-bit samples through run_host in two calls; every output must agree.  The first
// call ends on a block that does not dump, so sums are pending between the calls: there the state of the flagged engine crosses into a fresh
// unflagged engine and that of the unflagged one into a fresh flagged engine (the blob holds ACC words, not samples: it moves both ways), and
// both must continue the stream like the originals.  Unsigned samples likewise.
#include <ac_fixed.h>
#include <ac_dsp/acdsp_engine.h>

#include <iostream>
#include <vector>

template <class IN, class ACC, class OUT>
static int run_case(const char *name) {
  const int NS = 64, CHN = 4, N_OBJ = 3;
  typedef acdsp::intgdump_engine<IN, ACC, OUT> engine_t;
  engine_t bytes(NS, CHN, N_OBJ, -1, ACDSP_FLAG_IN_BYTES), words(NS, CHN, N_OBJ);
  engine_t bytes_on_words(NS, CHN, N_OBJ, -1, ACDSP_FLAG_IN_BYTES), words_on_bytes(NS, CHN, N_OBJ);
  int fails = 0;
  if (bytes.in_bytes() != 1 || words.in_bytes() != 2) { std::cout << name << ": in_bytes() " << bytes.in_bytes() << " / " << words.in_bytes() << "\n"; fails++; }
  // call 0: 40 blocks that dump, then one whose n_sample = 0 (NS rounds, sums pending); call 1: a short block dumps them, then 32 whole ones
  std::vector<int64_t> tbl[2];
  tbl[0].assign(40, NS); tbl[0].push_back(0);
  tbl[1].assign(1, 9); tbl[1].insert(tbl[1].end(), 32, NS);
  uint32_t lcg = 2463534242u;
  long total = 0;
  for (unsigned k = 0; k < 2; k++) {
    int64_t ni = 0, no = 0;
    bytes.counts(tbl[k].data(), (int64_t)tbl[k].size(), &ni, &no);
    std::vector<int64_t> raw((size_t)(N_OBJ * ni));
    for (size_t i = 0; i < raw.size(); i++) {
      lcg = lcg * 1664525u + 1013904223u;
      IN v;
      v.set_slc(0, ac_int<8, false>((lcg >> 13) & 0xff));   // every raw word of the 8-bit type
      raw[i] = acdsp::raw_of(v);
    }
    std::vector<unsigned char> xb, xw;
    acdsp::pack(raw, 1, xb);
    acdsp::pack(raw, 2, xw);
    const size_t ob = (size_t)bytes.out_bytes();
    std::vector<unsigned char> yb((size_t)(N_OBJ * no) * ob), yw(yb.size()), ybw(yb.size()), ywb(yb.size());
    int64_t nb = -1, nw = -1;
    bytes.run_host(xb.data(), tbl[k].data(), (int64_t)tbl[k].size(), yb.data(), no, &nb);
    words.run_host(xw.data(), tbl[k].data(), (int64_t)tbl[k].size(), yw.data(), no, &nw);
    if (nb != no || nw != no || no == 0) { std::cout << name << ": call " << k << " output counts " << nb << " / " << nw << " / " << no << "\n"; fails++; continue; }
    if (yb != yw) { std::cout << name << ": call " << k << ": the flagged engine differs from the int16 engine\n"; fails++; }
    if (k == 0) {
      const std::vector<unsigned char> sb = bytes.state(), sw = words.state();
      if (sb != sw) { std::cout << name << ": the state blobs of the two engines differ\n"; fails++; }
      words_on_bytes.set_state(sb);
      bytes_on_words.set_state(sw);
    } else {
      int64_t n1 = -1, n2 = -1;
      bytes_on_words.run_host(xb.data(), tbl[k].data(), (int64_t)tbl[k].size(), ybw.data(), no, &n1);
      words_on_bytes.run_host(xw.data(), tbl[k].data(), (int64_t)tbl[k].size(), ywb.data(), no, &n2);
      if (n1 != no || n2 != no || ybw != yw || ywb != yw) { std::cout << name << ": an engine that took the other kind's state does not continue the stream\n"; fails++; }
    }
    total += (long)(N_OBJ * ni);
  }
  if (acdsp_intgdump_in_elem_bytes(bytes.handle()) != 1 || acdsp_intgdump_in_elem_bytes(words.handle()) != 2) { std::cout << name << ": acdsp_intgdump_in_elem_bytes\n"; fails++; }
  std::cout << name << ": " << total << " samples in 2 calls, " << fails << " mismatches\n";
  return fails;
}

int main() {
  int fails = run_case<ac_fixed<8, 4, true>, ac_fixed<32, 16, true>, ac_fixed<32, 16, true> >("signed <8,4>");
  fails += run_case<ac_fixed<8, 8, false>, ac_fixed<24, 24, false>, ac_fixed<20, 20, false, AC_TRN, AC_SAT> >("unsigned <8,8>");
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
