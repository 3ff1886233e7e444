// tb_ddc_polydec.cpp -- acdsp::ddc_polydec_engine: the DDC cascade with a decimating second stage through the C++ layer.  The engine is fed
// ac_fixed<16,1> samples in two calls -- the first leaves one INT_TYPE word waiting, the second runs on a COPY of the engine, which must
// continue the stream of its original, waiting word included -- and every channel equals the two drop-in classes chained,
// ac_cic_dec_full -> ac_poly_dec, on the same values.
#include <ac_dsp/ac_poly_dec.h>
#include <ac_dsp/ac_cic_dec_full.h>

#include <iostream>
#include <vector>

typedef ac_fixed<16, 1, true> DIN;
typedef ac_fixed<36, 21, true> DINT;     // find_inter_type_cic_dec for R 16, M 1, N 5 on <16,1>
typedef ac_fixed<16, 1, true> DCF;
typedef ac_fixed<60, 30, true> DACC;
typedef ac_fixed<24, 9, true, AC_RND, AC_SAT> DOUT;
enum { DT = 64, DDF = 2 };
struct DSTR { DCF coeffs[DT * DDF]; };

int main() {
  const int dev = acdsp::default_device();
  const int DCH = 3;
  const int calls[2] = {16 * (2 * (1024 * 2 + 300) + 1), 16 * 513};   // whole chunks, a ragged end and an odd word count; a short second call
  const int DN = calls[0] + calls[1];
  DSTR dc;
  for (int i = 0; i < DT * DDF; i++) { dc.coeffs[i] = DCF(0.4 * (((i * 29) % 23) - 11) / 32.0); }
  typedef acdsp::ddc_polydec_engine<DIN, DCF, DACC, DOUT> E;
  E first(16, 1, 5, DT, DDF, DCH);
  first.set_coeffs(dc.coeffs);
  int fails = 0;
  if (first.int_type().W != 36 || first.int_type().I != 21) { std::cout << "INT_TYPE <" << first.int_type().W << "," << first.int_type().I << ">\n"; fails++; }
  if (!first.fused()) { std::cout << "the config-5 class at DF 2 did not resolve to the fused kernel\n"; fails++; }

  std::vector<int16_t> hx((size_t)DCH * DN);
  uint32_t lcg = 4711u;
  for (size_t i = 0; i < hx.size(); i++) {
    lcg = lcg * 1664525u + 1013904223u;
    hx[i] = (int16_t)((lcg >> 11) & 0xffff);   // every raw word of the 16-bit type
  }
  const int64_t no_all = DN / 16 / DDF, so = (no_all + 11) / 4 * 4;   // output rows: 16-byte multiples of int32 containers
  void *d_in = 0, *d_out = 0;
  acdsp::check(acdsp_dev_alloc(dev, (uint64_t)DCH * DN * 2, &d_in), "alloc");
  acdsp::check(acdsp_dev_alloc(dev, (uint64_t)DCH * so * 4, &d_out), "alloc");
  acdsp::check(acdsp_copy_h2d(dev, d_in, hx.data(), hx.size() * 2), "h2d");
  std::vector<int32_t> hy((size_t)DCH * no_all);

  // call 0 on the engine, call 1 on a copy made behind call 0 (rows of the second call start calls[0] samples into every channel's row)
  int64_t got0 = 0, got1 = 0;
  first.run_device(d_in, DN, calls[0], d_out, so, &got0);
  acdsp::check(acdsp_sync(dev, 0), "sync");
  std::vector<int32_t> part((size_t)DCH * so);
  acdsp::check(acdsp_copy_d2h(dev, part.data(), d_out, part.size() * 4), "d2h");
  if (got0 != calls[0] / 16 / DDF || got0 > no_all) { std::cout << "output count of call 0: " << got0 << "\n"; fails++; got0 = 0; }
  for (int ch = 0; ch < DCH; ch++) { for (int64_t t = 0; t < got0; t++) { hy[(size_t)ch * no_all + t] = part[(size_t)ch * so + t]; } }
  E second(first);
  if (!second.fused()) { std::cout << "the copy lost the kernel mode\n"; fails++; }
  second.run_device((const char *)d_in + (size_t)calls[0] * 2, DN, calls[1], d_out, so, &got1);
  acdsp::check(acdsp_sync(dev, 0), "sync");
  acdsp::check(acdsp_copy_d2h(dev, part.data(), d_out, part.size() * 4), "d2h");
  // (1 + 513 words: the waiting one completes the first group of the second call)
  if (got0 + got1 != no_all) { std::cout << "output counts " << got0 << " / " << got1 << "\n"; fails++; got1 = 0; }
  for (int ch = 0; ch < DCH; ch++) { for (int64_t t = 0; t < got1; t++) { hy[(size_t)ch * no_all + got0 + t] = part[(size_t)ch * so + t]; } }

  for (int ch = 0; ch < DCH; ch++) {
    ac_cic_dec_full<DIN, DINT, 16, 1, 5> cic;
    ac_poly_dec<DINT, DCF, DSTR, DACC, DOUT, DT, DDF> pd;
    ac_channel<DIN> in;
    ac_channel<DINT> mid;
    ac_channel<DOUT> out;
    ac_channel<DSTR> cch;
    for (int t = 0; t < DN; t++) { in.write(acdsp::from_raw<DIN>(hx[(size_t)ch * DN + t])); }
    cch.write(dc);
    cic.run(in, mid);
    pd.run(mid, out, cch);
    int bad = 0;
    for (int64_t t = 0; t < got0 + got1; t++) {
      const int64_t want = acdsp::raw_of(out.read());
      if (want != hy[(size_t)ch * no_all + t]) {
        if (bad < 3) { std::cout << "channel " << ch << " output " << t << ": " << hy[(size_t)ch * no_all + t] << " != " << want << "\n"; }
        bad++;
      }
    }
    fails += bad;
  }
  std::cout << "polydec DDC cascade, " << DN << " samples in 2 calls (the second on a copy) vs chained per-channel objects: " << fails << " mismatches\n";
  acdsp::check(acdsp_dev_free(dev, d_in), "free");
  acdsp::check(acdsp_dev_free(dev, d_out), "free");
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
