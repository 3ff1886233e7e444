// tb_ddc_bytes.cpp -- acdsp::ddc_engine with ACDSP_DDC_IN_BYTES: the DDC cascade on int8_t rows through the C++ layer.  The engine is fed
// ac_fixed<8,1> samples in 1-byte containers in two calls -- the second one by a COPY of the engine, which must continue the stream of its
// original -- and every channel checked equals the two drop-in classes chained, ac_cic_dec_full -> ac_fir_const_coeffs, on the same values.
#include <ac_dsp/ac_fir_const_coeffs.h>
#include <ac_dsp/ac_cic_dec_full.h>

#include <iostream>
#include <vector>

typedef ac_fixed<8, 1, true> DIN;
typedef ac_fixed<28, 21, true> DINT;     // find_inter_type_cic_dec for R 16, M 1, N 5 on <8,1>
typedef ac_fixed<16, 1, true> DCF;
typedef ac_fixed<60, 30, true> DACC;
typedef ac_fixed<24, 9, true, AC_RND, AC_SAT> DOUT;

int main() {
  const int dev = acdsp::default_device();
  const int DCH = 3, DT = 127;
  const int calls[2] = {16 * (256 * 9 + 40), 16 * (256 * 2 + 3)};   // whole chunks and a ragged end; a short second call
  const int DN = calls[0] + calls[1];
  std::vector<DCF> dc(DT);
  for (int i = 0; i < DT; i++) { dc[i] = DCF(0.4 * (((i * 29) % 23) - 11) / 32.0); }
  typedef acdsp::ddc_engine<DIN, DINT, DOUT, DCF, DACC> E;
  E first(16, 1, 5, ACDSP_FIR_CONST, SHIFT_REG, DT, DCH, -1, ACDSP_DDC_IN_BYTES);
  first.set_coeffs(dc.data());
  int fails = 0;
  if (first.in_bytes() != 1 || acdsp_ddc_in_elem_bytes(first.handle()) != 1) { std::cout << "in_bytes() " << first.in_bytes() << "\n"; fails++; }
  if (!first.fused()) { std::cout << "the byte cascade did not resolve to the fused kernel\n"; fails++; }

  std::vector<int8_t> hx((size_t)DCH * DN);
  uint32_t lcg = 4711u;
  for (size_t i = 0; i < hx.size(); i++) {
    lcg = lcg * 1664525u + 1013904223u;
    hx[i] = (int8_t)((lcg >> 13) & 0xff);   // every raw word of the 8-bit type
  }
  const int64_t no_all = DN / 16, so = (no_all + 11) / 4 * 4;   // output rows: 16-byte multiples of int32 containers
  void *d_in = 0, *d_out = 0;
  acdsp::check(acdsp_dev_alloc(dev, (uint64_t)DCH * DN, &d_in), "alloc");
  acdsp::check(acdsp_dev_alloc(dev, (uint64_t)DCH * so * 4, &d_out), "alloc");
  acdsp::check(acdsp_copy_h2d(dev, d_in, hx.data(), hx.size()), "h2d");
  std::vector<int32_t> hy((size_t)DCH * no_all);

  // call 0 on the engine, call 1 on a copy made behind call 0 (rows of the second call start calls[0] samples into every channel's row)
  int64_t got0 = 0, got1 = 0;
  first.run_device(d_in, DN, calls[0], d_out, so, &got0);
  acdsp::check(acdsp_sync(dev, 0), "sync");
  std::vector<int32_t> part((size_t)DCH * so);
  acdsp::check(acdsp_copy_d2h(dev, part.data(), d_out, part.size() * 4), "d2h");
  for (int ch = 0; ch < DCH; ch++) { for (int64_t t = 0; t < got0; t++) { hy[(size_t)ch * no_all + t] = part[(size_t)ch * so + t]; } }
  E second(first);
  if (second.in_bytes() != 1 || !second.fused() || acdsp_ddc_in_elem_bytes(second.handle()) != 1) { std::cout << "the copy lost the byte flag or the kernel mode\n"; fails++; }
  second.run_device((const char *)d_in + calls[0], DN, calls[1], d_out, so, &got1);
  acdsp::check(acdsp_sync(dev, 0), "sync");
  acdsp::check(acdsp_copy_d2h(dev, part.data(), d_out, part.size() * 4), "d2h");
  if (got0 != calls[0] / 16 || got1 != calls[1] / 16) { std::cout << "output counts " << got0 << " / " << got1 << "\n"; fails++; got1 = 0; }
  for (int ch = 0; ch < DCH; ch++) { for (int64_t t = 0; t < got1; t++) { hy[(size_t)ch * no_all + got0 + t] = part[(size_t)ch * so + t]; } }

  for (int ch = 0; ch < DCH; ch++) {
    ac_cic_dec_full<DIN, DINT, 16, 1, 5> cic;
    ac_fir_const_coeffs<DINT, DOUT, DCF, DACC, DT, SHIFT_REG> fir(dc.data());
    ac_channel<DIN> in;
    ac_channel<DINT> mid;
    ac_channel<DOUT> out;
    for (int t = 0; t < DN; t++) { in.write(acdsp::from_raw<DIN>(hx[(size_t)ch * DN + t])); }
    cic.run(in, mid);
    fir.run(mid, out);
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
  std::cout << "byte DDC cascade, " << DN << " samples in 2 calls (the second on a copy) vs chained per-channel objects: " << fails << " mismatches\n";
  acdsp::check(acdsp_dev_free(dev, d_in), "free");
  acdsp::check(acdsp_dev_free(dev, d_out), "free");
  std::cout << (fails ? "Test FAILED." : "Test PASSED.") << std::endl;
  return fails ? 1 : 0;
}
