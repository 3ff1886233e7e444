// ac_poly_dec.h -- drop-in for hlslibs/ac_dsp's polyphase FIR decimator, MI355X back end.
//
// Same class template and run() signature as the reference (include/ac_dsp/ac_poly_dec.h:82-107):
// coefficients arrive as a struct { COEFF_TYPE coeffs[NTAPS*DF]; } on their own channel (the last one queued
// wins, :101-106), data is consumed in whole groups of DF samples (`while (data_in.available(DF))`, :109 --
// fewer than DF left-over samples stay in the channel) and every group yields one output.  The loop nest
// (:112-128) runs as HIP kernels behind include/acdsp.h.
// Like the reference class the object is copyable: a copy carries the stream (the engine's input history = taps[]) and the
// coefficient struct, and the two objects are independent afterwards.
#ifndef _INCLUDED_AC_POLY_DEC_H_
#define _INCLUDED_AC_POLY_DEC_H_

#include <ac_fixed.h>
#include <ac_channel.h>
#include <mc_scverify.h>
#include <ac_dsp/acdsp_engine.h>

template < class IN_TYPE, class COEFF_TYPE, class STR_COEFF_TYPE, class ACC_TYPE, class OUT_TYPE, int NTAPS, int DF >
class ac_poly_dec
{
public:
  ac_poly_dec() : eng_(NTAPS, DF), have_coeffs_(false) {}

#pragma hls_pipeline_init_interval 1
#pragma hls_design interface
  void CCS_BLOCK(run)( ac_channel < IN_TYPE > &data_in, ac_channel < OUT_TYPE > &data_out, ac_channel < STR_COEFF_TYPE > &coeffs_st ) {
    while (coeffs_st.available(1)) { coeffs_t = coeffs_st.read(); have_coeffs_ = true; }
    std::vector<int64_t> raw;
    while (data_in.available(DF)) {
      for (int i = 0; i < DF; i++) { raw.push_back(acdsp::raw_of(data_in.read())); }
    }
    if (raw.empty()) { return; }
    std::vector<int64_t> c((size_t)NTAPS * DF, 0);   // coefficients are zero until the first struct arrives (don't care in the reference)
    if (have_coeffs_) { for (int i = 0; i < NTAPS * DF; i++) { c[(size_t)i] = acdsp::raw_of(coeffs_t.coeffs[i]); } }
    eng_.set_coeffs_raw(c);   // (uploaded only when the set changed)
    const int ib = acdsp_elem_bytes(IN_TYPE::width), ob = acdsp_elem_bytes(OUT_TYPE::width);
    std::vector<unsigned char> bi, bo(raw.size() / DF * (size_t)ob);
    acdsp::pack(raw, ib, bi);
    eng_.run_host(bi.data(), (int64_t)raw.size(), bo.data());
    for (size_t i = 0; i < raw.size() / DF; i++) {
      data_out.write(acdsp::from_raw<OUT_TYPE>(acdsp::unpack_one(&bo[i * ob], ob, OUT_TYPE::sign)));
    }
  }

private:
  // members copy one by one: the engine clones its handle (stream state and the coefficient set on it), the struct is plain data
  acdsp::polydec_engine<IN_TYPE, COEFF_TYPE, ACC_TYPE, OUT_TYPE> eng_;
  bool have_coeffs_;
  STR_COEFF_TYPE coeffs_t;
};

#endif
