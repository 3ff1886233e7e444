"""Value semantics at the boundary, the part that needs no device: the drop-in classes and the batched engines are copyable types
(a compile-only translation unit), and the clone / state entry points of the later operator families exist, are declared, and refuse
null arguments before they touch a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATE_FAMILIES = ("polydec", "polyintr", "intgdump")
CLONE_FAMILIES = ("polydec", "polyintr", "intgdump", "mvavg", "ddc")
NEW_SYMBOLS = (["acdsp_%s_clone" % f for f in CLONE_FAMILIES] +
               ["acdsp_%s_state_%s" % (f, op) for f in STATE_FAMILIES for op in ("size", "get", "set")])

COPYABLE_TU = r"""
#include <ac_dsp/ac_poly_intr.h>   // (its FTYPE enum first: it cannot share a translation unit with the FIR headers' one)
#include <ac_dsp/ac_poly_dec.h>
#include <ac_dsp/ac_intg_dump.h>
#include <ac_dsp/ac_mv_avg.h>

#include <type_traits>
#include <vector>

typedef ac_fixed<16, 2, true> IN_T;
typedef ac_fixed<16, 2, true> CF_T;
typedef ac_fixed<40, 12, true> ACC_T;
typedef ac_fixed<16, 3, true, AC_RND, AC_SAT> OUT_T;
struct STR_CF { CF_T coeffs[6 * 4]; };
struct STR_ICF { CF_T coeffs[32]; };
struct STR_CTRL { bool sign[4]; ac_int<8, false> corr[4]; };

typedef ac_poly_dec<IN_T, CF_T, STR_CF, ACC_T, OUT_T, 6, 4> DEC;
typedef ac_poly_intr<IN_T, CF_T, ACC_T, OUT_T, STR_CTRL, STR_ICF, 16, 32, 4, FOLD_EVEN> INTR;
typedef ac_intg_dump<IN_T, ACC_T, OUT_T, ac_int<8, false>, 16, 3> DUMP;
typedef ac_mv_avg<64, 5, AC_MIRROR, IN_T, OUT_T, ACC_T, CF_T, ac_int<8, false> > AVG;
typedef acdsp::polydec_engine<IN_T, CF_T, ACC_T, OUT_T> DEC_E;
typedef acdsp::polyintr_engine<IN_T, CF_T, ACC_T, OUT_T> INTR_E;
typedef acdsp::intgdump_engine<IN_T, ACC_T, OUT_T> DUMP_E;
typedef acdsp::mvavg_engine<IN_T, CF_T, ACC_T, OUT_T> AVG_E;
typedef acdsp::ddc_engine<ac_fixed<16, 2, true>, ac_fixed<36, 22, true>, ac_fixed<24, 6, true>, CF_T, ac_fixed<56, 26, true> > DDC_E;

#define COPYABLE(T) \
  static_assert(std::is_copy_constructible<T>::value, #T " is copy-constructible"); \
  static_assert(std::is_copy_assignable<T>::value, #T " is copy-assignable")
COPYABLE(DEC); COPYABLE(INTR); COPYABLE(DUMP); COPYABLE(AVG);
COPYABLE(DEC_E); COPYABLE(INTR_E); COPYABLE(DUMP_E); COPYABLE(AVG_E); COPYABLE(DDC_E);

void holds_filters_by_value() {
  std::vector<DEC> v(3);
  v.push_back(v[0]);
  struct bank { DEC dec; INTR intr; DUMP dump; } a, b;
  b = a;
  bank c(a);
  (void)c;
}
"""


def test_drop_in_classes_and_engines_are_copyable_types(tmp_path):
    src = tmp_path / "copyable.cpp"
    src.write_text(COPYABLE_TU)
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include", "ac_types"), "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")


def test_header_declares_and_library_exports_the_new_symbols():
    from ac_dsp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acdsp.h")).read()
    declared = set(re.findall(r"\b(acdsp_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/acdsp.h"
        assert name in _lib.SYMBOLS, name + " has no prototype in _lib.SYMBOLS"
        assert hasattr(_lib.lib, name), name + " is not exported by libacdsp.so"
    assert _lib.lib.acdsp_abi_version() == 1


def test_null_arguments_are_refused_without_a_device():
    from ac_dsp_amd._lib import lib
    EINVAL = 1
    buf = (C.c_char * 64)()
    out = C.c_void_p()
    for fam in STATE_FAMILIES:
        assert getattr(lib, "acdsp_%s_state_size" % fam)(None) == -1
        assert getattr(lib, "acdsp_%s_state_get" % fam)(None, buf, 64) == EINVAL
        assert getattr(lib, "acdsp_%s_state_set" % fam)(None, buf, 64) == EINVAL
        assert b"null" in lib.acdsp_last_error()
    for fam in CLONE_FAMILIES:
        assert getattr(lib, "acdsp_%s_clone" % fam)(None, C.byref(out)) == EINVAL
        assert out.value is None
