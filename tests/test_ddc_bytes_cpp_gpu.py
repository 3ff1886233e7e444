"""GPU test of the C++ layer on byte samples of the DDC cascade: tests/cpp/tb_ddc_bytes.cpp runs acdsp::ddc_engine with ACDSP_DDC_IN_BYTES on
int8_t rows in two calls, the second one on a copy of the engine, against the chained drop-in classes ac_cic_dec_full -> ac_fir_const_coeffs
on the same values."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_ddc_bytes")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_ddc_engine_on_byte_rows_equals_the_chained_drop_in_classes(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
