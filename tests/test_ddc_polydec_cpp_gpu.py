"""GPU test of the C++ layer of the polydec cascade: tests/cpp/tb_ddc_polydec.cpp runs acdsp::ddc_polydec_engine on int16 rows in two calls,
the first leaving a word waiting and the second on a copy of the engine, against the chained drop-in classes ac_cic_dec_full -> ac_poly_dec
on the same values."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_ddc_polydec")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_ddc_polydec_engine_equals_the_chained_drop_in_classes(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
