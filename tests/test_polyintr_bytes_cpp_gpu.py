"""GPU test of the C++ layer on byte rows of ac_poly_intr: tests/cpp/tb_polyintr_bytes.cpp runs acdsp::polyintr_engine with ACDSP_FLAG_IN_BYTES |
ACDSP_FLAG_OUT_BYTES, and with the input flag alone, against an unflagged engine on the same values through run_host."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_polyintr_bytes")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_polyintr_engine_with_byte_containers_equals_the_int16_engine(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
