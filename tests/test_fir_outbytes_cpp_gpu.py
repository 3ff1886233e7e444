"""GPU test of the C++ layer on byte outputs: tests/cpp/tb_fir_outbytes.cpp runs acdsp::fir_engine with ACDSP_FLAG_IN_BYTES |
ACDSP_FLAG_OUT_BYTES at 255 taps, typed ac_fixed values in and out, against the same filter written as a loop on the ac_fixed templates."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_fir_outbytes")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_fir_engine_with_byte_containers_on_both_sides_equals_the_ac_fixed_loop(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
