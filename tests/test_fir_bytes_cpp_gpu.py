"""GPU test of the C++ layer on byte samples: tests/cpp/tb_bytes.cpp runs acdsp::fir_engine with ACDSP_FLAG_IN_BYTES against an unflagged engine
on the same values, host-loop and GPU calls in turn, so the state crosses the 1-byte state blob both ways."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_bytes")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_fir_engine_with_byte_containers_equals_the_int16_engine(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
