"""GPU test of the C++ boundary's value semantics: tests/cpp/tb_value.cpp copies, assigns and reallocates the drop-in ac_poly_dec,
ac_poly_intr, ac_intg_dump and ac_mv_avg objects mid-stream and compares each with an uncopied object fed the same whole sequence."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "tb_value")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), EXE])   # the Makefile's pattern rule $(BIN)/%: %.cpp
    return EXE


def test_drop_in_objects_copy_their_streams(built):
    p = subprocess.run([built], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "Test PASSED." in out, out
