"""Every A/B environment switch of libacdsp.so against the CPU oracle.

The library reads its ACDSP_* switches once per process (function-local statics), so none of them can be flipped from inside the pytest
process: each row of tests/knob_legs.py LEGS runs as one child process (tests/knob_child.py) with that row's environment.  A leg must show
  (a) exit status 0 and no word that differs from the oracle,
  (b) the witness the row expects under the switch -- what the ABI reports about the kernel that ran,
  (c) the row's "without" witness in the default leg, different from (b): the switch took effect and the shapes reach the default side,
  (d) the default leg's state_size for every handle (a switch does not change the state geometry), but for the rows that say why theirs differs.
Rows without a witness (nothing the ABI or the trace lines report tells their two sides apart) run (a) and (d).

One child at a time.  A child that is killed by its time limit, dies of a signal or reports a GPU fault sets a latch: every later test of the
module fails at once and nothing more is started on the GPU."""
import json
import os
import subprocess
import sys
import time

import pytest

from knob_legs import DEFAULT_BATTERIES, all_legs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "knob_child.py")
KEEP = ("ACDSP_LIB", "ACDSP_ORACLE_LIB")
LATCH = {"leg": None}
TIMES = {}


def run_leg(name, env, batteries):
    """-> {battery: its JSON line}; asserts (a)"""
    if LATCH["leg"] is not None:
        pytest.fail("not started: leg %s ended abnormally" % LATCH["leg"])
    e = {k: v for k, v in os.environ.items() if not k.startswith("ACDSP_") or k in KEEP}   # a switch exported in the caller's shell must not leak into a leg
    e.update(env)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, CHILD] + list(batteries), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    except subprocess.TimeoutExpired:
        LATCH["leg"] = name
        pytest.fail("leg %s: the child ran into its time limit" % name)
    TIMES[name] = time.perf_counter() - t0
    out, err = p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (134, 137, 139) or "illegal memory access" in out + err:
        LATCH["leg"] = name
        pytest.fail("leg %s ended abnormally (return code %d)\n%s\n%s" % (name, p.returncode, out[-2000:], err[-4000:]))
    res = {}
    for ln in out.splitlines():
        if ln.startswith("{"):
            r = json.loads(ln)
            res[r["battery"]] = r
    print("leg %s: %.1f s, %s" % (name, TIMES[name], {b: (r["cases"], r["mismatches"]) for b, r in res.items()}))
    bad = {b: r["first"] for b, r in res.items() if r["mismatches"]}
    assert not bad, "leg %s: words differ from the oracle: %s" % (name, bad)
    assert p.returncode == 0 and sorted(res) == sorted(batteries), "leg %s: return code %d, batteries %s of %s\n%s" % (name, p.returncode, sorted(res), batteries, err[-4000:])
    assert all(r["cases"] > 0 for r in res.values())
    return res


def flat(res, field):
    return {"%s:%s" % (b, k): v for b, r in res.items() for k, v in r[field].items()}


@pytest.fixture(scope="module")
def default_leg():
    """every battery once with no switch set: the witnesses and state sizes the switch legs are held against"""
    res = run_leg("default", {}, DEFAULT_BATTERIES)
    return flat(res, "witness"), flat(res, "state_size")


def test_default_leg_runs_every_battery(default_leg):
    witness, sizes = default_leg
    assert witness and sizes
    used = {b for _, row in all_legs() for b in row["batteries"]}
    assert used == set(DEFAULT_BATTERIES), used ^ set(DEFAULT_BATTERIES)


@pytest.mark.parametrize("name,row", all_legs(), ids=[n for n, _ in all_legs()])
def test_switch_leg(name, row, default_leg):
    d_witness, d_sizes = default_leg
    res = run_leg(name, row["env"], row["batteries"])                                  # (a)
    witness, sizes = flat(res, "witness"), flat(res, "state_size")
    if row["under"] is not None:
        assert set(row["under"]) == set(row["without"]) and row["under"] != row["without"], "the row's two witnesses must name the same entries and differ"
        got = {k: witness.get(k) for k in row["under"]}
        assert got == row["under"], "leg %s: witness under the switch %s, expected %s" % (name, got, row["under"])          # (b)
        base = {k: d_witness.get(k) for k in row["without"]}
        assert base == row["without"], "leg %s: the default leg shows %s where the row expects %s: the shape does not reach the default side" % (name, base, row["without"])   # (c)
    if row["state"] is None:
        assert sizes == {k: d_sizes.get(k) for k in sizes}, "leg %s: state sizes %s, default leg %s" % (name, sizes, {k: d_sizes.get(k) for k in sizes})   # (d)
    else:
        assert isinstance(row["state"], str) and row["state"].strip()

