"""The tables of tests/knob_legs.py against the sources and INTEGRATION.md section 6: every ACDSP_* environment variable the library reads, or the
document lists, is a key of LEGS (tests/test_knobs_gpu.py runs it against the oracle) or of EXCLUDED (with the reason why not), and neither
table names a variable nothing reads any more.  A new switch fails here until it gets a leg or a stated reason.  No torch, no GPU."""
import glob
import os
import re

from knob_legs import DEFAULT_BATTERIES, EXCLUDED, LEGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ = re.compile(r'getenv\(\s*"(ACDSP_[A-Z0-9_]+)"|ACDSP_TUNE_ENV\(\s*\w+\s*,\s*"(ACDSP_[A-Z0-9_]+)"')
PY_READ = re.compile(r'environ(?:\.get\(|\[)\s*"(ACDSP_[A-Z0-9_]+)"')


def names_read(paths, pattern=READ):
    out = set()
    for path in paths:
        with open(path, errors="replace") as f:
            for m in pattern.finditer(f.read()):
                out.add(next(g for g in m.groups() if g))
    return out


def library_reads(csrc=os.path.join(ROOT, "ac_dsp_amd", "csrc")):
    return names_read(glob.glob(os.path.join(csrc, "*")))


def section6_names():
    """the environment variables of the table in INTEGRATION.md section 6 (build-time -DACDSP_... macros are not environment variables)"""
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    sec = text[text.index("## 6."):text.index("## 7.")]
    rows = [ln for ln in sec.splitlines() if ln.startswith("| ") and not ln.startswith("| variable") and not ln.startswith("|---")]
    assert len(rows) > 30, len(rows)
    out = set()
    for ln in rows:
        first = ln.split("|")[1]
        out.update(re.findall(r"(?<![-\w])(ACDSP_[A-Z0-9_]*[A-Z0-9])", first))
    return out


def test_every_variable_the_library_reads_has_a_leg_or_a_reason():
    src = library_reads()
    assert len(src) > 40 and "ACDSP_NO_MID" in src and "ACDSP_XCD_MAP" in src and "ACDSP_FIR_SPW" in src, sorted(src)
    missing = sorted(n for n in src if n not in LEGS and n not in EXCLUDED)
    assert not missing, "read by ac_dsp_amd/csrc but neither in LEGS nor in EXCLUDED (tests/knob_legs.py): %s" % missing


def test_every_variable_of_section_6_has_a_leg_or_a_reason():
    doc = section6_names()
    assert "ACDSP_NO_GEN" in doc and "ACDSP_MVAVG_ROWW_MAX" in doc and "ACDSP_CASC_ABL_" not in doc and "ACDSP_FIR_NT" not in doc, sorted(doc)
    missing = sorted(n for n in doc if n not in LEGS and n not in EXCLUDED)
    assert not missing, "listed in INTEGRATION.md section 6 but neither in LEGS nor in EXCLUDED: %s" % missing
    undocumented = sorted(n for n in library_reads() if n not in doc)
    assert not undocumented, "read by the library but missing from the table of INTEGRATION.md section 6: %s" % undocumented


def test_no_table_names_a_variable_nothing_reads():
    read = library_reads() | names_read(glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True)) | \
        names_read(glob.glob(os.path.join(ROOT, "ac_dsp_amd", "*.py")), PY_READ)
    stale = sorted(n for n in list(LEGS) + list(EXCLUDED) if n not in read)
    assert not stale, "in tests/knob_legs.py but no longer read by the sources: %s" % stale
    assert not set(LEGS) & set(EXCLUDED)


def test_rows_are_well_formed():
    for name, reason in EXCLUDED.items():
        assert isinstance(reason, str) and reason.strip(), name
    n_rows = n_blind = 0
    for name, rows in LEGS.items():
        assert rows
        for r in rows:
            n_rows += 1
            n_blind += r["under"] is None
            assert name in r["env"] and all(k.startswith("ACDSP_") for k in r["env"])
            assert r["batteries"] and set(r["batteries"]) <= set(DEFAULT_BATTERIES)
            assert (r["under"] is None) == (r["without"] is None)
            if r["under"] is not None:
                assert set(r["under"]) == set(r["without"]) and r["under"] != r["without"]
                assert all(k.split(":")[0] in r["batteries"] for k in r["under"])
    assert n_rows >= 30


def test_a_new_switch_in_the_sources_is_noticed(tmp_path):
    src = tmp_path / "engine_new.hip"
    src.write_text('static const bool foo = getenv("ACDSP_FOO") != nullptr;\nACDSP_TUNE_ENV(bar_env, "ACDSP_BAR_SPW");\n')
    found = library_reads(str(tmp_path))
    assert found == {"ACDSP_FOO", "ACDSP_BAR_SPW"}
    assert [n for n in found if n not in LEGS and n not in EXCLUDED]
