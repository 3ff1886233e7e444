"""The A/B environment switches of libacdsp.so and what the suite does with each of them.

LEGS: one row per switch setting that tests/test_knobs_gpu.py runs in a child process (tests/knob_child.py) against the CPU oracle.
EXCLUDED: every other ACDSP_* variable the sources read or section 6 lists, with the reason why it has no leg.
tests/test_knob_table_cpu.py holds the two tables against the sources and the document: a new switch fails the suite until it has a row here.
No torch, no GPU: plain data.

A row:
  env        what the parent sets for the child (everything else named ACDSP_* is stripped, but ACDSP_LIB / ACDSP_ORACLE_LIB)
  batteries  batteries of tests/knob_child.py to run
  under      expected witness entries ("battery:case.field" -> value) with the switch set
  without    the same entries in the default leg; must differ from `under`, so that the leg proves the switch took effect
             (both None: nothing the ABI or the trace lines report tells the two sides apart -- such rows still run the oracle comparison)
  state      None: state_size of every handle must equal the default leg's (engine_fir.hip: a switch does not change the state geometry);
             else the reason why this switch's state blobs are documented to differ
"""


def leg(env, batteries, under=None, without=None, state=None):
    assert (under is None) == (without is None)
    return dict(env=env, batteries=list(batteries), under=under, without=without, state=state)


# every battery once, no switch set
DEFAULT_BATTERIES = ["fir_mid", "fir_reg33", "fir_epi4", "fir_gq", "fir_nar", "fir_cshift", "fir_u16", "satfree", "fir_rt", "fir_lossy", "fir_unaligned",
                     "fir_gen", "cic_gen", "polydec", "polyintr", "cic_dec", "cic_up", "ddc", "intg", "mvavg", "host", "xcd"]

LEGS = {
    # 319 taps = 11 K-blocks: the register-resident shape issues the 5 central high-byte blocks (2 * 11 + 2 * 5 MFMAs per step), the LDS-resident
    # kernel the set's own band: 5 blocks at unit gain (no difference), 3 at gain 0.3 (2 * 11 + 2 * 3)
    "ACDSP_NO_MID": [leg({"ACDSP_NO_MID": "1"}, ["fir_mid"], {"fir_mid:t319_g03.issued": 28}, {"fir_mid:t319_g03.issued": 32})],
    # 1025 taps = 33 K-blocks: 14 + 14 blocks skipped (2 * 33 + 2 * 5) against the set's own band of 3 at gain 0.3 (2 * 33 + 2 * 3)
    "ACDSP_NO_REG33": [leg({"ACDSP_NO_REG33": "1"}, ["fir_reg33"], {"fir_reg33:t1025_g03.issued": 72}, {"fir_reg33:t1025_g03.issued": 76})],
    "ACDSP_NO_EPI4": [leg({"ACDSP_NO_EPI4": "1"}, ["fir_epi4"], {"fir_epi4:full_scale300.epi": 0}, {"fir_epi4:full_scale300.epi": 4})],
    "ACDSP_NO_GQ": [leg({"ACDSP_NO_GQ": "1"}, ["fir_gq"], {"fir_gq:rnd_zero_sat_zero.epi": 0, "fir_gq:trn_zero_sat_sym.epi": 0},
                        {"fir_gq:rnd_zero_sat_zero.epi": 2, "fir_gq:trn_zero_sat_sym.epi": 2})],
    # 9 K-blocks, empty high plane: 3 + 3 blocks skipped (2 * 9 + 2 * 3 MFMAs per step) against none (4 * 9)
    "ACDSP_NO_NAR_SKIP": [leg({"ACDSP_NO_NAR_SKIP": "1"}, ["fir_nar"], {"fir_nar:w12_empty_hi.issued": 36, "fir_nar:gq_empty_hi.issued": 36},
                              {"fir_nar:w12_empty_hi.issued": 24, "fir_nar:gq_empty_hi.issued": 24})],
    "ACDSP_NO_CSHIFT": [leg({"ACDSP_NO_CSHIFT": "1"}, ["fir_cshift"], {"fir_cshift:w14_keep_all.cshift": 0, "fir_cshift:w8.cshift": 0},
                            {"fir_cshift:w14_keep_all.cshift": 1, "fir_cshift:w8.cshift": 2})],
    "ACDSP_NO_UNSIGNED16": [leg({"ACDSP_NO_UNSIGNED16": "1"}, ["fir_u16"], {"fir_u16:acc44.kernel": "lossless64", "fir_u16:acc34.kernel": "lossless64"},
                                {"fir_u16:acc44.kernel": "mfma_i8", "fir_u16:acc34.kernel": "mfma_i8"})],
    # read in engine_fir.hip, engine_poly.hip, engine_misc.hip (ac_intg_dump) and mv_avg_plan.hip (ac_mv_avg: the call plan)
    "ACDSP_NO_SAT_FREE": [leg({"ACDSP_NO_SAT_FREE": "1"}, ["satfree"],
                              {"satfree:fir.kernel": "satacc16", "satfree:polydec.path": "generic", "satfree:intg.path": "exact_order", "satfree:mvavg.path": "exact_order"},
                              {"satfree:fir.kernel": "mfma_i8", "satfree:polydec.path": "mfma_gen", "satfree:intg.path": "stream", "satfree:mvavg.path": "stream32"})],
    "ACDSP_NO_RT_HYBRID": [leg({"ACDSP_NO_RT_HYBRID": "1"}, ["fir_rt"], {"fir_rt:reload40.kernel": "generic"}, {"fir_rt:reload40.kernel": "mfma_i8"})],
    # class B: <16,2> x <16,2> into <24,8> (16-bit types: both kernels serve it), <28,6> x <23,7> into <60,31,RND,WRAP>; <14,4> x <12,2> into <20,8,RND,SAT>
    "ACDSP_NO_LOSSY_FAST": [leg({"ACDSP_NO_LOSSY_FAST": "1"}, ["fir_lossy"], {"fir_lossy:sat20.kernel": "generic"}, {"fir_lossy:sat20.kernel": "satacc16"})],
    "ACDSP_NO_MFMA_LOSSY": [leg({"ACDSP_NO_MFMA_LOSSY": "1"}, ["fir_lossy"], {"fir_lossy:w16.kernel": "lossy16", "fir_lossy:w28.kernel": "generic"},
                                {"fir_lossy:w16.kernel": "mfma_lossy", "fir_lossy:w28.kernel": "mfma_lossy"})],
    "ACDSP_LOSSY16_FIRST": [leg({"ACDSP_LOSSY16_FIRST": "1"}, ["fir_lossy"], {"fir_lossy:w16.kernel": "lossy16"}, {"fir_lossy:w16.kernel": "mfma_lossy"})],
    # witness-less: the staging copy and the guarded stores are internal to acdsp_fir_run / launch_fir_mfma
    "ACDSP_ALIGNED_ONLY": [leg({"ACDSP_ALIGNED_ONLY": "1"}, ["fir_unaligned"])],
    "ACDSP_NO_GEN": [leg({"ACDSP_NO_GEN": "1"}, ["fir_gen", "cic_gen", "polydec", "polyintr"],
                         {"fir_gen:w36.kernel": "lossless64", "cic_gen:r8n5.path": "recurrence", "polydec:nt8df5.path": "generic", "polyintr:fold_odd15.path": "lossless64"},
                         {"fir_gen:w36.kernel": "mfma_gen", "cic_gen:r8n5.path": "mfma_gen", "polydec:nt8df5.path": "mfma_gen", "polyintr:fold_odd15.path": "mfma_gen"})],
    # witness-less: the recombination form is a kernel argument (GenArgs::pw); ACDSP_GEN_TRACE prints the compiled shape, which does not change
    "ACDSP_GEN_NO_PW": [leg({"ACDSP_GEN_NO_PW": "1"}, ["fir_gen", "cic_gen", "polydec", "cic_dec"])],
    "ACDSP_NO_CIC2": [leg({"ACDSP_NO_CIC2": "1"}, ["cic_dec"], {"cic_dec:r64_c3.path": "recurrence", "cic_dec:r64_c65.path": "recurrence"},
                          {"cic_dec:r64_c3.path": "two_stage", "cic_dec:r64_c65.path": "two_stage"},
                          state="the two-stage kernel keeps its warm-up steps of input history (engine_cic.hip: cic2_hist_len): documented to differ")],
    "ACDSP_CIC2_ALL": [leg({"ACDSP_CIC2_ALL": "1"}, ["cic_dec"], {"cic_dec:r16_c3.path": "two_stage", "cic_dec:r16_c65.path": "two_stage"},
                           {"cic_dec:r16_c3.path": "mfma_gen", "cic_dec:r16_c65.path": "mfma_gen"},
                           state="the other setting of the ACDSP_NO_CIC2 choice: a handle on the two-stage kernel keeps that kernel's longer history")],
    # witness-less: how acdsp_cic_run copies the call's tail into the history buffer
    "ACDSP_NO_HIST_VEC": [leg({"ACDSP_NO_HIST_VEC": "1"}, ["cic_dec"])],
    "ACDSP_NO_CIC_UP": [leg({"ACDSP_NO_CIC_UP": "1"}, ["cic_up"], {"cic_up:r8n5.path": "fir_identity"}, {"cic_up:r8n5.path": "mfma_gen"})],
    "ACDSP_NO_FUSE": [leg({"ACDSP_NO_FUSE": "1"}, ["ddc"], {"ddc:cfg5.path": "two_kernels"}, {"ddc:cfg5.path": "fused"},
                          state="the fused cascade's state is its own input history (kind-4 blob), the two kernels' the two stage blobs (kind 5): engine.hip, ddc_state_hdr")],
    # witness-less: the epilogue form is a template argument of cascade_kernel
    "ACDSP_NO_LIMB": [leg({"ACDSP_NO_LIMB": "1"}, ["ddc"])],
    "ACDSP_NO_INTG_MFMA": [leg({"ACDSP_NO_INTG_MFMA": "1"}, ["intg"], {"intg:chn3.path": "tile"}, {"intg:chn3.path": "mfma"})],
    # witness-less: both kernels report the path "stream"
    "ACDSP_NO_INTG_BATCH": [leg({"ACDSP_NO_INTG_BATCH": "1"}, ["intg"])],
    "ACDSP_NO_INTG_STREAM": [leg({"ACDSP_NO_INTG_STREAM": "1"}, ["intg"], {"intg:chn8.path": "mfma", "intg:chn4.path": "mfma"}, {"intg:chn8.path": "stream", "intg:chn4.path": "stream"})],
    "ACDSP_NO_MVAVG_W32": [leg({"ACDSP_NO_MVAVG_W32": "1"}, ["mvavg"], {"mvavg:w32.path": "int64_sums"}, {"mvavg:w32.path": "stream32"})],
    # (the sliding-window kernel of the 32-bit samples takes 16-bit containers too)
    "ACDSP_NO_MVAVG_STREAM": [leg({"ACDSP_NO_MVAVG_STREAM": "1"}, ["mvavg"], {"mvavg:mirror33.path": "stream32", "mvavg:pack128.path": "stream32"},
                                  {"mvavg:mirror33.path": "stream_mfma", "mvavg:pack128.path": "stream"})],
    # witness-less: epilogue / store / tiling variants of mv_avg_stream_kernel, all reported as "stream"
    "ACDSP_NO_MVAVG_PK16": [leg({"ACDSP_NO_MVAVG_PK16": "1"}, ["mvavg"])],
    "ACDSP_NO_MVAVG_RUN": [leg({"ACDSP_NO_MVAVG_RUN": "1"}, ["mvavg"])],
    "ACDSP_NO_MVAVG_PACK": [leg({"ACDSP_NO_MVAVG_PACK": "1"}, ["mvavg"])],
    # AC_WIN, 9 taps, frames of 1000: the tiles walk the output row ("stream"); without the walk a 9-tap AC_WIN window goes to the matrix cores
    "ACDSP_NO_MVAVG_ROW": [leg({"ACDSP_NO_MVAVG_ROW": "1"}, ["mvavg"], {"mvavg:win9_row.path": "stream_mfma"}, {"mvavg:win9_row.path": "stream"})],
    # witness-less: on which stream the head / tail kernels are queued
    "ACDSP_NO_SIDE_STREAM": [leg({"ACDSP_NO_SIDE_STREAM": "1"}, ["polyintr"])],
    # witness-less: where acdsp_fir_run_host stages the call
    "ACDSP_NO_PINNED": [leg({"ACDSP_NO_PINNED": "1"}, ["host"])],
    # witness-less: the work order of the workgroups
    "ACDSP_XCD_MAP": [leg({"ACDSP_XCD_MAP": "0"}, ["xcd"]), leg({"ACDSP_XCD_MAP": "1"}, ["xcd"])],
}

_TUNING = "numeric tuning variable: its values select launch geometries nobody has run, and the suite does not probe them"
_WRONG = "timing ablation that gives WRONG results by design"

EXCLUDED = {
    "ACDSP_FIR_SPW": _TUNING, "ACDSP_GEN_SPW": _TUNING, "ACDSP_CASC_SPW": _TUNING, "ACDSP_GEN_RING": _TUNING, "ACDSP_GEN_LDS_PAD": _TUNING,
    "ACDSP_CASC_LDS_PAD": _TUNING, "ACDSP_INTG_RPW": _TUNING, "ACDSP_MVAVG_TPW": _TUNING, "ACDSP_CIC2_NST": _TUNING, "ACDSP_CIC2_R1": _TUNING,
    "ACDSP_MVAVG_MFMA_MIN": _TUNING, "ACDSP_MVAVG_ROWW_MAX": _TUNING,
    "ACDSP_TRACE": "diagnostic: stderr lines per handle, no kernel choice (tests/test_cpp_gpu.py reads them)",
    "ACDSP_GEN_TRACE": "diagnostic: one stderr line per launch, no kernel choice",
    "ACDSP_DEBUG_CLOCK": "diagnostic: per-wave clock readings into a scratch buffer of its own, printed to stderr",
    "ACDSP_TUNE_LIVE": "diagnostic: re-reads the tuning variables at every launch; it selects nothing by itself",
    "ACDSP_CIC2_DBG": _WRONG,
    "ACDSP_DIAG_ENV_ORDER": "diagnostic: operand order of the acdsp_diag_fir_envelope_copygeom_ms timing probe, which has no results to compare",
    "ACDSP_LIB": "Python binding only: the path of the library to load; the legs keep it",
    "ACDSP_HOST_SMALL_MACS": "read by include/ac_dsp/acdsp_engine.h, not by the library: tests/test_cpp_gpu.py runs both sides of the threshold",
}


def all_legs():
    """(id, row) of every leg, in table order"""
    out = []
    for name, rows in LEGS.items():
        for r in rows:
            out.append((name if len(rows) == 1 else "%s=%s" % (name, r["env"][name]), r))
    return out
