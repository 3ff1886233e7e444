/* acdsp.h -- C ABI of the MI355X fixed-point streaming-filter engine (libacdsp.so).
 *
 * hlslibs/ac_dsp has no FFI/plugin layer: its boundary is the C++ class-template
 * API (`ac_fir_*_coeffs::run`, `ac_cic_*_full::run`).  The drop-in headers in
 * include/ac_dsp/ keep those templates and call the entry points below, which
 * replace the reference's per-sample core loops:
 *
 *   acdsp_fir_*   <- fir_{const,load,prog}_coeffs_core member functions
 *                    reference include/ac_dsp/ac_fir_const_coeffs.h:153-296,
 *                    ac_fir_load_coeffs.h:145-278, ac_fir_prog_coeffs.h:110-247
 *                    driven by run(): ac_fir_const_coeffs.h:321-355,
 *                    ac_fir_load_coeffs.h:320-365, ac_fir_prog_coeffs.h:277-303
 *   acdsp_cic_*   <- ac_cic_full_core_intg / _diff, ac_cic_full_core.h:80-160,198-255
 *                    driven by run(): ac_cic_dec_full.h:163-222, ac_cic_intr_full.h:150-215
 *
 * Data model: every sample is the raw W-bit two's-complement word of an
 * ac_fixed<W,I,S,Q,O> value (value = raw * 2^-(W-I)), stored sign-/zero-extended
 * in the smallest of int16/int32/int64 that holds W bits (acdsp_elem_bytes).
 * Streams are laid out [channel][time]: sample t of channel c is element
 * c*stride + t.  Channels are independent filter objects (one reference object
 * each); all filter state lives in the handle and carries across run() calls
 * exactly like the reference's object members.
 *
 * There is no CPU fallback: every entry point runs HIP kernels on gfx950 and
 * fails with ACDSP_ENODEVICE / ACDSP_EHIP otherwise.
 */
#ifndef ACDSP_H
#define ACDSP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACDSP_ABI_VERSION 1

/* ac_fixed<W,I,S,Q,O> */
typedef struct { int32_t W, I, S, Q, O; } acdsp_fmt_t;

enum { ACDSP_TRN = 0, ACDSP_RND, ACDSP_TRN_ZERO, ACDSP_RND_ZERO, ACDSP_RND_INF, ACDSP_RND_MIN_INF, ACDSP_RND_CONV, ACDSP_RND_CONV_ODD };
enum { ACDSP_WRAP = 0, ACDSP_SAT, ACDSP_SAT_ZERO, ACDSP_SAT_SYM };
/* FTYPE, reference ac_fir_const_coeffs.h:96.  For the const/load/prog classes the *_ANTI values are rejected:
 * their run() has no branch for them and writes an unassigned value; ac_fir_reg_share gives them a meaning. */
enum { ACDSP_SHIFT_REG = 0, ACDSP_ROTATE_SHIFT, ACDSP_C_BUFF, ACDSP_FOLD_EVEN, ACDSP_FOLD_ODD, ACDSP_TRANSPOSED, ACDSP_FOLD_EVEN_ANTI, ACDSP_FOLD_ODD_ANTI };
enum { ACDSP_FIR_CONST = 0, ACDSP_FIR_LOAD = 1, ACDSP_FIR_PROG = 2,
       /* ac_fir_reg_share (reference ac_fir_reg_share.h:101-310): ftype is one of SHIFT_REG, FOLD_EVEN, FOLD_EVEN_ANTI,
        * FOLD_ODD, FOLD_ODD_ANTI (run() has no branch for the others, :288-306); the MAC loops walk the taps in ascending
        * order (:136-260).  Coefficients are handed over in TAP order: the header resolves the class's coefficient-memory
        * addressing (MEM_WORD_WIDTH / BLK_SZ / BLK_OFFSET) before acdsp_fir_set_coeffs. */
       ACDSP_FIR_REG_SHARE = 3 };

enum {
  ACDSP_OK = 0,
  ACDSP_EINVAL = 1,       /* bad argument / descriptor */
  ACDSP_EUNSUPPORTED = 2, /* valid in the reference but outside this engine's limits */
  ACDSP_EHIP = 3,         /* a HIP call failed */
  ACDSP_ENODEVICE = 4,    /* no gfx950 device */
  ACDSP_ESTATE = 5        /* call sequence error (e.g. run before coefficients are set) */
};

/* flags */
#define ACDSP_FLAG_FORCE_GENERIC 1 /* never pick the MFMA / fast kernels (parity tests) */
/* acdsp_fir_desc_t::flags, acdsp_polydec_desc_t::flags, acdsp_polyintr_desc_t::flags, acdsp_intgdump_desc_t::flags, acdsp_mvavg_desc_t::flags,
 * and acdsp_cic_desc_t::flags of a decimator (interp == 0).  IN_TYPE has W <= 8 (signed or unsigned) and travels in 1-BYTE containers: the
 * caller's input rows, the handle's history and the FIR / CIC / poly_dec / poly_intr state blob hold int8_t / uint8_t raw words
 * (acdsp_fir_in_elem_bytes() / acdsp_cic_in_elem_bytes() / acdsp_polydec_in_elem_bytes() / acdsp_polyintr_in_elem_bytes() /
 * acdsp_intgdump_in_elem_bytes() / acdsp_mvavg_in_elem_bytes() == 1; acdsp_elem_bytes() is not asked for the input).  A flagged ac_poly_dec handle resolves as an unflagged one does: ACDSP_PATH_MFMA_GEN on one
 * sample plane where the ring / window kernels plan the shape, ACDSP_PATH_MFMA_S8 (polydec_s8.hip) on long prototypes, the exact-order kernel
 * elsewhere.  A flagged ac_intg_dump handle keeps no samples: its state blob (the ACC words of temp[]) is that of an unflagged handle and
 * moves both ways; acdsp_intgdump_path below names its kernels.  A flagged ac_mv_avg handle has no state at all; acdsp_mvavg_path below names
 * its kernels (5, the byte-plane streaming kernel, or the container-agnostic 0 / 1).  A flagged ac_poly_intr handle keeps its history and the
 * history part of its state blob (kind 7) in 1-byte containers, so its blobs and those of an unflagged handle refuse each other
 * (ACDSP_EINVAL); acdsp_polyintr_path below names its kernels; its refusals beyond the common ones: more than 2048 taps (the long kernels read
 * int16 rows): ACDSP_EUNSUPPORTED at create.  in_stride stays in elements; the output containers are
 * unchanged unless ACDSP_FLAG_OUT_BYTES is set as well.  W > 8: ACDSP_EINVAL (every family; the only refusal of ac_intg_dump and ac_mv_avg);
 * ACC_TYPE / OUT_TYPE wider than 64 bits, a CIC interpolator (interp == 1: its input stream is the thin one) and either stage descriptor of
 * acdsp_ddc_create[_ex] / acdsp_node_ddc_create[_ex]: ACDSP_EUNSUPPORTED, all before any device use -- the cascade takes byte rows through its
 * own flag, ACDSP_DDC_IN_BYTES below: the FIR stage reads INT_TYPE words whatever the rows hold, so the container is a property of the
 * composite, not of a stage.  INTEGRATION.md "Byte samples". */
#define ACDSP_FLAG_IN_BYTES 2
/* acdsp_fir_desc_t::flags, acdsp_mvavg_desc_t::flags and acdsp_polyintr_desc_t::flags, and only together with ACDSP_FLAG_IN_BYTES.  OUT_TYPE has W <= 8 (signed or
 * unsigned) and travels in 1-BYTE containers: the rows acdsp_fir_run / acdsp_node_fir_run / acdsp_mvavg_run / acdsp_node_mvavg_run write and
 * the output of the run_host calls hold int8_t / uint8_t raw words (acdsp_fir_out_elem_bytes() / acdsp_mvavg_out_elem_bytes() /
 * acdsp_polyintr_out_elem_bytes() == 1; acdsp_polyintr_run / acdsp_node_polyintr_run / acdsp_polyintr_run_host likewise), so a
 * flagged handle's output row feeds a second handle under ACDSP_FLAG_IN_BYTES as it is (mv_avg -> FIR -> CIC decimator without a narrowing
 * pass).  out_stride stays in elements.  FIR rows take 16-byte stores where d_out % 16 == 0 and out_stride % 16 == 0, mv_avg rows 8-byte
 * stores where d_out, out_stride and the outputs per frame are multiples of 8, ac_poly_intr rows 8-byte stores from the matrix-core kernel where
 * d_out, out_stride and the call's first output offset are multiples of 4 bytes (the first call of a folded core starts IF outputs in front
 * of the row: with IF % 4 != 0 that one call runs the exact VALU kernels); element stores elsewhere.  The handle resolves exactly as under
 * ACDSP_FLAG_IN_BYTES alone (path, acdsp_fir_mfma_issued); the FIR state blob holds input history only and moves both ways between handles
 * with and without this flag, and so does the ac_poly_intr blob (input history + ACC words).  Refusals, in this order and all before any device use: the flag without ACDSP_FLAG_IN_BYTES (the int16-sample
 * kernels have no 1-byte output tile) and the flag on any other family's descriptor -- acdsp_{cic,polydec,intgdump}_create, either
 * stage of acdsp_ddc_create: ACDSP_EUNSUPPORTED; then out.W > 8: ACDSP_EINVAL.  INTEGRATION.md "Byte samples". */
#define ACDSP_FLAG_OUT_BYTES 4
/* ddc_flags of acdsp_ddc_create_ex / acdsp_node_ddc_create_ex (NOT a descriptor flag).  The decimator's IN_TYPE has W <= 8 (signed or unsigned)
 * and the cascade's input rows, its input history and the history part of its state blob are 1-BYTE containers: int8_t rows, uint8_t for an
 * unsigned IN_TYPE (acdsp_ddc_in_elem_bytes() == 1).  in_stride stays in elements; the output containers are those of the FIR's OUT_TYPE. */
#define ACDSP_DDC_IN_BYTES 1

/* which kernel family a FIR handle resolved to (acdsp_fir_path) */
enum { ACDSP_PATH_GENERIC = 0, ACDSP_PATH_LOSSLESS64 = 1, ACDSP_PATH_MFMA_I8 = 2, ACDSP_PATH_MFMA_GEN = 3,
       ACDSP_PATH_WIDE = 4 /* a format wider than 64 bits: exact-order kernels on 128-bit words, 256-bit intermediates */,
       ACDSP_PATH_MFMA_LOSSY = 5 /* lossy wrapping accumulator (per-tap AC_TRN / AC_RND): exact sum on the matrix cores minus the dropped bits */,
       ACDSP_PATH_CIC_2STAGE = 6 /* ac_cic_dec_full with R = R1 R2: FIR identity of rate R1 on the matrix cores, integrators / combs of rate R2 behind it, one launch */,
       ACDSP_PATH_MFMA_LONG = 8 /* 1026 .. 16384 taps of the exact-sum class on 16-bit types: the int8 split of ACDSP_PATH_MFMA_I8 with the coefficient
                                  * fragments walked in LDS segments (7 is ACDSP_KCLASS_SATACC16 in the value space of acdsp_fir_kernel_class) */,
       ACDSP_PATH_MFMA_S8 = 9 /* ACDSP_FLAG_IN_BYTES, 1 .. 16384 taps of the exact-sum class: the samples are ONE byte plane, one product per K-block
                                * and one more where the coefficient set has a high byte (fir_s8.hip) */ };
/* finer: the kernel family inside ACDSP_PATH_GENERIC (acdsp_fir_kernel_class; the other values equal the path) */
enum { ACDSP_KCLASS_LOSSY16 = 6 /* fir_lossy_kernel: class B on 16-bit types, int32 VALU */,
       ACDSP_KCLASS_SATACC16 = 7 /* fir_satacc_kernel: saturating accumulator of <= 32 bits on 16-bit types, reference tap order */ };

typedef struct {
  int32_t kind;               /* ACDSP_FIR_*: which reference class this mirrors (informational) */
  int32_t ftype;              /* ACDSP_SHIFT_REG ... */
  int32_t n_taps;             /* 1 .. 2048 for every class; 2049 .. 16384 only for descriptors the long matrix-core kernel takes (one shared
                               * coefficient set, 16-bit samples and coefficients, exact-sum ACC_TYPE of <= 64 bits, no carried reg_trans:
                               * INTEGRATION.md "Long filters"; with ACDSP_FLAG_IN_BYTES the same conditions on 8-bit samples: "Byte samples"),
                               * else acdsp_fir_create fails with ACDSP_EUNSUPPORTED */
  int32_t n_channels;
  int32_t coeffs_per_channel; /* 0: one coefficient set shared by all channels, 1: one set per channel */
  acdsp_fmt_t in, coeff, acc, out;
  int32_t device;             /* HIP device ordinal */
  int32_t flags;
} acdsp_fir_desc_t;

typedef struct {
  int32_t interp;             /* 0: ac_cic_dec_full, 1: ac_cic_intr_full */
  int32_t R, M, N;
  int32_t n_channels;
  acdsp_fmt_t in, out;
  int32_t device;
  int32_t flags;
} acdsp_cic_desc_t;

/* ac_poly_dec<IN, COEFF, STR_COEFF, ACC, OUT, NTAPS, DF> (reference include/ac_dsp/ac_poly_dec.h:82) */
typedef struct {
  int32_t n_taps;             /* NTAPS: taps per polyphase branch; the coefficient struct holds NTAPS*DF words */
  int32_t df;                 /* decimation factor */
  int32_t n_channels;
  acdsp_fmt_t in, coeff, acc, out;
  int32_t device;
  int32_t flags;
} acdsp_polydec_desc_t;

/* ac_poly_intr<IN, COEFF, ACC, OUT, STR_CTRL, STR_COEFF, NTAPS, COEFFSZ, IF, ftype> (reference include/ac_dsp/ac_poly_intr.h:275).
 * ftype is THAT header's enum (ac_poly_intr.h:71), not the FIR FTYPE. */
enum { ACDSP_POLY_FOLD_EVEN = 0, ACDSP_POLY_FOLD_ODD = 1, ACDSP_POLY_FOLD_ANTI = 2 };
typedef struct {
  int32_t n_taps;             /* NTAPS: length of the shift register.  1 .. 2048 for every class; up to 16384 (16383 on the folded cores, whose sums
                               * leave one sample late) only for descriptors the long matrix-core kernels take (signed samples of up to 16 bits,
                               * coefficients of up to 16 bits signed / 15 bits unsigned, exact wrapping ACC_TYPE of <= 64 bits, IF * K-blocks per phase <= 1024: INTEGRATION.md
                               * "Long interpolators"), else acdsp_polyintr_create fails with ACDSP_EUNSUPPORTED */
  int32_t coeff_sz;           /* COEFFSZ: words in the coefficient struct */
  int32_t ifac;               /* IF: interpolation factor = outputs per input sample */
  int32_t ftype;              /* ACDSP_POLY_* */
  int32_t n_channels;
  acdsp_fmt_t in, coeff, acc, out;
  int32_t device;
  int32_t flags;
} acdsp_polyintr_desc_t;

/* ac_intg_dump<IN, ACC, OUT, N_TYPE, NS, CHN> (reference include/ac_dsp/ac_intg_dump.h:113) */
typedef struct {
  int32_t ns;                 /* NS: most rounds a block may accumulate */
  int32_t chn;                /* CHN: channels interleaved in one object's stream */
  int32_t n_objects;          /* independent ac_intg_dump objects (rows of the buffers) */
  acdsp_fmt_t in, acc, out;
  int32_t device;
  int32_t flags;
} acdsp_intgdump_desc_t;

/* ac_mv_avg<MAX_SAMPLE, TAPS, WIN_TYPE, IN, OUT, ACC, COEFF, S_TYPE> (reference include/ac_dsp/ac_mv_avg.h:135) */
enum { ACDSP_WIN_PLAIN = 0 /* AC_WIN */, ACDSP_WIN_MIRROR = 1 /* AC_MIRROR */, ACDSP_WIN_CLIP = 2 /* AC_CLIP */ };
typedef struct {
  int32_t max_sample;         /* MAX_SAMPLE: longest frame the object accepts */
  int32_t taps;               /* TAPS: window length, odd (the reference's MAC loop reads coeffs[TAPS] on even values) */
  int32_t win_mode;           /* ACDSP_WIN_* */
  int32_t n_objects;          /* independent ac_mv_avg objects (rows of the buffers) */
  acdsp_fmt_t in, coeff, acc, out;
  int32_t device;
  int32_t flags;
} acdsp_mvavg_desc_t;

/* Raw-integer stream file / wire format: this 64-byte little-endian header, then n_channels rows of `stride` containers
 * (two's-complement raw words, acdsp_elem_bytes(W) bytes each) -- the [channel][time] layout the kernels take. */
typedef struct {
  char magic[8];              /* "ACDSPRAW" (filled in by acdsp_stream_write) */
  uint32_t version;           /* 1 */
  uint32_t elem_bytes;        /* 2, 4 or 8 = acdsp_elem_bytes(fmt.W) */
  acdsp_fmt_t fmt;            /* the ac_fixed<W,I,S,Q,O> the words are in */
  uint32_t reserved;          /* 0 */
  uint64_t n_channels, n_samples, stride;   /* stride >= n_samples, in elements */
} acdsp_stream_hdr_t;

typedef struct acdsp_fir *acdsp_fir_t;
typedef struct acdsp_polydec *acdsp_polydec_t;
typedef struct acdsp_cic *acdsp_cic_t;
typedef struct acdsp_ddc *acdsp_ddc_t;
typedef struct acdsp_polyintr *acdsp_polyintr_t;
typedef struct acdsp_intgdump *acdsp_intgdump_t;
typedef struct acdsp_mvavg *acdsp_mvavg_t;

/* ---- general ---- */
int32_t acdsp_abi_version(void);
const char *acdsp_last_error(void);            /* message for the last failing call on this thread */
int32_t acdsp_device_count(void);              /* number of gfx950 devices, 0 if none */
int32_t acdsp_elem_bytes(int32_t W);           /* 2, 4 or 8 */

/* device-memory helpers so that pure C/C++ callers need no HIP headers */
int32_t acdsp_dev_alloc(int32_t device, uint64_t bytes, void **d_ptr);
int32_t acdsp_dev_free(int32_t device, void *d_ptr);
/* Allocation with a placement probe: the HBM-bound operators run 3 - 8 % apart on different (input, output) allocation pairs
 * (profiles/r3_placement_modes.txt).  n_candidates blocks of `bytes` are allocated, each is timed with a bare mixed stream against the partner block
 * (partner_reads != 0: the partner is read and the new block written -- an output allocated beside its input; 0: the other way round), the
 * fastest is kept, the others freed.  probe_ms: optional [n_candidates] probe times.  Without a partner (or n_candidates <= 1): plain allocation. */
int32_t acdsp_dev_alloc_paired(int32_t device, uint64_t bytes, const void *d_partner, uint64_t partner_bytes, int32_t partner_reads,
                               int32_t n_candidates, void **d_ptr, float *probe_ms);
/* ... with the caller's own call as the probe (the bare stream ranks pairs like the operator only for thin streams: 16 : 1 and beyond):
 * trial(ctx, d_candidate) enqueues ONE call of the operator on the NULL stream with the candidate as its output (or input) and returns 0.  Every
 * candidate is timed over `reps` calls behind one untimed call, twice round; the fastest is kept, the others freed.  The trial runs the
 * operator for real: point it at a clone of the handle (acdsp_*_clone) when the stream's state must not advance.  trial_ms: optional [n_candidates]. */
int32_t acdsp_dev_alloc_shop(int32_t device, uint64_t bytes, int32_t n_candidates, int32_t (*trial)(void *ctx, void *d_candidate), void *ctx, int32_t reps,
                             void **d_ptr, float *trial_ms);
/* the probe itself: average ms of a bare stream reading [d_src, +src_bytes) and writing [d_dst, +dst_bytes) at their byte ratio */
int32_t acdsp_diag_mix_ms(int32_t device, const void *d_src, uint64_t src_bytes, void *d_dst, uint64_t dst_bytes, int32_t warmup, int32_t reps, void *stream,
                          float *ms_avg);
int32_t acdsp_copy_h2d(int32_t device, void *d_dst, const void *h_src, uint64_t bytes);
int32_t acdsp_copy_d2h(int32_t device, void *h_dst, const void *d_src, uint64_t bytes);
int32_t acdsp_sync(int32_t device, void *stream);

/* Counter-hash stimulus written straight into HBM (bench/test inputs too big to
 * ship over PCIe).  Element (c,t) = top `bits` bits of splitmix64(seed, ((ch0+c)<<32)|(t0+t)),
 * sign-extended, stored in an elem_bytes-wide integer. */
int32_t acdsp_fill_stimulus(int32_t device, void *d_ptr, int32_t elem_bytes, int64_t n_ch, int64_t n, int64_t stride,
                            uint64_t seed, int32_t bits, uint64_t ch0, uint64_t t0, void *stream);

/* ---- diagnostics: the two reference speeds bench.py prints beside a FIR row's roofline ("also report vs a measured
 * device-copy bandwidth"; DESIGN 5.2: the envelope of the int8-split formulation).  Measurement kernels only -- nothing a filter
 * caller needs; they run on the caller's buffers and stream, `warmup` untimed launches then `reps` launches between two events.
 *   copy:      dst[i] = src[i], one 16-byte element per thread, 256-thread workgroups in memory order.  GB/s = 2 * bytes / ms.
 *   envelope:  streams `bytes` from d_x to d_y (d_y receives meaningless words) in 32 KB spans with 8-load / 8-store non-temporal
 *              bursts while issuing `mfma_per_step` v_mfma_i32_32x32x32_i8 per 1024 int16 samples, `mfma_hi_per_step` of them on
 *              high-byte-plane Toeplitz fragments of `coeffs` (n_taps raw 16-bit words) -- no byte-plane split, no LDS, no
 *              epilogue.  Compiled (per_step, hi): (0,0) (26,8) (36,18) (76,10) (132,66); anything else is ACDSP_EUNSUPPORTED. */
int32_t acdsp_diag_copy_ms(int32_t device, const void *d_src, void *d_dst, uint64_t bytes, int32_t warmup, int32_t reps, void *stream,
                           float *ms_avg);
/* shader clock (MHz) measured by a short spin kernel on `stream`, i.e. right behind whatever the stream ran last: the clock state of a bench row */
int32_t acdsp_diag_shader_clock_mhz(int32_t device, void *stream, float *mhz);
int32_t acdsp_diag_fir_envelope_ms(int32_t device, const int64_t *coeffs, int32_t n_taps, int32_t mfma_per_step, int32_t mfma_hi_per_step,
                                   const void *d_x, void *d_y, uint64_t bytes, int32_t warmup, int32_t reps, void *stream, float *ms_avg);

/* the same MFMA counts in the COPY kernel's geometry (256-thread workgroups in memory order, every wave lives for its loads, their MFMAs and
 * stores).  coeffs == NULL: one 16-byte element per thread, A operands are stand-ins made of the loaded bytes (such a wave cannot keep
 * fragments resident); coeffs != NULL: four elements per thread, the real Toeplitz fragments of the set loaded once per wave */
int32_t acdsp_diag_fir_envelope_copygeom_ms(int32_t device, const int64_t *coeffs, int32_t n_taps, int32_t mfma_per_step, int32_t mfma_hi_per_step,
                                            const void *d_x, void *d_y, uint64_t bytes, int32_t warmup, int32_t reps, void *stream, float *ms_avg);

/* ---- FIR ---- */
int32_t acdsp_fir_create(const acdsp_fir_desc_t *desc, acdsp_fir_t *out);
int32_t acdsp_fir_destroy(acdsp_fir_t h);
/* Deep copy, state included (the reference objects are plain aggregates: copying one copies its
 * shift register / reg_trans / coefficients). */
int32_t acdsp_fir_clone(acdsp_fir_t h, acdsp_fir_t *out);
/* Raw coefficient words from host memory: [n_taps] or [n_channels][n_taps].
 * const_coeffs: call once (the reference borrows the pointer for the object's
 * life); load_coeffs: the coefficient-load phase of run(); prog_coeffs: before
 * every run().  Takes effect for samples processed by later run() calls.
 * More than 2048 taps have no fallback kernel: ACDSP_EUNSUPPORTED when a coefficient is >= 32640 (not two signed
 * bytes) or when a saturating ACC_TYPE cannot be proven saturation-free for the set; the handle is then without a set. */
int32_t acdsp_fir_set_coeffs(acdsp_fir_t h, const int64_t *coeffs);
/* Filter n_samples per channel.  d_in / d_out are device pointers to IN / OUT
 * containers, strides in elements.  Asynchronous on `stream` (a hipStream_t, or
 * NULL for the default stream). */
int32_t acdsp_fir_run(acdsp_fir_t h, const void *d_in, int64_t in_stride, int64_t n_samples, void *d_out,
                      int64_t out_stride, void *stream);
/* Same, host buffers, dense [n_channels][n_samples]; synchronous. */
int32_t acdsp_fir_run_host(acdsp_fir_t h, const void *h_in, int64_t n_samples, void *h_out);
int32_t acdsp_fir_reset(acdsp_fir_t h);        /* back to the freshly constructed state (coefficients kept) */
int32_t acdsp_fir_path(acdsp_fir_t h);         /* ACDSP_PATH_* chosen for the current coefficients */
/* int8 matrix-core path only (else -1): epilogue class (0 generic, 1 / 2 the 32-bit classes, 3 wide, 4 64-bit branch-free) | coefficient pre-shift << 8 |
 * sign-flipped unsigned samples << 16 -- diagnostic, recorded by tests/test_pathmap_gpu.py */
int32_t acdsp_fir_mfma_epilogue(acdsp_fir_t h);
int32_t acdsp_fir_kernel_class(acdsp_fir_t h); /* the same, with ACDSP_KCLASS_* inside ACDSP_PATH_GENERIC; -1 before set_coeffs */
/* Duration of the main kernel of the most recent TIMED run(), from HIP events
 * recorded on the launch stream (blocks until that kernel has finished).  Small host-side
 * calls (run_host of at most 64 KB: the drop-in classes' one-channel path) are launch-bound
 * and record no events: after such a call these two report the last timed run (ACDSP_ESTATE
 * when there has been none). */
int32_t acdsp_fir_last_kernel_ms(acdsp_fir_t h, float *ms);
/* Average / minimum main-kernel duration over the last `last_k` (<= 64) run() calls. */
int32_t acdsp_fir_kernel_stats(acdsp_fir_t h, int32_t last_k, float *avg_ms, float *min_ms);
/* 32x32x32 int8 MFMA instructions the selected kernel issues per 1024 samples of one channel (0 when the current
 * coefficients run on none of ACDSP_PATH_MFMA_I8, ACDSP_PATH_MFMA_LONG and ACDSP_PATH_MFMA_S8): the numerator of an MFMA-utilisation figure.
 * All-zero high-byte blocks of the coefficient set are not issued, so this is <= 4 * (ceil((n_taps - 1) / 32) + 1).  ACDSP_PATH_MFMA_S8:
 * nb + (hb1 - hb0 + 1), nb = max(2, ceil((n_taps - 1) / 32) + 1) K-blocks and [hb0, hb1] those that hold a non-zero high coefficient byte. */
int32_t acdsp_fir_mfma_issued(acdsp_fir_t h, int32_t *per_1024_samples);
/* bytes of one INPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES, else acdsp_elem_bytes(in.W) */
int32_t acdsp_fir_in_elem_bytes(acdsp_fir_t h);
/* bytes of one OUTPUT container of the handle: 1 under ACDSP_FLAG_OUT_BYTES, else acdsp_elem_bytes(out.W) */
int32_t acdsp_fir_out_elem_bytes(acdsp_fir_t h);

/* ---- CIC ---- */
int32_t acdsp_cic_create(const acdsp_cic_desc_t *desc, acdsp_cic_t *out);
int32_t acdsp_cic_destroy(acdsp_cic_t h);
int32_t acdsp_cic_clone(acdsp_cic_t h, acdsp_cic_t *out);
int32_t acdsp_cic_int_type(const acdsp_cic_desc_t *desc, acdsp_fmt_t *it); /* the reference's lossless INT_TYPE */
int64_t acdsp_cic_out_count(acdsp_cic_t h, int64_t n_in); /* outputs per channel the next run(n_in) produces */
int32_t acdsp_cic_run(acdsp_cic_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                      int64_t *n_out, void *stream);
int32_t acdsp_cic_run_host(acdsp_cic_t h, const void *h_in, int64_t n_in, void *h_out, int64_t out_cap, int64_t *n_out);
int32_t acdsp_cic_reset(acdsp_cic_t h);
int32_t acdsp_cic_path(acdsp_cic_t h);         /* last run(): 0 recurrence kernel, 3 FIR-identity MFMA kernel (ACDSP_PATH_MFMA_GEN), 6 two-stage kernel (ACDSP_PATH_CIC_2STAGE; decimation
                                                  factors from 32 on that a compiled stage-1 rate divides -- others keep the recurrence kernel), 4 wide.  Under ACDSP_FLAG_IN_BYTES: 6 for every
                                                  rate a byte stage-1 rate (16, 8, 4) divides, rates below 32 included, else 0; never 3 */
/* bytes of one INPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES, else acdsp_elem_bytes(in.W).  A flagged handle's path is 6 or 0,
 * never 3; its state blobs carry elem_bytes = 1 and move between flagged handles of one descriptor only (two-stage or
 * ACDSP_FLAG_FORCE_GENERIC alike, under the history-length rule of acdsp_cic_state_set); blobs of unflagged handles are ACDSP_EINVAL there,
 * and the other way round */
int32_t acdsp_cic_in_elem_bytes(acdsp_cic_t h);
/* Host only, no device: the rates R = R1 * R2 of the two-stage kernel if the handle takes it (ACDSP_PATH_CIC_2STAGE: slot-aligned rows, calls
 * of at least a chunk; the A/B environment switches are not its business), flagged with ACDSP_FLAG_IN_BYTES or not.  R1 = R2 = 0 where no
 * compiled stage-1 rate of the descriptor's input container serves it, for interpolators, types wider than 64 bits and
 * ACDSP_FLAG_FORCE_GENERIC.  Fails as acdsp_cic_create does on a descriptor that is invalid in itself. */
int32_t acdsp_cic_two_stage_rates(const acdsp_cic_desc_t *desc, int32_t *R1, int32_t *R2);
int32_t acdsp_cic_last_kernel_ms(acdsp_cic_t h, float *ms);
int32_t acdsp_cic_kernel_stats(acdsp_cic_t h, int32_t last_k, float *avg_ms, float *min_ms);

/* ---- polyphase decimator (replaces the loop nest of ac_poly_dec::run, ac_poly_dec.h:109-128) ---- */
int32_t acdsp_polydec_create(const acdsp_polydec_desc_t *desc, acdsp_polydec_t *out);
int32_t acdsp_polydec_destroy(acdsp_polydec_t h);
int32_t acdsp_polydec_set_coeffs(acdsp_polydec_t h, const int64_t *coeffs); /* [NTAPS*DF], the STR_COEFF_TYPE array */
/* n_in must be a multiple of DF (run() consumes whole groups: `while (data_in.available(DF))`); n_in/DF outputs */
int32_t acdsp_polydec_run(acdsp_polydec_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out,
                          int64_t out_stride, void *stream);
int32_t acdsp_polydec_run_host(acdsp_polydec_t h, const void *h_in, int64_t n_in, void *h_out);
int32_t acdsp_polydec_reset(acdsp_polydec_t h);
int32_t acdsp_polydec_clone(acdsp_polydec_t h, acdsp_polydec_t *out);   /* deep copy, stream state included: "clone" below */
int32_t acdsp_polydec_path(acdsp_polydec_t h);  /* last run(): ACDSP_PATH_GENERIC, ACDSP_PATH_MFMA_GEN (ring kernel), ACDSP_PATH_MFMA_LONG (long prototypes) or, with ACDSP_FLAG_IN_BYTES on long prototypes, ACDSP_PATH_MFMA_S8 */
/* bytes of one INPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES, else acdsp_elem_bytes(in.W) */
int32_t acdsp_polydec_in_elem_bytes(acdsp_polydec_t h);
/* the ring-shape id (the number ACDSP_GEN_TRACE prints) of the compiled ring row that ran in the last run(), 0 when no ring row ran */
int32_t acdsp_polydec_ring_shape(acdsp_polydec_t h);
/* Long prototypes (NTAPS*DF up to 16384, DF up to 256; exact-sum types of up to 16 bits whose shape the ring kernel cannot plan) run as DF
 * matrix-core FIRs on the phase streams, which a first kernel writes into a scratch buffer owned by the handle.  A call is walked as channel
 * groups x time slabs sized so that the scratch stays within a cap (default 128 MiB; at least 8 channels x 1024 outputs).  set_scratch_cap
 * re-derives the geometry and reallocates (it synchronises the device; graphs captured before it hold the old buffer and must be re-captured);
 * on a handle that is not long it does nothing; if the new buffer cannot be allocated the call fails and cap, geometry and buffer stay as they were.  long_geometry reports outputs per slab, channels per group and the scratch bytes, all zero
 * for a handle that is not long. */
int32_t acdsp_polydec_set_scratch_cap(acdsp_polydec_t h, uint64_t bytes);
int32_t acdsp_polydec_long_geometry(acdsp_polydec_t h, int64_t *slab_outputs, int32_t *group_channels, uint64_t *scratch_bytes);

/* ---- DDC cascade: ac_cic_dec_full -> FIR on the decimator's lossless INT_TYPE words ----
 * Replaces the pair of run() calls `cic.run(in, mid); fir.run(mid, out);` on many channels (the reference couples the
 * two blocks through an ac_channel of INT_TYPE words, cf. ac_cic_dec_full.h:164-177).  cic->out and fir->in must both be
 * the decimator's INT_TYPE (acdsp_cic_int_type).  For the BASELINE config-5 shape class (int16 input, 36-bit words,
 * <= 127 taps, int32 output containers) both stages run in ONE kernel and the INT_TYPE stream never reaches HBM
 * (acdsp_ddc_path = 1); otherwise the two stage kernels run back to back through an internal buffer (path 0).
 * Results are identical to running the two handles separately; state carries across calls like theirs.
 * acdsp_ddc_create_ex takes ddc_flags (acdsp_ddc_create = flags 0).  ACDSP_DDC_IN_BYTES: 8-bit samples in 1-byte rows.  The fused kernel
 * takes them on ONE sample plane for the same decimator class (R 16 N 5 and its neighbours) where the INT_TYPE has 25 .. 32 bits -- <8,1>
 * samples: <28,21>, <8,8,false>: 29 bits -- with <= 127 taps in two coefficient digit planes and int32 output containers; every other byte
 * cascade (other rates, an INT_TYPE below 25 bits, other output containers, ACDSP_NO_FUSE, ACDSP_FLAG_FORCE_GENERIC on a stage, a
 * coefficient set outside the fused plan) runs the two stage kernels, the decimator as under ACDSP_FLAG_IN_BYTES.  Refusals, in this order and
 * before any device use: null arguments; unknown bits in ddc_flags: ACDSP_EINVAL; ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES on a stage
 * descriptor: ACDSP_EUNSUPPORTED (1-byte OUTPUT rows are not part of the cascade); ACDSP_DDC_IN_BYTES with cic->in.W > 8: ACDSP_EINVAL; then
 * everything acdsp_ddc_create checks.  Fused rows obey the 16-byte rule in units of the 1-byte container (ACDSP_EUNSUPPORTED otherwise). */
int32_t acdsp_ddc_create(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, acdsp_ddc_t *out);
int32_t acdsp_ddc_create_ex(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, int32_t ddc_flags, acdsp_ddc_t *out);
/* The cascade with a DECIMATING second stage, `cic.run(in, mid); polydec.run(mid, out, coeffs);`: ac_cic_dec_full -> ac_poly_dec on the INT_TYPE
 * words (cic->out and pd->in must both be the INT_TYPE).  The handle is an acdsp_ddc_t and every call of this section and of the state / clone
 * sections serves it; acdsp_ddc_set_coeffs takes the [NTAPS*DF] array in the order of acdsp_polydec_set_coeffs.  Results are bit-identical to
 * acdsp_cic_run followed by acdsp_polydec_run on whole groups of DF words: the fewer-than-DF words behind the last whole group of a call wait
 * for the next one, as they would in the reference's ac_channel (ac_poly_dec.h:110), so output m of the stream leaves with word m DF + DF - 1
 * and a call with fewer than DF words returns *n_out = 0 with ACDSP_OK.  Refusals, in this order and before any device use: null arguments;
 * unknown ddc_flags bits: ACDSP_EINVAL; a byte flag on either stage descriptor: ACDSP_EUNSUPPORTED; ACDSP_DDC_IN_BYTES with cic->in.W > 8:
 * ACDSP_EINVAL; cic->interp: ACDSP_EINVAL; channel count / device mismatch: ACDSP_EINVAL; cic->out or pd->in not the INT_TYPE: ACDSP_EINVAL;
 * then whatever acdsp_cic_create and acdsp_polydec_create refuse.
 * Fused (acdsp_ddc_path = 1): int16 rows, the config-5 decimator class (R 16 N 5 and its neighbours, INT_TYPE of 33 .. 40 bits), DF = 2,
 * NTAPS*DF <= 128, coefficients in two digit planes, an exact-sum ACC_TYPE, int32 output containers, 16-byte aligned rows.  A step of 256
 * outputs runs DF stage-A sub-steps into a ring of 32 DF slots and one decimating stage B on it; the words never reach HBM.  Everything else
 * (byte rows, other DF, longer prototypes, ACDSP_NO_FUSE, ACDSP_FLAG_FORCE_GENERIC on a stage, a coefficient set outside the plan) runs the
 * two stage kernels through the handle's intermediate rows, the waiting words at their front.  Under graph capture a call whose word count
 * is not a multiple of DF (fused: n_in % (R DF) != 0) is ACDSP_ESTATE: a replay would repeat the captured queue length.
 * Measured on 4096 x 2^20 int16 samples (R 16 N 5, NTAPS 64 x DF 2; profiles/ddc_polydec_shapes.txt): the fused composite takes 0.784 of the time of a
 * Cic + PolyDec pair and 0.957 of the full-rate fused cascade with the same 128 taps; 512 streams: 0.873 and 0.947; two runs of one arm differ by
 * 0.1 - 0.7 %.  DESIGN.md 4.25. */
int32_t acdsp_ddc_create_polydec(const acdsp_cic_desc_t *cic, const acdsp_polydec_desc_t *pd, int32_t ddc_flags, acdsp_ddc_t *out);
int32_t acdsp_ddc_in_elem_bytes(acdsp_ddc_t h);                         /* 1 under ACDSP_DDC_IN_BYTES, else acdsp_elem_bytes(cic->in.W); -1 on a null handle */
int32_t acdsp_ddc_destroy(acdsp_ddc_t h);
int32_t acdsp_ddc_set_coeffs(acdsp_ddc_t h, const int64_t *coeffs);   /* FIR coefficients, raw COEFF_TYPE words [n_taps]; polydec cascade: [NTAPS*DF], as acdsp_polydec_set_coeffs */
int64_t acdsp_ddc_out_count(acdsp_ddc_t h, int64_t n_in);
int32_t acdsp_ddc_run(acdsp_ddc_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                      int64_t *n_out, void *stream);
int32_t acdsp_ddc_reset(acdsp_ddc_t h);
int32_t acdsp_ddc_clone(acdsp_ddc_t h, acdsp_ddc_t *out);               /* deep copy in the same kernel mode, stream state included: "clone" below */
int32_t acdsp_ddc_path(acdsp_ddc_t h);                                  /* 1: fused kernel, 0: two kernels */
int32_t acdsp_ddc_kernel_stats(acdsp_ddc_t h, int32_t last_k, float *avg_ms, float *min_ms);

/* ---- polyphase interpolator (reference ac_poly_intr.h:104-320) ----
 * One input sample -> IF outputs.  The folded cores emit the sums of a sample one sample later (accumulator banks
 * acc_a / acc_b, :153-175), so the stream's very first sample produces nothing.  set_ctrl = the `read_ctrl` call of run()
 * (:291-294): coeffs[COEFFSZ] from the coefficient struct, sign[IF] / corr[IF] from the control struct. */
int32_t acdsp_polyintr_create(const acdsp_polyintr_desc_t *desc, acdsp_polyintr_t *out);
int32_t acdsp_polyintr_destroy(acdsp_polyintr_t h);
int32_t acdsp_polyintr_set_ctrl(acdsp_polyintr_t h, const int64_t *coeffs, const uint8_t *sign, const uint8_t *corr);
int64_t acdsp_polyintr_out_count(acdsp_polyintr_t h, int64_t n_in);
int32_t acdsp_polyintr_run(acdsp_polyintr_t h, const void *d_in, int64_t in_stride, int64_t n_in, void *d_out, int64_t out_stride,
                           int64_t *n_out, void *stream);
int32_t acdsp_polyintr_run_host(acdsp_polyintr_t h, const void *h_in, int64_t n_in, void *h_out, int64_t out_cap, int64_t *n_out);
int32_t acdsp_polyintr_reset(acdsp_polyintr_t h);
int32_t acdsp_polyintr_clone(acdsp_polyintr_t h, acdsp_polyintr_t *out);   /* deep copy, stream state included: "clone" below */
/* kernel family of the last run(): ACDSP_PATH_GENERIC, _LOSSLESS64, _MFMA_GEN or _MFMA_LONG.  Under ACDSP_FLAG_IN_BYTES: _MFMA_GEN (fir_up_s8.hip:
 * the interpolating matrix-core kernel on one sample plane) for the exact-accumulation class as without the flag -- signed IN_TYPE, control
 * words that keep the cores linear and the sums inside ACC_TYPE, IF one of 2 .. 8 or 16, at most two K blocks per phase (NTAPS + lag <= 65 - SPC, SPC = 16, 8, 4, 2 for IF 2, 3 .. 4, 5 .. 8, 16), calls of at least
 * 544 / 576 samples -- into 1-byte (ACDSP_FLAG_OUT_BYTES) or 2-byte rows, with d_in % 16 == 0, in_stride % 16 == 0 and d_out, out_stride and
 * the first output offset on 4 bytes; _LOSSLESS64 / _GENERIC elsewhere: unsigned IN_TYPEs (exact-order kernel, bit-exact), OUT_TYPEs in 4- / 8-byte
 * rows, other alignments, 65 .. 2048 taps per phase; never _MFMA_LONG.  Refusals of acdsp_polyintr_create under the flags, in this order and
 * all before any device use: in.W > 8 under ACDSP_FLAG_IN_BYTES: ACDSP_EINVAL; ACDSP_FLAG_OUT_BYTES without ACDSP_FLAG_IN_BYTES:
 * ACDSP_EUNSUPPORTED; out.W > 8 under both: ACDSP_EINVAL; then NTAPS > 2048 under ACDSP_FLAG_IN_BYTES: ACDSP_EUNSUPPORTED. */
int32_t acdsp_polyintr_path(acdsp_polyintr_t h);
/* bytes of one INPUT / OUTPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, else acdsp_elem_bytes(in.W) /
 * acdsp_elem_bytes(out.W).  The state blob (kind 7) carries the input container width in its header: blobs of handles with and without
 * ACDSP_FLAG_IN_BYTES refuse each other (ACDSP_EINVAL); its saved sums are ACC words, so blobs move both ways between handles with and
 * without ACDSP_FLAG_OUT_BYTES. */
int32_t acdsp_polyintr_in_elem_bytes(acdsp_polyintr_t h);
int32_t acdsp_polyintr_out_elem_bytes(acdsp_polyintr_t h);
/* Long sub-filters (NTAPS + lag >= 65 taps per phase, lag = 1 on the folded cores; up to 16384) of the exact-accumulation class on 16-bit
 * types run as IF matrix-core FIRs on the input stream.  Their phase rows go to a scratch buffer owned by the handle, and a second kernel
 * interleaves them into the caller's rows.  A call is walked as channel groups x time slabs so that the scratch stays under a cap (default
 * 128 MiB).  set_scratch_cap re-derives the geometry and reallocates (it synchronises the device; not for a capturing stream); on a handle
 * that is not long it does nothing; if the new buffer cannot be allocated the call fails and cap, geometry and buffer stay as they were.
 * long_geometry reports input samples per slab, channels per group and the scratch bytes, all zero for a handle that is not long.
 * Above 2048 taps acdsp_polyintr_set_ctrl refuses (ACDSP_EUNSUPPORTED, the handle keeps its state) control words the long kernels cannot
 * take: a phase with sign[j] = 0 on the folded cores, sums that may wrap ACC_TYPE, a folded tap outside -32768 .. 32639. */
int32_t acdsp_polyintr_set_scratch_cap(acdsp_polyintr_t h, uint64_t bytes);
int32_t acdsp_polyintr_long_geometry(acdsp_polyintr_t h, int64_t *slab_inputs, int32_t *group_channels, uint64_t *scratch_bytes);

/* ---- integrate and dump (reference ac_intg_dump.h:93-147) ----
 * Rows = objects; a row is the interleaved stream the reference reads from data_in (round-major, channel-minor).
 * n_sample[n_blocks] (host array, shared by the objects) are the N_TYPE words read at the start of each block: a block
 * with 1 <= n_sample <= NS takes n_sample rounds and yields CHN outputs, any other value takes NS rounds and yields none
 * (its sums carry on, :138-146).  The call must hold whole blocks (the reference would read an empty channel otherwise). */
int32_t acdsp_intgdump_create(const acdsp_intgdump_desc_t *desc, acdsp_intgdump_t *out);
int32_t acdsp_intgdump_destroy(acdsp_intgdump_t h);
int32_t acdsp_intgdump_counts(acdsp_intgdump_t h, const int64_t *n_sample, int64_t n_blocks, int64_t *n_in, int64_t *n_out);
int32_t acdsp_intgdump_run(acdsp_intgdump_t h, const void *d_in, int64_t in_stride, const int64_t *n_sample, int64_t n_blocks,
                           void *d_out, int64_t out_stride, int64_t *n_out, void *stream);
int32_t acdsp_intgdump_run_host(acdsp_intgdump_t h, const void *h_in, const int64_t *n_sample, int64_t n_blocks, void *h_out,
                                int64_t out_cap, int64_t *n_out);
int32_t acdsp_intgdump_reset(acdsp_intgdump_t h);
int32_t acdsp_intgdump_clone(acdsp_intgdump_t h, acdsp_intgdump_t *out);   /* deep copy, temp[] included: "clone" below */
/* kernel family of the last run(): 0 exact order (ragged blocks / carried sums / saturating ACC), 1 LDS-tiled, 2 streaming, 3 matrix cores
 * (selection-matrix product: CHN that does not divide a 16-byte load).  Under ACDSP_FLAG_IN_BYTES: 3 for the shapes of 2 and 3 together --
 * wrapping or sat-free ACC_TYPE, every block dumps the same number of rounds (< 2^23), 1 <= CHN <= 16, blocks of a multiple of 16 samples,
 * 16-byte aligned rows and row pitch, 0 <= acc.F - in.F < 32 -- on one sample plane (there is no byte form of 2); 1 for the other uniform
 * lossless shapes up to CHN 256, and under ACDSP_NO_INTG_MFMA; 0 elsewhere. */
int32_t acdsp_intgdump_path(acdsp_intgdump_t h);
/* bytes of one INPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES, else acdsp_elem_bytes(in.W).  temp[] and its state blob (kind 8,
 * int64 ACC words) do not depend on it: a blob of a flagged handle restores into an unflagged one of the same NS / CHN / object count and
 * the other way round. */
int32_t acdsp_intgdump_in_elem_bytes(acdsp_intgdump_t h);

/* ---- moving average (reference ac_mv_avg.h:93-196) ----
 * One run() = one run() call of every object: n_frames frames of n_sample input samples each, back to back in the row (the
 * reference reads n_sample once per call, :155, and loops `while (data_in.available(1))` over frames).  A frame yields
 * n_sample outputs in the boundary modes and n_sample - TAPS + 1 (or none) under AC_WIN.  The window class behind it,
 * ac_window_1d_flag, is not part of ac_dsp: see include/ac_types/ac_window.h for the semantics assumed.  No state crosses
 * calls (the reference constructs its core object inside run(), :154); coefficients are bound like ac_fir_const_coeffs'. */
int32_t acdsp_mvavg_create(const acdsp_mvavg_desc_t *desc, acdsp_mvavg_t *out);
int32_t acdsp_mvavg_destroy(acdsp_mvavg_t h);
int32_t acdsp_mvavg_clone(acdsp_mvavg_t h, acdsp_mvavg_t *out);           /* descriptor and bound coefficients (there is no stream state): "clone" below */
int32_t acdsp_mvavg_set_coeffs(acdsp_mvavg_t h, const int64_t *coeffs);   /* raw COEFF_TYPE words [TAPS] */
int64_t acdsp_mvavg_out_per_frame(acdsp_mvavg_t h, int64_t n_sample);     /* -1: n_sample outside 1..MAX_SAMPLE */
/* kernel family of the last run(): 0 exact per-tap order, 1 order-free int64 sums, 2 streaming (16-bit samples, int32 sums), 3 sliding window
 * on 32-bit samples (int64 sums), 4 streaming with the window sums on the matrix cores (16-bit samples, 17 taps and more), 5 byte-plane
 * streaming kernel (mv_avg_s8.hip).  A handle without ACDSP_FLAG_IN_BYTES never reports 5; a flagged one reports 5, 1 or 0 only: 5 for 1 .. 65
 * taps of the linear class (exact cast of a sample to a wrapping or sat-free AC_TRN / AC_RND ACC_TYPE with acc.F - in.F >= coeff.F >= 0,
 * coefficients <= 32639 with sum |c| <= 32767, AC_TRN / AC_RND into AC_WRAP / AC_SAT outputs) on frames of n_sample >= TAPS, n_sample % 16 ==
 * 0, with d_in % 16 == 0 and in_stride % 16 == 0; elsewhere -- the per-tap class acc.F - in.F < coeff.F, longer windows, accumulators that
 * can saturate, other frame lengths and alignments, ACDSP_FLAG_FORCE_GENERIC -- the container-agnostic kernels 1 / 0 (exact, and slow). */
int32_t acdsp_mvavg_path(acdsp_mvavg_t h);
/* bytes of one INPUT / OUTPUT container of the handle: 1 under ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, else acdsp_elem_bytes(in.W) /
 * acdsp_elem_bytes(out.W) */
int32_t acdsp_mvavg_in_elem_bytes(acdsp_mvavg_t h);
int32_t acdsp_mvavg_out_elem_bytes(acdsp_mvavg_t h);
/* Host only -- no device, no handle: the matrix-core fragments acdsp_mvavg_set_coeffs builds for a coefficient set, for tests of the digit
 * split and the Toeplitz indexing.  out[ACDSP_MVAVG_FRAG_WORDS] is laid out [row order m (2)][K block b (nb)][digit plane (2)][lane (64)][4
 * dwords]: lane (i = lane & 15, kg = lane >> 4) holds A[i][16 kg .. 16 kg + 15] of K block b, A[i][kk] = digit(c[64 b + kk - s - off]) with
 * s = 8 (i >> 2) + (i & 3) + 4 m, off = hb - TAPS / 2, hb = TAPS / 2 rounded up to 8 (in_bytes != 0: to 16; 0 under ACDSP_WIN_PLAIN).
 * Returns nb (1 / 2; 0: the set or the window does not fit; -1: bad arguments); *csum = sum of the coefficients, *hi_any = a high digit exists. */
#define ACDSP_MVAVG_FRAG_WORDS 2048
int32_t acdsp_mvavg_frags_host(const int64_t *coeffs, int32_t taps, int32_t win_mode, int32_t in_bytes, uint32_t *out, int64_t *csum, int32_t *hi_any);
int32_t acdsp_mvavg_run(acdsp_mvavg_t h, const void *d_in, int64_t in_stride, int64_t n_sample, int64_t n_frames, void *d_out,
                        int64_t out_stride, int64_t *n_out, void *stream);
int32_t acdsp_mvavg_run_host(acdsp_mvavg_t h, const void *h_in, int64_t n_sample, int64_t n_frames, void *h_out, int64_t out_cap,
                             int64_t *n_out);

/* ---- state save / restore (checkpoint / resume, moving a stream to another GPU) ----
 * The reference's filter state is plain object members (shift register / reg_trans: ac_fir_const_coeffs.h:124-127;
 * integrator / comb registers and rate counters: ac_cic_full_core.h:71-74,219) that a caller can copy with the object.
 * Here it is a versioned little-endian blob: a 64-byte header (magic "ACDSPST1", kind, channel count, word size, words per
 * channel, the CIC input count, the filter parameters) followed by the raw state words [channel][word]:
 *   FIR   -- the last `per_channel` input samples of every channel, oldest first (word per_channel-1-k is reg[k] of the
 *            reference's shift register); TRANSPOSED load/prog filters: reg_trans[0..N_TAPS-1] as int64 ACC raw words;
 *   CIC   -- the last `per_channel` input samples (both directions are FIR systems of the input)
 *            plus the number of inputs consumed so far (= rate_cnt phase).
 *   ac_poly_dec  (kind 6; p0 = NTAPS, p1 = DF) -- the last `per_channel` input samples of every channel, oldest first, in IN containers
 *            (taps[NTAPS*DF], ac_poly_dec.h:132; acc and acc1[] are rebuilt by every group).  A call consumes whole groups of DF: no phase.
 *   ac_poly_intr (kind 7; p0 .. p3 = NTAPS, IF, ftype, COEFFSZ) -- the input history as above (taps[NTAPS], ac_poly_intr.h:106), the number of
 *            inputs consumed so far in t_total (the folded cores emit nothing for a stream's first sample), and behind the histories
 *            [channel][IF] int64 ACC raw words: the sub-filter sums of the last sample, i.e. the bank of acc_a / acc_b (:107-108) the next
 *            sample emits.  They were formed with the control words of their own time, so they are carried, not recomputed; FOLD_ANTI emits
 *            at once and carries zeros.
 *   ac_intg_dump (kind 8; p0 = NS, p1 = CHN; elem_bytes 8, per_channel = CHN, n_channels = objects) -- temp[] of every object,
 *            [object][CHN] int64 ACC raw words (ac_intg_dump.h:96-103); bit 0 of the header's last quadword is set when the stream stands
 *            behind a block that did not dump (sums are pending in temp[]).  state_set refuses words outside ACC_TYPE, treats any non-zero
 *            sum as pending, and the next run() rebuilds its block table instead of reusing the cached one.
 *   ac_mv_avg keeps nothing between calls (ac_mv_avg.h:154) and has no blob.
 * state_get waits for the handle's pending run() calls.  state_set accepts only a blob from a handle of the same class,
 * parameters and channel count (ACDSP_EINVAL otherwise, the handle is left as it was); coefficients and control words are not part of
 * the state.  A blob restores into any handle of the same descriptor whatever kernel path that handle takes (ACDSP_FLAG_FORCE_GENERIC set or
 * clear, ring or long kernel, another set_scratch_cap): the payload is the reference's state, not a kernel's.  An input-history blob of
 * another history LENGTH is taken when it covers the filter memory (n_taps - 1 samples; NTAPS*DF - 1; NTAPS): the newest samples are kept,
 * older ones zero.
 * clone (acdsp_*_clone) creates a new handle on the same device with the same descriptor, the same coefficients / control words when set,
 * the same scratch cap on long handles and the same stream state; scratch, side stream, staging buffers, block tables and timers are its
 * own, and afterwards neither handle is affected by what the other does.
 * state_get, state_set and clone are synchronising host calls (they drain the device): not for a stream that is capturing a graph. */
int64_t acdsp_fir_state_size(acdsp_fir_t h);                                   /* bytes state_get writes; -1 on a null handle */
int32_t acdsp_fir_state_get(acdsp_fir_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_fir_state_set(acdsp_fir_t h, const void *h_buf, uint64_t bytes);
int64_t acdsp_cic_state_size(acdsp_cic_t h);
int32_t acdsp_cic_state_get(acdsp_cic_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_cic_state_set(acdsp_cic_t h, const void *h_buf, uint64_t bytes);
/* cascade (acdsp_ddc_*): the input history and input count of the fused kernel (its FIR window is recomputed from them), or
 * the two stage blobs behind one header when the handle runs the stages as two kernels.  Under ACDSP_DDC_IN_BYTES the history words are
 * 1-byte containers: such a blob moves between byte cascades of the same descriptors and is refused by every other handle (and theirs by it).
 * Polydec cascade (acdsp_ddc_create_polydec): the same in fused mode -- the waiting words are recomputed from history and count --, and the two
 * stage blobs plus the waiting INT_TYPE words in two-kernel mode; the header carries NTAPS and DF, and a FIR cascade and a polydec cascade refuse
 * each other's blobs (ACDSP_EINVAL).  A refused blob leaves a polydec cascade as it was, also when the outer header fits and a stage blob inside it
 * is refused: the handle's own state is put back. */
int64_t acdsp_ddc_state_size(acdsp_ddc_t h);
int32_t acdsp_ddc_state_get(acdsp_ddc_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_ddc_state_set(acdsp_ddc_t h, const void *h_buf, uint64_t bytes);
int64_t acdsp_polydec_state_size(acdsp_polydec_t h);
int32_t acdsp_polydec_state_get(acdsp_polydec_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_polydec_state_set(acdsp_polydec_t h, const void *h_buf, uint64_t bytes);
int64_t acdsp_polyintr_state_size(acdsp_polyintr_t h);
int32_t acdsp_polyintr_state_get(acdsp_polyintr_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_polyintr_state_set(acdsp_polyintr_t h, const void *h_buf, uint64_t bytes);
int64_t acdsp_intgdump_state_size(acdsp_intgdump_t h);
int32_t acdsp_intgdump_state_get(acdsp_intgdump_t h, void *h_buf, uint64_t cap_bytes);
int32_t acdsp_intgdump_state_set(acdsp_intgdump_t h, const void *h_buf, uint64_t bytes);

/* ---- node level: one filter bank sharded over the GPUs of a node ----
 * Channels are independent filter objects (reference ac_fir_const_coeffs.h:124-127, ac_cic_full_core.h:71-74,219), so a bank of
 * desc->n_channels filters is cut into n_devices CONTIGUOUS channel slices (acdsp_node_shard: the first n_channels % n_devices
 * slices hold one channel more), one per entry of `devices` (NULL: devices 0 .. n_devices-1; a device may be listed more than once:
 * its shards are then concurrent streams of that GPU).  Per shard the node handle owns an ordinary engine handle (`desc` with that
 * slice's channel count and device), a non-blocking stream and a host thread bound to the device.  Coefficients are replicated
 * (or, with coeffs_per_channel, sliced); there is NO collective and no cross-device traffic.
 * run():      d_in[s] / d_out[s] = device pointers ON shard s's device to its [ch_hi - ch_lo][stride] block; every shard's thread
 *             launches its slice on its stream and waits for it; the call returns when all have.  Aggregate rate of a call =
 *             n_channels * n / acdsp_node_last_ms's maximum (per-shard times: the engine handles' own HIP events).
 *             PRECONDITION: the shard streams are non-blocking and order with no other stream -- every d_in block must be complete
 *             and every d_out block unused by pending work of other streams when run() is called (synchronise the producer first).
 * run_host(): dense host block [n_channels][n]: every thread moves and filters its rows (acdsp_fir_run_host of the slice).
 * The shard handles (acdsp_node_shard_info) take every per-handle call of this header: state get / set, reset, path, kernel_stats. */
typedef struct acdsp_node *acdsp_node_t;
int32_t acdsp_node_shard(int64_t n_total, int32_t n_shards, int32_t shard, int64_t *lo, int64_t *hi);
int32_t acdsp_node_n_shards(acdsp_node_t h);   /* -1 on a null handle */
int32_t acdsp_node_shard_info(acdsp_node_t h, int32_t shard, int32_t *device, int64_t *ch_lo, int64_t *ch_hi, void **handle, void **stream);
int32_t acdsp_node_last_ms(acdsp_node_t h, float *per_shard_ms /* [n_shards] or NULL */, float *max_ms);
int32_t acdsp_node_destroy(acdsp_node_t h);
int32_t acdsp_node_fir_create(const acdsp_fir_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_fir_set_coeffs(acdsp_node_t h, const int64_t *coeffs);   /* [n_taps], or [n_channels][n_taps] with coeffs_per_channel */
int32_t acdsp_node_fir_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_samples, void *const *d_out, int64_t out_stride);
int32_t acdsp_node_fir_run_host(acdsp_node_t h, const void *h_in, int64_t n_samples, void *h_out);
int32_t acdsp_node_cic_create(const acdsp_cic_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int64_t acdsp_node_cic_out_count(acdsp_node_t h, int64_t n_in);
int32_t acdsp_node_cic_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_in, void *const *d_out, int64_t out_stride,
                           int64_t *n_out);
int32_t acdsp_node_ddc_create(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, int32_t n_devices, const int32_t *devices,
                              acdsp_node_t *out);
/* ... with the ddc_flags of acdsp_ddc_create_ex (acdsp_node_ddc_create = flags 0): every shard is created from these descriptors and flags */
int32_t acdsp_node_ddc_create_ex(const acdsp_cic_desc_t *cic, const acdsp_fir_desc_t *fir, int32_t ddc_flags, int32_t n_devices,
                                 const int32_t *devices, acdsp_node_t *out);
/* ... and the polydec cascade of acdsp_ddc_create_polydec: the other acdsp_node_ddc_* calls serve the handle */
int32_t acdsp_node_ddc_create_polydec(const acdsp_cic_desc_t *cic, const acdsp_polydec_desc_t *pd, int32_t ddc_flags, int32_t n_devices,
                                      const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_ddc_set_coeffs(acdsp_node_t h, const int64_t *coeffs);
int64_t acdsp_node_ddc_out_count(acdsp_node_t h, int64_t n_in);
int32_t acdsp_node_ddc_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_in, void *const *d_out, int64_t out_stride,
                           int64_t *n_out);
/* the f-row classes: rows = channels (poly_dec, poly_intr) or objects (intg_dump, mv_avg), sliced the same way; coefficients /
 * control words / block counts are replicated.  acdsp_node_last_ms: the shard's whole call between two events of its stream. */
int32_t acdsp_node_polydec_create(const acdsp_polydec_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_polydec_set_coeffs(acdsp_node_t h, const int64_t *coeffs);
int32_t acdsp_node_polydec_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_in, void *const *d_out, int64_t out_stride);
int32_t acdsp_node_polyintr_create(const acdsp_polyintr_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_polyintr_set_ctrl(acdsp_node_t h, const int64_t *coeffs, const uint8_t *sign, const uint8_t *corr);
int64_t acdsp_node_polyintr_out_count(acdsp_node_t h, int64_t n_in);
int32_t acdsp_node_polyintr_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_in, void *const *d_out, int64_t out_stride,
                                int64_t *n_out);
int32_t acdsp_node_intgdump_create(const acdsp_intgdump_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_intgdump_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, const int64_t *n_sample, int64_t n_blocks,
                                void *const *d_out, int64_t out_stride, int64_t *n_out);
int32_t acdsp_node_mvavg_create(const acdsp_mvavg_desc_t *desc, int32_t n_devices, const int32_t *devices, acdsp_node_t *out);
int32_t acdsp_node_mvavg_set_coeffs(acdsp_node_t h, const int64_t *coeffs);
int32_t acdsp_node_mvavg_run(acdsp_node_t h, const void *const *d_in, int64_t in_stride, int64_t n_sample, int64_t n_frames, void *const *d_out,
                             int64_t out_stride, int64_t *n_out);

/* ---- raw-integer stream files (host side; no device needed) ---- */
int32_t acdsp_stream_write(const char *path, const acdsp_stream_hdr_t *hdr, const void *data);
int32_t acdsp_stream_read_header(const char *path, acdsp_stream_hdr_t *hdr);
int32_t acdsp_stream_read(const char *path, void *data, uint64_t cap_bytes);

#ifdef __cplusplus
}
#endif
#endif
