"""Thin object wrappers over the C ABI for tests and bench.py (torch tensors as device buffers)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, Fmt, FirDesc, CicDesc, PolyDecDesc, PolyIntrDesc, IntgDumpDesc, MvAvgDesc, StreamHdr, FTYPES, KINDS, PATHS, KCLASSES


def device_count():
    return lib.acdsp_device_count()


def torch_dtype_for(fmt):
    """Container dtype of a format; formats wider than 64 bits use 16-byte containers = int64 pairs (low quadword first)."""
    return {2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.int64}[lib.acdsp_elem_bytes(fmt.W)]


def _np_dtype_for(fmt):
    return {2: np.int16, 4: np.int32, 8: np.int64, 16: np.int64}[lib.acdsp_elem_bytes(fmt.W)]


def _np_in_dtype(fmt, in_bytes):
    """numpy dtype of FIR / CIC input rows: 1-byte containers under in_bytes (ACDSP_FLAG_IN_BYTES)"""
    if in_bytes:
        return np.int8 if fmt.S else np.uint8
    return _np_dtype_for(fmt)


def is_wide(fmt):
    return lib.acdsp_elem_bytes(fmt.W) == 16


def _byte_dtype(fmt, as_bytes):
    """torch dtype of a row of `fmt` words: int8 / uint8 by signedness in 1-byte containers, else the format's own container"""
    if as_bytes:
        return torch.int8 if fmt.S else torch.uint8
    return torch_dtype_for(fmt)


def _flags(force_generic=False, in_bytes=False, out_bytes=False):
    """flag word of a descriptor"""
    return (_lib.FLAG_FORCE_GENERIC if force_generic else 0) | (_lib.FLAG_IN_BYTES if in_bytes else 0) | (_lib.FLAG_OUT_BYTES if out_bytes else 0)


def _alloc_out(fmt, n_ch, n, device, as_bytes=False):
    """[n_ch][n] OUT containers; 16-byte containers are a trailing dimension of two int64 (low, high); as_bytes: 1-byte containers."""
    shape = (n_ch, n, 2) if is_wide(fmt) and not as_bytes else (n_ch, n)
    return torch.empty(shape, dtype=_byte_dtype(fmt, as_bytes), device=device)


def _alloc_out_host(fmt, n_ch, n, out_bytes=False):
    """Host twin of _alloc_out: the C side writes n containers of acdsp_elem_bytes(W) bytes per row, 16 for formats wider than 64 bits;
    1-byte containers under out_bytes (ACDSP_FLAG_OUT_BYTES)."""
    if out_bytes:
        return np.empty((n_ch, n), dtype=np.int8 if fmt.S else np.uint8)
    shape = (n_ch, n, 2) if is_wide(fmt) else (n_ch, n)
    return np.empty(shape, dtype=_np_dtype_for(fmt))


def _row_stride(t, fmt):
    """Row stride in containers; checks the inner layout."""
    if is_wide(fmt):
        assert t.dim() == 3 and t.shape[2] == 2 and t.stride(2) == 1 and t.stride(1) == 2 and t.stride(0) % 2 == 0
        return t.stride(0) // 2
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


def wide_to_int(a):
    """[..., 2] int64 (low, high) containers -> object array of Python ints (two's complement, 128 bits)."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    lo = a[..., 0].astype(np.uint64).astype(object)
    hi = a[..., 1].astype(object)
    return hi * (1 << 64) + lo


def _stream_ptr(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dev_index(dev):
    d = torch.device(dev)
    return d.index if d.index is not None else torch.cuda.current_device()


def fill_stimulus(out, seed, bits, ch0=0, t0=0):
    """Fill a [n_ch][n] device tensor with the counter-hash stimulus (bit-identical to oracle.stimulus)."""
    assert out.is_cuda and out.dim() == 2 and out.stride(1) == 1
    check(lib.acdsp_fill_stimulus(_dev_index(out.device), C.c_void_p(out.data_ptr()), out.element_size(), out.shape[0],
                                  out.shape[1], out.stride(0), seed, bits, ch0, t0, _stream_ptr(out)))
    return out


def diag_copy_ms(src, dst, warmup=3, reps=10):
    """Average ms of the plain 16-byte-per-thread device copy src -> dst (acdsp_diag_copy_ms): bench.py's roofline.copy_GBps."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()
    nbytes = min(src.numel() * src.element_size(), dst.numel() * dst.element_size()) // 16 * 16
    ms = C.c_float()
    check(lib.acdsp_diag_copy_ms(_dev_index(src.device), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), nbytes, warmup, reps,
                                 _stream_ptr(src), C.byref(ms)))
    return ms.value, nbytes


def diag_shader_clock_mhz(device=0):
    """Shader clock in MHz right behind the work torch's current stream of `device` ran last (acdsp_diag_shader_clock_mhz)."""
    mhz = C.c_float()
    check(lib.acdsp_diag_shader_clock_mhz(device, C.c_void_p(torch.cuda.current_stream(device).cuda_stream), C.byref(mhz)))
    return mhz.value


def diag_mix_ms(src, dst, warmup=2, reps=5):
    """Average ms of the bare mixed stream src (read) -> dst (written) at the byte ratio of the two blocks (acdsp_diag_mix_ms): the placement probe."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()
    ms = C.c_float()
    check(lib.acdsp_diag_mix_ms(_dev_index(src.device), C.c_void_p(src.data_ptr()), src.numel() * src.element_size() // 1024 * 1024,
                                C.c_void_p(dst.data_ptr()), dst.numel() * dst.element_size() // 1024 * 1024, warmup, reps, _stream_ptr(src), C.byref(ms)))
    return ms.value


def empty_paired(shape, dtype, partner, candidates=4, partner_reads=True, cap_bytes=1 << 50):
    """torch.empty(shape, dtype) on the partner's device with a placement probe (the torch-side twin of acdsp_dev_alloc_paired): `candidates` blocks are
    allocated, each timed with diag_mix_ms against `partner` (read when partner_reads, else written), the fastest kept.  Returns (tensor, probe ms list)."""
    import torch
    cands = [torch.empty(shape, dtype=dtype, device=partner.device) for _ in range(max(1, candidates))]
    if len(cands) == 1 or not partner.is_contiguous() or cands[0].numel() * cands[0].element_size() < (1 << 20):
        return cands[0], [0.0]
    pf, big = partner.view(-1), max(partner.numel() * partner.element_size(), cands[0].numel() * cands[0].element_size())
    f = min(1.0, cap_bytes / big)
    pn = int(pf.numel() * f)
    best, times = None, []
    for pas in range(2):
        for i, c in enumerate(cands):
            cf = c.view(-1)
            cn = int(cf.numel() * f)
            t = diag_mix_ms(pf[:pn], cf[:cn]) if partner_reads else diag_mix_ms(cf[:cn], pf[:pn])
            if pas == 0:
                times.append(t)
            else:
                times[i] = min(times[i], t)
    best = min(range(len(cands)), key=lambda i: times[i])
    keep = cands[best]
    del cands
    return keep, times


def shop_output(trial, shape, dtype, device, candidates=4, reps=3):
    """torch.empty(shape, dtype) chosen among `candidates` separately allocated blocks by timing the caller's own call -- trial(y) runs the operator
    with y as its output -- `reps` times behind one untimed call, twice round (the torch-side twin of acdsp_dev_alloc_shop).  The HBM-bound operators
    run up to 12 % apart on different (input, output) allocation pairs (profiles/r6_placement.txt).  Returns (tensor, ms per candidate)."""
    import torch
    cands = [torch.empty(shape, dtype=dtype, device=device) for _ in range(max(1, candidates))]
    if len(cands) == 1:
        return cands[0], [0.0]
    times = [0.0] * len(cands)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for pas in range(2):
        for i, y in enumerate(cands):
            trial(y)
            e0.record()
            for _ in range(reps):
                trial(y)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / reps
            times[i] = t if pas == 0 else min(times[i], t)
    best = min(range(len(cands)), key=lambda i: times[i])
    keep = cands[best]
    del cands
    return keep, times


def diag_fir_envelope_ms(coeffs, mfma_per_step, mfma_hi_per_step, x, y, warmup=3, reps=10):
    """Average ms of the stream + issued-MFMA envelope of a FIR row over x -> y (acdsp_diag_fir_envelope_ms): roofline.envelope_ms."""
    assert x.is_cuda and y.is_cuda and x.is_contiguous() and y.is_contiguous()
    nbytes = min(x.numel() * x.element_size(), y.numel() * y.element_size()) // 16 * 16
    c = np.ascontiguousarray(coeffs if coeffs is not None else [0], dtype=np.int64)
    ms = C.c_float()
    check(lib.acdsp_diag_fir_envelope_ms(_dev_index(x.device), c.ctypes.data_as(C.POINTER(C.c_int64)), len(c), mfma_per_step, mfma_hi_per_step,
                                         C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), nbytes, warmup, reps, _stream_ptr(x), C.byref(ms)))
    return ms.value, nbytes


def diag_fir_envelope_copygeom_ms(coeffs, mfma_per_step, mfma_hi_per_step, x, y, warmup=3, reps=10):
    """The same MFMA counts in the plain copy's launch geometry (acdsp_diag_fir_envelope_copygeom_ms): roofline.envelope_copy_geometry_ms.
    coeffs None: one element per thread, stand-in A operands; else four elements per thread and the set's real Toeplitz fragments."""
    assert x.is_cuda and y.is_cuda and x.is_contiguous() and y.is_contiguous()
    nbytes = min(x.numel() * x.element_size(), y.numel() * y.element_size()) // 16 * 16
    ms = C.c_float()
    c = None if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.int64)
    check(lib.acdsp_diag_fir_envelope_copygeom_ms(_dev_index(x.device), None if c is None else c.ctypes.data_as(C.POINTER(C.c_int64)), 0 if c is None else len(c),
                                                  mfma_per_step, mfma_hi_per_step, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                                  nbytes, warmup, reps, _stream_ptr(x), C.byref(ms)))
    return ms.value, nbytes


class _Rows:
    """Row containers of an engine or node object: self.fin / self.fout, in 1-byte containers under self.in_bytes / self.out_bytes."""
    in_bytes = out_bytes = False
    in_dtype = property(lambda self: _byte_dtype(self.fin, self.in_bytes), doc="torch dtype of the input rows: int8 / uint8 containers under in_bytes, else the container of IN_TYPE")
    out_dtype = property(lambda self: _byte_dtype(self.fout, self.out_bytes), doc="torch dtype of the output rows: int8 / uint8 containers under out_bytes, else the container of OUT_TYPE")


class _Handle(_Rows):
    """Owner of one engine handle self._h of the family acdsp_<_c>_*."""
    _c = None   # the family's C prefix

    def _fn(self, name):
        return getattr(lib, "acdsp_%s_%s" % (self._c, name))

    def clone(self):
        """Deep copy -- descriptor, coefficients and stream state; the two objects are independent afterwards (acdsp_*_clone)."""
        h = C.c_void_p()
        check(self._fn("clone")(self._h, C.byref(h)))
        twin = object.__new__(type(self))
        twin.__dict__.update(self.__dict__)
        twin._h = h
        return twin

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()


class _Stateful(_Handle):
    """... whose stream state can be saved, restored and cleared (acdsp_*_state_size / _state_get / _state_set / _reset)."""

    def state(self):
        """Versioned state blob (bytes): the family's stream state of every channel (include/acdsp.h lists what each kind holds)."""
        buf = (C.c_char * self._fn("state_size")(self._h))()
        check(self._fn("state_get")(self._h, buf, len(buf)))
        return bytes(buf)

    def set_state(self, blob):
        check(self._fn("state_set")(self._h, C.c_char_p(blob), len(blob)))

    def reset(self):
        check(self._fn("reset")(self._h))


class Fir(_Stateful):
    """n_channels independent reference FIR objects (ac_fir_{const,load,prog}_coeffs) behind one handle."""
    _c = "fir"

    def __init__(self, n_taps, ftype, fin, fcoeff, facc, fout, n_channels=1, kind="load", coeffs_per_channel=False,
                 device=0, force_generic=False, in_bytes=False, out_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8
        out_bytes (with in_bytes): OUT_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_OUT_BYTES): output rows are torch.int8 / torch.uint8"""
        self.fin, self.fcoeff, self.facc, self.fout = fin, fcoeff, facc, fout
        self.n_taps, self.n_channels, self.device = n_taps, n_channels, device
        self.coeffs_per_channel = bool(coeffs_per_channel)
        self.in_bytes = bool(in_bytes)
        self.out_bytes = bool(out_bytes)
        d = FirDesc(KINDS[kind] if isinstance(kind, str) else kind, FTYPES[ftype] if isinstance(ftype, str) else ftype,
                    n_taps, n_channels, int(self.coeffs_per_channel), fin, fcoeff, facc, fout, device,
                    _flags(force_generic, in_bytes, out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_fir_create(C.byref(d), C.byref(self._h)))

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        want = (self.n_channels, self.n_taps) if self.coeffs_per_channel else (self.n_taps,)
        assert c.shape == want, (c.shape, want)
        check(lib.acdsp_fir_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    @property
    def path(self):
        return PATHS[lib.acdsp_fir_path(self._h)]

    @property
    def kernel(self):
        """path, with the VALU fast kernels inside "generic" told apart ("lossy16", "satacc16"): acdsp_fir_kernel_class"""
        return KCLASSES[lib.acdsp_fir_kernel_class(self._h)]

    def mfma_epilogue(self):
        """(epilogue class, coefficient pre-shift, samples sign-flipped) on the int8 matrix-core path, else None (acdsp_fir_mfma_epilogue)"""
        v = lib.acdsp_fir_mfma_epilogue(self._h)
        return None if v < 0 else (v & 255, (v >> 8) & 255, bool(v >> 16))

    def run(self, x, out=None):
        """x: [n_channels][n] device tensor of IN containers -> [n_channels][n] OUT containers."""
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_channels and x.stride(1) == 1
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        n = x.shape[1]
        if out is None:
            out = _alloc_out(self.fout, self.n_channels, n, x.device, self.out_bytes)
        assert out.dtype == self.out_dtype and out.shape[1] >= n
        check(lib.acdsp_fir_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), n, C.c_void_p(out.data_ptr()),
                                _row_stride(out, self.fout), _stream_ptr(x)))
        return out

    def run_host(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_in_dtype(self.fin, self.in_bytes))
        assert x.shape[0] == self.n_channels
        y = _alloc_out_host(self.fout, self.n_channels, x.shape[1], self.out_bytes)
        check(lib.acdsp_fir_run_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1], y.ctypes.data_as(C.c_void_p)))
        return y

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib.acdsp_fir_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def kernel_stats(self, last_k):
        """(avg_ms, min_ms) of the main kernel over the last_k run() calls (HIP events on the launch stream)."""
        a, m = C.c_float(), C.c_float()
        check(lib.acdsp_fir_kernel_stats(self._h, last_k, C.byref(a), C.byref(m)))
        return a.value, m.value

    def mfma_issued(self):
        """32x32x32 int8 MFMAs the selected kernel issues per 1024 samples of one channel (0 off the "mfma_i8", "mfma_long" and "mfma_s8" paths)."""
        v = C.c_int32()
        check(lib.acdsp_fir_mfma_issued(self._h, C.byref(v)))
        return v.value


class Cic(_Stateful):
    """n_channels independent ac_cic_dec_full (interp=False) / ac_cic_intr_full (interp=True) objects."""
    _c = "cic"

    def __init__(self, interp, R, M, N, fin, fout, n_channels=1, device=0, force_generic=False, in_bytes=False):
        """in_bytes: decimator on an IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8"""
        self.interp, self.R, self.M, self.N = bool(interp), R, M, N
        self.fin, self.fout, self.n_channels, self.device = fin, fout, n_channels, device
        self.in_bytes = bool(in_bytes)
        self._d = CicDesc(int(self.interp), R, M, N, n_channels, fin, fout, device,
                          _flags(force_generic, in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_cic_create(C.byref(self._d), C.byref(self._h)))

    @property
    def int_type(self):
        it = Fmt()
        check(lib.acdsp_cic_int_type(C.byref(self._d), C.byref(it)))
        return it

    @property
    def two_stage_rates(self):
        """(R1, R2) of the two-stage kernel if the handle takes it, (0, 0) where no compiled stage-1 rate serves the descriptor
        (acdsp_cic_two_stage_rates: host only)"""
        r1, r2 = C.c_int32(), C.c_int32()
        check(lib.acdsp_cic_two_stage_rates(C.byref(self._d), C.byref(r1), C.byref(r2)))
        return r1.value, r2.value

    def out_count(self, n_in):
        return lib.acdsp_cic_out_count(self._h, n_in)

    @property
    def path(self):
        return {0: "recurrence", 1: "fir_identity", 3: "mfma_gen", 4: "wide", 6: "two_stage"}[lib.acdsp_cic_path(self._h)]

    def run(self, x, out=None):
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_channels and x.stride(1) == 1
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        n_in = x.shape[1]
        no = self.out_count(n_in)
        if out is None:
            dt = torch_dtype_for(self.fout)
            per64 = max(1, 64 // lib.acdsp_elem_bytes(self.fout.W))      # rows start on 64-byte boundaries (vector stores)
            out = _alloc_out(self.fout, self.n_channels, (max(no, 1) + per64 - 1) // per64 * per64, x.device)
        assert out.dtype == torch_dtype_for(self.fout) and out.shape[1] >= no
        n_out = C.c_int64()
        check(lib.acdsp_cic_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), n_in, C.c_void_p(out.data_ptr()),
                                _row_stride(out, self.fout), C.byref(n_out), _stream_ptr(x)))
        return out[:, :n_out.value]

    def run_host(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_in_dtype(self.fin, self.in_bytes))
        no = self.out_count(x.shape[1])
        y = _alloc_out_host(self.fout, self.n_channels, max(no, 1))
        n_out = C.c_int64()
        check(lib.acdsp_cic_run_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1], y.ctypes.data_as(C.c_void_p),
                                     y.shape[1], C.byref(n_out)))
        return y[:, :n_out.value]

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib.acdsp_cic_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def kernel_stats(self, last_k):
        a, m = C.c_float(), C.c_float()
        check(lib.acdsp_cic_kernel_stats(self._h, last_k, C.byref(a), C.byref(m)))
        return a.value, m.value


class PolyDec(_Stateful):
    """n_channels independent ac_poly_dec objects (NTAPS taps per branch, decimation DF)."""
    _c = "polydec"

    def __init__(self, n_taps, df, fin, fcoeff, facc, fout, n_channels=1, device=0, force_generic=False, in_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8"""
        self.n_taps, self.df, self.n_channels = n_taps, df, n_channels
        self.fin, self.fcoeff, self.facc, self.fout = fin, fcoeff, facc, fout
        self.in_bytes = bool(in_bytes)
        d = PolyDecDesc(n_taps, df, n_channels, fin, fcoeff, facc, fout, device,
                        _flags(force_generic, in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_polydec_create(C.byref(d), C.byref(self._h)))

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps * self.df,)
        check(lib.acdsp_polydec_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    @property
    def path(self):
        return PATHS[lib.acdsp_polydec_path(self._h)]

    @property
    def ring_shape(self):
        """ring-shape id of the last run(), 0 when no ring row ran (acdsp_polydec_ring_shape)"""
        return lib.acdsp_polydec_ring_shape(self._h)

    def run(self, x, out=None):
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_channels and x.stride(1) == 1
        assert x.dtype == self.in_dtype and x.shape[1] % self.df == 0, (x.dtype, self.fin, x.shape)
        n_out = x.shape[1] // self.df
        if out is None:
            out = torch.empty((self.n_channels, max(n_out, 1)), dtype=torch_dtype_for(self.fout), device=x.device)
        check(lib.acdsp_polydec_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), x.shape[1], C.c_void_p(out.data_ptr()),
                                    out.stride(0), _stream_ptr(x)))
        return out[:, :n_out]

    def run_host(self, x):
        """x: [n_channels][groups * DF] host array of IN raw words -> [n_channels][groups] OUT containers (acdsp_polydec_run_host)"""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_in_dtype(self.fin, self.in_bytes))
        assert x.shape[0] == self.n_channels and x.shape[1] % self.df == 0
        y = _alloc_out_host(self.fout, self.n_channels, x.shape[1] // self.df)
        check(lib.acdsp_polydec_run_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1], y.ctypes.data_as(C.c_void_p)))
        return y

    def set_scratch_cap(self, n_bytes):
        """long prototypes: bound the scratch of the phase streams (re-derives the slab / group geometry, reallocates, synchronises)"""
        check(lib.acdsp_polydec_set_scratch_cap(self._h, int(n_bytes)))

    def long_geometry(self):
        """(outputs per slab, channels per group, scratch bytes) of a long handle; (0, 0, 0) otherwise"""
        slab, group, nbytes = C.c_int64(), C.c_int32(), C.c_uint64()
        check(lib.acdsp_polydec_long_geometry(self._h, C.byref(slab), C.byref(group), C.byref(nbytes)))
        return slab.value, group.value, nbytes.value


class Ddc(_Stateful):
    """n_channels independent cascades ac_cic_dec_full(R, M, N) -> FIR on the decimator's lossless INT_TYPE words
    (C ABI acdsp_ddc_*): one fused kernel for the BASELINE config-5 shape class, the two stage kernels otherwise."""
    _c = "ddc"

    def __init__(self, R, M, N, fin, n_taps, ftype, fcoeff, facc, fout, n_channels=1, kind="const", device=0, flags=0, in_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_DDC_IN_BYTES, a flag of the cascade and not of its stage descriptors, on
        which `flags` lands): rows are torch.int8 / torch.uint8"""
        self.fin, self.fout, self.n_channels, self.n_taps = fin, fout, n_channels, n_taps
        self.in_bytes = bool(in_bytes)
        probe = CicDesc(0, R, M, N, n_channels, fin, fin, device, flags)
        it = Fmt()
        check(lib.acdsp_cic_int_type(C.byref(probe), C.byref(it)))
        self.int_type = Fmt(it.W, it.I, True)
        cd = CicDesc(0, R, M, N, n_channels, fin, self.int_type, device, flags)
        fd = FirDesc(KINDS[kind], FTYPES[ftype] if isinstance(ftype, str) else ftype, n_taps, n_channels, 0, self.int_type, fcoeff,
                     facc, fout, device, flags)
        self._h = C.c_void_p()
        check(lib.acdsp_ddc_create_ex(C.byref(cd), C.byref(fd), _lib.DDC_IN_BYTES if in_bytes else 0, C.byref(self._h)))

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps,)
        check(lib.acdsp_ddc_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    @property
    def path(self):
        return {0: "two_kernels", 1: "fused"}[lib.acdsp_ddc_path(self._h)]

    def out_count(self, n_in):
        return lib.acdsp_ddc_out_count(self._h, n_in)

    def run(self, x, out=None):
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_channels and x.stride(1) == 1
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        n_in = x.shape[1]
        no = self.out_count(n_in)
        if out is None:
            out = torch.empty((self.n_channels, (max(no, 1) + 7) // 8 * 8), dtype=torch_dtype_for(self.fout), device=x.device)
        assert out.dtype == torch_dtype_for(self.fout) and out.stride(1) == 1 and out.shape[1] >= no
        n_out = C.c_int64()
        check(lib.acdsp_ddc_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), n_in, C.c_void_p(out.data_ptr()), out.stride(0),
                                C.byref(n_out), _stream_ptr(x)))
        return out[:, :n_out.value]

    def kernel_stats(self, last_k):
        a, m = C.c_float(), C.c_float()
        check(lib.acdsp_ddc_kernel_stats(self._h, last_k, C.byref(a), C.byref(m)))
        return a.value, m.value


class DdcPolyDec(Ddc):
    """n_channels independent cascades ac_cic_dec_full(R, M, N) -> ac_poly_dec(NTAPS, DF) on the decimator's lossless INT_TYPE words
    (acdsp_ddc_create_polydec; every other call is Ddc's): one fused kernel for the config-5 class at DF = 2 with NTAPS*DF <= 128, the two
    stage kernels otherwise.  A call emits the whole groups of DF words; the rest waits for the next call."""

    def __init__(self, R, M, N, fin, n_taps, df, fcoeff, facc, fout, n_channels=1, device=0, in_bytes=False, flags=0):
        """in_bytes: as for Ddc (ACDSP_DDC_IN_BYTES); `flags` lands on both stage descriptors"""
        self.fin, self.fout, self.n_channels, self.n_taps, self.df = fin, fout, n_channels, n_taps, df
        self.in_bytes = bool(in_bytes)
        probe = CicDesc(0, R, M, N, n_channels, fin, fin, device, flags)
        it = Fmt()
        check(lib.acdsp_cic_int_type(C.byref(probe), C.byref(it)))
        self.int_type = Fmt(it.W, it.I, True)
        cd = CicDesc(0, R, M, N, n_channels, fin, self.int_type, device, flags)
        pd = PolyDecDesc(n_taps, df, n_channels, self.int_type, fcoeff, facc, fout, device, flags)
        self._h = C.c_void_p()
        check(lib.acdsp_ddc_create_polydec(C.byref(cd), C.byref(pd), _lib.DDC_IN_BYTES if in_bytes else 0, C.byref(self._h)))

    def set_coeffs(self, coeffs):
        """[NTAPS*DF] STR_COEFF raw words, ordered as PolyDec.set_coeffs takes them"""
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps * self.df,)
        check(lib.acdsp_ddc_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))


POLY_FTYPES = {"FOLD_EVEN": 0, "FOLD_ODD": 1, "FOLD_ANTI": 2}   # the enum of ac_poly_intr.h:71


class PolyIntr(_Stateful):
    """n_channels independent ac_poly_intr objects (C ABI acdsp_polyintr_*): IF outputs per input sample."""
    _c = "polyintr"

    def __init__(self, n_taps, coeff_sz, ifac, ftype, fin, fcoeff, facc, fout, n_channels=1, device=0, force_generic=False, in_bytes=False,
                 out_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8
        out_bytes (with in_bytes): OUT_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_OUT_BYTES): output rows are torch.int8 / torch.uint8"""
        self.fin, self.fout, self.n_channels, self.coeff_sz, self.ifac = fin, fout, n_channels, coeff_sz, ifac
        self.in_bytes, self.out_bytes = bool(in_bytes), bool(out_bytes)
        d = PolyIntrDesc(n_taps, coeff_sz, ifac, POLY_FTYPES[ftype] if isinstance(ftype, str) else ftype, n_channels, fin, fcoeff,
                         facc, fout, device, _flags(force_generic, in_bytes, out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_polyintr_create(C.byref(d), C.byref(self._h)))

    def set_ctrl(self, coeffs, sign, corr):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        sg = np.ascontiguousarray(sign, dtype=np.uint8)
        cr = np.ascontiguousarray(corr, dtype=np.uint8)
        assert c.shape == (self.coeff_sz,) and sg.shape == (self.ifac,) and cr.shape == (self.ifac,)
        check(lib.acdsp_polyintr_set_ctrl(self._h, c.ctypes.data_as(C.POINTER(C.c_int64)), sg.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          cr.ctypes.data_as(C.POINTER(C.c_uint8))))

    def out_count(self, n_in):
        return lib.acdsp_polyintr_out_count(self._h, n_in)

    def run(self, x, out=None):
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_channels and x.stride(1) == 1
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        no = self.out_count(x.shape[1])
        if out is None:
            out = torch.empty((self.n_channels, max(no, 1)), dtype=self.out_dtype, device=x.device)
        assert out.shape[0] == self.n_channels and out.shape[1] >= no and out.stride(1) == 1 and out.dtype == self.out_dtype
        n_out = C.c_int64()
        check(lib.acdsp_polyintr_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), x.shape[1], C.c_void_p(out.data_ptr()),
                                     out.stride(0), C.byref(n_out), _stream_ptr(x)))
        return out[:, :n_out.value]

    def run_host(self, x):
        """run() on host rows [n_channels][n] (numpy; int8 / uint8 under in_bytes) -> host rows [n_channels][n_out] of the output containers"""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_in_dtype(self.fin, self.in_bytes))
        assert x.shape[0] == self.n_channels
        no = self.out_count(x.shape[1])
        y = _alloc_out_host(self.fout, self.n_channels, max(no, 1), self.out_bytes)
        n_out = C.c_int64()
        check(lib.acdsp_polyintr_run_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1], y.ctypes.data_as(C.c_void_p), y.shape[1], C.byref(n_out)))
        return y[:, :n_out.value]

    @property
    def path(self):
        """kernel family of the last run(): "generic", "lossless64" (tiled int64 VALU kernel), "mfma_gen" (fir_up.hip; fir_up_s8.hip under in_bytes) or "mfma_long"
        (polyintr_long.hip: 65 taps per phase and more)"""
        return PATHS[lib.acdsp_polyintr_path(self._h)]

    def set_scratch_cap(self, n_bytes):
        """long sub-filters: bound the scratch of the phase rows (re-derives the slab / group geometry, reallocates, synchronises)"""
        check(lib.acdsp_polyintr_set_scratch_cap(self._h, int(n_bytes)))

    def long_geometry(self):
        """(input samples per slab, channels per group, scratch bytes) of a long handle; (0, 0, 0) otherwise"""
        slab, group, nbytes = C.c_int64(), C.c_int32(), C.c_uint64()
        check(lib.acdsp_polyintr_long_geometry(self._h, C.byref(slab), C.byref(group), C.byref(nbytes)))
        return slab.value, group.value, nbytes.value


class IntgDump(_Stateful):
    """n_objects independent ac_intg_dump<IN, ACC, OUT, N_TYPE, NS, CHN> objects (C ABI acdsp_intgdump_*); rows are the
    interleaved streams, n_sample the per-block N_TYPE words (shared by the objects)."""
    _c = "intgdump"

    def __init__(self, ns, chn, fin, facc, fout, n_objects=1, device=0, in_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8"""
        self.fin, self.fout, self.n_objects, self.chn = fin, fout, n_objects, chn
        self.in_bytes = bool(in_bytes)
        d = IntgDumpDesc(ns, chn, n_objects, fin, facc, fout, device, _flags(in_bytes=in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_intgdump_create(C.byref(d), C.byref(self._h)))

    def counts(self, n_sample):
        ns = np.ascontiguousarray(n_sample, dtype=np.int64)
        ni, no = C.c_int64(), C.c_int64()
        check(lib.acdsp_intgdump_counts(self._h, ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns), C.byref(ni), C.byref(no)))
        return ni.value, no.value

    def run(self, x, n_sample):
        ns = np.ascontiguousarray(n_sample, dtype=np.int64)
        ni, no = self.counts(ns)
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_objects and x.stride(1) == 1 and x.shape[1] >= ni
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        out = torch.empty((self.n_objects, max(no, 1)), dtype=torch_dtype_for(self.fout), device=x.device)
        n_out = C.c_int64()
        check(lib.acdsp_intgdump_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns),
                                     C.c_void_p(out.data_ptr()), out.stride(0), C.byref(n_out), _stream_ptr(x)))
        return out[:, :n_out.value]

    def run_host(self, x, n_sample):
        """run() on host rows [n_objects][>= the samples n_sample consumes] (dense rows of exactly that many samples go to the device)"""
        ns = np.ascontiguousarray(n_sample, dtype=np.int64)
        ni, no = self.counts(ns)
        x = np.atleast_2d(x)
        assert x.shape[0] == self.n_objects and x.shape[1] >= ni
        x = np.ascontiguousarray(x[:, :ni], dtype=_np_in_dtype(self.fin, self.in_bytes))
        y = _alloc_out_host(self.fout, self.n_objects, max(no, 1))
        n_out = C.c_int64()
        check(lib.acdsp_intgdump_run_host(self._h, x.ctypes.data_as(C.c_void_p), ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns),
                                          y.ctypes.data_as(C.c_void_p), y.shape[1], C.byref(n_out)))
        return y[:, :n_out.value]

    @property
    def path(self):
        """kernel family of the last run() (acdsp_intgdump_path)"""
        return {0: "exact_order", 1: "tile", 2: "stream", 3: "mfma"}[lib.acdsp_intgdump_path(self._h)]


WIN_MODES = {"WIN": 0, "MIRROR": 1, "CLIP": 2}   # AC_WIN / AC_MIRROR / AC_CLIP


class MvAvg(_Handle):
    """n_objects independent ac_mv_avg<MAX_SAMPLE, TAPS, WIN_TYPE, ...> objects (C ABI acdsp_mvavg_*): rows hold n_frames
    frames of n_sample inputs back to back; run() is one run() call of every object."""
    _c = "mvavg"

    def __init__(self, max_sample, taps, win_mode, fin, fcoeff, facc, fout, n_objects=1, device=0, force_generic=False, in_bytes=False,
                 out_bytes=False):
        """in_bytes: IN_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_IN_BYTES): rows are torch.int8 / torch.uint8
        out_bytes (with in_bytes): OUT_TYPE of up to 8 bits in 1-byte containers (ACDSP_FLAG_OUT_BYTES): output rows are torch.int8 / torch.uint8"""
        self.fin, self.fout, self.n_objects, self.taps = fin, fout, n_objects, taps
        self.in_bytes, self.out_bytes = bool(in_bytes), bool(out_bytes)
        d = MvAvgDesc(max_sample, taps, WIN_MODES[win_mode] if isinstance(win_mode, str) else win_mode, n_objects, fin, fcoeff, facc,
                      fout, device, _flags(force_generic, in_bytes, out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_mvavg_create(C.byref(d), C.byref(self._h)))

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.taps,)
        check(lib.acdsp_mvavg_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    def out_per_frame(self, n_sample):
        return lib.acdsp_mvavg_out_per_frame(self._h, n_sample)

    @property
    def path(self):
        """kernel family of the last run()"""
        return {0: "exact_order", 1: "int64_sums", 2: "stream", 3: "stream32", 4: "stream_mfma", 5: "stream_s8"}[lib.acdsp_mvavg_path(self._h)]

    def run(self, x, n_sample, out=None):
        assert x.is_cuda and x.dim() == 2 and x.shape[0] == self.n_objects and x.stride(1) == 1 and x.shape[1] % n_sample == 0
        assert x.dtype == self.in_dtype, (x.dtype, self.fin)
        n_frames = x.shape[1] // n_sample
        no = max(self.out_per_frame(n_sample), 0) * n_frames
        if out is None:
            out = torch.empty((self.n_objects, max(no, 1)), dtype=self.out_dtype, device=x.device)
        assert out.element_size() == torch.empty((), dtype=self.out_dtype).element_size(), (out.dtype, self.fout)
        n_out = C.c_int64()
        check(lib.acdsp_mvavg_run(self._h, C.c_void_p(x.data_ptr()), x.stride(0), n_sample, n_frames, C.c_void_p(out.data_ptr()), out.stride(0),
                                  C.byref(n_out), _stream_ptr(x)))
        return out[:, :n_out.value]

    def run_host(self, x, n_sample):
        """run() on host rows [n_objects][n_frames * n_sample] (numpy; int8 / uint8 under in_bytes) -> host rows of the output containers"""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_in_dtype(self.fin, self.in_bytes))
        assert x.shape[0] == self.n_objects and x.shape[1] % n_sample == 0
        n_frames = x.shape[1] // n_sample
        no = max(self.out_per_frame(n_sample), 0) * n_frames
        y = _alloc_out_host(self.fout, self.n_objects, max(no, 1), self.out_bytes)
        n_out = C.c_int64()
        check(lib.acdsp_mvavg_run_host(self._h, x.ctypes.data_as(C.c_void_p), n_sample, n_frames, y.ctypes.data_as(C.c_void_p), y.shape[1], C.byref(n_out)))
        return y[:, :n_out.value]


def node_shard(n_total, n_shards, shard):
    """Channel slice [lo, hi) of shard `shard` (acdsp_node_shard: contiguous, the first n_total % n_shards slices one longer)."""
    lo, hi = C.c_int64(), C.c_int64()
    check(lib.acdsp_node_shard(n_total, n_shards, shard, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


class _Node(_Rows):
    """Common part of the node-level handles (acdsp_node_*): one filter bank cut into contiguous channel slices, one per entry of
    `devices` (a device may repeat: its shards are then concurrent streams of one GPU), one engine handle + stream + host thread each."""

    def _finish_create(self, devices):
        self.devices = list(devices)
        self.n_shards = lib.acdsp_node_n_shards(self._h)
        self.slices = []
        for s in range(self.n_shards):
            dev, lo, hi = C.c_int32(), C.c_int64(), C.c_int64()
            check(lib.acdsp_node_shard_info(self._h, s, C.byref(dev), C.byref(lo), C.byref(hi), None, None))
            assert dev.value == self.devices[s]
            self.slices.append((lo.value, hi.value))

    @staticmethod
    def _dev_array(devices):
        return (C.c_int32 * len(devices))(*devices)

    def _ptrs(self, tensors, fmt, dtype=None):
        assert len(tensors) == self.n_shards
        dtype = dtype or torch_dtype_for(fmt)
        for t, (lo, hi), d in zip(tensors, self.slices, self.devices):
            assert t.is_cuda and _dev_index(t.device) == d and t.shape[0] == hi - lo and t.dtype == dtype, (t.shape, t.device, lo, hi, d)
        strides = {_row_stride(t, fmt) for t in tensors}
        assert len(strides) == 1, "every shard's block must have the same row stride"
        # The node handle launches on its workers' own non-blocking streams, which do not order with torch's streams: the blocks must be
        # complete (inputs) / free (outputs recycled by the caching allocator) before acdsp_node_*_run -- the precondition include/acdsp.h states.
        for d in set(self.devices):
            torch.cuda.current_stream(d).synchronize()
        return (C.c_void_p * self.n_shards)(*[t.data_ptr() for t in tensors]), strides.pop()

    def alloc(self, fmt, n, fill=None, as_bytes=False):
        """One [slice channels][n] device block per shard, on that shard's device (as_bytes: of 1-byte containers)."""
        out = []
        for (lo, hi), d in zip(self.slices, self.devices):
            t = _alloc_out(fmt, hi - lo, n, torch.device("cuda", d), as_bytes)
            if fill is not None:
                fill(t, lo)
            out.append(t)
        return out

    def last_ms(self):
        """(per-shard kernel ms of the last run(), their maximum): aggregate rate = channels x samples / max."""
        per = (C.c_float * self.n_shards)()
        mx = C.c_float()
        check(lib.acdsp_node_last_ms(self._h, per, C.byref(mx)))
        return list(per), mx.value

    def shard_handle(self, s):
        h = C.c_void_p()
        check(lib.acdsp_node_shard_info(self._h, s, None, None, None, C.byref(h), None))
        return h

    def close(self):
        if getattr(self, "_h", None):
            lib.acdsp_node_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class NodeFir(_Node):
    """A Fir bank sharded over `devices` (acdsp_node_fir_*): no collective, coefficients replicated (or sliced when per channel)."""

    def __init__(self, n_taps, ftype, fin, fcoeff, facc, fout, n_channels, devices, kind="load", coeffs_per_channel=False, in_bytes=False,
                 out_bytes=False):
        """in_bytes / out_bytes: as for Fir (ACDSP_FLAG_IN_BYTES, ACDSP_FLAG_OUT_BYTES)"""
        self.fin, self.fout, self.n_taps, self.n_channels = fin, fout, n_taps, n_channels
        self.coeffs_per_channel = bool(coeffs_per_channel)
        self.in_bytes = bool(in_bytes)
        self.out_bytes = bool(out_bytes)
        d = FirDesc(KINDS[kind], FTYPES[ftype] if isinstance(ftype, str) else ftype, n_taps, n_channels, int(self.coeffs_per_channel),
                    fin, fcoeff, facc, fout, 0, _flags(in_bytes=in_bytes, out_bytes=out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_fir_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == ((self.n_channels, self.n_taps) if self.coeffs_per_channel else (self.n_taps,))
        check(lib.acdsp_node_fir_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    def run(self, xs, outs=None):
        """xs: one [slice channels][n] device tensor per shard (on that shard's device) -> list of output tensors."""
        n = xs[0].shape[1]
        assert all(x.shape[1] == n for x in xs)
        if outs is None:
            outs = self.alloc(self.fout, n, as_bytes=self.out_bytes)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout, self.out_dtype)
        check(lib.acdsp_node_fir_run(self._h, pin, sin, n, pout, sout))
        return outs

    def run_host(self, x):
        x = np.ascontiguousarray(x, dtype=_np_in_dtype(self.fin, self.in_bytes))
        assert x.shape[0] == self.n_channels
        y = _alloc_out_host(self.fout, self.n_channels, x.shape[1], self.out_bytes)
        check(lib.acdsp_node_fir_run_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1], y.ctypes.data_as(C.c_void_p)))
        return y


class NodeCic(_Node):
    """A Cic bank sharded over `devices` (acdsp_node_cic_*)."""

    def __init__(self, interp, R, M, N, fin, fout, n_channels, devices, in_bytes=False):
        self.fin, self.fout, self.n_channels = fin, fout, n_channels
        self.in_bytes = bool(in_bytes)
        d = CicDesc(int(bool(interp)), R, M, N, n_channels, fin, fout, 0, _flags(in_bytes=in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_cic_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def out_count(self, n_in):
        return lib.acdsp_node_cic_out_count(self._h, n_in)

    def run(self, xs, outs=None):
        n_in = xs[0].shape[1]
        no = self.out_count(n_in)
        if outs is None:
            per64 = max(1, 64 // lib.acdsp_elem_bytes(self.fout.W))
            outs = self.alloc(self.fout, (max(no, 1) + per64 - 1) // per64 * per64)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout)
        n_out = C.c_int64()
        check(lib.acdsp_node_cic_run(self._h, pin, sin, n_in, pout, sout, C.byref(n_out)))
        return [o[:, :n_out.value] for o in outs]


class NodeDdc(_Node):
    """A Ddc bank sharded over `devices` (acdsp_node_ddc_*)."""

    def __init__(self, R, M, N, fin, n_taps, ftype, fcoeff, facc, fout, n_channels, devices, kind="const", in_bytes=False):
        """in_bytes: as for Ddc (ACDSP_DDC_IN_BYTES)"""
        self.fin, self.fout, self.n_channels, self.n_taps = fin, fout, n_channels, n_taps
        self.in_bytes = bool(in_bytes)
        probe = CicDesc(0, R, M, N, n_channels, fin, fin, 0, 0)
        it = Fmt()
        check(lib.acdsp_cic_int_type(C.byref(probe), C.byref(it)))
        self.int_type = Fmt(it.W, it.I, True)
        cd = CicDesc(0, R, M, N, n_channels, fin, self.int_type, 0, 0)
        fd = FirDesc(KINDS[kind], FTYPES[ftype] if isinstance(ftype, str) else ftype, n_taps, n_channels, 0, self.int_type, fcoeff, facc, fout, 0, 0)
        self._h = C.c_void_p()
        check(lib.acdsp_node_ddc_create_ex(C.byref(cd), C.byref(fd), _lib.DDC_IN_BYTES if in_bytes else 0, len(devices), self._dev_array(devices),
                                           C.byref(self._h)))
        self._finish_create(devices)

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps,)
        check(lib.acdsp_node_ddc_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    def out_count(self, n_in):
        return lib.acdsp_node_ddc_out_count(self._h, n_in)

    def run(self, xs, outs=None):
        n_in = xs[0].shape[1]
        no = self.out_count(n_in)
        if outs is None:
            outs = self.alloc(self.fout, (max(no, 1) + 7) // 8 * 8)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout)
        n_out = C.c_int64()
        check(lib.acdsp_node_ddc_run(self._h, pin, sin, n_in, pout, sout, C.byref(n_out)))
        return [o[:, :n_out.value] for o in outs]


class NodeDdcPolyDec(NodeDdc):
    """A DdcPolyDec bank sharded over `devices` (acdsp_node_ddc_create_polydec; set_coeffs / out_count / run are acdsp_node_ddc_*)."""

    def __init__(self, R, M, N, fin, n_taps, df, fcoeff, facc, fout, n_channels, devices, in_bytes=False):
        self.fin, self.fout, self.n_channels, self.n_taps, self.df = fin, fout, n_channels, n_taps, df
        self.in_bytes = bool(in_bytes)
        probe = CicDesc(0, R, M, N, n_channels, fin, fin, 0, 0)
        it = Fmt()
        check(lib.acdsp_cic_int_type(C.byref(probe), C.byref(it)))
        self.int_type = Fmt(it.W, it.I, True)
        cd = CicDesc(0, R, M, N, n_channels, fin, self.int_type, 0, 0)
        pd = PolyDecDesc(n_taps, df, n_channels, self.int_type, fcoeff, facc, fout, 0, 0)
        self._h = C.c_void_p()
        check(lib.acdsp_node_ddc_create_polydec(C.byref(cd), C.byref(pd), _lib.DDC_IN_BYTES if in_bytes else 0, len(devices), self._dev_array(devices),
                                                C.byref(self._h)))
        self._finish_create(devices)

    def set_coeffs(self, coeffs):
        """[NTAPS*DF] STR_COEFF raw words, ordered as PolyDec.set_coeffs takes them; replicated to every shard"""
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps * self.df,)
        check(lib.acdsp_node_ddc_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))


class NodePolyDec(_Node):
    """A PolyDec bank sharded over `devices` (acdsp_node_polydec_*)."""

    def __init__(self, n_taps, df, fin, fcoeff, facc, fout, n_channels, devices, in_bytes=False):
        self.fin, self.fout, self.n_channels, self.n_taps, self.df = fin, fout, n_channels, n_taps, df
        self.in_bytes = bool(in_bytes)
        d = PolyDecDesc(n_taps, df, n_channels, fin, fcoeff, facc, fout, 0, _flags(in_bytes=in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_polydec_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.n_taps * self.df,)
        check(lib.acdsp_node_polydec_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    def run(self, xs, outs=None):
        n_in = xs[0].shape[1]
        assert n_in % self.df == 0
        if outs is None:
            outs = self.alloc(self.fout, n_in // self.df + 8)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout)
        check(lib.acdsp_node_polydec_run(self._h, pin, sin, n_in, pout, sout))
        return [o[:, :n_in // self.df] for o in outs]


class NodePolyIntr(_Node):
    """A PolyIntr bank sharded over `devices` (acdsp_node_polyintr_*)."""

    def __init__(self, n_taps, coeff_sz, ifac, ftype, fin, fcoeff, facc, fout, n_channels, devices, in_bytes=False, out_bytes=False):
        """in_bytes / out_bytes: as for PolyIntr (ACDSP_FLAG_IN_BYTES, ACDSP_FLAG_OUT_BYTES)"""
        self.fin, self.fout, self.n_channels, self.ifac, self.coeff_sz = fin, fout, n_channels, ifac, coeff_sz
        self.in_bytes, self.out_bytes = bool(in_bytes), bool(out_bytes)
        d = PolyIntrDesc(n_taps, coeff_sz, ifac, POLY_FTYPES[ftype] if isinstance(ftype, str) else ftype, n_channels, fin, fcoeff, facc, fout, 0,
                         _flags(in_bytes=in_bytes, out_bytes=out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_polyintr_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def set_ctrl(self, coeffs, sign, corr):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        sg, cr = np.ascontiguousarray(sign, dtype=np.uint8), np.ascontiguousarray(corr, dtype=np.uint8)
        assert c.shape == (self.coeff_sz,) and sg.shape == (self.ifac,) and cr.shape == (self.ifac,)
        check(lib.acdsp_node_polyintr_set_ctrl(self._h, c.ctypes.data_as(C.POINTER(C.c_int64)), sg.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               cr.ctypes.data_as(C.POINTER(C.c_uint8))))

    def out_count(self, n_in):
        return lib.acdsp_node_polyintr_out_count(self._h, n_in)

    def run(self, xs, outs=None):
        n_in = xs[0].shape[1]
        no = self.out_count(n_in)
        if outs is None:
            outs = self.alloc(self.fout, (max(no, 1) + 7) // 8 * 8, as_bytes=self.out_bytes)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout, self.out_dtype)
        n_out = C.c_int64()
        check(lib.acdsp_node_polyintr_run(self._h, pin, sin, n_in, pout, sout, C.byref(n_out)))
        return [o[:, :n_out.value] for o in outs]


class NodeIntgDump(_Node):
    """An IntgDump bank (rows = objects) sharded over `devices` (acdsp_node_intgdump_*)."""

    def __init__(self, ns, chn, fin, facc, fout, n_objects, devices, in_bytes=False):
        self.fin, self.fout, self.n_objects, self.ns, self.chn = fin, fout, n_objects, ns, chn
        self.in_bytes = bool(in_bytes)
        d = IntgDumpDesc(ns, chn, n_objects, fin, facc, fout, 0, _flags(in_bytes=in_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_intgdump_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def run(self, xs, n_sample, outs=None):
        ns = np.ascontiguousarray(n_sample, dtype=np.int64)
        n_dump = int(((ns >= 1) & (ns <= self.ns)).sum()) * self.chn
        if outs is None:
            outs = self.alloc(self.fout, (max(n_dump, 1) + 7) // 8 * 8)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout)
        n_out = C.c_int64()
        check(lib.acdsp_node_intgdump_run(self._h, pin, sin, ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns), pout, sout, C.byref(n_out)))
        return [o[:, :n_out.value] for o in outs]


class NodeMvAvg(_Node):
    """A MvAvg bank (rows = objects) sharded over `devices` (acdsp_node_mvavg_*)."""

    def __init__(self, max_sample, taps, win_mode, fin, fcoeff, facc, fout, n_objects, devices, in_bytes=False, out_bytes=False):
        """in_bytes / out_bytes: as for MvAvg (ACDSP_FLAG_IN_BYTES, ACDSP_FLAG_OUT_BYTES)"""
        self.fin, self.fout, self.n_objects, self.taps = fin, fout, n_objects, taps
        self.in_bytes, self.out_bytes = bool(in_bytes), bool(out_bytes)
        d = MvAvgDesc(max_sample, taps, WIN_MODES[win_mode] if isinstance(win_mode, str) else win_mode, n_objects, fin, fcoeff, facc, fout, 0,
                      _flags(in_bytes=in_bytes, out_bytes=out_bytes))
        self._h = C.c_void_p()
        check(lib.acdsp_node_mvavg_create(C.byref(d), len(devices), self._dev_array(devices), C.byref(self._h)))
        self._finish_create(devices)

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, dtype=np.int64)
        assert c.shape == (self.taps,)
        check(lib.acdsp_node_mvavg_set_coeffs(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))))

    def run(self, xs, n_sample, outs=None):
        n = xs[0].shape[1]
        assert n % n_sample == 0
        if outs is None:
            outs = self.alloc(self.fout, n, as_bytes=self.out_bytes)
        pin, sin = self._ptrs(xs, self.fin, self.in_dtype)
        pout, sout = self._ptrs(outs, self.fout, self.out_dtype)
        n_out = C.c_int64()
        check(lib.acdsp_node_mvavg_run(self._h, pin, sin, n_sample, n // n_sample, pout, sout, C.byref(n_out)))
        return [o[:, :n_out.value] for o in outs]


def save_stream(path, x, fmt):
    """[n_channels][n] raw words (numpy, any integer dtype) -> ACDSPRAW file (include/acdsp.h: acdsp_stream_hdr_t)."""
    a = np.ascontiguousarray(np.atleast_2d(x), dtype=_np_dtype_for(fmt))
    h = StreamHdr(b"", 1, a.dtype.itemsize, fmt, 0, a.shape[0], a.shape[1], a.shape[1])
    check(lib.acdsp_stream_write(str(path).encode(), C.byref(h), a.ctypes.data_as(C.c_void_p)))


def load_stream(path):
    """ACDSPRAW file -> (raw words [n_channels][n_samples] int64, Fmt)."""
    h = StreamHdr()
    check(lib.acdsp_stream_read_header(str(path).encode(), C.byref(h)))
    a = np.empty((h.n_channels, h.stride), dtype=_np_dtype_for(h.fmt))
    check(lib.acdsp_stream_read(str(path).encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
    return a[:, :h.n_samples].astype(np.int64), Fmt(h.fmt.W, h.fmt.I, h.fmt.S, h.fmt.Q, h.fmt.O)
