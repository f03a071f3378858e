"""Python-side handles over the libsdrgpu C ABI, named after the reference blocks.

Each class mirrors one ``dsp::`` block of the reference (file:line in the C
header ``include/sdrgpu.h``): ``process(x)`` is the reference's
``process(count, in, out) -> outCount`` on host numpy buffers (synchronous,
staged through pinned memory), ``process_dev(in_ptr, count, out_ptr, stream)``
runs on device-resident buffers (torch tensors' ``data_ptr()``) on a caller
stream and returns the output count without synchronising.
"""
import ctypes

import numpy as np

from . import lib, check, F32, C64

_vp = ctypes.c_void_p


def _fptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _taps_arg(taps):
    t = np.ascontiguousarray(taps)
    if np.iscomplexobj(t):
        t = t.astype(np.complex64)
        return t, C64
    return t.astype(np.float32), F32


class Block:
    """Owns one sdrgpu_block handle."""

    def __init__(self, handle, in_dtype, out_dtype):
        self._h = handle
        self.in_dtype = in_dtype      # numpy dtype of one input element
        self.out_dtype = out_dtype

    def out_count(self, count):
        return check(lib.sdrgpu_block_out_count(self._h, int(count)))

    def process(self, x):
        x = np.ascontiguousarray(x, dtype=self.in_dtype)
        n = x.shape[0]
        out = np.empty(max(self.out_count(n), 1), dtype=self.out_dtype)
        m = check(lib.sdrgpu_block_process(self._h, _fptr(x), n, _fptr(out)))
        return out[:m]

    def process_dev(self, in_ptr, count, out_ptr, stream=None):
        return check(lib.sdrgpu_block_process_dev(self._h, _vp(in_ptr), int(count), _vp(out_ptr), _vp(stream or 0)))

    def reset(self):
        check(lib.sdrgpu_block_reset(self._h))

    def close(self):
        if self._h:
            lib.sdrgpu_block_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make(fn, *args):
    h = ctypes.c_void_p()
    check(fn(ctypes.byref(h), *args))
    return h


STEREO = np.dtype([("l", np.float32), ("r", np.float32)])


class FrequencyXlator(Block):
    """dsp::channel::FrequencyXlator (channel/frequency_xlator.h:15-50); offset in rad/sample."""

    def __init__(self, offset_rad, device=0):
        super().__init__(_make(lib.sdrgpu_xlator_create, device, float(offset_rad)), np.complex64, np.complex64)

    def set_offset(self, offset_rad):
        check(lib.sdrgpu_xlator_set_offset(self._h, float(offset_rad)))


class FIR(Block):
    """dsp::filter::FIR<D,T> (filter/fir.h) / DecimatingFIR<D,T> (filter/decimating_fir.h)."""

    def __init__(self, taps, decim=1, complex_data=True, device=0):
        t, ttype = _taps_arg(taps)
        dtype = C64 if complex_data else F32
        self._taps = t
        h = _make(lib.sdrgpu_fir_create, device, dtype, ttype, _fptr(t), int(t.shape[0]), int(decim))
        npd = np.complex64 if complex_data else np.float32
        super().__init__(h, npd, npd)

    def set_taps(self, taps):
        t, _ = _taps_arg(taps)
        self._taps = t
        check(lib.sdrgpu_fir_set_taps(self._h, _fptr(t), int(t.shape[0])))

    def set_decimation(self, decim):
        check(lib.sdrgpu_fir_set_decimation(self._h, int(decim)))


def DecimatingFIR(taps, decim, complex_data=True, device=0):
    return FIR(taps, decim, complex_data, device)


class Quadrature(Block):
    """dsp::demod::Quadrature (demod/quadrature.h:41-56); deviation in rad/sample."""

    def __init__(self, deviation_rad, device=0):
        super().__init__(_make(lib.sdrgpu_quadrature_create, device, float(deviation_rad)), np.complex64, np.float32)

    def set_deviation(self, deviation_rad):
        """setDeviation (demod/quadrature.h:29-33)."""
        check(lib.sdrgpu_quadrature_set_deviation(self._h, float(deviation_rad)))


class PowerDecimator(Block):
    """dsp::multirate::PowerDecimator<T> (multirate/power_decimator.h)."""

    def __init__(self, ratio, complex_data=True, device=0):
        npd = np.complex64 if complex_data else np.float32
        super().__init__(_make(lib.sdrgpu_power_decimator_create, device, C64 if complex_data else F32, int(ratio)), npd, npd)


class PolyphaseResampler(Block):
    """dsp::multirate::PolyphaseResampler<T> (multirate/polyphase_resampler.h)."""

    def __init__(self, interp, decim, taps, complex_data=True, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_polyphase_resampler_create, device, C64 if complex_data else F32, int(interp), int(decim),
                  _fptr(t), int(t.shape[0]))
        super().__init__(h, npd, npd)


class RationalResampler(Block):
    """dsp::multirate::RationalResampler<T> (multirate/rational_resampler.h)."""

    def __init__(self, in_sr, out_sr, complex_data=True, device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_rational_resampler_create, device, C64 if complex_data else F32, float(in_sr), float(out_sr))
        super().__init__(h, npd, npd)


class RxVFO(Block):
    """dsp::channel::RxVFO (channel/rx_vfo.h)."""

    def __init__(self, in_sr, out_sr, bandwidth, offset, device=0):
        h = _make(lib.sdrgpu_rxvfo_create, device, float(in_sr), float(out_sr), float(bandwidth), float(offset))
        super().__init__(h, np.complex64, np.complex64)

    def set_offset(self, offset):
        check(lib.sdrgpu_rxvfo_set_offset(self._h, float(offset)))


class _FusedDDC(Block):
    """The FIR stage's setters on a fused handle (sdrgpu_fir_set_taps / _set_decimation take it: the handle
    is a FIR block with the xlator fused in)."""

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._taps = t
        check(lib.sdrgpu_fir_set_taps(self._h, _fptr(t), int(t.shape[0])))

    def set_decimation(self, decim):
        check(lib.sdrgpu_fir_set_decimation(self._h, int(decim)))


class DDC(_FusedDDC):
    """Fused FrequencyXlator -> DecimatingFIR<complex_t,float> (complex out): the FIR stage of DDCFM."""

    def __init__(self, offset_rad, taps, decim, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._taps = t
        h = _make(lib.sdrgpu_ddc_create, device, float(offset_rad), _fptr(t), int(t.shape[0]), int(decim))
        super().__init__(h, np.complex64, np.complex64)


class DDCFM(_FusedDDC):
    """Fused FrequencyXlator -> DecimatingFIR<complex_t,float> -> Quadrature (BASELINE config C3)."""

    def __init__(self, offset_rad, taps, decim, deviation_rad, device=0):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._taps = t
        h = _make(lib.sdrgpu_ddc_fm_create, device, float(offset_rad), _fptr(t), int(t.shape[0]), int(decim),
                  float(deviation_rad))
        super().__init__(h, np.complex64, np.float32)

    def set_deviation(self, deviation_rad):
        check(lib.sdrgpu_quadrature_set_deviation(self._h, float(deviation_rad)))


class FM(Block):
    """dsp::demod::FM<float> (demod/fm.h)."""

    def __init__(self, samplerate, bandwidth, low_pass=True, high_pass=False, device=0):
        h = _make(lib.sdrgpu_fm_create, device, float(samplerate), float(bandwidth), int(low_pass), int(high_pass))
        super().__init__(h, np.complex64, np.float32)


class BroadcastFM(Block):
    """dsp::demod::BroadcastFM (demod/broadcast_fm.h:144-215); stereo_t out. stereo=False is
    the mono path (the C5 bench chain); stereo=True adds the pilot PLL stereo decoder."""

    def __init__(self, deviation, samplerate, low_pass=True, device=0, stereo=False, rds=False):
        if stereo or rds:   # the RDS branch lives in the full BroadcastFM block (mono or stereo)
            h = _make(lib.sdrgpu_broadcast_fm_create, device, float(deviation), float(samplerate), int(stereo),
                      int(low_pass))
        else:
            h = _make(lib.sdrgpu_wfm_create, device, float(deviation), float(samplerate), int(low_pass))
        super().__init__(h, np.complex64, STEREO)
        if rds:
            self.set_rds(True)

    def set_rds(self, enabled):
        """setRDSOut (broadcast_fm.h:121-127)."""
        check(lib.sdrgpu_broadcast_fm_set_rds(self._h, int(bool(enabled))))

    def set_rds_out(self, enabled):
        """The reference's setRDSOut (broadcast_fm.h:121-128): the flag, then reset()."""
        self.set_rds(enabled)
        self.reset()

    def rds_output(self):
        """RDS baseband (complex64, 5 kS/s) produced by the last process() call."""
        n = ctypes.c_int()
        check(lib.sdrgpu_broadcast_fm_rds_dev(self._h, None, ctypes.byref(n)))
        out = np.empty(n.value, np.complex64)
        if n.value:
            check(lib.sdrgpu_broadcast_fm_read_rds(self._h, _fptr(out), n.value))
        return out


class FFTSpectrum:
    """IQFrontEnd's FFT path (signal_path/iq_frontend.cpp:230-249, 272-296)."""

    def __init__(self, fft_size, nz=None, window=6, device=0, precision="f32"):
        """precision "f64": the fp64-interior parity mode (sdrgpu_fft_set_precision(h, 1))."""
        self.N = int(fft_size)
        self.nz = int(nz if nz is not None else fft_size)
        self._h = _make(lib.sdrgpu_fft_create, device, self.N, self.nz, int(window))
        if precision != "f32":
            self.set_precision(precision)

    def set_precision(self, precision):
        check(lib.sdrgpu_fft_set_precision(self._h, {"f32": 0, "f64": 1}[precision]))

    def set_tail_stream(self, stream):
        """sdrgpu_fft_set_tail_stream: the fused VFO's later stages and the zoom fold of
        execute_zoom_vfo_dev on `stream` (a HIP stream handle, or 0 / None to turn it off)."""
        check(lib.sdrgpu_fft_set_tail_stream(self._h, stream or None))

    def set_kernel(self, mode):
        """64k transform form (sdrgpu_fft_set_kernel): "two-pass", "one-pass" or "auto" (per call size,
        the default). Returns the previous mode's name."""
        names = ("two-pass", "one-pass", "auto")
        return names[check(lib.sdrgpu_fft_set_kernel(self._h, names.index(mode)))]

    @property
    def precision(self):
        return ("f32", "f64")[check(lib.sdrgpu_fft_get_precision(self._h))]

    def set_window(self, w):
        w = np.ascontiguousarray(w, dtype=np.float32)
        check(lib.sdrgpu_fft_set_window(self._h, _fptr(w), int(w.shape[0])))
        self.nz = int(w.shape[0])

    def logmag(self, x):
        """Host drop-in: x = complex64[nz] -> float32[N] dB."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        assert x.shape[0] >= self.nz
        out = np.empty(self.N, dtype=np.float32)
        check(lib.sdrgpu_fft_logmag(self._h, _fptr(x), _fptr(out)))
        return out

    def execute_dev(self, in_ptr, frame_stride, frames, out_ptr, stream=None):
        return check(lib.sdrgpu_fft_execute_dev(self._h, _vp(in_ptr), int(frame_stride), int(frames), _vp(out_ptr),
                                                _vp(stream or 0)))

    def execute_zoom_dev(self, in_ptr, frame_stride, frames, out_ptr, zoom_ptr, zoom_size, stream=None):
        """dB rows + the waterfall's full-span zoom rows (frames x zoom_size; fused at 64k / 2048)."""
        return check(lib.sdrgpu_fft_execute_zoom_dev(self._h, _vp(in_ptr), int(frame_stride), int(frames), _vp(out_ptr),
                                                     _vp(zoom_ptr), int(zoom_size), _vp(stream or 0)))

    def execute_vfo_dev(self, in_ptr, frames, out_ptr, vfo, vfo_out_ptr, stream=None):
        """Spectra of `frames` back-to-back frames + one RxVFO over the same device batch (the VFO's
        first stage fused into the 64k spectrum's input pass); returns the VFO's output count."""
        return check(lib.sdrgpu_fft_execute_vfo_dev(self._h, _vp(in_ptr), int(frames), _vp(out_ptr), vfo._h,
                                                    _vp(vfo_out_ptr), _vp(stream or 0)))

    def execute_zoom_vfo_dev(self, in_ptr, frames, out_ptr, zoom_ptr, zoom_size, vfo, vfo_out_ptr, stream=None):
        """Spectra (+ zoom rows when zoom_ptr) + one RxVFO over `frames` back-to-back frames; the VFO's
        first stage runs inside the spectrum launches where the plan allows. Returns the VFO's output count."""
        return check(lib.sdrgpu_fft_execute_zoom_vfo_dev(self._h, _vp(in_ptr), int(frames), _vp(out_ptr), _vp(zoom_ptr or 0),
                                                         int(zoom_size), vfo._h, _vp(vfo_out_ptr), _vp(stream or 0)))

    def set_timing(self, on=True):
        check(lib.sdrgpu_fft_set_timing(self._h, int(bool(on))))

    def group_times(self, n=256):
        """ms of the spectrum launch group of the last n timed calls (waits for them)."""
        ms = np.zeros(n, dtype=np.float32)
        k = check(lib.sdrgpu_fft_group_times(self._h, _fptr(ms), int(n)))
        return ms[:k]

    def close(self):
        if self._h:
            lib.sdrgpu_fft_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def convert(kind, x, device=0):
    """file_source / rtl_sdr / hackrf ingest converters on the GPU (host buffers)."""
    x = np.ascontiguousarray(x)
    n = x.size if kind != 2 else x.size // 3
    out = np.empty(n, dtype=np.float32)
    check(lib.sdrgpu_convert(device, int(kind), _fptr(x), n, _fptr(out)))
    return out


def convert_mono(kind, x, device=0):
    """One-channel file_source ingest (main.cpp:294-430): n samples -> complex64 with I = Q."""
    x = np.ascontiguousarray(x)
    n = x.size if kind != 2 else x.size // 3
    out = np.empty(n, dtype=np.complex64)
    check(lib.sdrgpu_convert_mono(device, int(kind), _fptr(x), n, _fptr(out)))
    return out


_CONV_BYTES = (1, 2, 3, 4, 8, 1, 4)
_CONV_VIEW = (np.uint8, np.int16, np.uint8, np.int32, np.float64, np.int8, np.float32)   # (i24: packed bytes)


class WavFile:
    """file_source's WavReader (C++ in libsdrgpu: sdrgpu_wav_*, wavreader.h:34-226) with the
    worker's framing: ``read()`` returns the next raw block of block_size frames (fs / 200), as
    bytes, and ``samples(block)`` converts it on the GPU to complex64 exactly as worker_1ch /
    worker_2ch do (main.cpp:294-560)."""

    def __init__(self, path, device=0):
        self._h = _make(lib.sdrgpu_wav_open, str(path).encode())
        f, c, b, sr, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
        check(lib.sdrgpu_wav_info(self._h, ctypes.byref(f), ctypes.byref(c), ctypes.byref(b), ctypes.byref(sr),
                                  ctypes.byref(n)))
        self.format, self.channels, self.bits = f.value, c.value, b.value
        self.sample_rate, self.sample_count = sr.value, n.value
        self.device = device
        self.kind = check(lib.sdrgpu_wav_kind(self._h))
        self.block_size = check(lib.sdrgpu_wav_block_size(self._h))
        self.frame_bytes = self.channels * _CONV_BYTES[self.kind]

    def read(self, max_frames=None):
        n = self.block_size if max_frames is None else int(max_frames)
        buf = np.empty(n * self.frame_bytes, np.uint8)
        got = check(lib.sdrgpu_wav_read(self._h, _fptr(buf), n))
        return buf[:got * self.frame_bytes]

    def samples(self, raw):
        if raw.size == 0:
            return np.empty(0, np.complex64)
        typed = raw.view(_CONV_VIEW[self.kind])
        if self.channels == 1:
            return convert_mono(self.kind, typed, self.device)
        return convert(self.kind, typed, self.device).view(np.complex64)

    def blocks(self):
        while True:
            raw = self.read()
            if raw.size == 0:
                return
            yield raw

    def seek(self, frame):
        check(lib.sdrgpu_wav_seek(self._h, int(frame)))

    def close(self):
        if self._h:
            lib.sdrgpu_wav_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-side design functions (no GPU) ----------------------------------
def create_window(wtype, size, centered=True):
    w = np.empty(size, dtype=np.float32)
    check(lib.sdrgpu_create_window(int(wtype), _fptr(w), int(size), int(centered)))
    return w


def _taps(fn, *args):
    n = check(fn(*args, None))
    t = np.empty(n, dtype=np.float32)
    fn(*args, _fptr(t))
    return t


def windowed_sinc(count, omega, norm=1.0):
    """taps::windowedSinc<float>(count, omega, window::nuttall, norm) (taps/windowed_sinc.h:9)."""
    out = np.empty(int(count), np.float32)
    check(lib.sdrgpu_taps_windowed_sinc(int(count), float(omega), float(norm), _fptr(out)))
    return out


class PolyphaseChannelizer(Block):
    """M-channel critically sampled polyphase channelizer (BASELINE C4): channel k of frame m is
    FrequencyXlator(-k fs/M) -> DecimatingFIR(taps, M) with an exact NCO. ``process`` returns
    complex64 [frames * M] laid out out[m * M + k]. ``dft="gemm"`` (M = 1024) computes each
    frame's DFT as two complex 32x32 matrix products on the f32 matrix cores instead of the LDS
    FFT (sdrgpu_channelizer_set_dft)."""

    def __init__(self, channels, taps, device=0, dft="fft"):
        t = np.ascontiguousarray(taps, np.float32)
        self._taps = t
        self.channels = int(channels)
        h = _make(lib.sdrgpu_channelizer_create, device, int(channels), _fptr(t), int(t.shape[0]))
        super().__init__(h, np.complex64, np.complex64)
        if dft not in ("fft", "gemm"):
            raise ValueError(f"dft must be 'fft' or 'gemm', not {dft!r}")
        check(lib.sdrgpu_channelizer_set_dft(self._h, 1 if dft == "gemm" else 0))


class AGC(Block):
    """dsp::loop::AGC<T> (loop/agc.h); complex_data selects T = complex_t (else float)."""

    def __init__(self, set_point, attack, decay, max_gain, max_output_amp, init_gain=1.0, complex_data=False, device=0):
        dt = C64 if complex_data else F32
        h = _make(lib.sdrgpu_agc_create, device, dt, float(set_point), float(attack), float(decay), float(max_gain),
                  float(max_output_amp), float(init_gain))
        npd = np.complex64 if complex_data else np.float32
        super().__init__(h, npd, npd)

    def set_enabled(self, enabled):
        check(lib.sdrgpu_agc_set_enabled(self._h, int(bool(enabled))))

    def set_gain(self, gain):
        check(lib.sdrgpu_agc_set_gain(self._h, float(gain)))

    def get_gain(self):
        g = ctypes.c_float()
        check(lib.sdrgpu_agc_get_gain(self._h, ctypes.byref(g)))
        return g.value


class FMIF(Block):
    """dsp::noise_reduction::FMIF (noise_reduction/fm_if.h): the radio module's "IF Noise
    Reduction"; bins in [3, 32]."""

    def __init__(self, bins, device=0):
        super().__init__(_make(lib.sdrgpu_fmif_create, device, int(bins)), np.complex64, np.complex64)
        self.bins = int(bins)

    def set_bins(self, bins):
        """setBins (fm_if.h:26-34): new window, history cleared."""
        check(lib.sdrgpu_fmif_set_bins(self._h, int(bins)))
        self.bins = int(bins)


def fmif_window(bins):
    """FMIF's window (fm_if.h:112): float32 nuttall(i, bins - 1), i < bins (host only)."""
    w = np.empty(max(int(bins), 1), dtype=np.float32)
    check(lib.sdrgpu_fmif_window(int(bins), _fptr(w)))
    return w


class NoiseBlanker(Block):
    """dsp::noise_reduction::NoiseBlanker (noise_reduction/noise_blanker.h); bit-exact recurrence."""

    def __init__(self, rate, level, device=0):
        super().__init__(_make(lib.sdrgpu_noise_blanker_create, device, float(rate), float(level)), np.complex64, np.complex64)

    def set(self, rate, level):
        """setRate / setLevel (noise_blanker.h:19-30): the running amplitude is kept."""
        check(lib.sdrgpu_noise_blanker_set(self._h, float(rate), float(level)))


class Squelch(Block):
    """dsp::noise_reduction::Squelch (noise_reduction/squelch.h); level in dB. The unmute count
    is per handle (the reference's is one static for the whole process)."""

    def __init__(self, level, device=0):
        super().__init__(_make(lib.sdrgpu_squelch_create, device, float(level)), np.complex64, np.complex64)

    def set_level(self, level):
        check(lib.sdrgpu_squelch_set_level(self._h, float(level)))

    def is_muted(self):
        """The state after the last call (waits for the queued work)."""
        m = ctypes.c_int()
        check(lib.sdrgpu_squelch_get_muted(self._h, ctypes.byref(m)))
        return bool(m.value)


# ---- symbol recovery (include/sdrgpu.h "symbol recovery") -------------------
def root_raised_cosine(count, beta, Ts):
    """taps::rootRaisedCosine<float>(count, beta, Ts) (taps/root_raised_cosine.h:8-29); Ts = samplerate / symbolrate."""
    out = np.empty(check(lib.sdrgpu_taps_root_raised_cosine(int(count), float(beta), float(Ts), None)), np.float32)
    check(lib.sdrgpu_taps_root_raised_cosine(int(count), float(beta), float(Ts), _fptr(out)))
    return out


def mm_interp_bank(phases=128, taps_per_phase=8):
    """MM's interpolator bank (clock_recovery/mm.h:173-178): float32 [phases, taps_per_phase] (host only)."""
    n = check(lib.sdrgpu_mm_interp_bank(int(phases), int(taps_per_phase), None))
    out = np.empty(n, np.float32)
    check(lib.sdrgpu_mm_interp_bank(int(phases), int(taps_per_phase), _fptr(out)))
    return out.reshape(int(phases), int(taps_per_phase))


class FastAGC(Block):
    """dsp::loop::FastAGC<T> (loop/fast_agc.h); bit-exact recurrence."""

    def __init__(self, set_point, max_gain, rate, init_gain=1.0, complex_data=False, device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_fast_agc_create, device, C64 if complex_data else F32, float(set_point), float(max_gain),
                  float(rate), float(init_gain))
        super().__init__(h, npd, npd)

    def set(self, set_point, max_gain, rate, init_gain=1.0):
        """setSetPoint / setMaxGain / setRate / setInitGain (fast_agc.h:24-46): the gain is kept."""
        check(lib.sdrgpu_fast_agc_set(self._h, float(set_point), float(max_gain), float(rate), float(init_gain)))

    def set_gain(self, gain):
        check(lib.sdrgpu_fast_agc_set_gain(self._h, float(gain)))

    def get_gain(self):
        g = ctypes.c_float()
        check(lib.sdrgpu_fast_agc_get_gain(self._h, ctypes.byref(g)))
        return g.value


class Costas(Block):
    """dsp::loop::Costas<ORDER> (loop/costas.h); arguments in PLL::init's order (loop/pll.h:15)."""

    def __init__(self, order, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-float(np.float32(3.1415926535)),
                 max_freq=float(np.float32(3.1415926535)), device=0):
        h = _make(lib.sdrgpu_costas_create, device, int(order), float(bandwidth), float(init_phase), float(init_freq),
                  float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)

    def set_bandwidth(self, bandwidth):
        check(lib.sdrgpu_costas_set_bandwidth(self._h, float(bandwidth)))

    def set_freq_limits(self, min_freq, max_freq):
        check(lib.sdrgpu_costas_set_freq_limits(self._h, float(min_freq), float(max_freq)))


_PI32 = float(np.float32(3.1415926535))                        # FL_M_PI, the loops' default frequency limits


class _PLLSetters:
    """setBandwidth / setFrequencyLimits (loop/pll.h:27, 49) of every loop that is a PLL."""

    def set_bandwidth(self, bandwidth):
        check(lib.sdrgpu_costas_set_bandwidth(self._h, float(bandwidth)))

    def set_freq_limits(self, min_freq, max_freq):
        check(lib.sdrgpu_costas_set_freq_limits(self._h, float(min_freq), float(max_freq)))


class PLL(Block, _PLLSetters):
    """dsp::loop::PLL (loop/pll.h): the VCO's phasor; arguments in PLL::init's order (loop/pll.h:15)."""

    def __init__(self, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-_PI32, max_freq=_PI32, device=0):
        h = _make(lib.sdrgpu_pll_create, device, float(bandwidth), float(init_phase), float(init_freq), float(min_freq),
                  float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class CarrierPLL(Block, _PLLSetters):
    """dsp::loop::CarrierTrackingPLL (loop/carrier_tracking_pll.h): the input derotated by the VCO; arguments as PLL."""

    def __init__(self, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-_PI32, max_freq=_PI32, device=0):
        h = _make(lib.sdrgpu_carrier_pll_create, device, float(bandwidth), float(init_phase), float(init_freq), float(min_freq),
                  float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class MeteorCostas(Block, _PLLSetters):
    """dsp::loop::MeteorCostas (decoder_modules/meteor_demodulator/src/meteor_costas.h); arguments in its init's order."""

    def __init__(self, bandwidth, broken_modulation=False, init_phase=0.0, init_freq=0.0, min_freq=-_PI32, max_freq=_PI32,
                 device=0):
        h = _make(lib.sdrgpu_meteor_costas_create, device, float(bandwidth), int(bool(broken_modulation)), float(init_phase),
                  float(init_freq), float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)

    def set_broken_modulation(self, enabled):
        check(lib.sdrgpu_meteor_costas_set_broken_modulation(self._h, int(bool(enabled))))


class _MMSetters:
    """The MM setters (clock_recovery/mm.h:40-71), on an MM or on a chain that ends in one."""

    def set_omega(self, omega):
        check(lib.sdrgpu_mm_set_omega(self._h, float(omega)))

    def set_gains(self, omega_gain, mu_gain):
        check(lib.sdrgpu_mm_set_gains(self._h, float(omega_gain), float(mu_gain)))

    def set_omega_rel_limit(self, rel):
        check(lib.sdrgpu_mm_set_omega_rel_limit(self._h, float(rel)))


class MM(Block, _MMSetters):
    """dsp::clock_recovery::MM<T> (clock_recovery/mm.h). ``out_count`` is the capacity (= count);
    ``process`` / ``process_dev`` return the exact count (process_dev waits for the stream)."""

    def __init__(self, omega, omega_gain, mu_gain, omega_rel_limit, interp_phases=128, interp_taps=8, complex_data=False,
                 device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_mm_create, device, C64 if complex_data else F32, float(omega), float(omega_gain), float(mu_gain),
                  float(omega_rel_limit), int(interp_phases), int(interp_taps))
        super().__init__(h, npd, npd)


class BinarySlicer(Block):
    """dsp::digital::BinarySlicer (digital/binary_slicer.h): float32 -> uint8."""

    def __init__(self, device=0):
        super().__init__(_make(lib.sdrgpu_binary_slicer_create, device), np.float32, np.uint8)


class DifferentialDecoder(Block):
    """dsp::digital::DifferentialDecoder (digital/differential_decoder.h): uint8 -> uint8."""

    def __init__(self, modulus, init_sym=0, device=0):
        super().__init__(_make(lib.sdrgpu_differential_decoder_create, device, int(modulus), int(init_sym)), np.uint8, np.uint8)


class PSK(Block, _MMSetters):
    """dsp::demod::PSK<ORDER> (demod/psk.h): complex64 samples -> complex64 symbols."""

    def __init__(self, order, symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bandwidth, omega_gain, mu_gain,
                 omega_rel_limit=0.01, device=0):
        h = _make(lib.sdrgpu_psk_create, device, int(order), float(symbolrate), float(samplerate), int(rrc_taps), float(rrc_beta),
                  float(agc_rate), float(costas_bandwidth), float(omega_gain), float(mu_gain), float(omega_rel_limit))
        super().__init__(h, np.complex64, np.complex64)


class Meteor(Block, _MMSetters):
    """dsp::demod::Meteor (decoder_modules/meteor_demodulator/src/meteor_demod.h), the LRPT demodulator: complex64
    samples -> complex64 symbols; arguments in its init's order."""

    def __init__(self, symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bandwidth, broken_modulation, oqpsk,
                 omega_gain, mu_gain, omega_rel_limit=0.01, device=0):
        h = _make(lib.sdrgpu_meteor_create, device, float(symbolrate), float(samplerate), int(rrc_taps), float(rrc_beta),
                  float(agc_rate), float(costas_bandwidth), int(bool(broken_modulation)), int(bool(oqpsk)), float(omega_gain),
                  float(mu_gain), float(omega_rel_limit))
        super().__init__(h, np.complex64, np.complex64)

    def set_broken_modulation(self, enabled):
        check(lib.sdrgpu_meteor_set_broken_modulation(self._h, int(bool(enabled))))

    def set_oqpsk(self, enabled):
        check(lib.sdrgpu_meteor_set_oqpsk(self._h, int(bool(enabled))))

    def set_costas_bandwidth(self, bandwidth):
        check(lib.sdrgpu_costas_set_bandwidth(self._h, float(bandwidth)))


class GFSK(Block, _MMSetters):
    """dsp::demod::GFSK (demod/gfsk.h): complex64 samples -> float32 soft symbols."""

    def __init__(self, symbolrate, samplerate, deviation, rrc_taps, rrc_beta, omega_gain, mu_gain, omega_rel_limit=0.01,
                 device=0):
        h = _make(lib.sdrgpu_gfsk_create, device, float(symbolrate), float(samplerate), float(deviation), int(rrc_taps),
                  float(rrc_beta), float(omega_gain), float(mu_gain), float(omega_rel_limit))
        super().__init__(h, np.complex64, np.float32)


class RDSBits(Block):
    """WFM's RDS symbol chain (radio module, demodulators/wfm.h:57-68): complex64 RDS baseband at
    5 kS/s (``BroadcastFM.rds_output()``, or its device pointer through ``process_dev``) -> uint8
    differentially decoded bits; ``symbols()`` is the last call's soft symbols."""

    def __init__(self, device=0):
        super().__init__(_make(lib.sdrgpu_rds_create, device), np.complex64, np.uint8)

    def symbols_dev(self):
        """(device pointer, count) of the last call's soft symbols."""
        ptr, n = ctypes.c_void_p(), ctypes.c_int()
        check(lib.sdrgpu_rds_symbols_dev(self._h, ctypes.byref(ptr), ctypes.byref(n)))
        return ptr.value, n.value

    def symbols(self):
        ptr, n = self.symbols_dev()
        out = np.empty(n, np.float32)
        if n:
            check(lib.sdrgpu_memcpy_d2h(_fptr(out), _vp(ptr), out.nbytes, None))
        return out


# ---- stream banks (include/sdrgpu.h "stream banks") --------------------------
class Bank:
    """Owns one sdrgpu_bank handle: S independent streams with shared parameters, element m of stream
    k at x[m, k] (the channelizer's layout). ``process(x)`` takes (frames, S) and returns (rows, S);
    after a call of a bank that ends in MM, ``counts`` is the int32[S] array of per-stream output
    counts, rows is the largest of them, and the elements of a row past a stream's count keep what
    ``out`` held (zeros where ``process`` allocates it)."""

    def __init__(self, handle, in_dtype, out_dtype):
        self._h = handle
        self.in_dtype = in_dtype
        self.out_dtype = out_dtype
        self.streams = check(lib.sdrgpu_bank_streams(self._h))

    def out_rows(self, frames):
        return check(lib.sdrgpu_bank_out_rows(self._h, int(frames)))

    def process(self, x, out=None):
        x = np.ascontiguousarray(x, dtype=self.in_dtype)
        if x.ndim != 2 or x.shape[1] != self.streams:
            raise ValueError(f"a bank of {self.streams} streams takes (frames, {self.streams}), not {x.shape}")
        frames = x.shape[0]
        cap = max(self.out_rows(frames), 1)
        if out is None:
            out = np.zeros((cap, self.streams), self.out_dtype)
        elif out.dtype != self.out_dtype or out.shape != (cap, self.streams) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous {np.dtype(self.out_dtype)} array of shape {(cap, self.streams)}")
        rows = check(lib.sdrgpu_bank_process(self._h, _fptr(x), frames, _fptr(out)))
        return out[:rows]

    def process_dev(self, in_ptr, frames, out_ptr, stream=None):
        return check(lib.sdrgpu_bank_process_dev(self._h, _vp(in_ptr), int(frames), _vp(out_ptr), _vp(stream or 0)))

    @property
    def counts(self):
        c = np.empty(self.streams, np.int32)
        check(lib.sdrgpu_bank_out_counts(self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return c

    def reset(self):
        check(lib.sdrgpu_bank_reset(self._h))

    def close(self):
        if self._h:
            lib.sdrgpu_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BankQuadrature(Bank):
    """dsp::demod::Quadrature per stream; deviation in rad/sample."""

    def __init__(self, streams, deviation_rad, device=0):
        super().__init__(_make(lib.sdrgpu_bank_quadrature_create, device, int(streams), float(deviation_rad)), np.complex64,
                         np.float32)


class BankFIR(Bank):
    """dsp::filter::FIR<D, float> per stream: real taps shared by all streams."""

    def __init__(self, streams, taps, complex_data=True, device=0):
        t = np.ascontiguousarray(taps, np.float32)
        self._taps = t
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_bank_fir_create, device, int(streams), C64 if complex_data else F32, _fptr(t), int(t.shape[0]))
        super().__init__(h, npd, npd)


class BankFastAGC(Bank):
    """dsp::loop::FastAGC<T> per stream."""

    def __init__(self, streams, set_point, max_gain, rate, init_gain=1.0, complex_data=False, device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_bank_fast_agc_create, device, int(streams), C64 if complex_data else F32, float(set_point),
                  float(max_gain), float(rate), float(init_gain))
        super().__init__(h, npd, npd)


class BankCostas(Bank):
    """dsp::loop::Costas<ORDER> per stream; arguments as Costas."""

    def __init__(self, streams, order, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-float(np.float32(3.1415926535)),
                 max_freq=float(np.float32(3.1415926535)), device=0):
        h = _make(lib.sdrgpu_bank_costas_create, device, int(streams), int(order), float(bandwidth), float(init_phase),
                  float(init_freq), float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class BankMM(Bank):
    """dsp::clock_recovery::MM<T> per stream; arguments as MM. ``out_rows`` is the capacity (= frames)."""

    def __init__(self, streams, omega, omega_gain, mu_gain, omega_rel_limit, interp_phases=128, interp_taps=8, complex_data=False,
                 device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_bank_mm_create, device, int(streams), C64 if complex_data else F32, float(omega), float(omega_gain),
                  float(mu_gain), float(omega_rel_limit), int(interp_phases), int(interp_taps))
        super().__init__(h, npd, npd)


class BankPSK(Bank):
    """dsp::demod::PSK<ORDER> per stream: complex64 samples -> complex64 symbols; arguments as PSK."""

    def __init__(self, streams, order, symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bandwidth, omega_gain, mu_gain,
                 omega_rel_limit=0.01, device=0):
        h = _make(lib.sdrgpu_bank_psk_create, device, int(streams), int(order), float(symbolrate), float(samplerate), int(rrc_taps),
                  float(rrc_beta), float(agc_rate), float(costas_bandwidth), float(omega_gain), float(mu_gain),
                  float(omega_rel_limit))
        super().__init__(h, np.complex64, np.complex64)


class BankPLL(Bank):
    """dsp::loop::PLL per stream; arguments as PLL."""

    def __init__(self, streams, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-_PI32, max_freq=_PI32, device=0):
        h = _make(lib.sdrgpu_bank_pll_create, device, int(streams), float(bandwidth), float(init_phase), float(init_freq),
                  float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class BankCarrierPLL(Bank):
    """dsp::loop::CarrierTrackingPLL per stream; arguments as CarrierPLL."""

    def __init__(self, streams, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-_PI32, max_freq=_PI32, device=0):
        h = _make(lib.sdrgpu_bank_carrier_pll_create, device, int(streams), float(bandwidth), float(init_phase), float(init_freq),
                  float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class BankMeteorCostas(Bank):
    """dsp::loop::MeteorCostas per stream; arguments as MeteorCostas."""

    def __init__(self, streams, bandwidth, broken_modulation=False, init_phase=0.0, init_freq=0.0, min_freq=-_PI32,
                 max_freq=_PI32, device=0):
        h = _make(lib.sdrgpu_bank_meteor_costas_create, device, int(streams), float(bandwidth), int(bool(broken_modulation)),
                  float(init_phase), float(init_freq), float(min_freq), float(max_freq))
        super().__init__(h, np.complex64, np.complex64)


class BankMeteor(Bank):
    """dsp::demod::Meteor per stream: complex64 samples -> complex64 symbols; arguments as Meteor."""

    def __init__(self, streams, symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bandwidth, broken_modulation, oqpsk,
                 omega_gain, mu_gain, omega_rel_limit=0.01, device=0):
        h = _make(lib.sdrgpu_bank_meteor_create, device, int(streams), float(symbolrate), float(samplerate), int(rrc_taps),
                  float(rrc_beta), float(agc_rate), float(costas_bandwidth), int(bool(broken_modulation)), int(bool(oqpsk)),
                  float(omega_gain), float(mu_gain), float(omega_rel_limit))
        super().__init__(h, np.complex64, np.complex64)


class BankGFSK(Bank):
    """dsp::demod::GFSK per stream: complex64 samples -> float32 soft symbols; arguments as GFSK."""

    def __init__(self, streams, symbolrate, samplerate, deviation, rrc_taps, rrc_beta, omega_gain, mu_gain, omega_rel_limit=0.01,
                 device=0):
        h = _make(lib.sdrgpu_bank_gfsk_create, device, int(streams), float(symbolrate), float(samplerate), float(deviation),
                  int(rrc_taps), float(rrc_beta), float(omega_gain), float(mu_gain), float(omega_rel_limit))
        super().__init__(h, np.complex64, np.float32)


class BankAGC(Bank):
    """dsp::loop::AGC<T> per stream; arguments as AGC. ``enabled=False`` is the fixed-gain limiter."""

    def __init__(self, streams, set_point, attack, decay, max_gain, max_output_amp, init_gain=1.0, complex_data=False, enabled=True,
                 device=0):
        npd = np.complex64 if complex_data else np.float32
        h = _make(lib.sdrgpu_bank_agc_create, device, int(streams), C64 if complex_data else F32, float(set_point), float(attack),
                  float(decay), float(max_gain), float(max_output_amp), float(init_gain), int(bool(enabled)))
        super().__init__(h, npd, npd)

    def set_gain(self, gain):
        """AGC::setGain for every stream, latched at the next call."""
        check(lib.sdrgpu_bank_agc_set_gain(self._h, float(gain)))


class BankDCBlocker(Bank):
    """dsp::correction::DCBlocker<T> per stream; rate in 1/sample."""

    def __init__(self, streams, rate, complex_data=False, device=0):
        npd = np.complex64 if complex_data else np.float32
        super().__init__(_make(lib.sdrgpu_bank_dc_blocker_create, device, int(streams), C64 if complex_data else F32, float(rate)),
                         npd, npd)


class BankDeemphasis(Bank):
    """dsp::filter::Deemphasis<float> per stream; ``stereo=True``: Deemphasis<stereo_t>, complex64 rows of (l, r)."""

    def __init__(self, streams, tau, samplerate, device=0, stereo=False):
        fn = lib.sdrgpu_bank_deemphasis_stereo_create if stereo else lib.sdrgpu_bank_deemphasis_create
        npd = np.complex64 if stereo else np.float32
        super().__init__(_make(fn, device, int(streams), float(tau), float(samplerate)), npd, npd)


class BankSquelch(Bank):
    """dsp::noise_reduction::Squelch per stream; level in dB, the unmute count per stream."""

    def __init__(self, streams, level, device=0):
        super().__init__(_make(lib.sdrgpu_bank_squelch_create, device, int(streams), float(level)), np.complex64, np.complex64)

    @property
    def muted(self):
        """int32[S]: the streams' mute state after the last call (waits for the queued work)."""
        m = np.empty(self.streams, np.int32)
        check(lib.sdrgpu_bank_squelch_muted(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return m


class BankFM(Bank):
    """dsp::demod::FM<float> per stream: complex64 -> float32 mono; arguments as FM."""

    def __init__(self, streams, samplerate, bandwidth, low_pass=True, high_pass=False, device=0):
        h = _make(lib.sdrgpu_bank_fm_create, device, int(streams), float(samplerate), float(bandwidth), int(bool(low_pass)),
                  int(bool(high_pass)))
        super().__init__(h, np.complex64, np.float32)


class BankAM(Bank):
    """dsp::demod::AM<float> per stream: complex64 -> float32 mono; agc_mode 0 OFF, 1 CARRIER, 2 AUDIO."""

    def __init__(self, streams, agc_mode, bandwidth, attack, decay, dc_rate, samplerate, device=0):
        h = _make(lib.sdrgpu_bank_am_create, device, int(streams), int(agc_mode), float(bandwidth), float(attack), float(decay),
                  float(dc_rate), float(samplerate))
        super().__init__(h, np.complex64, np.float32)

    def set_agc_gain(self, gain):
        """setAGCGain: the gain of the chain's AGC for every stream, latched at the next call."""
        check(lib.sdrgpu_bank_agc_set_gain(self._h, float(gain)))


class BankXlator(Bank):
    """dsp::channel::FrequencyXlator per stream: one offset (rad/sample) and one running phase for the bank.
    ``real=True`` keeps the real part only (complex64 -> float32, one launch): the first stage of BankSSB / BankCW."""

    def __init__(self, streams, offset_rad, real=False, device=0):
        fn = lib.sdrgpu_bank_xlator_real_create if real else lib.sdrgpu_bank_xlator_create
        super().__init__(_make(fn, device, int(streams), float(offset_rad)), np.complex64, np.float32 if real else np.complex64)

    def set_offset(self, offset_rad):
        """setOffset: the phase is kept, the offset applies from the next call."""
        check(lib.sdrgpu_bank_xlator_set_offset(self._h, float(offset_rad)))


class _XlateAgcBank(Bank):
    """translate -> real part -> AGC per stream: complex64 -> float32 mono (BankSSB, BankCW)."""

    def set_offset(self, offset_rad):
        """setOffset of the chain's xlator (rad/sample): the phase is kept."""
        check(lib.sdrgpu_bank_xlator_set_offset(self._h, float(offset_rad)))

    def set_agc_gain(self, gain):
        """setAGCGain: the gain of the chain's AGC for every stream, latched at the next call."""
        check(lib.sdrgpu_bank_agc_set_gain(self._h, float(gain)))


class BankSSB(_XlateAgcBank):
    """dsp::demod::SSB<float> per stream; mode 0 USB, 1 LSB, 2 DSB; arguments as SSB."""

    def __init__(self, streams, mode, bandwidth, samplerate, agc_enabled, attack, decay, device=0):
        h = _make(lib.sdrgpu_bank_ssb_create, device, int(streams), int(mode), float(bandwidth), float(samplerate),
                  int(bool(agc_enabled)), float(attack), float(decay))
        super().__init__(h, np.complex64, np.float32)


class BankCW(_XlateAgcBank):
    """dsp::demod::CW<float> per stream; arguments as CW."""

    def __init__(self, streams, tone, agc_enabled, attack, decay, samplerate, device=0):
        h = _make(lib.sdrgpu_bank_cw_create, device, int(streams), float(tone), int(bool(agc_enabled)), float(attack),
                  float(decay), float(samplerate))
        super().__init__(h, np.complex64, np.float32)


class _RateBank(Bank):
    """A bank that writes another number of rows than it reads: ``out_rows(frames)`` is the exact count of
    the next call, ``counts`` is that count for every stream."""

    def __init__(self, fn, streams, complex_data, device, *args):
        npd = np.complex64 if complex_data else np.float32
        super().__init__(_make(fn, device, int(streams), C64 if complex_data else F32, *args), npd, npd)


class BankDecimatingFIR(_RateBank):
    """dsp::filter::DecimatingFIR<D, float> per stream: real taps shared by all streams."""

    def __init__(self, streams, taps, decim, complex_data=True, device=0):
        t = np.ascontiguousarray(taps, np.float32)
        self._taps = t
        super().__init__(lib.sdrgpu_bank_decimating_fir_create, streams, complex_data, device, _fptr(t), int(t.shape[0]), int(decim))


class BankPolyphaseResampler(_RateBank):
    """dsp::multirate::PolyphaseResampler<T> per stream; arguments as PolyphaseResampler."""

    def __init__(self, streams, interp, decim, taps, complex_data=True, device=0):
        t = np.ascontiguousarray(taps, np.float32)
        self._taps = t
        super().__init__(lib.sdrgpu_bank_polyphase_resampler_create, streams, complex_data, device, int(interp), int(decim),
                         _fptr(t), int(t.shape[0]))


class BankPowerDecimator(_RateBank):
    """dsp::multirate::PowerDecimator<T> per stream: the stages of decim_plan(ratio); ratio 1 copies."""

    def __init__(self, streams, ratio, complex_data=True, device=0):
        super().__init__(lib.sdrgpu_bank_power_decimator_create, streams, complex_data, device, int(ratio))


class BankRationalResampler(_RateBank):
    """dsp::multirate::RationalResampler<T> per stream; the plan and taps of RationalResampler."""

    def __init__(self, streams, in_sr, out_sr, complex_data=True, device=0):
        super().__init__(lib.sdrgpu_bank_rational_resampler_create, streams, complex_data, device, float(in_sr), float(out_sr))


class BankFIRComplex(Bank):
    """dsp::filter::FIR<complex_t, complex_t> per stream: complex taps shared by all streams, complex64 out.
    ``real_input=True``: float32 rows, convert::RealToComplex first in the same launch."""

    def __init__(self, streams, taps, real_input=False, device=0):
        t = np.ascontiguousarray(taps, np.complex64)
        self._taps = t
        h = _make(lib.sdrgpu_bank_fir_complex_create, device, int(streams), F32 if real_input else C64, _fptr(t), int(t.shape[0]))
        super().__init__(h, np.float32 if real_input else np.complex64, np.complex64)


class BankStereoDecoder(Bank):
    """The stereo decoder of dsp::demod::BroadcastFM per stream (pilot filter -> PLL -> matrix): float32 MPX ->
    complex64 (l, r) = (re, im)."""

    def __init__(self, streams, samplerate, device=0):
        super().__init__(_make(lib.sdrgpu_bank_stereo_decoder_create, device, int(streams), float(samplerate)), np.float32,
                         np.complex64)


class BankBroadcastFM(Bank):
    """dsp::demod::BroadcastFM per stream, without the RDS branch: complex64 -> complex64 (l, r) = (re, im);
    arguments as BroadcastFM."""

    def __init__(self, streams, deviation, samplerate, low_pass=True, stereo=True, device=0):
        h = _make(lib.sdrgpu_bank_broadcast_fm_create, device, int(streams), float(deviation), float(samplerate), int(bool(stereo)),
                  int(bool(low_pass)))
        super().__init__(h, np.complex64, np.complex64)


class DCBlocker(Block):
    """dsp::correction::DCBlocker<T> (correction/dc_blocker.h); rate in 1/sample."""

    def __init__(self, rate, complex_data=False, device=0):
        dt = C64 if complex_data else F32
        npd = np.complex64 if complex_data else np.float32
        super().__init__(_make(lib.sdrgpu_dc_blocker_create, device, dt, float(rate)), npd, npd)


class AM(Block):
    """dsp::demod::AM<T> (demod/am.h); agc_mode 0 OFF, 1 CARRIER, 2 AUDIO."""

    def __init__(self, agc_mode, bandwidth, attack, decay, dc_rate, samplerate, stereo=False, device=0):
        h = _make(lib.sdrgpu_am_create, device, int(agc_mode), float(bandwidth), float(attack), float(decay),
                  float(dc_rate), float(samplerate), int(bool(stereo)))
        super().__init__(h, np.complex64, STEREO if stereo else np.float32)
        self._carrier = int(agc_mode) == 1

    def set_agc_gain(self, gain):
        """setAGCGain (am.h:71-75): the audio AGC, which CARRIER mode does not run."""
        if not self._carrier:
            check(lib.sdrgpu_demod_agc_set_gain(self._h, 1, float(gain)))

    def set_agc_attack_decay(self, attack, decay):
        check(lib.sdrgpu_demod_agc_set_attack_decay(self._h, float(attack), float(decay)))

    def set_dc_block_rate(self, rate):
        check(lib.sdrgpu_dc_blocker_set_rate(self._h, float(rate)))

    def set_low_pass_taps(self, taps):
        """The low-pass filter's taps (what setBandwidth designs anew, am.h:51-60); the history is kept."""
        t = np.ascontiguousarray(taps, np.float32)
        check(lib.sdrgpu_fir_set_taps(self._h, _fptr(t), int(t.shape[0])))


class _DemodAgcSetters:
    """setAGCEnabled / setAGCGain / setAGCAttack + setAGCDecay of SSB and CW (ssb.h:64-88, cw.h:37-63)."""

    def set_agc_enabled(self, enabled):
        check(lib.sdrgpu_demod_agc_set_enabled(self._h, 0, int(bool(enabled))))

    def set_agc_gain(self, gain):
        check(lib.sdrgpu_demod_agc_set_gain(self._h, 0, float(gain)))

    def set_agc_attack_decay(self, attack, decay):
        check(lib.sdrgpu_demod_agc_set_attack_decay(self._h, float(attack), float(decay)))


class SSB(Block, _DemodAgcSetters):
    """dsp::demod::SSB<T> (demod/ssb.h); mode 0 USB, 1 LSB, 2 DSB."""

    def __init__(self, mode, bandwidth, samplerate, agc_enabled, attack, decay, stereo=False, device=0):
        h = _make(lib.sdrgpu_ssb_create, device, int(mode), float(bandwidth), float(samplerate), int(bool(agc_enabled)),
                  float(attack), float(decay), int(bool(stereo)))
        super().__init__(h, np.complex64, STEREO if stereo else np.float32)


class CW(Block, _DemodAgcSetters):
    """dsp::demod::CW<T> (demod/cw.h); arguments in CW::init's order."""

    def __init__(self, tone, agc_enabled, attack, decay, samplerate, stereo=False, device=0):
        h = _make(lib.sdrgpu_cw_create, device, float(tone), int(bool(agc_enabled)), float(attack), float(decay),
                  float(samplerate), int(bool(stereo)))
        super().__init__(h, np.complex64, STEREO if stereo else np.float32)

    def set_tone(self, tone):
        """setTone: the xlator's phase is kept."""
        check(lib.sdrgpu_cw_set_tone(self._h, float(tone)))


class IQFrontEnd:
    """Device IQ front end (signal_path/iq_frontend.cpp; include/sdrgpu.h sdrgpu_frontend_*):
    ingest conversion -> [decimation] -> [DC block] -> [IQ inversion] -> VFOs + spectrum rows.
    ``push(block, kind=-1)`` takes a host block (complex64, or raw interleaved samples of a
    SDRGPU_CONV_* kind) and returns the dB rows completed by it; ``vfo_output(id)`` is that
    VFO's output for the block."""

    def __init__(self, sample_rate, decim=1, dc_blocking=False, fft_size=65536, fft_rate=15.0, window=6, device=0):
        self._h = _make(lib.sdrgpu_frontend_create, device, float(sample_rate), int(decim), int(bool(dc_blocking)),
                        int(fft_size), float(fft_rate), int(window))
        self.fft_size = int(fft_size)

    def framing(self):
        nz, skip, sr = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        check(lib.sdrgpu_frontend_framing(self._h, ctypes.byref(nz), ctypes.byref(skip), ctypes.byref(sr)))
        return nz.value, skip.value, sr.value

    def configure(self, sample_rate, decim=1, dc_blocking=False):
        check(lib.sdrgpu_frontend_configure(self._h, float(sample_rate), int(decim), int(bool(dc_blocking))))

    def set_invert_iq(self, enabled):
        check(lib.sdrgpu_frontend_set_invert_iq(self._h, int(bool(enabled))))

    def set_fft(self, fft_size, fft_rate, window=6):
        check(lib.sdrgpu_frontend_set_fft(self._h, int(fft_size), float(fft_rate), int(window)))
        self.fft_size = int(fft_size)

    def add_vfo(self, out_sr, bandwidth, offset):
        i = ctypes.c_int()
        check(lib.sdrgpu_frontend_add_vfo(self._h, ctypes.byref(i), float(out_sr), float(bandwidth), float(offset)))
        return i.value

    def remove_vfo(self, vid):
        check(lib.sdrgpu_frontend_remove_vfo(self._h, int(vid)))

    def set_vfo_offset(self, vid, offset):
        check(lib.sdrgpu_frontend_set_vfo_offset(self._h, int(vid), float(offset)))

    def push(self, block, kind=-1):
        a = np.ascontiguousarray(block)
        count = a.shape[0] if kind < 0 else a.size // 2
        nf = check(lib.sdrgpu_frontend_push(self._h, _fptr(a), int(count), int(kind)))
        rows = np.empty((nf, self.fft_size), np.float32)
        if nf:
            check(lib.sdrgpu_frontend_read_spectra(self._h, _fptr(rows), nf))
        return rows

    def push_dev(self, ptr, count, kind=-1, stream=None):
        return check(lib.sdrgpu_frontend_push_dev(self._h, _vp(ptr), int(count), int(kind), _vp(stream or 0)))

    # pipelined host call style (the C++ drop-in's worker): submit returns a ticket at once; collect
    # waits for it and copies its results out of the pinned result slot; at most two in flight
    def submit(self, block, kind=-1, want_iq=False, ptr=None, count=None):
        """Host block (numpy array, or `ptr`/`count` of host memory) -> ticket."""
        if ptr is None:
            a = np.ascontiguousarray(block)
            ptr, count = a.ctypes.data, (a.shape[0] if kind < 0 else a.size // 2)
        return check(lib.sdrgpu_frontend_submit(self._h, _vp(ptr), int(count), int(kind), 1 if want_iq else 0))

    def collect(self, ticket, vfos=(), copy=True):
        """(rows [nrows, N] float32, {vid: complex64 output}, iq complex64 or None) of a ticket; the
        ticket is released afterwards. copy=False only waits and releases (timing)."""
        rows_p, iq_p, niq = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        nf = check(lib.sdrgpu_frontend_collect(self._h, int(ticket), ctypes.byref(rows_p), ctypes.byref(iq_p),
                                               ctypes.byref(niq)))
        rows, outs, iq = None, {}, None
        if copy:
            rows = np.empty((nf, self.fft_size), np.float32)
            if nf:
                ctypes.memmove(rows.ctypes.data, rows_p.value, rows.nbytes)
            for vid in vfos:
                p, n = ctypes.c_void_p(), ctypes.c_int()
                check(lib.sdrgpu_frontend_collected_vfo(self._h, int(ticket), int(vid), ctypes.byref(p), ctypes.byref(n)))
                o = np.empty(n.value, np.complex64)
                if n.value:
                    ctypes.memmove(o.ctypes.data, p.value, o.nbytes)
                outs[vid] = o
            if niq.value:
                iq = np.empty(niq.value, np.complex64)
                ctypes.memmove(iq.ctypes.data, iq_p.value, iq.nbytes)
        check(lib.sdrgpu_frontend_release(self._h, int(ticket)))
        return rows, outs, iq

    def vfo_dev(self, vid):
        """(device pointer, count) of the VFO's output for the last push."""
        ptr, n = ctypes.c_void_p(), ctypes.c_int()
        check(lib.sdrgpu_frontend_vfo_dev(self._h, int(vid), ctypes.byref(ptr), ctypes.byref(n)))
        return ptr.value, n.value

    def vfo_output(self, vid):
        n = ctypes.c_int()
        check(lib.sdrgpu_frontend_vfo_dev(self._h, int(vid), None, ctypes.byref(n)))
        out = np.empty(n.value, np.complex64)
        if n.value:
            check(lib.sdrgpu_frontend_read_vfo(self._h, int(vid), _fptr(out), n.value))
        return out

    def close(self):
        if self._h:
            lib.sdrgpu_frontend_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Deemphasis(Block):
    """dsp::filter::Deemphasis<T> (filter/deephasis.h); stereo=True for stereo_t."""

    def __init__(self, tau, samplerate, stereo=False, device=0):
        h = _make(lib.sdrgpu_deemphasis_create, device, C64 if stereo else F32, float(tau), float(samplerate))
        super().__init__(h, STEREO if stereo else np.float32, STEREO if stereo else np.float32)


def gather_id():
    """Rank 0: a new RCCL communicator id (bytes) for SpectraGather."""
    buf = ctypes.create_string_buffer(128)
    check(lib.sdrgpu_gather_get_id(buf))
    return buf.raw


class SpectraGather:
    """Rank-0 gather of spectrum rows over RCCL (sdrgpu_gather_*): one rank per GPU / IQ stream."""

    def __init__(self, rank, world, comm_id, device=0, timeout=None):
        """device < 0: the calling thread's current HIP device. Every wait on the peers (this
        constructor, gather_dev, wait) has a deadline: `timeout` s, else SDRGPU_GATHER_TIMEOUT_S
        (default 120); on expiry the communicator is aborted and SdrGpuError names the rank."""
        assert len(comm_id) == 128
        self.rank, self.world = rank, world
        self._id = ctypes.create_string_buffer(bytes(comm_id), 128)
        self._h = _make(lib.sdrgpu_gather_create, int(device), int(rank), int(world), self._id)
        if timeout is not None:
            check(lib.sdrgpu_gather_set_timeout(self._h, float(timeout)))

    def gather_dev(self, rows_ptr, count, out_ptr, stream=None):
        """count device floats -> rank 0's out (world x count); asynchronous on `stream`."""
        check(lib.sdrgpu_gather_rows(self._h, _vp(rows_ptr), int(count), _vp(out_ptr or 0), _vp(stream or 0)))

    def wait(self, stream=None, timeout=0.0):
        """Wait for the gathers enqueued on `stream` against the deadline (timeout <= 0: the
        handle's); raises SdrGpuError (communicator aborted) when a peer never completes its part."""
        check(lib.sdrgpu_gather_wait(self._h, _vp(stream or 0), float(timeout)))

    def close(self):
        if self._h:
            lib.sdrgpu_gather_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Zoom:
    """fft_scaler::doZoom on device dB rows (gui/widgets/fft_scaler.h)."""

    def __init__(self, view_offset, view_bw, whole_bw, fft_size, out_size, device=0):
        self._h = _make(lib.sdrgpu_zoom_create, device, float(view_offset), float(view_bw), float(whole_bw), int(fft_size),
                        int(out_size))
        self.out_size = int(out_size)

    def execute_dev(self, rows_ptr, nrows, out_ptr, stream=None):
        return check(lib.sdrgpu_zoom_execute_dev(self._h, _vp(rows_ptr), int(nrows), _vp(out_ptr), _vp(stream or 0)))

    def __del__(self):
        try:
            if self._h:
                lib.sdrgpu_zoom_destroy(self._h)
        except Exception:
            pass


def low_pass(cutoff, trans, fs, odd=False):
    return _taps(lib.sdrgpu_taps_low_pass, float(cutoff), float(trans), float(fs), int(odd))


def high_pass(cutoff, trans, fs, odd=False):
    return _taps(lib.sdrgpu_taps_high_pass, float(cutoff), float(trans), float(fs), int(odd))


def band_pass(start, stop, trans, fs, odd=False, complex_taps=False):
    if complex_taps:
        n = check(lib.sdrgpu_taps_band_pass_c(float(start), float(stop), float(trans), float(fs), int(odd), None))
        t = np.empty(n, dtype=np.complex64)
        lib.sdrgpu_taps_band_pass_c(float(start), float(stop), float(trans), float(fs), int(odd), _fptr(t))
        return t
    return _taps(lib.sdrgpu_taps_band_pass_f, float(start), float(stop), float(trans), float(fs), int(odd))


def gen_reshape_params(fs, size, rate):
    skip, nz = ctypes.c_int(), ctypes.c_int()
    lib.sdrgpu_gen_reshape_params(float(fs), int(size), float(rate), ctypes.byref(skip), ctypes.byref(nz))
    return skip.value, nz.value


def decim_plan(ratio):
    d = (ctypes.c_int * 8)()
    n = (ctypes.c_int * 8)()
    t = (ctypes.POINTER(ctypes.c_float) * 8)()
    ns = check(lib.sdrgpu_decim_plan(int(ratio), d, n, t))
    return [(d[i], np.ctypeslib.as_array(t[i], shape=(n[i],)).copy()) for i in range(ns)]
