"""GPU parity: libsdrgpu (HIP, gfx950) vs the CPU restatement (oracle/) on the same
seeded inputs. Every call goes through the C ABI (ctypes). Tolerances: tests/_util.py."""
import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import (EPS32, GOLDEN, assert_close_c, corpus_aggregate, corpus_ulp_rows, db_check, db_ulp_errors,
                   fir_atol, iq, ref32_fft_db, ulp_summary, write_report)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    n = sdrpp_amd.lib.sdrgpu_device_count()
    assert n > 0, "no HIP device visible: gpu tests need an MI355X"


# ------------------------------------------------------------------ spectrum
@pytest.mark.parametrize("N", [64, 256, 1024, 4096, 8192, 65536, 262144])
def test_fft_logmag_random(N, rng):
    x = iq(rng, N)
    w = oracle.create_window(6, N)
    f = dsp.FFTSpectrum(N, N, 6)
    db = f.logmag(x)
    truth = oracle.fft_truth_power(x, N, N, w)
    db_check(db, truth, N, ref32_fft_db(x, N, N, w))


def test_fft_logmag_1M_zero_pad(rng):
    # C2: fs 10 MS/s, fftRate 10 -> nz = 1,000,000, zero-padded to 2^20
    skip, nz = dsp.gen_reshape_params(10e6, 1 << 20, 10.0)
    assert (skip, nz) == (0, 1000000)
    N = 1 << 20
    x = iq(rng, nz)
    w = oracle.create_window(6, nz)
    f = dsp.FFTSpectrum(N, nz, 6)
    db = f.logmag(x)
    truth = oracle.fft_truth_power(x, nz, N, w)
    db_check(db, truth, N, ref32_fft_db(x, nz, N, w))


@pytest.mark.parametrize("N,k0,A", [(65536, 1000, 0.5), (4096, -77, 1.0), (1 << 20, 12345, 0.25)])
def test_fft_tone_unity_gain_centred(N, k0, A):
    # a bin-centred tone of amplitude A reads 20 log10 A at bin N/2 + k0 (unity coherent gain, centred)
    n = np.arange(N)
    x = (A * np.exp(2j * np.pi * k0 * n / N)).astype(np.complex64)
    f = dsp.FFTSpectrum(N, N, 6)
    db = f.logmag(x)
    k = N // 2 + k0
    assert int(np.argmax(db)) == k
    assert abs(db[k] - 20 * np.log10(A)) < 0.01


@pytest.mark.parametrize("wtype", range(7))
def test_fft_all_windows(wtype, rng):
    N = 16384
    x = iq(rng, N)
    w = oracle.create_window(wtype, N)
    f = dsp.FFTSpectrum(N, N, wtype)
    db = f.logmag(x)
    db_check(db, oracle.fft_truth_power(x, N, N, w), N, ref32_fft_db(x, N, N, w))


def test_fft_batch_dev_matches_host(rng):
    import torch
    N, frames, stride = 65536, 5, 70000       # skip = stride - N (reshaper keep/skip framing)
    x = iq(rng, stride * frames)
    f = dsp.FFTSpectrum(N, N, 6)
    xd = torch.from_numpy(x.view(np.float32)).cuda()
    out = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    f.execute_dev(xd.data_ptr(), stride, frames, out.data_ptr(), s)
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(frames, N)
    for i in range(frames):
        np.testing.assert_array_equal(o[i], f.logmag(x[i * stride:i * stride + N]))


def test_fft_aes17_fixture():
    # test_source AES17 14-bit table (source_modules/test_source/src/main.cpp:41-48), 16 samples/period
    g = np.load(GOLDEN + "/fft_aes17.npz")
    f = dsp.FFTSpectrum(int(g["N"]), int(g["N"]), 6)
    db = f.logmag(g["x"])
    truth = g["power_f64"]
    db_check(db, truth, int(g["N"]), g["db_ref32"])


# ----------------------------------------------------------------------- FIR
@pytest.mark.parametrize("ntaps,decim,cplx", [(1, 1, True), (91, 1, True), (228, 1, False), (256, 8, True),
                                                (143, 32, True), (27, 4, True), (69, 2, False), (726, 128, True),
                                                (5, 3, True), (33, 32, True), (256, 32, True), (200, 32, True)])
def test_fir_vs_oracle(ntaps, decim, cplx, rng):
    taps = rng.standard_normal(ntaps).astype(np.float32) / ntaps
    g = dsp.FIR(taps, decim, cplx)
    o = oracle.FIR(taps, decim, cplx)
    for n in [1000, 7, 50000, 0, 123457]:
        x = iq(rng, n) if cplx else rng.uniform(-1, 1, n).astype(np.float32)
        yo = o.process(x)
        yg = g.process(x)
        assert len(yg) == len(yo), (n, len(yg), len(yo))
        assert_close_c(yg, yo, fir_atol(taps, x) if n else 0, f"fir {ntaps}/{decim}")


def test_fir_rows_kernel_tap_change(rng):
    # D = 32 runs on the row-streaming kernel (2..8 taps per phase); a setTaps across a
    # taps-per-phase boundary keeps the history (fir.h:31-52) and resets the phase
    t1 = rng.standard_normal(143).astype(np.float32) / 143
    t2 = rng.standard_normal(230).astype(np.float32) / 230
    g, o = dsp.FIR(t1, 32, True), oracle.FIR(t1, 32, True)
    for taps in (t1, t2, t1):
        g.set_taps(taps)
        o.set_taps(taps)
        for n in [40000, 333, 70001]:
            x = iq(rng, n)
            yg, yo = g.process(x), o.process(x)
            assert len(yg) == len(yo)
            assert_close_c(yg, yo, fir_atol(taps, x), "rows FIR tap change")


def test_fir_complex_taps(rng):
    taps = dsp.band_pass(18750.0, 19250.0, 3000.0, 240000.0, True, True)   # WFM stereo pilot BPF, 305 taps
    assert len(taps) == 305
    g = dsp.FIR(taps, 1, True)
    o = oracle.FIR(taps, 1, True)
    for n in [4000, 1, 30001]:
        x = iq(rng, n)
        assert_close_c(g.process(x), o.process(x), fir_atol(taps, x), "complex-tap FIR")


def test_fir_block_split_invariance(rng):
    # splitting the stream into arbitrary counts yields the identical output stream (bit-exact)
    taps = dsp.low_pass(3.0e6, 912000.0, 61.44e6)
    x = iq(rng, 200000)
    a = dsp.FIR(taps, 8).process(x)
    g = dsp.FIR(taps, 8)
    cuts = np.sort(rng.choice(np.arange(1, len(x)), 40, replace=False))
    parts = [g.process(p) for p in np.split(x, cuts)]
    np.testing.assert_array_equal(np.concatenate(parts).view(np.uint32), a.view(np.uint32))


def test_fir_impulse_is_taps_correlation_order(rng):
    taps = rng.standard_normal(33).astype(np.float32)
    x = np.zeros(100, dtype=np.complex64)
    x[0] = 1
    y = dsp.FIR(taps, 1).process(x)
    # correlation (no tap reversal): y[i] = sum_j buf[i+j] h[j], buf = [32 zeros | x] -> y[i] = h[32 - i]
    np.testing.assert_array_equal(y[:33].real, taps[::-1])


def test_fir_set_taps_keeps_history(rng):
    t1 = rng.standard_normal(40).astype(np.float32)
    t2 = rng.standard_normal(17).astype(np.float32)
    g, o = dsp.FIR(t1, 3), oracle.FIR(t1, 3)
    x = iq(rng, 1000)
    assert_close_c(g.process(x), o.process(x), fir_atol(t1, x))
    g.set_taps(t2); o.set_taps(t2)
    x = iq(rng, 999)
    assert_close_c(g.process(x), o.process(x), fir_atol(t2, x))
    g.set_taps(t1); o.set_taps(t1)
    x = iq(rng, 555)
    assert_close_c(g.process(x), o.process(x), fir_atol(t1, x))


# ---------------------------------------------------------------- xlator/quad
def test_xlator_vs_fp64_nco(rng):
    w = 2 * np.pi * (-1.5e6 / 61.44e6)
    g, o = dsp.FrequencyXlator(w), oracle.Xlator(w)
    for n in [100000, 3, 777777]:
        x = iq(rng, n)
        assert_close_c(g.process(x), o.process(x), 2e-6, "xlator")


def test_xlator_long_run_phase_drift():
    # phase drift vs the fp64 NCO after 1e7 samples <= 1e-5 rad
    w = 2 * np.pi * (2.5e6 / 61.44e6)
    g = dsp.FrequencyXlator(w)
    x = np.ones(1_000_000, dtype=np.complex64)
    for _ in range(10):
        y = g.process(x)
    weff = oracle.lib.orc_xlator_effective_omega(w)
    n = 10_000_000 - 1
    ph_true = np.angle(np.exp(1j * np.fmod(weff * n, 2 * np.pi)))
    assert abs(np.angle(y[-1] * np.exp(-1j * ph_true))) < 1e-5


def test_quadrature_vs_oracle(rng):
    dev = 2 * np.pi * 100e3 / 7.68e6
    g, o = dsp.Quadrature(dev), oracle.Quadrature(dev)
    for n in [5000, 1, 77777]:
        x = iq(rng, n)
        assert_close_c(g.process(x), o.process(x), 1e-5 * (1 / dev), "quadrature")


# ------------------------------------------------------------ multirate
@pytest.mark.parametrize("ratio", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_power_decimator(ratio, rng):
    g, o = dsp.PowerDecimator(ratio), oracle.PowerDecimator(ratio)
    for n in [ratio * 50 + 3, 100000, 17]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        assert_close_c(yg, yo, 2e-5, f"power decim {ratio}")


@pytest.mark.parametrize("interp,decim", [(4, 5), (3, 2), (1, 7), (5, 4)])
def test_polyphase(interp, decim, rng):
    taps = dsp.low_pass(0.4 / max(interp, decim), 0.05 / max(interp, decim), 1.0) * interp
    g, o = dsp.PolyphaseResampler(interp, decim, taps), oracle.PolyphaseResampler(interp, decim, taps)
    for n in [1000, 13, 40000]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        assert_close_c(yg, yo, fir_atol(taps, x), "polyphase")


@pytest.mark.parametrize("ins,outs,cplx", [(240000, 48000, False), (61.44e6, 240000, True), (2.4e6, 48000, True),
                                           (48000, 44100, False), (8e6, 200000, True)])
def test_rational_resampler(ins, outs, cplx, rng):
    g, o = dsp.RationalResampler(ins, outs, cplx), oracle.RationalResampler(ins, outs, cplx)
    for n in [int(ins / 200), 5000, 123]:
        x = iq(rng, n) if cplx else rng.uniform(-1, 1, n).astype(np.float32)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        assert_close_c(yg, yo, 5e-5, "rational")


# ------------------------------------------------------------ VFO / demods
def test_rxvfo_c5(rng):
    g = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    o = oracle.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    for n in [307200, 307200, 1000, 999999]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        assert_close_c(yg, yo, 5e-5, "rxvfo")


_TAIL_CASES = [
    ("rxvfo", (61.44e6, 240000, 200000, 2.5e6)),     # plan 256 (32, 4, 2) + 91-tap LPF: 3 tail stages
    ("rxvfo", (61.44e6, 480000, 150000, -3.1e6)),    # plan 128 (16, 4, 2) + LPF
    ("rxvfo", (3.84e6, 60000, 60000, 1.7e5)),        # plan 64 (8, 4, 2), no LPF: 2 tail stages
    ("rxvfo", (61.44e6, 120000, 90000, 7e5)),        # plan 512 + LPF: 4 tail stages
    ("decim", (64,)),                                # PowerDecimator(64): no xlator
]
_TAIL_SIZES = [307200, 1, 5000, 31, 33333, 307200, 7, 100000, 1200000, 4099]


def _tail_block(kind, args):
    return dsp.RxVFO(*args) if kind == "rxvfo" else dsp.PowerDecimator(*args)


@pytest.mark.parametrize("kind,args", _TAIL_CASES)
def test_fir_tail_bit_identical_to_stage_launches(kind, args, monkeypatch, rng):
    """fir_tail_kernel (a chain's FIR stages 2.. in one launch for short calls, halos recomputed per
    workgroup) gives the per-stage fir_kernel launches' stream bit for bit, across ragged calls
    (single samples, calls with no output, calls past the tail's size limit that take the
    per-stage path, so the carried histories and decimation phases cross between the two paths).
    Stage-2 kernels default to the MFMA phase-split tiles for big calls; they are pinned to
    fir_kernel here (SDRGPU_FIR_MFMA_PS=0) so both paths run the same fmaf chain."""
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FIR_MFMA_PS", "0")
    a, b = _tail_block(kind, args), _tail_block(kind, args)
    x = iq(rng, sum(_TAIL_SIZES)) * (1.0 + 0.5j)
    pos, ya, yb = 0, [], []
    for k, n in enumerate(_TAIL_SIZES):
        blk = x[pos:pos + n]
        pos += n
        if k == 0:   # the tail switch is read at a chain's first call
            monkeypatch.setenv("SDRGPU_VFO_TAIL", "0")
            ya.append(a.process(blk))
            monkeypatch.setenv("SDRGPU_VFO_TAIL", "1")
            yb.append(b.process(blk))
        else:
            ya.append(a.process(blk))
            yb.append(b.process(blk))
        assert ya[-1].shape == yb[-1].shape, k
        assert np.array_equal(ya[-1].view(np.uint32), yb[-1].view(np.uint32)), (k, n, np.abs(ya[-1] - yb[-1]).max())


def test_fir_tail_rxvfo_vs_oracle(rng):
    """The default RxVFO path at the reference block size (one tail launch at every size)
    against the oracle, ragged calls switching between the tail and the per-stage path."""
    g = dsp.RxVFO(61.44e6, 120000, 90000, 7e5)
    o = oracle.RxVFO(61.44e6, 120000, 90000, 7e5)
    for n in [307200, 4099, 262144 * 2, 1, 307200]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        if len(yo):
            assert_close_c(yg, yo, 5e-5, "rxvfo 512")


def test_fir_tail_big_calls(rng, monkeypatch):
    """SDRGPU_VFO_TAIL=2 (the default): the VFO's later stages as one tail launch at every call size (thousands of
    workgroups on big calls, the per-(size, offsets) plan cached): against the oracle over ragged big
    and small calls; the spectrum launches' fused stage 1 + tail bit-identical to the separate path
    (both run the same tail); a 2^22-sample call's plan reused on the next equal call."""
    import torch
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_VFO_TAIL", "2")
    fs, off = 61.44e6, 2.5e6
    g = dsp.RxVFO(fs, 240000, 200000, off)
    o = oracle.RxVFO(fs, 240000, 200000, off)
    for n in [1 << 22, 1 << 22, 4099, 3 * 307200 + 17, 1 << 21]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        if len(yo):
            assert_close_c(yg, yo, 5e-5, f"rxvfo big tail n={n}")
    N, frames = 65536, 40
    fa, fb = dsp.FFTSpectrum(N, N, 6), dsp.FFTSpectrum(N, N, 6)
    va, vb = dsp.RxVFO(fs, 240000, 200000, off), dsp.RxVFO(fs, 240000, 200000, off)
    for _ in range(2):
        x = iq(rng, frames * N)
        d_x = torch.from_numpy(x.view(np.float32)).cuda()
        ra, rb = torch.empty(frames * N, device="cuda"), torch.empty(frames * N, device="cuda")
        oa, ob = torch.empty(2 * (frames * N // 256 + 64), device="cuda"), torch.empty(2 * (frames * N // 256 + 64), device="cuda")
        ma = fa.execute_vfo_dev(d_x.data_ptr(), frames, ra.data_ptr(), va, oa.data_ptr())
        fb.execute_dev(d_x.data_ptr(), N, frames, rb.data_ptr())
        mb = vb.process_dev(d_x.data_ptr(), frames * N, ob.data_ptr())
        torch.cuda.synchronize()
        assert ma == mb
        assert torch.equal(oa[:2 * ma], ob[:2 * mb])


def _quad_bound(y_ref, y_prev0, e_fir, inv_dev):
    """Per-sample bound on the quadrature output (quadrature.h:41-56) of an FIR output stream
    known to within e_fir (absolute) of y_ref: an error e in y_i turns arg(y_i) by at most
    ~e/|y_i|, so |d out_i| <= [2 (e/|y_i| + e/|y_i-1|) + 8 eps pi] / dev (factor 2 = slack on the
    first-order term; 8 eps pi covers atan2f and the fp32 conjugate product)."""
    y = np.asarray(y_ref, np.complex128)
    yp = np.concatenate([[y_prev0], y[:-1]])
    with np.errstate(divide="ignore"):
        b = 2.0 * (e_fir / np.abs(y) + e_fir / np.abs(yp)) + 8 * EPS32 * np.pi
    return b * inv_dev


def _wrapped_diff(a, b, inv_dev):
    """|a - b| for quadrature outputs, modulo the 2 pi / dev wrap of atan2."""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) / inv_dev
    return np.abs(np.angle(np.exp(1j * d))) * inv_dev


def test_ddc_c3_fir_stage(rng):
    """The C3 kernel's FIR stage (xlator fused into the load, 256 taps, D = 8, f32 MFMA) on its own,
    complex out: every output within fir_atol of the oracle's xlator -> fp64-accumulated FIR."""
    fs = 61.44e6
    taps = dsp.low_pass(3.0e6, 912000.0, fs)
    w = 2 * np.pi * (-1.5e6 / fs)
    g = dsp.DDC(w, taps, 8)
    ox, of = oracle.Xlator(w), oracle.FIR(taps, 8)
    for n in [307200, 12345, 8, 500000, 7, 1 << 20]:
        x = iq(rng, n)
        yo = of.process(ox.process(x))
        yg = g.process(x)
        assert len(yg) == len(yo)
        assert_close_c(yg, yo, fir_atol(taps, x) if n else 0, "C3 FIR stage")


def test_ddc_rows_zero_output_calls():
    """The row kernel with the fused xlator (D = 32, 143 taps: the RxVFO stage-1 shape) across calls
    that yield no output: calls two to four (7, 0 and 5 samples) fall inside the decimation phase
    left by the first, so their history is carried by fir_hist_kernel<float2, true> from the
    per-call NCO table while the row kernel (which forms its phasors itself) is the one selected.
    Output counts equal the oracle's on every call; every output within fir_atol of the oracle's
    xlator -> fp64-accumulated FIR. (A generator of its own: the session's one hands every later
    test the inputs it had before this test existed.)"""
    rng = np.random.default_rng(0x9D0C)
    taps = (rng.standard_normal(143) / 143).astype(np.float32)
    w = 2 * np.pi * (-2.5e6 / 61.44e6)
    g = dsp.DDC(w, taps, 32)
    ox, of = oracle.Xlator(w), oracle.FIR(taps, 32)
    counts = []
    for n in [1000, 7, 0, 5, 40000]:
        x = iq(rng, n)
        yo = of.process(ox.process(x))
        yg = g.process(x)
        assert len(yg) == len(yo), (n, len(yg), len(yo))
        counts.append(len(yg))
        if len(yo):
            assert_close_c(yg, yo, fir_atol(taps, x), f"rows DDC, call of {n}")
    assert counts[1:4] == [0, 0, 0] and counts[0] > 0 and counts[4] > 0, counts


def _quad64(y, yprev0, inv_dev):
    """fp64 quadrature (quadrature.h:41-56) of an FIR output stream."""
    y = np.asarray(y, np.complex128)
    yp = np.concatenate([[yprev0], y[:-1]])
    return np.angle(y * np.conj(yp)) * inv_dev


def test_ddc_fm_c3(rng):
    """C3 fused xlator -> 256-tap FIR /8 -> quadrature, every output checked three ways:
    1. the kernel's FIR stage (sdrgpu_ddc_create: the same fused kernel, complex out) is within
       fir_atol of the oracle's xlator -> fp64-accumulated FIR;
    2. the fused quadrature epilogue agrees with the fp64 quadrature of that FIR stage's output
       within _quad_bound(e = the FIR stage's measured error): the quadrature kernel tiles by 1023
       outputs, the plain one by 1024, so an output's MFMA tap grouping (hence its last bits)
       differs between the two, which matters only where |y| is small;
    3. against the oracle's own quadrature, each output lies within _quad_bound with e = 2x the
       FIR stage's measured error.
    A wrong output anywhere (e.g. one per 1024-output tile) fails 2 (and 1 if it is in the FIR)."""
    fs = 61.44e6
    taps = dsp.low_pass(3.0e6, 912000.0, fs)
    w = 2 * np.pi * (-1.5e6 / fs)
    dev = 2 * np.pi * 100e3 / (fs / 8)
    inv = 1.0 / dev
    g, gf = dsp.DDCFM(w, taps, 8, dev), dsp.DDC(w, taps, 8)
    ox, of, oq = oracle.Xlator(w), oracle.FIR(taps, 8), oracle.Quadrature(dev)
    yprev = gprev = 0j
    worst = {"fir_err": 0.0, "epilogue_over_bound": 0.0, "err_over_bound": 0.0}
    for n in [307200, 12345, 8, 500000, 7, 1 << 20]:
        x = iq(rng, n)
        yf = of.process(ox.process(x))
        yo = oq.process(yf)
        yg, ygf = g.process(x), gf.process(x)
        assert len(yg) == len(yo) == len(yf) == len(ygf)
        if len(yf) == 0:
            continue
        e_fir = max(float(np.abs(ygf.astype(np.complex128) - yf).max()), 1e-9)
        ep = _wrapped_diff(yg, _quad64(ygf, gprev, inv), inv) / _quad_bound(ygf, gprev, 2 * e_fir, inv)
        r = _wrapped_diff(yg, yo, inv) / _quad_bound(yf, yprev, 2 * e_fir, inv)
        worst["fir_err"] = max(worst["fir_err"], e_fir)
        worst["epilogue_over_bound"] = max(worst["epilogue_over_bound"], float(ep.max()))
        worst["err_over_bound"] = max(worst["err_over_bound"], float(r.max()))
        assert e_fir <= fir_atol(taps, x), (n, e_fir)
        assert ep.max() <= 1.0, (n, int(np.sum(ep > 1)), np.nonzero(ep > 1)[0][:5])
        assert r.max() <= 1.0, (n, int(np.sum(r > 1)), np.nonzero(r > 1)[0][:5])
        yprev, gprev = complex(yf[-1]), complex(ygf[-1])
    write_report("c3_quadrature_bound", {"test": "test_ddc_fm_c3", **worst})


@pytest.mark.parametrize("ntaps,quad", [(256, True), (256, False), (150, False), (190, True)])
def test_rows_kernel_d8_on_request(ntaps, quad, rng, monkeypatch):
    # fir_rows_kernel at D = 8 (taps per phase padded to 16/24/32, optional fused quadrature) is
    # selected only with SDRGPU_TUNING=1 SDRGPU_FIR_ROWS=2 (read at block creation); check it
    # against the oracle with the same per-sample bounds as the default C3 kernel
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FIR_ROWS", "2")
    fs = 61.44e6
    taps = dsp.low_pass(3.0e6, 912000.0, fs) if ntaps == 256 else (rng.standard_normal(ntaps) / ntaps).astype(np.float32)
    w = 2 * np.pi * (-1.5e6 / fs)
    dev = 2 * np.pi * 100e3 / (fs / 8)
    g = dsp.DDCFM(w, taps, 8, dev) if quad else dsp.FIR(taps, 8)
    ox, of, oq = oracle.Xlator(w), oracle.FIR(taps, 8), oracle.Quadrature(dev)
    yprev = 0j
    for n in [307200, 12345, 8, 500000]:
        x = iq(rng, n)
        if quad:
            yf = of.process(ox.process(x))
            yo, yg = oq.process(yf), g.process(x)
            assert len(yg) == len(yo)
            bound = _quad_bound(yf, yprev, fir_atol(taps, x), 1.0 / dev)
            err = _wrapped_diff(yg, yo, 1.0 / dev)
            assert np.all(err <= bound), (n, int(np.sum(err > bound)))
            yprev = complex(yf[-1])
        else:
            yo, yg = of.process(x), g.process(x)
            assert len(yg) == len(yo)
            assert_close_c(yg, yo, fir_atol(taps, x), "rows FIR D=8")


@pytest.mark.parametrize("nw", ["4", "2"])
@pytest.mark.parametrize("quad,xl", [(True, True), (False, True), (False, False)])
def test_mfma_half_phase_lds_bit_identical(nw, quad, xl, rng, monkeypatch):
    # fir_mfma_kernel HALF (SDRGPU_FIR_MFMA_HALF=1, read at block creation) stages half of the D
    # phases' span in LDS at a time: the same MFMA chains in the same order, so its outputs must
    # equal the default kernel's bit for bit, across calls (history, NCO phase, quadrature carry)
    fs = 61.44e6
    taps = dsp.low_pass(3.0e6, 912000.0, fs)
    w = 2 * np.pi * (-1.5e6 / fs)
    dev = 2 * np.pi * 100e3 / (fs / 8)

    def make():
        if quad:
            return dsp.DDCFM(w, taps, 8, dev)
        return dsp.DDC(w, taps, 8) if xl else dsp.FIR(taps, 8)
    # The same holds for DC (SDRGPU_FIR_MFMA_DC, the decimation as a compile-time constant): the
    # reference kernel here is the full-LDS, run-time-D one; both others must match it bit for bit
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FIR_MFMA_NW", nw)
    monkeypatch.setenv("SDRGPU_FIR_MFMA_HALF", "0")
    monkeypatch.setenv("SDRGPU_FIR_MFMA_DC", "0")
    g0 = make()
    monkeypatch.setenv("SDRGPU_FIR_MFMA_HALF", "1")
    g1 = make()
    monkeypatch.setenv("SDRGPU_FIR_MFMA_DC", "1")
    g2 = make()
    monkeypatch.setenv("SDRGPU_FIR_MFMA_HALF", "0")
    g3 = make()
    for n in [307200, 12345, 8, 1 << 20]:
        x = iq(rng, n)
        y0, y1, y2, y3 = g0.process(x), g1.process(x), g2.process(x), g3.process(x)
        assert len(y0) == len(y1) == len(y2) == len(y3)
        np.testing.assert_array_equal(y1, y0)
        np.testing.assert_array_equal(y2, y0)
        np.testing.assert_array_equal(y3, y0)


def test_registered_host_buffers_dma_directly(rng):
    # sdrgpu_host_register'ed in/out buffers take the direct-DMA path of the host process calls
    # (no staging copy); the results are identical to the staged path
    import ctypes
    lib = sdrpp_amd.lib
    taps = dsp.low_pass(3.0e6, 912000.0, 61.44e6)
    x = iq(rng, 300000)
    ref = dsp.FIR(taps, 8).process(x)
    xin = np.ascontiguousarray(x)
    yout = np.zeros(len(ref) + 16, dtype=np.complex64)
    for a in (xin, yout):
        assert lib.sdrgpu_host_register(ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0
    try:
        g = dsp.FIR(taps, 8)
        m = lib.sdrgpu_block_process(g._h, ctypes.c_void_p(xin.ctypes.data), len(xin), ctypes.c_void_p(yout.ctypes.data))
        assert m == len(ref)
        np.testing.assert_array_equal(yout[:m], ref)
        f = dsp.FFTSpectrum(65536, 65536, 6)
        db_ref = f.logmag(xin[:65536])
        db = np.zeros(65536, dtype=np.float32)
        assert lib.sdrgpu_host_register(ctypes.c_void_p(db.ctypes.data), ctypes.c_size_t(db.nbytes)) == 0
        assert lib.sdrgpu_fft_logmag(f._h, ctypes.c_void_p(xin.ctypes.data), ctypes.c_void_p(db.ctypes.data)) == 65536
        np.testing.assert_array_equal(db, db_ref)
        assert lib.sdrgpu_host_unregister(ctypes.c_void_p(db.ctypes.data)) == 0
    finally:
        for a in (xin, yout):
            assert lib.sdrgpu_host_unregister(ctypes.c_void_p(a.ctypes.data)) == 0


def test_fm_tone_demod_amplitude():
    # 1 kHz tone FM-modulated at 75 kHz deviation, demodulated with dev 100 kHz -> amplitude 0.75
    fs = 240000.0
    t = np.arange(240000) / fs
    phase = 2 * np.pi * 75e3 * np.cumsum(np.sin(2 * np.pi * 1e3 * t)) / fs
    x = np.exp(1j * phase).astype(np.complex64)
    y = dsp.Quadrature(2 * np.pi * 100e3 / fs).process(x)
    assert abs(np.max(y[1000:]) - 0.75) < 2e-3


def test_wfm_mono_vs_oracle(rng):
    g = dsp.BroadcastFM(100000, 240000)
    o = oracle.BroadcastFM(100000, 240000)
    for n in [1200, 4800, 1]:
        x = iq(rng, n)
        yo, yg = o.process(x), g.process(x)
        assert len(yg) == len(yo)
        assert np.abs(yg["l"] - yo["l"]).max() < 1e-3
        np.testing.assert_array_equal(yg["l"], yg["r"])


def test_wfm_short_call_launch_bit_exact(rng):
    """Calls of up to 32,768 samples run BroadcastFM mono as one launch (quadrature + audio FIR +
    LRToStereo, wfm_short_kernel); longer calls run the quadrature and FIR kernels. Same tap order
    and fmaf chain, same quadrature expression: the stream is bit-identical whichever way it is
    cut, including the state handed between the two paths (FIR history, y[-1])."""
    x = iq(rng, 200000)
    one = dsp.BroadcastFM(100000, 240000).process(x)            # one long call: two launches
    g = dsp.BroadcastFM(100000, 240000)
    cuts = [1200, 1, 255, 256, 257, 40000, 1200, 32768, 32769, 999]
    parts, i = [], 0
    for n in cuts:
        parts.append(g.process(x[i:i + n]))
        i += n
    parts.append(g.process(x[i:]))
    got = np.concatenate(parts)
    assert got.shape == one.shape
    for ch in ("l", "r"):
        assert np.array_equal(got[ch].view(np.uint32), one[ch].view(np.uint32)), ch


@pytest.mark.parametrize("stereo", [False, True])
def test_broadcast_fm_rds_branch(stereo):
    """BroadcastFM's RDS output (broadcast_fm.h:164-171, 193-203): MPX -> FrequencyXlator(-57 kHz)
    -> RationalResampler(240 k -> 5 k), over ragged blocks, vs the oracle's quadrature, xlator and
    rational resampler on the same input; the audio path is unchanged by the branch."""
    fs = 240000.0
    n = 60000
    t = np.arange(n) / fs
    bits = np.sign(np.sin(2 * np.pi * 1187.5 * t + 0.3))
    mpx = 0.45 * np.sin(2 * np.pi * 1000 * t) + 0.1 * np.sin(2 * np.pi * 19000 * t) + 0.05 * bits * np.cos(2 * np.pi * 57000 * t)
    x = np.exp(1j * 2 * np.pi * 75000 / fs * np.cumsum(mpx)).astype(np.complex64)
    g = dsp.BroadcastFM(100000, fs, True, stereo=stereo, rds=True)
    plain = dsp.BroadcastFM(100000, fs, True, stereo=stereo, rds=False) if stereo else None
    got, audio = [], []
    for a, b in [(0, 7001), (7001, 7002), (7002, 33333), (33333, n)]:
        audio.append(g.process(x[a:b]))
        got.append(g.rds_output())
        if plain is not None:
            np.testing.assert_array_equal(audio[-1].view(np.float32), plain.process(x[a:b]).view(np.float32))
    got = np.concatenate(got)
    mp = oracle.Quadrature(2 * np.pi * 100000 / fs).process(x)
    ref = oracle.RationalResampler(fs, 5000.0, True).process(oracle.Xlator(2 * np.pi * -57000 / fs).process(mp.astype(np.complex64)))
    assert len(got) == len(ref) > 1000
    # cascade bar (FIR / resamplers): 5e-5 of the input scale, here the MPX peak; the
    # quadrature's atan2f last bits (device vs host libm) and the NCO enter the same way
    err = np.abs(got - ref).max()
    assert err <= 5e-5 * np.abs(mp).max(), (err, np.abs(mp).max())
    g.set_rds(False)
    g.process(x[:1000])
    assert g.rds_output().size == 0


def test_fm_nfm_vs_oracle(rng):
    for lp, hp in [(True, False), (False, True), (True, True), (False, False)]:
        g = dsp.FM(48000, 12500, lp, hp)
        o = oracle.FM(48000, 12500, lp, hp)
        x = iq(rng, 9600)
        assert np.abs(g.process(x) - o.process(x)).max() < 1e-3


# -------------------------------------------------------------- converters
def test_converters_bit_exact():
    u8 = np.arange(256, dtype=np.uint8)
    i16 = np.arange(-32768, 32768, dtype=np.int16)
    i8 = np.arange(-128, 128, dtype=np.int8)
    rng = np.random.default_rng(7)
    i32 = np.concatenate([rng.integers(-2**31, 2**31, 200000, dtype=np.int64).astype(np.int32),
                          np.array([-2**31, 2**31 - 1, 0, -1], dtype=np.int32)])
    f64 = rng.standard_normal(100000)
    i24v = np.arange(-(1 << 23), 1 << 23, 37, dtype=np.int32)
    i24 = np.stack([(i24v & 0xff), (i24v >> 8) & 0xff, (i24v >> 16) & 0xff], axis=1).astype(np.uint8).ravel()
    for kind, x in [(0, u8), (1, i16), (2, i24), (3, i32), (4, f64), (5, i8)]:
        a = dsp.convert(kind, x)
        b = oracle.convert(kind, x)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"kind {kind}")


def test_fft_merged_chunks_match_separate_launches(rng, monkeypatch):
    """The 64k plan's merged pass-B(c) + pass-A(c+1) launches (several small chunks, a ragged
    last chunk) agree with separate pass-A / pass-B launches to 1e-3 dB (not bit for bit: the two
    kernels contract different products into FMAs), and every row meets the spectrum parity bar."""
    N, frames = 65536, 7
    x = iq(rng, N * frames)
    import torch
    d_x = torch.from_numpy(x.view(np.float32)).cuda()

    def rows():
        f = dsp.FFTSpectrum(N, N, 6)
        out = torch.empty(frames * N, dtype=torch.float32, device="cuda")
        f.execute_dev(d_x.data_ptr(), N, frames, out.data_ptr())
        torch.cuda.synchronize()
        f.close()
        return out.cpu().numpy()

    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "0")                # the two-pass 64k launches
    monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", "1")          # 2 frames per chunk -> 4 chunks, merged
    a = rows()
    monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", "64")
    monkeypatch.setenv("SDRGPU_FFT_MERGE", "0")
    b = rows()
    # same arithmetic; the merged kernel may contract a*b+c into FMAs at other places, so the
    # rows agree to the last bits rather than bit for bit, and every row meets the parity bar
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    w = oracle.create_window(6, N)
    for j in range(frames):
        xs = x[j * N:(j + 1) * N]
        db_check(a[j * N:(j + 1) * N], oracle.fft_truth_power(xs, N, N, w), N, ref32_fft_db(xs, N, N, w))


@pytest.mark.parametrize("nz", [40000, 65535])
def test_fft_64k_zero_pad_strided(nz, rng):
    """64k plan with nz < N (zero-padded columns) on frames read in place with a reshaper
    stride nz + skip: every row meets the spectrum parity bar."""
    import torch
    N, frames, skip = 65536, 3, 123
    stride = nz + skip
    x = iq(rng, stride * frames)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    f = dsp.FFTSpectrum(N, nz, 6)
    out = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    f.execute_dev(d_x.data_ptr(), stride, frames, out.data_ptr())
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    w = oracle.create_window(6, nz)
    for j in range(frames):
        xs = x[j * stride:j * stride + nz]
        db_check(rows[j * N:(j + 1) * N], oracle.fft_truth_power(xs, nz, N, w), N, ref32_fft_db(xs, nz, N, w))


@pytest.mark.parametrize("nz,stride", [(1000000, 1000000), (666667, 666667), (1000000, 1000000 + 4321)])
def test_fft_1m_batch_multi_chunk(nz, stride, rng):
    """C2's bench path: a 1M-point batch of 17 frames read in place at the reshaper stride (16-frame
    chunks -> 2 chunks, the last one ragged). Even strides take the paired (16-B) pass A, the odd
    one (fftRate 15 at 10 MS/s: nz = 666,667, iq_frontend.h:56-60) the one-column pass A. Every
    row meets the spectrum parity bar against the fp64 truth."""
    import torch
    N, frames = 1 << 20, 17
    x = iq(rng, stride * (frames - 1) + nz)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    f = dsp.FFTSpectrum(N, nz, 6)
    out = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    assert f.execute_dev(d_x.data_ptr(), stride, frames, out.data_ptr()) == frames
    torch.cuda.synchronize()
    rows = out.cpu().numpy().reshape(frames, N)
    w = oracle.create_window(6, nz)
    for j in range(frames):
        xs = x[j * stride:j * stride + nz]
        db_check(rows[j], oracle.fft_truth_power(xs, nz, N, w), N, ref32_fft_db(xs, nz, N, w))


@pytest.mark.parametrize("chunk_mb,frames", [(16, 5), (24, 7)])
def test_fft_1m_chunking_bit_identical(chunk_mb, frames, rng, monkeypatch):
    """The persistent 1M passes over several small chunks (2-3 frames each, a ragged last chunk, the
    resident grid larger than a chunk's tiles) give every row bit-identical to one whole-batch call:
    the chunking is part of no output's arithmetic."""
    import torch
    N, nz = 1 << 20, 1000000
    x = iq(rng, nz * frames)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    ref = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    got = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    dsp.FFTSpectrum(N, nz, 6).execute_dev(d_x.data_ptr(), nz, frames, ref.data_ptr())
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", str(chunk_mb))
    assert dsp.FFTSpectrum(N, nz, 6).execute_dev(d_x.data_ptr(), nz, frames, got.data_ptr()) == frames
    torch.cuda.synchronize()
    assert torch.equal(ref, got), float((ref - got).abs().max())


def test_process_dev_across_streams(rng):
    """A handle driven from two streams in turn (the NCO table, history and quadrature state are
    per handle) gives the same output stream as one stream: each call waits for the previous one."""
    import torch
    x = iq(rng, 400000)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    ref = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6).process(x)
    g = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = torch.zeros(2 * (len(ref) + 16), dtype=torch.float32, device="cuda")
    m, a = 0, 0
    for k, b in enumerate([50000, 50001, 123456, 300000, 400000]):
        s = (s1 if k % 2 == 0 else s2).cuda_stream
        m += g.process_dev(d_x.data_ptr() + 8 * a, b - a, out.data_ptr() + 8 * m, s)
        a = b
    torch.cuda.synchronize()
    assert m == len(ref)
    got = out[:2 * m].cpu().numpy().view(np.complex64)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_stream_destroyed_between_calls(rng):
    """a handle whose last call ran on a stream the caller then destroyed, called next on
    another stream (the first stream change synchronises the device instead of touching the dead
    stream; later changes wait on the end-of-call event), gives the one-stream output stream."""
    import ctypes
    import torch
    x = iq(rng, 300000)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    ref = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6).process(x)
    g = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    out = torch.zeros(2 * (len(ref) + 16), dtype=torch.float32, device="cuda")
    cuts = [0, 70001, 150000, 220000, 300000]
    m = 0
    for k in range(len(cuts) - 1):
        st = ctypes.c_void_p()
        sdrpp_amd.check(sdrpp_amd.lib.sdrgpu_stream_create(0, ctypes.byref(st)))
        m += g.process_dev(d_x.data_ptr() + 8 * cuts[k], cuts[k + 1] - cuts[k], out.data_ptr() + 8 * m, st.value)
        sdrpp_amd.check(sdrpp_amd.lib.sdrgpu_stream_destroy(st))   # gone before the next call
    torch.cuda.synchronize()
    assert m == len(ref)
    got = out[:2 * m].cpu().numpy().view(np.complex64)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


SPECTRUM_ULP_CASES = [("random", 4096, 4096), ("random", 65536, 65536), ("random", 1 << 20, 1000000),
                      ("tones", 65536, 65536), ("tones", 1 << 20, 1000000), ("aes17", 0, 0)]


@pytest.mark.parametrize("kind,N,nz", SPECTRUM_ULP_CASES)
def test_spectrum_ulp_distribution(kind, N, nz, rng):
    """The north_star's "<= 1 ulp on FFT magnitude", measured literally: the dB error in fp32 ulps of
    the correctly rounded truth (fp64 DFT of the same float-windowed frame), next to pocketfft's
    (scipy single precision, the FFTW-class CPU reference) on the same frame. No fp32 FFT reaches
    1 ulp on every bin; the assertion is that the GPU's distribution is in the same
    class as pocketfft's: median no worse, the fraction within 1 ulp within 3 points of its own,
    p99 within 2x (+1 ulp). The numbers go to the report (profiles/)."""
    if kind == "aes17":
        g = np.load(GOLDEN + "/fft_aes17.npz")
        N = nz = int(g["N"])
        x, truth = g["x"], g["power_f64"]
        w = oracle.create_window(6, N)
    else:
        if kind == "random":
            x = iq(rng, nz)
        else:
            n = np.arange(nz)
            x = (0.5 * np.exp(2j * np.pi * 0.1234567 * n) + 0.01 * np.exp(-2j * np.pi * 0.3 * n)).astype(np.complex64)
            x = (x + iq(rng, nz, 1e-4)).astype(np.complex64)
        w = oracle.create_window(6, nz)
        truth = oracle.fft_truth_power(x, nz, N, w)
    db = dsp.FFTSpectrum(N, nz, 6).logmag(x)
    e_gpu = db_ulp_errors(db, truth)
    e_ref = db_ulp_errors(ref32_fft_db(x, nz, N, w), truth)
    sg, sr = ulp_summary(e_gpu), ulp_summary(e_ref)
    write_report("spectrum_ulp", {"case": kind, "N": N, "nz": nz, "gpu": sg, "pocketfft_f32": sr})
    if sg["bins"] >= 1000:
        # full random frames: the distribution in pocketfft's class -- median no worse, the fraction
        # within 1 ulp within 3 points of its own, p99 within 2x (+1 ulp) -- and the absolute bars (the
        # literal north_star metric, stated rather than only relative): at least 97% of the bins within
        # 1 ulp (measured 98.2% at 64k, 99.2% at 1M), p50 0 ulp, the worst bin no more than 2x
        # pocketfft's worst (or 16 ulp): measured max 6 / 41 / 38 ulp vs pocketfft 10 / 28 / 77 at
        # 4k / 64k / 1M (r5h)
        assert sg["p50"] <= sr["p50"], (sg, sr)
        assert sg["frac_le_1ulp"] >= sr["frac_le_1ulp"] - 0.03, (sg, sr)
        assert sg["p99"] <= 2 * sr["p99"] + 1, (sg, sr)
        assert sg["p50"] == 0, sg
        assert sg["frac_le_1ulp"] >= 0.97, sg
        assert sg["max"] <= max(2 * sr["max"], 16), (sg, sr)
    else:
        # The tonal frames and the AES17 table have 17-22 bins within 60 dB of the peak: a relative bar
        # against pocketfft on one such frame is a coin flip, so the relative comparison is
        # made over the tonal corpus (test_spectrum_ulp_tonal_corpus). Here only absolute floors, so a
        # regression to the fp32-twiddle form (7 of AES17's 22 bins beyond 1 ulp) still fails: at least
        # 85% of the bins within 1 ulp (measured 2 of 22 / 2 of 17 / 1 of 18 beyond) and no bin past 8 ulp
        assert sg["frac_le_1ulp"] >= 0.85, sg
        assert sg["max"] <= 8, sg


def _tonal_frame(N, nz, k):
    """Frame k of the tonal corpus: a 0.5-amplitude tone and a -34 dB second tone at seed-dependent
    frequencies over a -80 dB uniform noise floor (the test_spectrum_ulp_distribution 'tones' kind)."""
    r = np.random.default_rng(0x70E5 + 7919 * k + N)
    n = np.arange(nz)
    f1 = 0.1234567 + 0.0371 * k + r.uniform(-1e-3, 1e-3)
    f2 = -0.3 + 0.0113 * k + r.uniform(-1e-3, 1e-3)
    x = (0.5 * np.exp(2j * np.pi * f1 * n) + 0.01 * np.exp(2j * np.pi * f2 * n)).astype(np.complex64)
    return (x + iq(r, nz, 1e-4)).astype(np.complex64)


def test_spectrum_ulp_tonal_corpus():
    """the few-bin frames judged over a corpus instead of one frame at a time. 16
    tonal 64k frames and 6 tonal 1M frames (nz = 1e6) at fixed seeds, plus the AES17 golden table; the
    64k frames through both 64k forms (sdrgpu_fft_set_kernel: one-pass, the bench's headline kernel,
    and two-pass, the per-block front end's). Pooled over a form's frames (302 / 302 / 107 bins within
    60 dB of each frame's peak, fp32 ulps of the correctly rounded dB of the exact DFT), against
    pocketfft single precision on the same frames. Measured (r7a, r7b; profiles/r6/tonal_corpus_*):
      form          p50   mean ulp (pocketfft)   bins > 1 ulp (pocketfft)   worst (pocketfft)
      64k one-pass  0     0.404 (0.368)          15 (10)                     2 (2)
      64k two-pass  0     0.503 (0.368)          24 (10)                     6 (2)
      1M            0     0.318 (0.364)           5 (3)                      2 (4)
    pocketfft is more accurate on these near-peak bins than both 64k forms; fp64 twiddle products in
    the one-pass kernel's stage 1 / stage 2 moved its count only to 13 / 12 at +1.7 / +7.6% kernel time
    (profiles/r6/c5_tw64_ab_r7b.txt), so they were not kept. The bars, fixed from these numbers (the
    per-frame bars no longer move): pooled median <= pocketfft's; mean ulp error <= 1.15x pocketfft's
    for the one-pass and 1M forms and <= 1.4x for the two-pass; the count beyond 1 ulp <= 1.6x
    pocketfft's + 1 (one-pass, 1M) and <= 2.5x (two-pass); the worst bin <= pocketfft's worst + 0 ulp
    (one-pass, 1M) and <= 3x (two-pass). The fp64-interior mode meets <= 1 ulp on every bin
    (test_spectrum_f64_within_1ulp). The report goes to profiles/ (spectrum_tonal_corpus)."""
    g = np.load(GOLDEN + "/fft_aes17.npz")
    frames = [("aes17", 65536, 65536, g["x"], g["power_f64"])]
    for k in range(16):
        x = _tonal_frame(65536, 65536, k)
        frames.append((f"tones{k}", 65536, 65536, x, None))
    for k in range(6):
        x = _tonal_frame(1 << 20, 1000000, k)
        frames.append((f"tones{k}", 1 << 20, 1000000, x, None))
    forms = {"64k-one-pass": (65536, "one-pass"), "64k-two-pass": (65536, "two-pass"), "1M": (1 << 20, None)}
    pools = {name: {"gpu": [], "ref": [], "frames": []} for name in forms}
    plans = {}
    for tag, N, nz, x, truth in frames:
        w = oracle.create_window(6, nz)
        if truth is None:
            truth = oracle.fft_truth_power(x, nz, N, w)
        e_ref = db_ulp_errors(ref32_fft_db(x, nz, N, w), truth)
        for name, (fN, mode) in forms.items():
            if fN != N:
                continue
            if name not in plans:
                plans[name] = dsp.FFTSpectrum(N, nz, 6)
                if mode:
                    plans[name].set_kernel(mode)
            e = db_ulp_errors(plans[name].logmag(x), truth)
            pools[name]["gpu"].append(e)
            pools[name]["ref"].append(e_ref)
            pools[name]["frames"].append({"frame": tag, "bins": int(e.size), "gpu_gt1": int(np.sum(e > 1.0)),
                                          "pocketfft_gt1": int(np.sum(e_ref > 1.0)), "gpu_max": float(e.max()),
                                          "pocketfft_max": float(e_ref.max())})
    summary = {}
    for name, pl in pools.items():
        eg, er = np.concatenate(pl["gpu"]), np.concatenate(pl["ref"])
        summary[name] = {"frames": len(pl["gpu"]), "bins": int(eg.size),
                         "gpu": {"p50": float(np.median(eg)), "mean": float(eg.mean()), "gt1": int(np.sum(eg > 1.0)),
                                 "max": float(eg.max())},
                         "pocketfft": {"p50": float(np.median(er)), "mean": float(er.mean()), "gt1": int(np.sum(er > 1.0)),
                                       "max": float(er.max())},
                         "per_frame": pl["frames"]}
    write_report("spectrum_tonal_corpus", summary)
    bars = {"64k-one-pass": (1.15, 1.6, 1, 1.0), "64k-two-pass": (1.4, 2.5, 0, 3.0), "1M": (1.15, 1.6, 1, 1.0)}
    for name, sm in summary.items():
        gs, rs = sm["gpu"], sm["pocketfft"]
        k_mean, k_gt1, c_gt1, k_max = bars[name]
        assert gs["p50"] <= rs["p50"], (name, gs, rs)
        assert gs["mean"] <= k_mean * rs["mean"], (name, gs, rs)
        assert gs["gt1"] <= k_gt1 * rs["gt1"] + c_gt1, (name, gs, rs)
        assert gs["max"] <= max(k_max * rs["max"], rs["max"]), (name, gs, rs)


def test_spectrum_ulp_corpus():
    """The spectrum's accuracy class over the seed-fixed corpus (4k / 16k / 64k x 7 windows x 24 random
    frames + 6 1M frames, _util.corpus_ulp_rows), per bin in fp32 ulps of the correctly rounded dB of
    the exact DFT, against pocketfft single precision on the same frames:
      * every frame: within-1-ulp fraction >= pocketfft's - 1 point (measured: -0.59 points at worst),
        p99.9 <= pocketfft's + 4 ulp (measured +3);
      * per size: the worst bin over the corpus <= 1.25x pocketfft's worst over the corpus (measured
        1.02 / 0.71 / 0.75 / 0.80), and the mean of the per-frame worst bins <= pocketfft's (0.92 /
        0.84 / 0.84 / 0.79: the GPU's worst bins are smaller on average);
      * the fp64-interior mode: every bin of every frame within 1 ulp.
    The literal "98% within 1 ulp, p99.9 <= 4 ulp" fails for pocketfft itself at 4k (97.7%, 7 ulp), so
    the bars are relative to it. A per-frame bound on the ratio of the two worst bins is a heavy-tailed
    statistic (31 of 168 4k frames exceed 1.25x for this kernel, 31 for the plain-C complex multiply
    build, while pocketfft's own worst bins exceed the GPU's on 62% of frames), so the worst-bin bar
    is taken over the corpus."""
    rows = corpus_ulp_rows()
    agg = corpus_aggregate(rows)
    write_report("spectrum_corpus", {"aggregate": agg})
    for r in rows:
        if r["bins"] >= 1000:
            assert r["gpu"]["frac_le_1ulp"] >= r["pocketfft"]["frac_le_1ulp"] - 0.01, r
            assert r["gpu"]["p999"] <= r["pocketfft"]["p999"] + 4.0, r
        assert r["f64_max"] <= 1.0, r
    for N, a in agg.items():
        assert a["gpu_max"] <= 1.25 * a["pocketfft_max"], (N, a)
        assert a["gpu_mean_frame_max"] <= a["pocketfft_mean_frame_max"], (N, a)


# ------------------------------------------- fp64-interior spectrum (parity mode)
F64_CASES = [("random", 64, 64), ("random", 4096, 4096), ("random", 8192, 8192), ("random", 65536, 65536),
             ("random", 1 << 20, 1000000), ("tones", 65536, 65536), ("tones", 1 << 20, 1000000),
             ("random", 65536, 40000), ("aes17", 0, 0)]


@pytest.mark.parametrize("kind,N,nz", F64_CASES)
def test_spectrum_f64_within_1ulp(kind, N, nz, rng):
    """sdrgpu_fft_set_precision(h, 1): the north_star's "<= 1 ulp on FFT magnitude" literally. Every
    bin within 200 dB of the frame's peak is within 1 fp32 ulp of the correctly rounded dB of the
    fp64 DFT (numpy) of the same float-windowed frame, and all but a few in 10^4 are exact (the two
    fp64 evaluations differ by ~1e-15 relative; only a value that close to a rounding boundary can
    round the other way)."""
    if kind == "aes17":
        g = np.load(GOLDEN + "/fft_aes17.npz")
        N = nz = int(g["N"])
        x, truth = g["x"], g["power_f64"]
    else:
        if kind == "random":
            x = iq(rng, nz)
        else:
            n = np.arange(nz)
            x = (0.5 * np.exp(2j * np.pi * 0.1234567 * n) + 0.01 * np.exp(-2j * np.pi * 0.3 * n)).astype(np.complex64)
            x = (x + iq(rng, nz, 1e-4)).astype(np.complex64)
        truth = oracle.fft_truth_power(x, nz, N, oracle.create_window(6, nz))
    f = dsp.FFTSpectrum(N, nz, 6, precision="f64")
    assert f.precision == "f64"
    db = f.logmag(x)
    e = db_ulp_errors(db, truth, floor_db=200.0)
    s = ulp_summary(e)
    exact = float(np.mean(e == 0))
    # exactness is asked of the bins within 160 dB of the peak. Below that an fp64 evaluation's own
    # error (~eps64 x the frame's energy) reaches the fp32 dB rounding boundaries: the AES17 table -- a
    # quantised tone over a -200 dB floor -- rounds 0.15% of its bins the other way (r4b, all of them
    # deep), and an independent fp64 four-step evaluation of it disagrees with numpy's on 4% of its bins,
    # every one below -160 dB and none above (tools/f64_calibration.py, profiles/r4/f64_calibration_aes17.json)
    t64 = 10.0 * np.log10(np.maximum(np.asarray(truth, np.float64), 1e-300))
    near = (t64[t64 >= t64.max() - 200.0] >= t64.max() - 160.0)
    exact160 = float(np.mean(e[near] == 0))
    write_report("spectrum_ulp_f64", {"case": kind, "N": N, "nz": nz, "gpu_f64": s, "frac_exact": exact,
                                      "bins_160dB": int(near.sum()), "frac_exact_160dB": exact160})
    assert s["max"] <= 1.0, s
    assert exact160 >= 0.9999, (s, exact160)
    f.set_precision("f32")   # back to the fp32 kernels: same plan, FFTW-class bar
    assert f.precision == "f32"
    e32 = db_ulp_errors(f.logmag(x), truth)
    # (few bins: the absolute floor of test_spectrum_ulp_distribution; the relative comparison with
    # pocketfft is made over the tonal corpus, test_spectrum_ulp_tonal_corpus)
    assert np.mean(e32 <= 1.0) >= (0.97 if e32.size >= 1000 else 0.85)


@pytest.mark.parametrize("N,nz,stride,frames", [(65536, 65536, 65536, 300), (65536, 50000, 61000, 9),
                                                (1 << 20, 1000000, 1000000, 17), (1 << 20, 666667, 700001, 3),
                                                (4096, 4096, 4100, 33)])
def test_spectrum_f64_batch(N, nz, stride, frames, rng):
    """Batched fp64-interior transforms: several 128 MB chunks (64k: 64 frames per chunk), ragged last
    chunk, zero padding, odd strides. Every row is bit-identical to the same frame transformed alone,
    and the first / last rows are within 1 ulp of the fp64 truth."""
    import torch
    x = iq(rng, stride * (frames - 1) + nz)
    f = dsp.FFTSpectrum(N, nz, 6, precision="f64")
    xd = torch.from_numpy(x.view(np.float32)).cuda()
    out = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    # the row count comes back from every plan size (the single-kernel sizes returned 0)
    assert f.execute_dev(xd.data_ptr(), stride, frames, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == frames
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(frames, N)
    w = oracle.create_window(6, nz)
    for j in sorted({0, 1, frames // 2, frames - 1}):
        xs = x[j * stride:j * stride + nz]
        np.testing.assert_array_equal(o[j], f.logmag(xs))
        if j in (0, frames - 1):
            assert db_ulp_errors(o[j], oracle.fft_truth_power(xs, nz, N, w)).max() <= 1.0


def test_spectrum_f64_zoom_rows(rng):
    """execute_zoom_dev in fp64 mode: the dB rows are the fp64 ones and the zoom rows (unfused) are
    the oracle's doZoom of them."""
    import torch
    N, frames, zw = 65536, 5, 2048
    x = iq(rng, N * frames)
    f = dsp.FFTSpectrum(N, N, 6, precision="f64")
    xd = torch.from_numpy(x.view(np.float32)).cuda()
    rows = torch.empty(frames * N, dtype=torch.float32, device="cuda")
    zoom = torch.empty(frames * zw, dtype=torch.float32, device="cuda")
    f.execute_zoom_dev(xd.data_ptr(), N, frames, rows.data_ptr(), zoom.data_ptr(), zw,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = rows.cpu().numpy().reshape(frames, N)
    z = zoom.cpu().numpy().reshape(frames, zw)
    for j in range(frames):
        np.testing.assert_array_equal(r[j], f.logmag(x[j * N:(j + 1) * N]))
        np.testing.assert_array_equal(z[j], oracle.zoom(r[j], 0.0, 1.0, 1.0, zw))


# ------------------------------------------------- spectrum + VFO fused read
def _fused_vs_separate(frames_list, pre, rng, zoom=False, between=None):
    """sdrgpu_fft_execute_vfo_dev / _zoom_vfo_dev (the VFO's first stage inside the spectrum launches)
    against the same batches through sdrgpu_fft_execute_dev / _zoom_dev + RxVFO.process_dev, and the
    VFO stream (ragged plain calls mixed with batch calls: non-zero decimation phase and history at a
    batch call) against the oracle. The fused launches run the same tile and segment code as the
    separate ones (only the cache policy of pass A's input loads and the stage's row batch differ,
    neither of which touches an output's arithmetic), so rows, zoom rows and VFO output are
    bit-identical to the separate launches. `between` {k: (method, args...)}: a setter or reset issued on
    both VFO handles and on the oracle's ahead of batch k."""
    import torch
    N, zw = 65536, 2048
    fs, off = 61.44e6, 2.5e6
    fused_vfo, sep_vfo = dsp.RxVFO(fs, 240000, 200000, off), dsp.RxVFO(fs, 240000, 200000, off)
    ovfo = oracle.RxVFO(fs, 240000, 200000, off)
    fa, fb = dsp.FFTSpectrum(N, N, 6), dsp.FFTSpectrum(N, N, 6)
    ya, yb, yo = [], [], []
    if pre:   # a ragged plain call first: non-zero decimation phase and a history at the fused call
        x0 = iq(rng, pre)
        ya.append(fused_vfo.process(x0)); yb.append(sep_vfo.process(x0)); yo.append(ovfo.process(x0))
    for k, frames in enumerate(frames_list):
        if between and k in between:
            for v in (fused_vfo, sep_vfo, ovfo):
                getattr(v, between[k][0])(*between[k][1:])
        x = iq(rng, frames * N)
        d_x = torch.from_numpy(x.view(np.float32)).cuda()
        ra = torch.empty(frames * N, device="cuda")
        rb = torch.empty(frames * N, device="cuda")
        za = torch.empty(frames * zw, device="cuda")
        zb = torch.empty(frames * zw, device="cuda")
        cap = frames * N // 256 + 64
        va = torch.empty(2 * cap, device="cuda")
        vb = torch.empty(2 * cap, device="cuda")
        if zoom:
            ma = fa.execute_zoom_vfo_dev(d_x.data_ptr(), frames, ra.data_ptr(), za.data_ptr(), zw, fused_vfo, va.data_ptr())
            fb.execute_zoom_dev(d_x.data_ptr(), N, frames, rb.data_ptr(), zb.data_ptr(), zw)
        else:
            ma = fa.execute_vfo_dev(d_x.data_ptr(), frames, ra.data_ptr(), fused_vfo, va.data_ptr())
            fb.execute_dev(d_x.data_ptr(), N, frames, rb.data_ptr())
        mb = sep_vfo.process_dev(d_x.data_ptr(), frames * N, vb.data_ptr())
        torch.cuda.synchronize()
        assert ma == mb
        assert torch.equal(ra, rb), float((ra - rb).abs().max())
        if zoom:
            assert torch.equal(za, zb)
        w = oracle.create_window(6, N)
        rows = ra.cpu().numpy().reshape(frames, N)
        for j in {0, frames - 1}:
            xs = x[j * N:(j + 1) * N]
            db_check(rows[j], oracle.fft_truth_power(xs, N, N, w), N, ref32_fft_db(xs, N, N, w))
        ya.append(va[:2 * ma].cpu().numpy().view(np.complex64))
        yb.append(vb[:2 * mb].cpu().numpy().view(np.complex64))
        yo.append(ovfo.process(x))
    ya, yb, yo = (np.concatenate(v) for v in (ya, yb, yo))
    assert len(ya) == len(yb) == len(yo)
    np.testing.assert_array_equal(ya.view(np.uint64), yb.view(np.uint64))
    assert_close_c(ya, yo, 5e-5, "fused VFO vs oracle")


def _two_pass(monkeypatch):
    """The 64k plan's two-pass launches (fft_vfo_kernel group: the round-4 form, kept as the
    SDRGPU_FFT_1P=0 alternative to the one-pass transform)."""
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "0")


@pytest.mark.parametrize("frames_list,pre", [([8], 0), ([3, 5], 1000), ([1, 2], 307200), ([257], 77)])
def test_spectrum_vfo_fused(frames_list, pre, rng, monkeypatch):
    _two_pass(monkeypatch)
    _fused_vs_separate(frames_list, pre, rng)


@pytest.mark.parametrize("frames_list,pre,chunk_mb", [([8], 0, None), ([9, 4], 1001, 1), ([1, 3], 31, 1), ([3], 0, 2)])
def test_spectrum_zoom_vfo_fused(frames_list, pre, chunk_mb, rng, monkeypatch):
    """The C5 launch group (rows + zoom rows + the VFO's first stage in one set of launches): 1 MB
    chunks (2 frames per chunk: first pass-A launch, merged launches, last pass-B launch with the
    history workgroup) and single-chunk calls."""
    _two_pass(monkeypatch)
    if chunk_mb:
        monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", str(chunk_mb))
    _fused_vs_separate(frames_list, pre, rng, zoom=True)


@pytest.mark.parametrize("frames_list,pre,chunk_mb", [([13], 0, None), ([9, 4], 1001, 1), ([21], 77, 8)])
def test_spectrum_vfo_fused_xcd(frames_list, pre, chunk_mb, rng, monkeypatch):
    """The fused launch order (each XCD's workgroups take a frame's 4 stage-1 quarters, then its 8
    column tiles, after the pass-B tiles) at frame counts that are not multiples of 8 (padding
    workgroups of the last group of 8 frames) and 1 / 8 MB chunks (merged launches): rows, zoom rows
    and VFO output bit-identical to the separate launches."""
    _two_pass(monkeypatch)
    if chunk_mb:
        monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", str(chunk_mb))
    _fused_vs_separate(frames_list, pre, rng, zoom=True)


@pytest.mark.parametrize("plan", ["one-pass", "two-pass"])
def test_spectrum_vfo_fused_retune_and_reset(plan, rng, monkeypatch):
    """RxVFO::setOffset, then reset, between two-frame batches of the fused launches, after a ragged plain
    call: set_offset rewrites the NCO tables of the VFO's fused first stage, which the spectrum launches
    read themselves, and reset clears its history, decimation phase and NCO phase. Rows, zoom rows and
    VFO output stay bit-identical to the separate launches given the same calls, and the VFO stream within
    the bar of the oracle (pinned to the reference's setOffset and reset by test_ref_chain.py) given the
    same calls, on the one-pass plan and on the two-pass plan."""
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1" if plan == "one-pass" else "0")
    _fused_vs_separate([2, 2, 2], 1000, rng, zoom=True, between={1: ("set_offset", -1.5e6), 2: ("reset",)})


# ------------------------------------------------- the one-pass 64k spectrum (fft_1p_kernel)
@pytest.mark.parametrize("nz,skip,frames", [(65536, 0, 9), (40000, 123, 3), (65535, 7, 2), (65536, 0, 150),
                                             (50000, 3, 70), (65536, 1, 5)])
def test_spectrum_onepass_rows_and_zoom(nz, skip, frames, rng, monkeypatch):
    """The one-pass 64k transform (four 16k sub-transforms per frame, radix-4 decimation in frequency,
    two workgroups per frame with two sub-transforms each; SDRGPU_FFT_1P; at 70 / 150 frames more
    workgroups than CUs, and a ragged last group of 8 frames): every row meets the spectrum parity bar against the fp64 truth and
    pocketfft on the same frame, zero-padded frames (nz < N) and reshaper strides included; the zoom
    rows (the two workgroups' partial maxima folded) equal fft_scaler's doZoom of the row bit for bit; and the rows
    agree with the two-pass kernels to the last bits near the peak."""
    import torch
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    N, zw = 65536, 2048
    stride = nz + skip
    x = iq(rng, stride * (frames - 1) + nz)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    out = torch.empty(frames * N, device="cuda")
    z = torch.empty(frames * zw, device="cuda")
    ref = torch.empty(frames * N, device="cuda")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1")
    f = dsp.FFTSpectrum(N, nz, 6)
    assert f.execute_zoom_dev(d_x.data_ptr(), stride, frames, out.data_ptr(), z.data_ptr(), zw) == frames
    monkeypatch.setenv("SDRGPU_FFT_1P", "0")
    dsp.FFTSpectrum(N, nz, 6).execute_dev(d_x.data_ptr(), stride, frames, ref.data_ptr())
    torch.cuda.synchronize()
    rows = out.cpu().numpy().reshape(frames, N)
    d = np.abs(rows - ref.cpu().numpy().reshape(frames, N))
    # near the peak (within 40 dB: a form's fp32 error relative to a bin grows as the bin falls below the
    # frame's level, and 60 dB below a noise frame's peak two fp32 forms drew 5.4e-3 dB apart in r7y / r7z)
    assert d.max() <= 0.05 and np.all(d[rows >= rows.max(axis=1, keepdims=True) - 40] <= 1e-3), d.max()
    w = oracle.create_window(6, nz)
    zr = z.cpu().numpy().reshape(frames, zw)
    # every frame's zoom row; the fp64-truth bar on every frame of short calls and on the frames at the
    # persistent grid's step boundaries (64 frames per step) of long ones
    full = range(frames) if frames <= 16 else sorted({0, 1, 7, 8, 63, 64, 65, frames // 2, frames - 2, frames - 1})
    for j in range(frames):
        np.testing.assert_array_equal(zr[j], oracle.zoom(rows[j], 0.0, 1.0, 1.0, zw))
    for j in full:
        xs = x[j * stride:j * stride + nz]
        db_check(rows[j], oracle.fft_truth_power(xs, nz, N, w), N, ref32_fft_db(xs, nz, N, w))


@pytest.mark.parametrize("frames_list,pre", [([13], 1000), ([3, 8], 0), ([130, 67], 77)])
def test_spectrum_onepass_vfo(frames_list, pre, rng, monkeypatch):
    """The C5 group as ONE launch (SDRGPU_FFT_1P): each of a frame's two workgroups runs half of the
    VFO's first stage, then its two 16k sub-transforms. Rows and zoom rows bit-identical to the one-pass
    spectrum without the VFO, the VFO output bit-identical to RxVFO.process_dev and within the oracle
    bar (_fused_vs_separate)."""
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1")
    _fused_vs_separate(frames_list, pre, rng, zoom=True)


@pytest.mark.parametrize("zsize,precision", [(1800, "f32"), (4096, "f32"), (2048, "f64")])
def test_spectrum_zoom_vfo_unfused(zsize, precision, rng):
    """execute_zoom_vfo_dev where nothing fuses (a zoom width other than N / 32, or the fp64 plan): the
    spectrum launch group, the zoom kernel over the rows, then the whole VFO on the call's stream. Rows
    bit-equal to execute_dev of a second plan, every zoom row bit-equal to fft_scaler's doZoom of its
    row, and the VFO's output (after a ragged plain call: non-zero decimation phase and history) equal
    in count and bits to a second RxVFO's process_dev."""
    import torch
    N, frames = 65536, 3
    fs, off = 61.44e6, 2.5e6
    va, vb = dsp.RxVFO(fs, 240000, 200000, off), dsp.RxVFO(fs, 240000, 200000, off)
    x0 = iq(rng, 1000)
    ya, yb = [va.process(x0)], [vb.process(x0)]
    x = iq(rng, frames * N)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    rows = torch.empty(frames * N, device="cuda")
    ref = torch.empty(frames * N, device="cuda")
    z = torch.empty(frames * zsize, device="cuda")
    cap = frames * N // 256 + 64
    oa = torch.empty(2 * cap, device="cuda")
    ob = torch.empty(2 * cap, device="cuda")
    f = dsp.FFTSpectrum(N, N, 6, precision=precision)
    ma = f.execute_zoom_vfo_dev(d_x.data_ptr(), frames, rows.data_ptr(), z.data_ptr(), zsize, va, oa.data_ptr())
    assert dsp.FFTSpectrum(N, N, 6, precision=precision).execute_dev(d_x.data_ptr(), N, frames, ref.data_ptr()) == frames
    mb = vb.process_dev(d_x.data_ptr(), frames * N, ob.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(rows, ref)
    r = rows.cpu().numpy().reshape(frames, N)
    zr = z.cpu().numpy().reshape(frames, zsize)
    for j in range(frames):
        np.testing.assert_array_equal(zr[j], oracle.zoom(r[j], 0.0, 1.0, 1.0, zsize))
    assert ma == mb
    ya.append(oa[:2 * ma].cpu().numpy().view(np.complex64))
    yb.append(ob[:2 * mb].cpu().numpy().view(np.complex64))
    ya, yb = np.concatenate(ya), np.concatenate(yb)
    assert len(ya) == len(yb)
    np.testing.assert_array_equal(ya.view(np.uint64), yb.view(np.uint64))


@pytest.mark.parametrize("kernel", ["auto", "one-pass"])
def test_spectrum_tail_stream_bit_identical(kernel, rng):
    """sdrgpu_fft_set_tail_stream: the VFO's later stages and the zoom fold on a second stream,
    overlapping the next call's one-pass launch (their inputs double-buffered per call parity). Over
    five calls -- one-pass calls of both parities, a short call that takes the two-pass path, a zoom-less
    call -- the rows, zoom rows and the VFO output stream are bit-identical to the same calls on one
    stream, and the VFO continues correctly on a plain process_dev call afterwards. With the kernel
    pinned to "one-pass" the 8-frame call stays on the one-pass kernel, where its tail is no big-call
    tail: inside tail-stream mode it falls through to the same-stream sequence."""
    import torch
    N, zw = 65536, 2048
    fs, off = 61.44e6, 2.5e6
    plan = [70, 66, 8, 70, 65]
    xs = [iq(rng, n * N) for n in plan]
    xt = iq(rng, 307200)
    res = {}
    for mode in ("one", "tail"):
        f = dsp.FFTSpectrum(N, N, 6)
        if kernel != "auto":
            assert f.set_kernel(kernel) == "auto"
        v = dsp.RxVFO(fs, 240000, 200000, off)
        s = torch.cuda.Stream()
        ts = torch.cuda.Stream() if mode == "tail" else None
        if ts is not None:
            f.set_tail_stream(ts.cuda_stream)
        rows, zooms, vouts = [], [], []
        for k, (n, x) in enumerate(zip(plan, xs)):
            d_x = torch.from_numpy(x.view(np.float32)).cuda()
            torch.cuda.synchronize()
            r = torch.empty(n * N, device="cuda")
            z = torch.empty(n * zw, device="cuda") if k != 3 else None
            vo = torch.empty(2 * (n * N // 256 + 64), device="cuda")
            m = f.execute_zoom_vfo_dev(d_x.data_ptr(), n, r.data_ptr(), z.data_ptr() if z is not None else 0, zw, v,
                                       vo.data_ptr(), s.cuda_stream)
            rows.append(r); zooms.append(z); vouts.append((vo, m, d_x))
        d_t = torch.from_numpy(xt.view(np.float32)).cuda()
        torch.cuda.synchronize()
        vt = torch.empty(2 * 2000, device="cuda")
        mt = v.process_dev(d_t.data_ptr(), 307200, vt.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        res[mode] = ([r.cpu().numpy() for r in rows], [z.cpu().numpy() if z is not None else None for z in zooms],
                     np.concatenate([vo[:2 * m].cpu().numpy() for vo, m, _ in vouts] + [vt[:2 * mt].cpu().numpy()]))
        if ts is not None:
            f.set_tail_stream(None)
    a, b = res["one"], res["tail"]
    for k in range(len(plan)):
        np.testing.assert_array_equal(a[0][k], b[0][k])
        if a[1][k] is not None:
            np.testing.assert_array_equal(a[1][k], b[1][k])
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    ovfo = oracle.RxVFO(fs, 240000, 200000, off)
    yo = np.concatenate([ovfo.process(x) for x in xs] + [ovfo.process(xt)])
    assert_close_c(b[2].view(np.complex64), yo, 5e-5, "tail-stream VFO vs oracle")


def test_spectrum_64k_rows_vs_call_size(rng):
    """the 64k plan's default (sdrgpu_fft_set_kernel mode 2) runs the one-pass kernel on
    calls of >= 64 frames and the two-pass launches below, so the same frames give different bits as a
    64-frame call and as a 63 + 1 split. The bound sdrgpu.h states holds at the switch point (<= 0.05 dB
    anywhere, <= 1e-3 dB within 40 dB of the frame's peak), and pinning the form per plan (mode 1 or 0)
    makes every row independent of the call size, bit for bit."""
    import torch
    N, frames = 65536, 64
    x = iq(rng, N * frames)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()

    def rows(f, split):
        out = torch.empty(frames * N, device="cuda")
        f0 = 0
        for n in split:
            assert f.execute_dev(d_x.data_ptr() + 8 * N * f0, N, n, out.data_ptr() + 4 * N * f0) == n
            f0 += n
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(frames, N)

    f = dsp.FFTSpectrum(N, N, 6)
    auto64, auto63 = rows(f, [64]), rows(f, [63, 1])
    assert not np.array_equal(auto64, auto63)   # (the two forms really ran)
    d = np.abs(auto64 - auto63)
    near = auto64 >= auto64.max(axis=1, keepdims=True) - 40
    assert d.max() <= 0.05 and d[near].max() <= 1e-3, (d.max(), d[near].max())
    for mode in ("one-pass", "two-pass"):
        assert f.set_kernel(mode) in ("auto", "one-pass")
        a, b = rows(f, [64]), rows(f, [63, 1])
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, auto64 if mode == "one-pass" else auto63)
    w = oracle.create_window(6, N)
    for j in (0, 63):
        xs = x[j * N:(j + 1) * N]
        db_check(auto63[j], oracle.fft_truth_power(xs, N, N, w), N, ref32_fft_db(xs, N, N, w))


# ------------------------------------------------- waterfall zoom fused into the spectrum
@pytest.mark.parametrize("frames,chunk_mb,zsize", [(3, None, 2048), (9, 1, 2048), (4, None, 1800), (5, 1, 4096)])
def test_spectrum_zoom_rows(frames, chunk_mb, zsize, rng, monkeypatch):
    """sdrgpu_fft_execute_zoom_dev: the dB rows are those of execute_dev, and every zoom row equals
    fft_scaler(0, bw, bw, N, zoomSize).doZoom of its dB row (oracle restatement of
    gui/widgets/fft_scaler.h:27-64) bit for bit -- fused in the last pass at 2048 (single launch and
    merged chunk launches), as a separate kernel for other widths."""
    import torch
    if chunk_mb:
        _two_pass(monkeypatch)
        monkeypatch.setenv("SDRGPU_FFT_CHUNK_MB", str(chunk_mb))   # 2 frames per chunk -> merged launches
    N = 65536
    x = iq(rng, N * frames)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    f = dsp.FFTSpectrum(N, N, 6)
    rows = torch.empty(frames * N, device="cuda")
    ref = torch.empty(frames * N, device="cuda")
    z = torch.empty(frames * zsize, device="cuda")
    assert f.execute_zoom_dev(d_x.data_ptr(), N, frames, rows.data_ptr(), z.data_ptr(), zsize) == frames
    dsp.FFTSpectrum(N, N, 6).execute_dev(d_x.data_ptr(), N, frames, ref.data_ptr())
    torch.cuda.synchronize()
    r = rows.cpu().numpy().reshape(frames, N)
    d = np.abs(r - ref.cpu().numpy().reshape(frames, N))
    assert d.max() <= 0.05 and np.all(d[r >= r.max(axis=1, keepdims=True) - 60] <= 1e-3)
    zr = z.cpu().numpy().reshape(frames, zsize)
    for j in range(frames):
        np.testing.assert_array_equal(zr[j], oracle.zoom(r[j], 0.0, 1.0, 1.0, zsize))
