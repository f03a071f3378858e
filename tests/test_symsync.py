"""Symbol recovery on the device (libsdrgpu, HIP): FastAGC, Costas, MM, BinarySlicer,
DifferentialDecoder, and PSK / GFSK / the RDS chain composed of them, against numpy float32
restatements of the reference (tests/_restated.py: one scalar operation per reference operation, file:line
cited). The restatements themselves are held to the reference's own headers, compiled over scalar
stand-ins for VOLK and FFTW (oracle/ref_blocks.cpp), by tests/test_ref_blocks.py.

Bars:
* FastAGC, BinarySlicer, DifferentialDecoder, MM (count and every output) -- bit-exact. MM's
  interpolator dot product is VOLK's generic kernel: ascending taps, fp32, unfused.
* Costas -- the phasor is libm's cosf / sinf, which no two libms round alike. The restatement runs
  twice: with numpy's float32 cos / sin and with fp64 cos / sin rounded once to fp32. S = the largest
  gap between the two over 8 seeds of the configuration: the loop's own sensitivity to a last-bit
  change of the phasor. The device must be within 16 max(S, 4 eps32 max|y|) of the fp64-trig run (16:
  the device's libm is a third rounding of the same class and a loop amplifies differently per
  input). The bar never comes from the device's numbers. Recorded: profiles/r11/symsync_parity.json.
* PSK / GFSK / RDSBits -- bit-identical to the same blocks run one after another on the device.
* Known answers -- the restatement alone must recover the transmitted bits, then the device must.
* Every streaming test cuts its 12,000 samples into calls of [1, 6, 7, 8, 0, 1023, 1024, 1025, 4097,
  rest] (one sample, the T - 1 = 7 history edge, an empty call, the 1024-sample chunk edge) and
  requires the result bit-identical to a single call on a fresh handle.
"""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32
from _restated import (f32, N, CUTS, FL_M_PI, bits, same, ref_fast_agc, ref_costas, RefMM, ref_fir, ref_slicer, ref_diff,
                       shaped_psk, noise, parts, mm_input, W_RDS, COSTAS_CASES, costas_input, costas_ref_and_S, gfsk_signal,
                       GFSK_ARGS, rds_signal, RDS_CASES, errors_at_best_lag, quadrant, ref_rds_chain)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def in_calls(block, x):
    out, i = [], 0
    for c in CUTS:
        out.append(block.process(x[i:i + c]))
        i += c
    assert i == len(x) == N
    return np.concatenate(out)


def whole_and_cut(make, x, what):
    """One call on a fresh handle, and the same stream in CUTS on another: bit-identical. Returns it."""
    y = make().process(x)
    z = in_calls(make(), x)
    assert same(y, z), f"{what}: the stream in calls differs from one call"
    return y


# ------------------------------------------------------------------ FastAGC
@pytest.mark.parametrize("cplx", [False, True])
def test_fast_agc_bit_exact(cplx):
    x = shaped_psk(11, 4, amp=0.05)[0]
    x[5000:5100] = 0                                            # the gain runs into maxGain
    if not cplx:
        x = np.ascontiguousarray(x.real)
    args = (1.0, 50.0, 0.1, 2.0)                                # setPoint, maxGain, rate, initGain
    make = lambda: dsp.FastAGC(*args, complex_data=cplx)
    y = whole_and_cut(make, x, "fast_agc")
    xr, xi = parts(x)
    rr, ri, g_end = ref_fast_agc(xr, xi if cplx else None, 1.0, 50.0, 0.1, f32(2.0))
    ref = (rr[0] + 1j * ri[0]).astype(np.complex64) if cplx else rr[0]
    assert same(y, ref)
    assert np.any(np.abs(ref[5000:5100]) == 0) and g_end[0] != f32(2.0)
    # get_gain, set_gain (latched at the next call), reset -> initGain
    a = make()
    a.process(x[:3000])
    g3000 = ref_fast_agc(xr[:, :3000], xi[:, :3000] if cplx else None, 1.0, 50.0, 0.1, f32(2.0))[2][0]
    assert f32(a.get_gain()) == g3000
    a.set_gain(0.25)
    assert a.get_gain() == 0.25
    rr2, ri2, g2 = ref_fast_agc(xr[:, 3000:4000], xi[:, 3000:4000] if cplx else None, 1.0, 50.0, 0.1, f32(0.25))
    ref2 = (rr2[0] + 1j * ri2[0]).astype(np.complex64) if cplx else rr2[0]
    assert same(a.process(x[3000:4000]), ref2) and f32(a.get_gain()) == g2[0]
    a.reset()
    assert a.get_gain() == 2.0
    assert same(a.process(x[:1500]), ref[:1500])


# ---------------------------------------------- slicer, differential decoder
def test_binary_slicer_bit_exact():
    x = noise(5, False)
    x[::7] = 0.0
    x[3] = -0.0
    y = whole_and_cut(dsp.BinarySlicer, x, "slicer")
    assert y.dtype == np.uint8 and same(y, ref_slicer(x))


@pytest.mark.parametrize("modulus,init", [(2, 0), (4, 3)])
def test_differential_decoder_bit_exact(modulus, init):
    x = np.random.default_rng(modulus).integers(0, modulus, N).astype(np.uint8)
    make = lambda: dsp.DifferentialDecoder(modulus, init)
    y = whole_and_cut(make, x, "differential decoder")       # (the cuts carry the last symbol across calls)
    assert same(y, ref_diff(x, modulus, init))
    d = make()
    d.process(x[:100])
    d.reset()                                                   # last <- initSym
    assert same(d.process(x[100:300]), ref_diff(x[100:300], modulus, init))


# ----------------------------------------------------------------------- MM
MM_CASES = [(om, og, mg, 128, 8, kind)
            for om in (4.0, 5000.0 / 1187.5) for og, mg in ((2.5e-5, 0.01), (1e-6, 0.01)) for kind in ("psk", "noise")]
MM_CASES.append((4.0, 2.5e-5, 0.01, 4, 3, "psk"))


@pytest.mark.parametrize("cplx", [False, True])
def test_mm_count_and_outputs_bit_exact(cplx):
    for om, og, mg, P, T, kind in MM_CASES:
        what = f"mm cplx={cplx} omega={om} gains=({og}, {mg}) bank=({P}, {T}) {kind}"
        x = mm_input(kind, cplx)
        make = lambda: dsp.MM(om, og, mg, 0.01, P, T, complex_data=cplx)
        if T == 8:
            y = whole_and_cut(make, x, what)                    # (the cuts' history edge is T - 1 = 7)
        else:
            y = make().process(x)
        ref = RefMM(om, og, mg, 0.01, P, T, cplx).process(x)
        assert len(ref) > N / om * 0.98 - 2, what
        assert len(y) == len(ref), f"{what}: {len(y)} outputs, restatement {len(ref)}"
        assert same(y, ref), what


@pytest.mark.parametrize("cplx", [False, True])
def test_mm_reset_keeps_history_and_set_omega(cplx):
    x = mm_input("psk", cplx)
    args = (4.0, 2.5e-5, 0.01, 0.01)
    m, r = dsp.MM(*args, complex_data=cplx), RefMM(*args, cplx=cplx)
    assert m.out_count(777) == 777                              # the capacity, not the count
    assert same(m.process(x[:3001]), r.process(x[:3001]))
    m.reset()
    r.reset()                                                   # mm.h:87-98: the 7 history samples stay
    assert np.any(r.hr != 0)
    y, z = m.process(x[3001:6000]), r.process(x[3001:6000])
    assert same(y, z)
    fresh = RefMM(*args, cplx=cplx).process(x[3001:6000])
    assert not same(z[:2], fresh[:2]), "the history does not matter here: the check would show nothing"
    om2 = 5000.0 / 1187.5
    m.set_omega(om2)                                            # mm.h:40-50: offset, phase zeroed, freq and limits follow
    r.set_omega(om2)
    y, z = m.process(x[6000:]), r.process(x[6000:])
    assert same(y, z) and abs(len(z) - 6000 / om2) < 40
    with pytest.raises(sdrpp_amd.SdrGpuError):
        m.set_omega(1.0)                                        # an output would consume no input
    with pytest.raises(sdrpp_amd.SdrGpuError):
        m.set_gains(2.5e-5, 3.5)


# ------------------------------------------------------------------- Costas
@pytest.fixture(scope="module")
def costas_refs():
    """Per case: the fp64-trig restatement of seed 0's stream and S over the 8 seeds."""
    return {case: costas_ref_and_S(case) for case in COSTAS_CASES}


@pytest.mark.parametrize("case", sorted(COSTAS_CASES))
def test_costas_within_the_loops_own_sensitivity(case, costas_refs):
    c, r = COSTAS_CASES[case], costas_refs[case]
    kw = c["kw"]
    make = lambda: dsp.Costas(c["order"], c["bandwidth"], kw.get("init_phase", 0.0), kw.get("init_freq", 0.0),
                              kw.get("min_freq", -float(FL_M_PI)), kw.get("max_freq", float(FL_M_PI)))
    y = whole_and_cut(make, r["x"], case)
    ref = r["ref"]
    # the restatement locks: the loop output is the constellation, not a spinning copy of the input
    tail = ref[6000:]
    if case == "order2" or case == "rds_second_loop":
        assert np.mean(np.abs(tail.imag)) < 0.35 * np.mean(np.abs(tail.real)), "restatement did not lock"
    dev = float(max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max()))
    bar = 16 * max(r["S"], 4 * EPS32 * float(np.abs(ref).max()))
    print(f"costas {case}: S {r['S']:.3e}, device deviation {dev:.3e}, bar {bar:.3e}")
    assert dev <= bar
    # reset -> the initial phase and frequency
    m = make()
    m.process(r["x"][:2500])
    m.reset()
    assert same(m.process(r["x"][:2000]), y[:2000])


@pytest.mark.parametrize("order", [2, 4, 8])
def test_costas_zero_input_gives_exact_zeros(order):
    y = whole_and_cut(lambda: dsp.Costas(order, 0.005), np.zeros(N, np.complex64), "costas zeros")
    assert y.shape == (N,) and not np.any(bits(y) & np.uint64(0x7FFFFFFF7FFFFFFF))   # +-0 only


def test_costas_setters():
    x = costas_input("order2", 0)
    a, b = dsp.Costas(2, 0.005), dsp.Costas(2, 0.02, 0.0, 0.0, -0.5, 0.5)
    b.set_bandwidth(0.005)
    b.set_freq_limits(-float(FL_M_PI), float(FL_M_PI))
    assert same(a.process(x[:3000]), b.process(x[:3000]))


# ------------------------------------------------- composites are their parts
def run_parts(blocks, x):
    for b in blocks:
        x = b.process(x)
    return x


def test_psk_is_its_parts():
    x = shaped_psk(31, 4, amp=0.05)[0]
    make = lambda: dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)
    y = whole_and_cut(make, x, "psk")
    ps = [dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0)), dsp.FastAGC(1.0, 10e6, 0.01, complex_data=True),
          dsp.Costas(4, 0.005), dsp.MM(4.0, 2.5e-5, 0.01, 0.01, complex_data=True)]
    z = run_parts(ps, x)
    assert len(y) == len(z) and abs(len(y) - 3000) <= 2 and same(y, z)


def test_mm_setters_reach_the_chain():
    """The MM setters on a PSK handle act on the chain's last block (before the first sample here)."""
    x = shaped_psk(31, 4, amp=0.05)[0][:4000]
    p = dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)
    p.set_gains(1e-6, 0.02)
    p.set_omega_rel_limit(0.02)
    ps = [dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0)), dsp.FastAGC(1.0, 10e6, 0.01, complex_data=True),
          dsp.Costas(4, 0.005), dsp.MM(4.0, 1e-6, 0.02, 0.02, complex_data=True)]
    assert same(p.process(x), run_parts(ps, x))


def test_gfsk_is_its_parts():
    x = gfsk_signal()[0]
    y = whole_and_cut(lambda: dsp.GFSK(*GFSK_ARGS), x, "gfsk")
    ps = [dsp.Quadrature(2 * np.pi * 3000.0 / 48000.0), dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0), complex_data=False),
          dsp.MM(4.0, 2.5e-5, 0.01, 0.01)]
    z = run_parts(ps, x)
    assert y.dtype == f32 and len(y) == len(z) and same(y, z)


def rds_parts():
    w = W_RDS
    return [dsp.FastAGC(1.0, 1e6, 0.1, complex_data=True), dsp.Costas(2, float(f32(0.005))),
            dsp.FIR(dsp.band_pass(0, 2375, 100, 5000, complex_taps=True)),
            dsp.Costas(2, 0.01, 0.0, w, w - (w * 0.1), w + (w * 0.1))]


def test_rds_is_its_parts():
    x = rds_signal(*RDS_CASES[0])[0]
    y = whole_and_cut(dsp.RDSBits, x, "rds")
    r = dsp.RDSBits()
    assert same(r.process(x), y)
    soft = r.symbols()
    z = np.ascontiguousarray(run_parts(rds_parts(), x).real)                      # convert::ComplexToReal
    zs = dsp.MM(5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01).process(z)
    zb = run_parts([dsp.BinarySlicer(), dsp.DifferentialDecoder(2)], zs)
    assert y.dtype == np.uint8 and len(y) == len(zb) == len(soft)
    assert same(soft, zs) and same(y, zb)
    # the soft symbols of a later, shorter call, and of an empty one
    r.process(x[:500])
    assert abs(len(r.symbols()) - 500 / (5000.0 / 1187.5)) <= 2
    assert len(r.process(x[:0])) == 0 and len(r.symbols()) == 0


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("f0,snr_db,seed", RDS_CASES)
def test_rds_known_answer(f0, snr_db, seed):
    x, b = rds_signal(f0, snr_db, seed)
    ref_bits, ref_soft = ref_rds_chain(x)
    hi = min(len(b), len(ref_bits)) - 80
    e, lag = errors_at_best_lag(ref_bits, b, range(80), 600, hi)
    print(f"rds f0={f0} snr={snr_db}: restatement {e} errors at lag {lag} over {hi - 600} bits, {len(ref_soft)} symbols")
    assert e == 0, "the restatement alone does not recover the bits"
    r = dsp.RDSBits()
    y = r.process(x)
    assert abs(len(y) - len(ref_bits)) <= 1
    e, lag = errors_at_best_lag(y, b, range(80), 600, hi)
    print(f"rds f0={f0} snr={snr_db}: device {e} errors at lag {lag}")
    assert e == 0


def test_qpsk_known_answer():
    x, q = shaped_psk(61, 4, amp=0.05)
    dq = np.diff(q) % 4
    xr, xi = parts(x)
    h = dsp.root_raised_cosine(31, 0.6, 4.0)
    f = ref_fir(x, h)                                                             # psk.h:139
    fr, fi = parts(f)
    ar, ai, _ = ref_fast_agc(fr, fi, 1.0, 10e6, 0.01, f32(1.0))                  # psk.h:33, :140
    cr, ci = ref_costas(ar, ai, 4, 0.005)                                         # :34, :141
    sym = RefMM(4.0, 2.5e-5, 0.01, 0.01, cplx=True).process((cr[0] + 1j * ci[0]).astype(np.complex64))   # :35, :142
    e, lag = errors_at_best_lag(np.diff(quadrant(sym)) % 4, dq, range(40), 1000, 2800)
    print(f"qpsk: restatement {e} errors at lag {lag}, {len(sym)} symbols")
    assert e == 0, "the restatement alone does not recover the symbols"
    y = dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01).process(x)
    e, lag = errors_at_best_lag(np.diff(quadrant(y)) % 4, dq, range(40), 1000, 2800)
    print(f"qpsk: device {e} errors at lag {lag}, {len(y)} symbols")
    assert e == 0 and abs(len(y) - len(sym)) <= 1


def test_gfsk_known_answer():
    x, b = gfsk_signal()
    d = x[1:] * np.conj(x[:-1])
    q = np.concatenate([[np.angle(x[0])], np.angle(d)]) / (2 * np.pi * 3000.0 / 48000.0)   # quadrature.h:41-56
    h = dsp.root_raised_cosine(31, 0.6, 4.0)
    f = ref_fir(q.astype(f32), h)                                                 # gfsk.h:133
    soft = RefMM(4.0, 2.5e-5, 0.01, 0.01).process(f)                              # :134
    e, lag = errors_at_best_lag(ref_slicer(soft), b.astype(np.uint8), range(40), 1000, 2800)
    print(f"gfsk: restatement {e} errors at lag {lag}, {len(soft)} symbols")
    assert e == 0, "the restatement alone does not recover the bits"
    y = dsp.GFSK(*GFSK_ARGS).process(x)
    e, lag = errors_at_best_lag(ref_slicer(y), b.astype(np.uint8), range(40), 1000, 2800)
    print(f"gfsk: device {e} errors at lag {lag}, {len(y)} symbols")
    assert e == 0 and abs(len(y) - len(soft)) <= 1


# -------------------------------------------------------------- device path
def test_rds_bits_from_the_broadcast_fm_device_pointer():
    """BroadcastFM(stereo, RDS on) on an MPX-modulated IQ block; RDSBits fed the rds_dev device pointer
    on the same stream gives the bits RDSBits gives on the host copy from read_rds."""
    import ctypes
    import torch
    from sdrpp_amd import lib, check
    fs, n = 240000.0, 96000
    t = np.arange(n) / fs
    rng = np.random.default_rng(71)
    k = np.floor(1187.5 * t).astype(int)
    d = np.cumsum(rng.integers(0, 2, k.max() + 1)) % 2
    th = 2 * np.pi * 19000 * t
    mpx = 0.4 * np.sin(2 * np.pi * 1000 * t) + 0.1 * np.cos(th) + 0.05 * (2.0 * d[k] - 1.0) * np.sin(2 * np.pi * 1187.5 * t) * np.cos(3 * th)
    x = (0.5 * np.exp(1j * 2 * np.pi * 75000 * np.cumsum(mpx) / fs)).astype(np.complex64)
    fm = dsp.BroadcastFM(100000, fs, True, stereo=True, rds=True)
    s = torch.cuda.Stream()
    d_in = torch.from_numpy(x.view(f32).copy()).cuda()
    d_audio = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert fm.process_dev(d_in.data_ptr(), n, d_audio.data_ptr(), s.cuda_stream) == n
    ptr, cnt = ctypes.c_void_p(), ctypes.c_int()
    check(lib.sdrgpu_broadcast_fm_rds_dev(fm._h, ctypes.byref(ptr), ctypes.byref(cnt)))
    assert cnt.value == n * 5000 // 240000
    on_dev = dsp.RDSBits()
    m = on_dev.process_dev(ptr.value, cnt.value, d_bits.data_ptr(), s.cuda_stream)   # (returns after the stream)
    got = d_bits[:m].cpu().numpy()
    host = fm.rds_output()
    assert len(host) == cnt.value
    on_host = dsp.RDSBits()
    want = on_host.process(host)
    assert m == len(want) and abs(m - cnt.value / (5000.0 / 1187.5)) <= 2
    assert same(got, want) and same(on_dev.symbols(), on_host.symbols())
