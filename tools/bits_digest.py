"""Digest of the bits a build produces on fixed inputs (GPU): equal digests from two builds
(SDRGPU_LIB_PATH) show an A/B change kept every output bit.

  python tools/bits_digest.py            -> one JSON line {case: sha256[:16]}

Cases: RxVFO (C5: 61.44 MHz -> 240 kHz) over ragged host calls; BroadcastFM mono on one big call; the C5 launch group (spectrum rows,
zoom rows, VFO stage-1 + later stages) over 24 frames; the standalone spectrum over 24 frames; the fp64-interior
spectrum (64k over 300 frames, 1M over 3); the channel-chain kernels none of these reach (chain_cases); the serial
loops, the demodulators built on them, the IF noise reduction blocks and the channelizer (loop_cases)."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    import torch
    from sdrpp_amd import dsp
    rng = np.random.default_rng(1234)
    out = {}

    def h(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

    x = (rng.uniform(-1, 1, 24 * 65536 + 4099) + 1j * rng.uniform(-1, 1, 24 * 65536 + 4099)).astype(np.complex64)
    v = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    ys = [v.process(p) for p in np.split(x, [307200, 307201, 1000000])]
    out["rxvfo_host"] = h(np.concatenate(ys))

    N, F, ZW = 65536, 24, 2048
    d_x = torch.from_numpy(x[:F * N].view(np.float32)).cuda()
    rows = torch.empty(F * N, device="cuda")
    zoom = torch.empty(F * ZW, device="cuda")
    vo = torch.empty(2 * (F * N // 256 + 64), device="cuda")
    fft = dsp.FFTSpectrum(N, N, 6)
    vfo = dsp.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    m = fft.execute_zoom_vfo_dev(d_x.data_ptr(), F, rows.data_ptr(), zoom.data_ptr(), ZW, vfo, vo.data_ptr())
    torch.cuda.synchronize()
    out["c5_rows"] = h(rows.cpu().numpy())
    out["c5_zoom"] = h(zoom.cpu().numpy())
    out["c5_vfo"] = h(vo[:2 * m].cpu().numpy())
    w = dsp.BroadcastFM(100000, 240000, True)   # a 1,048,576-sample call: wfm_big_kernel
    out["wfm_big"] = h(w.process(x[:1 << 20]).view(np.uint32))
    r2 = torch.empty(F * N, device="cuda")
    dsp.FFTSpectrum(N, N, 6).execute_dev(d_x.data_ptr(), N, F, r2.data_ptr())
    torch.cuda.synchronize()
    out["spectrum_rows"] = h(r2.cpu().numpy())
    # the fp64-interior mode: 300 64k frames (three chunks, several pass-B tiles per workgroup) and 3 1M frames
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    for n, nz, f in ((65536, 65536, 300), (1 << 20, 1000000, 3)):
        xs = torch.rand(2 * nz * f, device="cuda", generator=g) * 2 - 1
        r = torch.empty(n * f, device="cuda")
        dsp.FFTSpectrum(n, nz, 6, precision="f64").execute_dev(xs.data_ptr(), nz, f, r.data_ptr())
        torch.cuda.synchronize()
        out[f"spectrum_f64_{n}"] = h(r.cpu().numpy())
    chain_cases(out, h)
    loop_cases(out, h)
    print(json.dumps(out))


def chain_cases(out, h):
    """The channel-chain kernels the cases above do not reach, each over 400,000 samples in ragged host
    calls of 100,001 / 0 (empty) / 1 (no output at any decimation >= 2: the history kernel) / 150,005 /
    149,993 samples."""
    from sdrpp_amd import dsp
    rng = np.random.default_rng(4321)
    x = (rng.uniform(-1, 1, 400000) + 1j * rng.uniform(-1, 1, 400000)).astype(np.complex64)
    cuts = [100001, 100001, 100002, 250007]

    def run(block, data):
        return h(np.concatenate([block.process(p) for p in np.split(data, cuts)]).view(np.uint32))

    fs = 61.44e6
    w = 2 * np.pi * (-1.5e6 / fs)
    c3 = dsp.low_pass(3.0e6, 912000.0, fs)   # the 256-tap C3 low-pass

    def rt(n):
        return (rng.standard_normal(n) / n).astype(np.float32)

    out["ddcfm_d8_256"] = run(dsp.DDCFM(w, c3, 8, 2 * np.pi * 100e3 / (fs / 8)), x)   # fir_mfma_kernel + quadrature
    out["ddc_d8_256"] = run(dsp.DDC(w, c3, 8), x)                                     # fir_mfma_kernel
    out["ddc_d4_27"] = run(dsp.DDC(w, rt(27), 4), x)                                  # fir_mfma_ps_kernel
    out["fir_real_d2_69"] = run(dsp.FIR(rt(69), 2, complex_data=False), x.real.copy())   # fir_kernel<float, float>
    out["fir_ctaps_d3_305"] = run(dsp.FIR(rt(305) + 1j * rt(305), 3), x)              # fir_kernel<float2, float2>
    out["fir_d128_726"] = run(dsp.FIR(rt(726), 128), x)                               # tile search: shrinking branch
    out["poly_3_2"] = run(dsp.PolyphaseResampler(3, 2, rt(96)), x)
    wfm = dsp.BroadcastFM(100000, 240000, True)   # 1,200-sample calls: wfm_short_kernel
    out["wfm_short"] = h(np.concatenate([wfm.process(p) for p in np.split(x[:3177], [1200, 2400, 2400])]).view(np.uint32))
    codes = rng.integers(-32768, 32768, 4096).astype(np.int16)
    out["convert_i16"] = h(dsp.convert(1, codes))
    out["convert_mono_i16"] = h(dsp.convert_mono(1, codes))


def loop_cases(out, h):
    """loops.hip, ifnr.hip and channelizer.hip: each block over 300,000 samples in ragged host calls of
    70,001 / 0 (empty) / 1 / 1,024 / 120,003 / 108,971 samples (the serial blocks walk 1024-sample chunks);
    the channelizers over 48 M + 333 / 0 / 1 / 17 M - 5 samples."""
    from sdrpp_amd import dsp
    rng = np.random.default_rng(8765)
    n = 300000
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    env = np.repeat(10.0 ** rng.uniform(-3, 0, n // 500 + 1), 500)[:n].astype(np.float32)
    xb = (x * env).astype(np.complex64)          # level steps over 60 dB, a silent gap, spikes: every AGC /
    xb[n // 3:n // 3 + 700] = 0                  # blanker branch runs
    xb[rng.integers(0, n, 40)] *= 50
    cuts = np.cumsum([70001, 0, 1, 1024, 120003])

    def run(block, data, view=np.uint32):
        return h(np.concatenate([np.ascontiguousarray(block.process(p)) for p in np.split(data, cuts)]).view(view))

    agc = (1.0, 50.0 / 48000, 5.0 / 48000, 10e6, 10.0, float("inf"))
    out["agc_f32"] = run(dsp.AGC(*agc, complex_data=False), xb.real.copy())
    out["agc_c64"] = run(dsp.AGC(*agc, complex_data=True), xb)
    out["dcb_c64"] = run(dsp.DCBlocker(10.0 / 48000, True), (x + np.complex64(0.3 + 0.2j)).astype(np.complex64))
    st = np.zeros(n, dsp.STEREO)
    st["l"], st["r"] = x.real, x.imag
    out["deemp_stereo"] = run(dsp.Deemphasis(50e-6, 48000, True), st)
    out["noise_blanker"] = run(dsp.NoiseBlanker(500.0 / 24000.0, 10.0), xb)
    fs = 48000.0
    out["am_mode1"] = run(dsp.AM(1, 10000.0, 50.0 / fs, 5.0 / fs, 10.0 / fs, fs), (0.05 * xb).astype(np.complex64))
    out["ssb_mode0_agc"] = run(dsp.SSB(0, 2800.0, 24000.0, True, 50.0 / 24000, 5.0 / 24000), (0.2 * xb).astype(np.complex64))
    # BroadcastFM stereo with RDS at 240 kS/s: a pilot, L - R on the 38 kHz subcarrier, a 57 kHz RDS-like carrier
    fm_fs = 240000.0
    t = np.arange(n) / fm_fs
    mpx = (0.45 * np.sin(2 * np.pi * 1000 * t) * (1 + np.cos(2 * np.pi * 38000 * t)) + 0.1 * np.cos(2 * np.pi * 19000 * t)
           + 0.05 * np.sign(np.sin(2 * np.pi * 1187.5 * t)) * np.cos(2 * np.pi * 57000 * t))
    iqfm = (0.5 * np.exp(2j * np.pi * 75000 * np.cumsum(mpx) / fm_fs) + 1e-3 * x).astype(np.complex64)
    bfm = dsp.BroadcastFM(100000, fm_fs, True, stereo=True, rds=True)
    audio, rds = [], []
    for p in np.split(iqfm, cuts):
        audio.append(np.ascontiguousarray(bfm.process(p)))
        rds.append(bfm.rds_output())
    out["bfm_stereo_audio"] = h(np.concatenate(audio).view(np.uint32))
    out["bfm_stereo_rds"] = h(np.concatenate(rds).view(np.uint32))
    for bins in (15, 32):
        out[f"fmif_b{bins}"] = run(dsp.FMIF(bins), x)
    # Squelch at -30 dB over calls at -6 / -60 / -6 dB: mutes on the first quiet call, unmutes after ten loud ones
    sq = dsp.Squelch(-30.0)
    lv = [0.5] * 2 + [1e-3] * 3 + [0.5] * 13
    out["squelch_step"] = h(np.concatenate([sq.process((g * x[k * 4099:(k + 1) * 4099]).astype(np.complex64))
                                            for k, g in enumerate(lv)]).view(np.uint32))
    for M, dft in ((256, "fft"), (1024, "fft"), (1024, "gemm")):
        taps = (rng.standard_normal(16 * M - 7) / (16 * M)).astype(np.float32)
        ch = dsp.PolyphaseChannelizer(M, taps, dft=dft)
        ccuts = np.cumsum([48 * M + 333, 0, 1])
        ys = [ch.process(p) for p in np.split(x[:48 * M + 333 + 1 + 17 * M - 5], ccuts)]
        out[f"chan_{M}_{dft}"] = h(np.concatenate(ys).view(np.uint32))


if __name__ == "__main__":
    main()
