"""Throughput bench for the MI355X streaming-DSP hot path (BASELINE.json metric).

Default workload (--config c5, one stream per GPU): BASELINE config C5's per-GPU slice,
i.e. a 61.44 MS/s-class IQ stream pushed as fast as the GPU takes it through
  * the IQ front end's spectrum: 65,536-point BH7 window * FFT * 10log10|X|^2, frames
    back to back (fftRate = fs/N -> skip 0), each row also zoomed to the waterfall's 2048
    display columns (fft_scaler doZoom, full span), and
  * one VFO: RxVFO(61.44 MHz -> 240 kHz, bw 200 kHz, offset +2.5 MHz; plan_256 + 91-tap
    LPF) -> BroadcastFM mono (dev 100 kHz, 228-tap audio LPF) -> stereo_t,
with every frame's display row gathered to rank 0 over RCCL each step (N > 1; libsdrgpu's
C-ABI gather on its own stream, overlapping the next step).
A step = one batch of B synthetic complex-float IQ samples resident in HBM
(uniform [-1, 1), SpeedTester distribution). Other configs: c2 (1M-point BH7 spectrum,
nz = 1e6, zero-padded), c3 (xlator + 256-tap FIR /8 + FM quadrature, fused), c4 (1024-channel
polyphase channelizer, 16384-tap prototype).

A plain run sets up --config, warms up, times the K steps and prints one JSON line (value, ms_per_step, the
dominant group's roofline from the timed steps' own events); --dump-outputs DIR also writes what the last timed
step computed. --full adds everything that takes runs of its own: the other configs, the per-call figures, the
spectrum ulp report and fp64-mode cost, the CPU baselines and the speed-ups against them.

Launch: python bench.py [--gpus N --steps K --warmup W]. N > 1 either under torch.distributed.run
(WORLD_SIZE must equal N) or directly: the parent then starts N rank processes itself before anything
touches the GPU (launch_ranks) and exits with the first failing rank's status.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c5", choices=["c5", "c2", "c3", "c4", "c4g"])
    ap.add_argument("--log2-batch", type=int, default=28, help="IQ samples per GPU per step = 2^k (c5/c3)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed config also: the other single-GPU configs, the per-call figures, the live "
                         "spectrum ulp report and fp64-mode cost, and the CPU baselines with the speed-ups against them "
                         "(a plain run times --config only and prints its line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step of --config computed to DIR/<name>.npy "
                         "(float32; arrays over 2^23 elements as a fixed seeded sample; at most 64 MB in all)")
    ap.add_argument("--cpu-seconds", type=float, default=6.0, help="per CPU-baseline leg (1-core, all-core; --full)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--no-sub", action="store_true", help="--full without the other configs and the per-call figures")
    ap.add_argument("--no-ulp", action="store_true", help="--full without the live spectrum ulp report and fp64-mode cost")
    ap.add_argument("--runtime", default="hip", choices=["hip", "cpu-rehearsal"],
                    help="cpu-rehearsal: the same launch / gather / timing control flow on the CPU over gloo with a "
                         "C5-shaped CPU stand-in workload (tests only; its line says so and is no measurement)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv, grace_s=None):
    """The parent of an N-GPU run started as `python bench.py --gpus N` (no WORLD_SIZE in the env):
    start N fresh rank processes of this script -- RANK = LOCAL_RANK = r, WORLD_SIZE = N,
    MASTER_ADDR 127.0.0.1 and a free port, the launcher torch.distributed.run would give them --
    and wait for them. The parent itself never touches HIP (it has not imported torch or the
    library when this runs), so the children are the only GPU processes. Rank 0 prints the JSON
    line on the inherited stdout. When a rank exits non-zero the others get `grace_s` (the gather
    deadline + 60 s: the survivors end through their own deadline first) and are then killed; the
    parent exits with the first failing rank's status. (Mirrors the reference's harness running
    independent block chains side by side, core/src/dsp/bench/speed_tester.h:31-56.)"""
    if grace_s is None:
        grace_s = float(os.environ.get("SDRGPU_BENCH_GRACE_S") or
                        float(os.environ.get("SDRGPU_GATHER_TIMEOUT_S", "120")) + 60.0)
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__)] + list(argv), env=env))
    first_bad, t_bad = None, None
    while True:
        codes = [p.poll() for p in procs]
        for r, c in enumerate(codes):
            if c not in (None, 0) and first_bad is None:
                first_bad, t_bad = (r, c), time.monotonic()
                print(f"bench.py: rank {r} exited with status {c}; waiting up to {grace_s:.0f} s for the other "
                      "ranks", file=sys.stderr, flush=True)
        if all(c is not None for c in codes):
            break
        if first_bad is not None and time.monotonic() - t_bad > grace_s:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            for p in procs:
                p.wait()
            break
        time.sleep(0.05)
    if first_bad is not None:
        r, c = first_bad
        return c if c > 0 else 128 - c   # a signal (-k) as the shell reports it
    return 0


def _launch_or_continue(argv):
    """Decides, before any GPU-touching import, whether this process is a rank or the parent of N."""
    a = parse(argv)
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != a.gpus:
            print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={ws}: refusing to time a different number of GPUs "
                  "than asked", file=sys.stderr, flush=True)
            sys.exit(2)
        return
    if a.gpus > 1:
        sys.exit(launch_ranks(a.gpus, argv))
    if a.gpus < 1:
        print(f"bench.py: --gpus {a.gpus}", file=sys.stderr, flush=True)
        sys.exit(2)


if __name__ == "__main__":
    _launch_or_continue(sys.argv[1:])

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import sdrpp_amd  # noqa: E402
from sdrpp_amd import dsp  # noqa: E402
from sdrpp_amd.multistream import CudaGather, GatherPipeline, StreamShard  # noqa: E402

METRIC = "IQ Msamples/s through FFT+FIR+demod chain; % HBM roofline at 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md chip table (spec)


class C5:
    """FFT(64k BH7) spectra (+ 2048-column waterfall rows) + RxVFO + BroadcastFM mono, one stream per GPU."""
    N = 65536
    FS = 61.44e6
    ZW = 2048

    def __init__(self, B, shard, dev):
        self.B = (B // self.N) * self.N
        self.frames = self.B // self.N
        self.fft = dsp.FFTSpectrum(self.N, self.N, 6, device=dev)
        self.vfo = dsp.RxVFO(self.FS, 240000, 200000, shard.vfo_offset(), device=dev)
        self.wfm = dsp.BroadcastFM(100000, 240000, True, device=dev)
        self.spectra = torch.empty(self.frames * self.N, dtype=torch.float32, device="cuda")
        self.ifbuf = torch.empty(2 * (self.B // 256 + 64), dtype=torch.float32, device="cuda")
        self.audio = torch.empty(2 * (self.B // 256 + 64), dtype=torch.float32, device="cuda")
        # the waterfall's display rows: every frame zoomed to ZW columns (full span, fft_scaler
        # doZoom), fused into the transform's last pass; double-buffered for the rank-0 gather
        self.zoom = [torch.empty(self.frames * self.ZW, dtype=torch.float32, device="cuda") for _ in range(2)]
        self.with_zoom = os.environ.get("BENCH_C5_ZOOM", "1") != "0"
        # one launch group for the spectrum, the zoom rows and the VFO's first stage, which reads the
        # IQ batch the spectrum reads (sdrgpu_fft_execute_zoom_vfo_dev); BENCH_C5_FUSE=0 (A/B only):
        # the spectrum group and the VFO as separate launch groups, as in round 3
        self.fuse = os.environ.get("BENCH_C5_FUSE", "1") != "0"
        self.zoom_count = self.frames * self.ZW
        # BENCH_C5_TAIL=1: the VFO's later stages, the zoom fold and the WFM on a stream of their own
        # (sdrgpu_fft_set_tail_stream), overlapping the next step's spectrum launch, as the reference runs the
        # spectrum and each VFO chain on threads of their own (iq_frontend.cpp:15-52). Off by default: the
        # step gained 5 us of 1.57 ms while the spectrum launch it overlaps stretched by 60 us (it fills every
        # CU), which the roofline of that launch would carry (profiles/r6/c5_tail_stream_ab_r7b.txt)
        self.tail = None
        if self.fuse and os.environ.get("BENCH_C5_TAIL", "0") != "0" and dev is not None:
            self.tail = torch.cuda.Stream()
            self.fft.set_tail_stream(self.tail.cuda_stream)
        self.bytes_per_sample = 8 + 4 + 4 / 32 + 8 / 256 + 8 / 256   # SURVEY 8(d) C5 (~12.06 B) + the zoom rows
        if self.fuse:
            # the group: 8 B in (read once), 4 B dB out, 8/32 B VFO stage-1 out (the zoom rows are folded
            # from the group's per-workgroup partial maxima in the VFO tail's launch, fft_1p_tail_fold_kernel)
            self.kernel_bytes = (12.0 + 8 / 32) * self.B
            self.kernel_name = ("spectrum N=65536 + zoom partials + RxVFO stage 1 (D=32, 143 taps, xlator): "
                                "fft_1p_kernel<zoom,vfo,false> (one pass: two workgroups per frame, each half the "
                                "VFO stage-1 outputs, then two adjacent 16k radix-4 DIF sub-transforms in LDS; the "
                                "rows stream in by LDS-DMA)")
            self.fft.set_timing(True)   # the group's own HIP events (the VFO's later stages are outside it)
            self.roofline_note = ("the group includes the VFO's first stage (8 B/sample of input it shares with "
                                  "the spectrum); the zoom fold (folding the two workgroups' partial maxima into "
                                  "the 2048-column rows) runs beside the VFO's later stages in one launch after "
                                  "the group; round 4's two-pass group (fft_vfo_kernel, SDRGPU_FFT_1P=0) took "
                                  "1.63 ms for the spectrum + zoom + stage 1, round 3's spectrum + separate stage 1.778 ms")
        else:
            self.kernel_bytes = (12.0 + 4 / 32) * self.B            # spectrum: 8 B in, 4 B dB + 4/32 B zoom out
            self.kernel_name = ("spectrum N=65536 + zoom to 2048: fft_passA_kernel<256,32> (chunk 0) + "
                                "fft_merged_kernel<256,32,256,32,false,zoom> (pass B chunk c + pass A chunk c+1) x15 + "
                                "fft_passB_kernel<256,32,zoom> (last chunk)")

    def rows_stream(self, stream):
        """The stream on which the zoom rows of a step are complete (the gather waits for it)."""
        return self.tail if self.tail is not None else stream

    def run(self, x, s, timed_call, buf=0):
        # the front end's splitter hands the same block to the spectrum and the VFO
        # (iq_frontend.cpp:15-52); the VFO output then feeds the WFM demodulator
        if self.fuse:
            z = self.zoom[buf].data_ptr() if self.with_zoom else 0
            m = self.fft.execute_zoom_vfo_dev(x.data_ptr(), self.frames, self.spectra.data_ptr(), z, self.ZW, self.vfo,
                                              self.ifbuf.data_ptr(), s)
            if self.tail is not None and self.with_zoom:   # the VFO output is complete on the tail stream
                self.counts = (buf, m, self.wfm.process_dev(self.ifbuf.data_ptr(), m, self.audio.data_ptr(),
                                                            self.tail.cuda_stream))
                return
        else:
            if self.with_zoom:
                timed_call(lambda: self.fft.execute_zoom_dev(x.data_ptr(), self.N, self.frames, self.spectra.data_ptr(),
                                                             self.zoom[buf].data_ptr(), self.ZW, s))
            else:   # (A/B only: BENCH_C5_ZOOM=0 drops the waterfall rows)
                timed_call(lambda: self.fft.execute_dev(x.data_ptr(), self.N, self.frames, self.spectra.data_ptr(), s))
            m = self.vfo.process_dev(x.data_ptr(), self.B, self.ifbuf.data_ptr(), s)
        self.counts = (buf, m, self.wfm.process_dev(self.ifbuf.data_ptr(), m, self.audio.data_ptr(), s))

    def outputs(self):
        """What the last step handed its caller: the dB rows, the waterfall rows it wrote, the VFO's
        complex output and the stereo audio (both interleaved, the counts the blocks returned)."""
        buf, m, na = self.counts
        out = {"spectra": self.spectra, "vfo_iq": self.ifbuf[:2 * m], "audio_stereo": self.audio[:2 * na]}
        if self.with_zoom:
            out["waterfall_rows"] = self.zoom[buf][:self.zoom_count]
        return out

    def group_ms(self, steps):
        """The dominant group's mean time over the timed steps from the library's own HIP events
        (sdrgpu_fft_group_times), or None when the group is timed by the bench's events."""
        if not self.fuse:
            return None
        n = min(steps, 256)   # the library keeps the last 256 calls' events (all of them timed steps here)
        t = self.fft.group_times(n)
        return float(np.mean(t)) if len(t) == n else None


class C2:
    """1,048,576-point BH7 spectrum, fftRate 10 at 10 MS/s -> nz = 1e6, zero-padded."""
    N = 1 << 20
    NZ = 1000000

    def __init__(self, B, shard, dev):
        self.frames = max(1, B // self.NZ)
        self.B = self.frames * self.NZ
        self.fft = dsp.FFTSpectrum(self.N, self.NZ, 6, device=dev)
        self.spectra = torch.empty(self.frames * self.N, dtype=torch.float32, device="cuda")
        self.bytes_per_sample = 8 + 4 * self.N / self.NZ
        self.kernel_bytes = self.bytes_per_sample * self.B
        self.kernel_name = ("spectrum N=2^20, nz=1e6: fft_passA_1m_kernel (16 columns, two tiles per workgroup, "
                            "tile-major intermediate) + fft_passB_1m_kernel (8 rows, XCD-grouped) per 8-frame chunk")

    def dominant(self, x, s):
        self.fft.execute_dev(x.data_ptr(), self.NZ, self.frames, self.spectra.data_ptr(), s)

    def outputs(self):
        return {"spectra": self.spectra}

    def rest(self, x, s):
        pass


class C3:
    """FrequencyXlator(-1.5 MHz) -> 256-tap DecimatingFIR /8 -> Quadrature(100 kHz), fused kernel."""
    FS = 61.44e6

    def __init__(self, B, shard, dev):
        self.B = B
        taps = dsp.low_pass(3.0e6, 912000.0, self.FS)
        w = 2 * np.pi * (-1.5e6 / self.FS)
        self.ddc = dsp.DDCFM(w, taps, 8, 2 * np.pi * 100e3 / (self.FS / 8), device=dev)
        self.out = torch.empty(B // 8 + 64, dtype=torch.float32, device="cuda")
        self.bytes_per_sample = 8 + 4 / 8
        self.kernel_bytes = self.bytes_per_sample * B
        self.kernel_name = "fir_mfma_kernel<4,XL,QUAD,HALF,D=8> (xlator + 256-tap FIR /8 on f32 MFMA + quadrature; half the phases' span in LDS at a time, 4 workgroups per CU; D a compile-time constant)"

    def dominant(self, x, s):
        self.count = self.ddc.process_dev(x.data_ptr(), self.B, self.out.data_ptr(), s)

    def outputs(self):
        return {"fm_demod": self.out[:self.count]}

    def rest(self, x, s):
        pass


class C4:
    """1024-channel critically sampled polyphase channelizer at 200 MS/s (prototype
    windowedSinc(16384, fs/(2M), fs, nuttall), 16 taps/branch), output [frame][channel]."""
    M = 1024

    def __init__(self, B, shard, dev):
        self.B = (B // self.M) * self.M
        taps = dsp.windowed_sinc(16 * self.M, np.pi / self.M)
        self.ch = dsp.PolyphaseChannelizer(self.M, taps, device=dev)
        self.out = torch.empty(2 * (self.B + self.M), dtype=torch.float32, device="cuda")
        self.bytes_per_sample = 16.0
        self.kernel_bytes = 16.0 * self.B
        self.kernel_name = "chan2_kernel<1024> (16-tap branch FIRs + 1024-pt FFT per frame)"

    def flop_roofline(self, kern_ms):
        # report the flop side too. Executed algorithm: 16-tap complex x real branch
        # FIR (64 flop/sample) + a 1024-point radix-16/4 FFT per frame (5 log2 M = 50 flop/sample,
        # the standard count); the dense DFT-GEMM formulation the survey names would do 64 + 512.
        fl = (64 + 5 * 10) * self.B
        tf = fl / (kern_ms * 1e-3) / 1e12
        gemm = (64 + 512) * self.B / (kern_ms * 1e-3) / 1e12
        return {"bound": "valu-fp32", "achieved": round(tf, 2), "peak": 157.3, "unit": "TFLOP/s",
                "frac": round(tf / 157.3, 4), "flop_per_sample": 114,
                "dft_gemm_equivalent_TFLOPs": round(gemm, 1),
                "note": "fp32 vector peak (MI355X_MICROARCH.md); gfx950's fp32 MFMA peak is the same 157 TF, "
                        "so the 576-flop DFT-GEMM form would be compute-bound where the FFT form is HBM-bound"}

    def dominant(self, x, s):
        self.count = self.ch.process_dev(x.data_ptr(), self.B, self.out.data_ptr(), s)

    def outputs(self):
        return {"channels_iq": self.out[:2 * self.count]}   # complex [frame][channel], interleaved

    def rest(self, x, s):
        pass


class C4G(C4):
    """C4 with the per-frame DFT "cast as batched MFMA GEMM" (SURVEY 8(d) C4 asks for both forms):
    the same branch FIRs, then two complex 32x32 products per frame on v_mfma_f32_16x16x4_f32."""

    def __init__(self, B, shard, dev):
        super().__init__(B, shard, dev)
        taps = dsp.windowed_sinc(16 * self.M, np.pi / self.M)
        self.ch = dsp.PolyphaseChannelizer(self.M, taps, device=dev, dft="gemm")
        self.kernel_name = "chan2_kernel<1024,GEMM> (16-tap branch FIRs + DFT as 2 complex 32x32 MFMA GEMMs per frame)"

    def flop_roofline(self, kern_ms):
        # executed: 64 flop/sample of branch FIR (VALU) + 512 flop/sample of DFT-GEMM (MFMA: 2 x 128
        # v_mfma_f32_16x16x4_f32 of 2048 flop per 1024-sample frame) + the twiddle (6 flop)
        tf = (64 + 512) * self.B / (kern_ms * 1e-3) / 1e12
        mf = 512 * self.B / (kern_ms * 1e-3) / 1e12
        return {"bound": "mfma-fp32", "achieved": round(tf, 2), "peak": 157.3, "unit": "TFLOP/s",
                "frac": round(tf / 157.3, 4), "flop_per_sample": 576, "mfma_TFLOPs": round(mf, 2),
                "note": "dense fp32 matrix-core peak 157.3 TF (MI355X_MICROARCH.md; 156 TF/s sustained measured, "
                        "tools/ubench/mfma_f32_peak.hip): this form is compute-bound at >= 0.88 ms of pure MFMA per "
                        "2^28 samples, the FFT form (c4) HBM-bound"}


def _run_generic(wl, x, s, timed_call):
    timed_call(lambda: wl.dominant(x, s))
    wl.rest(x, s)


def cpu_baseline(config, seconds, bytes_per_sample=None):
    """The reference CPU path for the config on the host cores, measured by
    oracle/cpu_baseline.py (test infrastructure, run only here): the oracle's C restatement built
    on this host with -O3 -march=native (vectorised VOLK-class dots) and, for the spectrum legs,
    pocketfft (scipy.fft, fp32, 1 worker); SpeedTester-style 1e6-sample blocks. `value` is the
    all-core aggregate (one independent stream per core, up to 16 cores = the box's CPU share),
    i.e. the faster CPU number every speed-up claim is made against; `value_1core` the reference's
    own model (one worker thread per block, single-threaded FFT)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_baseline as cb
    r = cb.measure(config, seconds)
    h = r["host"]
    out = {"value": round(r["value_all_cores"], 3), "unit": "MS/s", "cores": r["cores_all"], "kind": "port",
           "cores_source": r["cores_source"], "value_1core": round(r["value_1core"], 3),
           "value_1core_basis": (f"max(1-core run on CPU {r['value_1core_cpu']}: {r['value_1core_run']:.2f}, spread "
                                 f"streams' per-stream mean: {r['value_1core_spread_mean']:.2f})"),
           "value_packed": round(r["value_all_cores_packed"], 3), "value_spread": round(r["value_all_cores_spread"], 3),
           "placement": r["placement"],
           "sample": f"{r['variant']}: {r['cores_all']} independent streams x {seconds:.0f} s (all-core aggregate, the "
                     f"faster of two placements: packed on the first CPUs, spread one per L3 domain over the sockets), "
                     f"1 stream {r['value_1core']:.2f} MS/s; 1-core variants "
                     + ", ".join(f"{k} {v:.2f}" for k, v in r["variants_1core"].items())
                     + f"; {r['build']}; SpeedTester-style 1e6-sample blocks of uniform [-1,1) IQ",
           "host": {"nproc": h["nproc"], "affinity_cpus": h["affinity"], "cgroup_cpu_quota": h["cgroup_cpu_quota"],
                    "model": h["model"], "core_max_mhz": h["core_max_mhz"], "placement": h.get("placement")}}
    # the whole machine, extrapolated linearly from one core over every affinity CPU (SMT siblings
    # counted as cores: an upper bound for the CPU side)
    out["value_all_affinity_cpus_linear"] = round(r["value_1core"] * h["affinity"], 1)
    # ... and bounded by the host's DRAM: no CPU chain moves fewer bytes per sample than the
    # algorithmic ones (IQ in, results out), so a whole host delivers at most DRAM peak / bytes per
    # sample. The lease's own measured memcpy rate is reported beside it.
    out["host"]["sockets"] = h.get("sockets")
    out["host"]["dram_peak_GBs"] = h.get("dram_peak_GBs")
    out["host"]["lease_memcpy_GBs"] = h.get("lease_memcpy_GBs")
    if bytes_per_sample and h.get("dram_peak_GBs"):
        dram = h["dram_peak_GBs"] * 1e3 / bytes_per_sample   # MS/s
        out["value_whole_host_dram_bound"] = round(min(out["value_all_affinity_cpus_linear"], dram), 1)
        out["whole_host_bound_note"] = (f"min(1-core x {h['affinity']} CPUs, {h['dram_peak_GBs']:.0f} GB/s DRAM peak of "
                                        f"{h.get('sockets')} sockets / {bytes_per_sample:.2f} B per sample)")
    for k in ("gflops_1core", "fma_peak_frac_1core"):
        if k in r:
            out[k] = r[k]
    return out


def spectrum_ulp_report(dev=0, seed=20261017):
    """The spectrum's dB error in fp32 ulps of the correctly rounded truth, measured live on this box
    with the library under test: one random frame per size (4k, 64k, 1M with nz = 1e6), GPU dB rows
    against 10 log10 |DFT|^2 of the same float-windowed frame in fp64 (numpy), on bins within 60 dB
    of the frame's peak; pocketfft single precision (scipy, the FFTW-class CPU reference) on the
    same frame alongside. tests/test_gpu_parity.py::test_spectrum_ulp_distribution asserts the bars."""
    import scipy.fft
    rng = np.random.default_rng(seed)

    def ulps(db, p64):
        t64 = 10.0 * np.log10(np.maximum(p64, 1e-300))
        sel = t64 >= t64.max() - 60.0
        t32 = t64[sel].astype(np.float32)
        return np.abs(np.asarray(db, np.float32)[sel].astype(np.float64) - t32.astype(np.float64)) / \
            np.spacing(np.abs(t32)).astype(np.float64)

    out = {}
    for N, nz in ((4096, 4096), (65536, 65536), (1 << 20, 1000000)):
        x = (rng.uniform(-1, 1, nz) + 1j * rng.uniform(-1, 1, nz)).astype(np.complex64)
        w = dsp.create_window(6, nz)
        xw = np.zeros(N, dtype=np.complex64)
        xw[:nz] = (x * w).astype(np.complex64)
        X = np.fft.fft(xw.astype(np.complex128))
        p64 = X.real ** 2 + X.imag ** 2
        e = ulps(dsp.FFTSpectrum(N, nz, 6, device=dev).logmag(x), p64)
        e64 = ulps(dsp.FFTSpectrum(N, nz, 6, device=dev, precision="f64").logmag(x), p64)
        Xr = scipy.fft.fft(xw, workers=1)
        pr = Xr.real.astype(np.float32) ** 2 + Xr.imag.astype(np.float32) ** 2
        with np.errstate(divide="ignore"):
            er = ulps((10.0 * np.log10(pr.astype(np.float64))).astype(np.float32), p64)
        out[f"random_N{N}"] = {"bins": int(e.size), "max_ulp": float(e.max()), "p99_ulp": float(np.percentile(e, 99)),
                               "frac_le_1ulp": round(float(np.mean(e <= 1.0)), 4),
                               "pocketfft_max_ulp": float(er.max()),
                               "pocketfft_frac_le_1ulp": round(float(np.mean(er <= 1.0)), 4),
                               "f64_mode_max_ulp": float(e64.max()), "f64_mode_frac_exact": round(float(np.mean(e64 == 0)), 6)}
    out["source"] = "measured live in this run (fp64 numpy truth); f64_mode = sdrgpu_fft_set_precision(h, 1)"
    return out


def f64_roofline(N, nz, frames, ms):
    """HBM roofline of the fp64-interior spectrum (fft64.hip) for one call of `frames` frames in `ms`:
    algorithmic bytes = the fp32 op's (8 B per input sample in, 4 B per bin out); the two passes also
    write and read a double2 intermediate (16 + 16 B per transform element, 128-MB chunks kept in the
    Infinity Cache), reported as `moved_bytes` with its rate."""
    algo = 8 * nz * frames + 4 * N * frames
    moved = 8 * nz * frames + (16 + 16 + 4) * N * frames
    achieved = algo / (ms * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "algorithmic_bytes": algo, "moved_bytes": moved,
            "moved_GBs": round(moved / (ms * 1e-3) / 1e9, 1),
            "note": "fp64 interior, two passes through a double2 intermediate (N > 4096)"}


def spectrum_f64_cost(dev, stream, reps=5):
    """Cost of the fp64-interior parity mode (sdrgpu_fft_set_precision(h, 1)) against the fp32 kernels
    on the same device batch: 64k BH7 over 2^26 samples (1,024 back-to-back frames) and the C2 1M plan
    (nz = 1e6) over 32 frames; HIP events on the bench stream, median of `reps` calls after a warm-up."""
    out = {}
    for N, nz, frames in ((65536, 65536, 1024), (1 << 20, 1000000, 32)):
        x = torch.empty(2 * nz * frames, dtype=torch.float32, device="cuda").uniform_(-1, 1)
        o = torch.empty(N * frames, dtype=torch.float32, device="cuda")
        r = {}
        for prec in ("f32", "f64"):
            f = dsp.FFTSpectrum(N, nz, 6, device=dev, precision=prec)
            ts = []
            for k in range(reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f.execute_dev(x.data_ptr(), nz, frames, o.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if k:
                    ts.append(e0.elapsed_time(e1))
            r[prec] = float(np.median(ts))
            del f
        out[f"N{N}"] = {"frames": frames, "samples": nz * frames, "ms_f32": round(r["f32"], 4), "ms_f64": round(r["f64"], 4),
                        "f64_over_f32": round(r["f64"] / r["f32"], 3),
                        "MSps_f64": round(nz * frames / r["f64"] / 1e3, 1),
                        "roofline_f64": f64_roofline(N, nz, frames, r["f64"])}
        del x, o
    return out


def traffic_per_sample(config):
    """HBM bytes per input sample of the dominant launch group, from the newest committed
    rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE; tools/pmc_bytes_per_sample.py)."""
    for rnd in ("r6", "r5", "r4", "r3", "r2", "r1"):
        path = os.path.join(ROOT, "profiles", rnd, f"{config}_pmc_traffic.json")
        try:
            d = json.load(open(path))
            return float(d["bytes_per_sample"]), f"profiles/{rnd}/{config}_pmc_traffic.json"
        except (OSError, KeyError, ValueError):
            continue
    return None, None


DUMP_WHOLE = 1 << 23          # --dump-outputs: arrays up to this many elements are written whole,
DUMP_SAMPLE = 1 << 21         # larger ones as this many elements at fixed, seeded positions
DUMP_MAX_BYTES = 64 * 10**6   # of float32 in all
DUMP_SEED = 0xD0E5


def dump_plan(sizes):
    """{name: None (the whole array) or sorted int64 positions into it} for output arrays of
    `sizes[name]` elements. The positions depend only on the array's length, so two builds run
    with the same arguments write the same elements. Should the arrays written whole not fit in
    DUMP_MAX_BYTES (a --log2-batch above the default), the whole/sample sizes halve until they do."""
    whole = DUMP_WHOLE

    def kept(c):
        return c if c <= whole else min(DUMP_SAMPLE, whole)
    while 4 * sum(kept(c) for c in sizes.values()) > DUMP_MAX_BYTES:
        whole //= 2
    return {n: None if c <= whole else np.sort(np.random.default_rng([DUMP_SEED, c]).integers(0, c, kept(c)))
            for n, c in sizes.items()}


def dump_outputs(wl, path):
    """--dump-outputs: the workload's outputs() of its last step as <path>/<name>.npy (float32)."""
    torch.cuda.synchronize()
    os.makedirs(path, exist_ok=True)
    outs = wl.outputs()
    for name, pos in dump_plan({n: t.numel() for n, t in outs.items()}).items():
        t = outs[name]
        if pos is not None:
            t = t[torch.from_numpy(pos).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.to(torch.float32).cpu().numpy())


WORKLOADS = {"c5": "C5 per-GPU slice: 64k BH7 FFT+log-mag (back-to-back) + 2048-column waterfall zoom + RxVFO "
                   "61.44M->240k + BroadcastFM mono",
             "c2": "C2: 1M-point BH7 FFT + log-mag, nz=1e6 zero-padded, 256 frames/step",
             "c3": "C3: xlator + 256-tap FIR /8 + FM quadrature (fused), 2^28 samples/step",
             "c4": "C4: 1024-channel polyphase channelizer (16384-tap prototype), 2^28 samples/step",
             "c4g": "C4 as batched MFMA GEMM: 1024-channel polyphase channelizer, per-frame DFT as two complex "
                    "32x32 f32 MFMA products, 2^28 samples/step"}


WORKLOAD_CLASSES = {"c5": C5, "c2": C2, "c3": C3, "c4": C4, "c4g": C4G}


class CudaRuntime:
    """The device side of run_config on a GPU: torch.cuda streams / events and libsdrgpu's RCCL
    gather. tests/test_bench_multirank.py substitutes a CPU runtime (gloo, LazyGlooGather) to run
    the same control flow at world size 2 on the CPU."""
    reduce_device = "cuda"

    def rand(self, n, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return (torch.rand(n, device="cuda", generator=g) * 2 - 1).contiguous()

    def event(self):
        return torch.cuda.Event(enable_timing=True)

    def handle(self, stream):
        return stream.cuda_stream

    def synchronize(self):
        torch.cuda.synchronize()

    def gather_backend(self, shard, dev):
        return CudaGather(shard, dev)


class CpuRehearsalRuntime:
    """`--runtime cpu-rehearsal`: the device side of run_config on the CPU -- torch CPU tensors,
    perf_counter events and LazyGlooGather (gathers over gloo that run only when their completion is
    waited for, so a buffer rewritten before its gather ran would ship the wrong rows) in place of
    torch.cuda streams and libsdrgpu's RCCL gather. Used by tests/test_bench_multirank.py to run the
    whole `bench.py --gpus 2` path (self-launch, ranks, gather, verification) without a GPU."""
    reduce_device = None

    class Event:
        def record(self, stream=None):
            self.t = time.perf_counter()

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    def rand(self, n, seed):
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.rand(n, generator=g) * 2 - 1

    def event(self):
        return self.Event()

    def handle(self, stream):
        return stream

    def synchronize(self):
        pass

    def gather_backend(self, shard, dev):
        from sdrpp_amd.multistream import LazyGlooGather
        return LazyGlooGather()


class C5Rehearsal:
    """C5's interface on the CPU for the rehearsal runtime: `frames` rows of ZW columns per step, a
    function of the step's input, this rank's stream (seed) and the step number, so the gather's
    verification has something to catch. SDRGPU_BENCH_REHEARSAL_DIE="rank:step" makes that rank exit
    with status 3 at that step (the failure path of the launcher)."""
    N, ZW = 4096, 64

    def __init__(self, B, shard, dev):
        self.B = (B // self.N) * self.N
        self.frames = self.B // self.N
        self.zoom = [torch.empty(self.frames * self.ZW) for _ in range(2)]
        self.zoom_count = self.frames * self.ZW
        self.rank = shard.rank
        self.k = 0
        self.bytes_per_sample = 12.0
        self.kernel_bytes = 12.0 * self.B
        self.kernel_name = "cpu rehearsal stand-in (no kernel)"
        self.history = []
        die = os.environ.get("SDRGPU_BENCH_REHEARSAL_DIE")
        self.die = tuple(int(v) for v in die.split(":")) if die else None

    def run(self, x, s, timed_call, buf=0):
        if self.die is not None and self.die == (self.rank, self.k):
            print(f"bench.py rank {self.rank}: rehearsal failure injected at step {self.k}", file=sys.stderr, flush=True)
            os._exit(3)

        def body():
            rows = x[:2 * self.B].view(self.frames, -1)[:, :self.ZW] + 1000.0 * self.rank + self.k
            self.zoom[buf].copy_(rows.reshape(-1))
        timed_call(body)
        self.history.append(self.zoom[buf].clone())
        self.k += 1


def run_config(config, a, shard, dev, stream, rt=None, workloads=None):
    """Time `a.steps` steps of one config on this rank; returns (B, elapsed_s, kernel_ms, wl)."""
    rt = rt or CudaRuntime()
    world, rank = shard.world, shard.rank
    B = 1 << a.log2_batch
    if config == "c2":
        B = 256 * 1000000
    wl = (workloads or WORKLOAD_CLASSES)[config](B, shard, dev)
    B = wl.B
    x = rt.rand(2 * B, shard.seed())   # complex_t interleaved
    # N > 1: every step's waterfall rows go to rank 0 over RCCL (libsdrgpu's C-ABI gather) on a
    # stream of their own, overlapping the next step; the zoom rows are double-buffered and a step
    # waits only for the gather that last used its buffer (multistream.GatherPipeline; the same
    # protocol runs on the CPU over gloo in tests/test_multistream_gloo.py, and this whole function
    # at world size 2 in tests/test_bench_multirank.py)
    pipe = None
    if world > 1 and hasattr(wl, "zoom"):
        pipe = GatherPipeline(shard, wl.zoom_count, rt.gather_backend(shard, dev))
        wl.zoom = pipe.bufs

    ev = []
    # One stream for the whole step. Forking the spectrum and the VFO chain onto two streams
    # (the reference runs them on separate block threads, iq_frontend.cpp:49,115) was
    # measured twice: the step time does not change (2.95 vs 2.97 ms; with the MFMA VFO stage
    # 2.265 vs 2.261 ms; with the register-streaming VFO stage 1, 2.03-2.13 vs 2.01-2.04 ms)
    # but the spectrum's event/rocprof durations stretch by the overlap
    # (1.58 -> 1.89 ms), so the roofline numbers would stop describing the kernel.
    def step(timed):
        evs = []

        def timed_call(fn):   # HIP events around the dominant kernel's launches, on their stream
            if timed:
                e0, e1 = rt.event(), rt.event()
                e0.record(stream)
            fn()
            if timed:
                e1.record(stream)
                evs.append((e0, e1))
        rs = wl.rows_stream(stream) if hasattr(wl, "rows_stream") else stream   # where the zoom rows are written
        buf = pipe.acquire(rs) if pipe is not None else 0
        if hasattr(wl, "run"):
            wl.run(x, rt.handle(stream), timed_call, buf)
        else:
            _run_generic(wl, x, rt.handle(stream), timed_call)
        if timed:
            ev.append(evs)
        if pipe is not None:
            pipe.publish(buf, rs, timed=timed)

    def drain():
        if pipe is not None:
            pipe.drain(stream)

    for _ in range(a.warmup):
        step(False)
    drain()
    rt.synchronize()
    shard.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step(True)
    drain()   # the last step's gather is inside the timed region
    rt.synchronize()
    shard.barrier()
    elapsed = time.perf_counter() - t0
    kern_ms = sum(sum(e0.elapsed_time(e1) for e0, e1 in evs) for evs in ev) / max(len(ev), 1)
    if hasattr(wl, "group_ms") and wl.group_ms(a.steps) is not None:
        kern_ms = wl.group_ms(a.steps)
    if not kern_ms > 0:
        raise RuntimeError(f"{config}: no kernel time recorded for the dominant group (steps {a.steps})")
    elapsed, kern_ms = shard.max_over_ranks([elapsed, kern_ms], device=rt.reduce_device)
    if pipe is not None:
        # the first multi-GPU run proves the gather: rank 0's received rows of the last step carry
        # each sender's own checksum; the gather's own time is reported next to the step time
        ok, det = pipe.verify()
        gms = shard.max_over_ranks([pipe.gather_ms() or 0.0], device=rt.reduce_device)[0]
        wl.gather_report = {"verified": bool(ok), "ms_per_gather_max_rank": round(gms, 4),
                            "bytes_per_rank_per_step": 4 * wl.zoom_count, **(det or {})}
        pipe.close()
    del x
    return B, elapsed, kern_ms, wl


def per_call_c5(dev, stream, calls=300, block=307200, single_only=False):
    """C5 at the reference's block size: file/hardware sources push fs / 200 samples per block
    (source_modules/file_source/src/main.cpp:296,440: 307,200 at 61.44 MS/s). Each call is one
    block through the device front end (sdrgpu_frontend_push_dev: spectrum frames back to back,
    one RxVFO) + BroadcastFM mono on the VFO output -- the per-block launch sequence SDR++ would
    issue -- and, second, the same through the host drop-in call (sdrgpu_frontend_push: pinned
    staging, H2D, synchronise per block). Time per call = wall time of `calls` calls / calls."""
    fs, N = 61.44e6, 65536
    fe = dsp.IQFrontEnd(fs, fft_size=N, fft_rate=fs / N, device=dev)
    vid = fe.add_vfo(240000, 200000, 2.5e6)
    wfm = dsp.BroadcastFM(100000, 240000, True, device=dev)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    x = (torch.rand(2 * block * 8, device="cuda", generator=g) * 2 - 1).contiguous()
    audio = torch.empty(2 * 4096, dtype=torch.float32, device="cuda")
    s = stream.cuda_stream

    def one(k):
        fe.push_dev(x.data_ptr() + 8 * block * (k % 8), block, -1, s)
        p, n = fe.vfo_dev(vid)
        wfm.process_dev(p, n, audio.data_ptr(), s)
    for k in range(20):
        one(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        one(k)
    issue_us = (time.perf_counter() - t0) / calls * 1e6   # host time to issue a call's launches
    torch.cuda.synchronize()
    dev_us = (time.perf_counter() - t0) / calls * 1e6
    if single_only:
        fe.close()
        return {"block": block, "us_per_call_device": round(dev_us, 1), "MSps_device": round(block / dev_us, 1),
                "us_per_call_host_issue": round(issue_us, 1)}
    # K independent block streams on K HIP streams (one SDR each): each call's kernels fill only a
    # few CUs, so concurrent streams overlap on the device
    K = 16
    streams = [torch.cuda.Stream() for _ in range(K)]
    fes = [dsp.IQFrontEnd(fs, fft_size=N, fft_rate=fs / N, device=dev) for _ in range(K)]
    vids = [f.add_vfo(240000, 200000, 2.5e6 + 1e5 * i) for i, f in enumerate(fes)]
    wfms = [dsp.BroadcastFM(100000, 240000, True, device=dev) for _ in range(K)]
    auds = [torch.empty(2 * 4096, dtype=torch.float32, device="cuda") for _ in range(K)]

    def multi(k):
        for i in range(K):
            si = streams[i].cuda_stream
            fes[i].push_dev(x.data_ptr() + 8 * block * ((k + i) % 8), block, -1, si)
            p, n = fes[i].vfo_dev(vids[i])
            wfms[i].process_dev(p, n, auds[i].data_ptr(), si)
    for k in range(10):
        multi(k)
    torch.cuda.synchronize()
    rounds = max(calls // K, 20)
    t0 = time.perf_counter()
    for k in range(rounds):
        multi(k)
    torch.cuda.synchronize()
    multi_us = (time.perf_counter() - t0) / rounds * 1e6
    for f in fes:
        f.close()
    out_issue = round(issue_us, 1)
    xh = x[:2 * block].cpu().numpy().view(np.complex64)
    fe.push(xh)
    t0 = time.perf_counter()
    n_host = max(calls // 3, 20)
    for _ in range(n_host):
        fe.push(xh)
    sync_us = (time.perf_counter() - t0) / n_host * 1e6
    # the drop-in worker's call style (IQFrontEnd drop-in): blocks from the pinned input ring
    # (sdrgpu_host_alloc) submitted without waiting, two in flight, each block's rows and VFO output
    # copied out of the pinned result slot when collected (the hand-off to acquireFFTBuffer / the
    # VFO stream)
    import ctypes
    ring = []
    for k in range(4):
        hp = ctypes.c_void_p()
        sdrpp_amd.check(sdrpp_amd.lib.sdrgpu_host_alloc(ctypes.byref(hp), 8 * block))
        ctypes.memmove(hp.value, xh.ctypes.data, 8 * block)
        ring.append(hp)

    def pipelined(n):
        pend = []
        for k in range(n):
            pend.append(fe.submit(None, ptr=ring[k % 4].value, count=block))
            if len(pend) == 2:
                fe.collect(pend.pop(0), vfos=[vid])
        for t in pend:
            fe.collect(t, vfos=[vid])
    pipelined(20)
    # host-side timing on a shared box jitters (119 / 167 / 119 us in three runs of one session):
    # the median of three repetitions is reported, all three alongside
    host_runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        pipelined(n_host)
        host_runs.append((time.perf_counter() - t0) / n_host * 1e6)
    host_us = sorted(host_runs)[1]
    for hp in ring:
        sdrpp_amd.lib.sdrgpu_host_free(hp)
    fe.close()
    # PCIe floor of a block: its 2.46 MB H2D + the rows / VFO read-back, at the measured copy rate
    return {"block": block, "us_per_call_device": round(dev_us, 1), "MSps_device": round(block / dev_us, 1),
            "us_per_call_host_issue": out_issue, "concurrent_streams": K, "MSps_device_concurrent": round(K * block / multi_us, 1),
            "us_per_call_host_dropin": round(host_us, 1), "MSps_host_dropin": round(block / host_us, 1),
            "us_per_call_host_dropin_runs": [round(v, 1) for v in host_runs],
            "us_per_call_host_sync": round(sync_us, 1),
            "note": "one 307,200-sample block per call (fs/200 at 61.44 MS/s) through the device front end "
                    "(spectrum + 1 VFO) + WFM; concurrent: K independent front ends on K HIP streams; host drop-in: "
                    "the IQFrontEnd drop-in's pipelined call style (sdrgpu_frontend_submit/collect, blocks from "
                    "pinned ring slots, two in flight, rows + VFO output copied out per block); host sync: one "
                    "synchronous push per block (staging memcpy, H2D, kernels, read-back)"}


def config_result(config, a, world, B, elapsed, kern_ms, wl, wname=None):
    value = world * B * a.steps / elapsed / 1e6
    achieved = wl.kernel_bytes / (kern_ms * 1e-3) / 1e9
    tps, tsrc = traffic_per_sample(config)
    r = {"value": round(value, 3), "unit": "MS/s", "ms_per_step": round(elapsed / a.steps * 1e3, 4),
         "workload": wname or WORKLOADS[config], "samples_per_gpu_per_step": B,
         "bytes_per_sample": round(wl.bytes_per_sample, 4),
         "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": round(achieved / HBM_PEAK_GBS, 4),
                      "traffic": round(tps * B) if tps else None, "traffic_source": tsrc,
                      "kernel": wl.kernel_name, "kernel_ms": round(kern_ms, 4),
                      "algorithmic_bytes": round(wl.kernel_bytes)},
         "chain_hbm_GBs": round(wl.bytes_per_sample * value * 1e6 / world / 1e9, 1)}
    if getattr(wl, "roofline_note", None):
        r["roofline"]["note"] = wl.roofline_note
    if hasattr(wl, "flop_roofline"):
        r["roofline_flops"] = wl.flop_roofline(kern_ms)
    if getattr(wl, "gather_report", None):
        r["gather"] = wl.gather_report
    return r


def rehearsal_main(a):
    """`--runtime cpu-rehearsal`: this rank's run_config over gloo with the CPU stand-in; rank 0
    prints the line (marked as a rehearsal, with the gather report and this rank's last rows'
    checksums so a test can check what rank 0 received)."""
    if a.dump_outputs:
        raise SystemExit("bench.py: --dump-outputs needs --runtime hip (the rehearsal computes nothing to compare)")
    shard = StreamShard(backend="gloo")
    world, rank = shard.world, shard.rank
    B, elapsed, kern_ms, wl = run_config(a.config, a, shard, None, "compute", rt=CpuRehearsalRuntime(),
                                         workloads={a.config: C5Rehearsal})
    head = config_result(a.config, a, world, B, elapsed, kern_ms, wl, wname="C5-shaped CPU stand-in")
    from sdrpp_amd.multistream import row_checksum
    sums = shard.all_gather_tensor(row_checksum(wl.history[-1]))
    if rank == 0:
        out = {"metric": METRIC, "value": head["value"], "unit": "MS/s", "n_gpus": world, "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak",
               "runtime": "cpu-rehearsal", "data": "cpu-rehearsal: control flow only, not a measurement",
               "samples_per_rank_per_step": B, "last_rows_checksums": sums.tolist()}
        if "gather" in head:
            out["gather"] = head["gather"]
        print(json.dumps(out), flush=True)
    shard.close()


def main():
    a = parse()
    if a.runtime == "cpu-rehearsal":
        return rehearsal_main(a)
    shard = StreamShard(backend="nccl")
    world, rank = shard.world, shard.rank
    if world == 1:
        torch.cuda.set_device(0)
    dev = torch.cuda.current_device()
    # one explicit non-default stream for every kernel of the step (libsdrgpu treats a NULL
    # stream as "the handle's own stream", which would split the chain over several queues)
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    B, elapsed, kern_ms, wl = run_config(a.config, a, shard, dev, stream)
    head = config_result(a.config, a, world, B, elapsed, kern_ms, wl)
    if a.dump_outputs and rank == 0:
        dump_outputs(wl, a.dump_outputs)
    del wl
    # everything below the timed config is --full only; --no-sub / --no-ulp / --no-cpu drop parts of it
    sub, ulp, cpu = (a.full and not off for off in (a.no_sub, a.no_ulp, a.no_cpu))
    # the other single-GPU configs of BASELINE.json, timed the same way in the same run (N = 1 only:
    # C2 and C3 carry the north_star's >= 10x / >= 40% targets, C4 the channelizer)
    subs = {}
    if world == 1 and sub:
        for c in ("c2", "c3", "c4", "c4g", "c5"):
            if c == a.config:
                continue
            torch.cuda.empty_cache()
            b2, el2, km2, wl2 = run_config(c, a, shard, dev, stream)
            subs[c] = config_result(c, a, world, b2, el2, km2, wl2)
            del wl2
    if rank == 0:
        out = {
            "metric": METRIC, "value": head["value"], "unit": "MS/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic uniform[-1,1) complex IQ in HBM",
            "config": {"workload": head["workload"] + ("; every frame's 2048-column waterfall row gathered to rank 0 "
                                                       "over RCCL (sdrgpu_gather_rows) each step" if world > 1 else ""),
                       "samples_per_gpu_per_step": B, "parallelism": f"replica-streams x{world}",
                       "bytes_per_sample": head["bytes_per_sample"]},
            "roofline": head["roofline"],
            "chain_hbm_GBs": head["chain_hbm_GBs"],
        }
        if "roofline_flops" in head:
            out["roofline_flops"] = head["roofline_flops"]
        if "gather" in head:
            out["gather"] = head["gather"]
        if ulp:
            out["spectrum_ulp"] = spectrum_ulp_report(dev)
            out["spectrum_f64_mode_cost"] = spectrum_f64_cost(dev, stream)
        if world == 1 and cpu:
            out["cpu_baseline"] = cpu_baseline("c4" if a.config == "c4g" else a.config, a.cpu_seconds, head["bytes_per_sample"])
            out["speedup_vs_cpu_all_cores"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
            out["speedup_vs_cpu_all_affinity_linear"] = round(out["value"] / out["cpu_baseline"]["value_all_affinity_cpus_linear"], 2)
            if out["cpu_baseline"].get("value_whole_host_dram_bound"):
                out["speedup_vs_whole_host_bound"] = round(out["value"] / out["cpu_baseline"]["value_whole_host_dram_bound"], 2)
            out["speedup_basis"] = ("speedup_vs_cpu_all_cores (the north_star's >= 10x) is against the CPUs the box grants "
                                    "this job (cpu_baseline.cores, cgroup quota); speedup_vs_whole_host_bound against a whole "
                                    "host, every CPU at the 1-core rate but never past its DRAM peak / bytes per sample")
            cpu_cache = {}
            for c, r in subs.items():
                ck = "c4" if c == "c4g" else c   # both C4 forms against the same CPU channelizer
                if ck not in cpu_cache:
                    cpu_cache[ck] = cpu_baseline(ck, a.cpu_seconds, r["bytes_per_sample"])
                r["cpu_baseline"] = cpu_cache[ck]
                r["speedup_vs_cpu_all_cores"] = round(r["value"] / r["cpu_baseline"]["value"], 1)
                r["speedup_vs_cpu_all_affinity_linear"] = round(r["value"] / r["cpu_baseline"]["value_all_affinity_cpus_linear"], 2)
                if r["cpu_baseline"].get("value_whole_host_dram_bound"):
                    r["speedup_vs_whole_host_bound"] = round(r["value"] / r["cpu_baseline"]["value_whole_host_dram_bound"], 2)
        if subs:
            out["configs"] = subs
        if world == 1 and a.config == "c5" and sub:
            out["per_call"] = per_call_c5(dev, stream)
        print(json.dumps(out), flush=True)
    shard.close()


if __name__ == "__main__":
    try:
        main()
    except sdrpp_amd.SdrGpuError as e:
        # a peer rank that died or stalled (gather deadline, communicator aborted: sdrgpu_gather_*)
        # or any other library failure: report it and leave at once with a non-zero status, without
        # the interpreter's teardown (process-group destroy, device synchronise), which could block
        # on the peer that is gone
        rank = os.environ.get("RANK", "0")
        print(f"bench.py rank {rank}: {e}", file=sys.stderr, flush=True)
        os._exit(3)
