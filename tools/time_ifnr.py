"""Call times of the IF noise reduction blocks on device-resident buffers (needs an MI355X):
    python tools/time_ifnr.py [out.json]
FMIF at B = 32 and B = 15 on 2^22 samples, NoiseBlanker and Squelch on 2^20. Per block: warm-up,
then >= 50 process_dev calls on one stream between two device events, as many as fill a window of
>= 0.5 s. One JSON line per block: ms per call and samples/s. For FMIF also the GEMM's FLOP
(8 B_pad^2 per sample: n padded to a multiple of 4, the bins to 16 or 32 -- the MFMA work issued)
over the time as a share of the 157.3 TF f32 matrix peak; the kernel moves 16 B per sample, which at
8 TB/s is far below the compute time, so compute is the bound named."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrpp_amd  # noqa: E402
from sdrpp_amd import dsp  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
MIN_CALLS, MIN_WINDOW_S = 50, 0.5


def time_block(blk, n, stream):
    rng = np.random.default_rng(1)
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    d_in = torch.from_numpy(x.view(np.float32)).cuda()
    d_out = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def run(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            blk.process_dev(d_in.data_ptr(), n, d_out.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3
    run(3)                                                   # warm-up: code objects, buffers
    est = run(5) / 5
    calls = max(MIN_CALLS, int(np.ceil(1.2 * MIN_WINDOW_S / max(est, 1e-9))))
    t = run(calls)
    while t < MIN_WINDOW_S:                                  # (the estimate still held start-up cost)
        calls = int(np.ceil(1.5 * calls * MIN_WINDOW_S / t))
        t = run(calls)
    return calls, t


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rows = []
    cases = [("fmif_b32", lambda: dsp.FMIF(32), 1 << 22, 32), ("fmif_b15", lambda: dsp.FMIF(15), 1 << 22, 15),
             ("noise_blanker", lambda: dsp.NoiseBlanker(500.0 / 250000.0, 10.0), 1 << 20, 0),
             ("squelch", lambda: dsp.Squelch(-50.0), 1 << 20, 0)]
    for name, make, n, bins in cases:
        calls, t = time_block(make(), n, stream)
        row = {"block": name, "samples_per_call": n, "calls": calls, "window_s": round(t, 4),
               "ms_per_call": round(1e3 * t / calls, 5), "samples_per_s": round(n * calls / t, 1)}
        if bins:
            npad, kpad = 4 * ((bins + 3) // 4), (16 if bins <= 16 else 32)
            flop = 8.0 * npad * kpad * n
            row.update(bins=bins, n_pad=npad, bins_pad=kpad, flop_per_call=flop,
                       tflops=round(flop * calls / t / 1e12, 3),
                       share_of_f32_matrix_peak=round(flop * calls / t / F32_MATRIX_PEAK, 4), bound="compute (f32 MFMA)")
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
