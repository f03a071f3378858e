"""The one-pass 64k kernel's row ring (fft_1p_kernel, the LDS-DMA instantiations) against its register path.

The range-checked (PAD) instantiations load every sample through buffer loads into registers and share every
arithmetic helper with the LDS-DMA ring, so the two must give the same bits on the same samples. One sample
stream (the ragged 1,000-sample VFO pre-call, then two calls of `frames` frames) is put into two device
buffers: one whose frames start 16-byte aligned (launch_1p takes the ring) and one shifted by one complex
sample (not 16-byte aligned: launch_1p takes the register path). Rows, zoom rows and the fused VFO's output
of both are compared as bit patterns, for the four (zoom, vfo) variants, at one item per workgroup, at three
items per workgroup (slot reuse across items, the cross-item prefetch) and at nine. A ring slot refilled before
its readers are done, or read before its pieces have landed, depends on timing: the three-item case is also run
three times on one plan and must give the same bits every time."""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from test_onepass_persistent import FS, N, OFF, PRE, VARIANTS, ZW, _input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


_bufs = {}


def _buffers(frames):
    """The stream at a 16-byte-aligned base and at a base shifted by one complex sample (device tensors, built
    once per size and only read afterwards)."""
    if frames not in _bufs:
        import torch
        n = 2 * (PRE + 2 * frames * N)
        src = _input(frames)[:n]
        aligned = src.clone()
        shifted = torch.empty(n + 2, device="cuda")
        shifted[:2] = 0
        shifted[2:] = src
        torch.cuda.synchronize()
        assert (aligned.data_ptr() + 8 * PRE) % 16 == 0 and (shifted.data_ptr() + 8 + 8 * PRE) % 16 == 8
        _bufs[frames] = (aligned, aligned.data_ptr()), (shifted, shifted.data_ptr() + 8)
    return _bufs[frames]


def _env(monkeypatch, grid):
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1")
    if grid is None:
        monkeypatch.delenv("SDRGPU_FFT_1P_GRID", raising=False)
    else:
        monkeypatch.setenv("SDRGPU_FFT_1P_GRID", str(grid))


def _calls(f, start, frames, zoom, vfo):
    """The pre-call and the two calls of `frames` frames on plan f, the stream starting at device address
    `start`: per call the rows, the zoom rows (or None) and the VFO's output (or None) as uint32 bit patterns."""
    import torch
    v = dsp.RxVFO(FS, 240000, 200000, OFF) if vfo else None
    bufs = []
    for c in range(2):
        rows = torch.full((frames * N,), float("nan"), device="cuda")
        z = torch.full((frames * ZW,), float("nan"), device="cuda") if zoom else None
        vo = torch.zeros(2 * (frames * N // 256 + 64), device="cuda") if vfo else None
        bufs.append((rows, z, vo))
    scratch = torch.empty(2 * (frames * N // 256 + 64), device="cuda")
    torch.cuda.synchronize()   # (the library launches on its own stream: torch's fills are done first)
    if vfo:
        v.process_dev(start, PRE, scratch.data_ptr())
    res = []
    for c, (rows, z, vo) in enumerate(bufs):
        x_ptr = start + 8 * (PRE + c * frames * N)
        if vfo:
            m = f.execute_zoom_vfo_dev(x_ptr, frames, rows.data_ptr(), z.data_ptr() if zoom else 0, ZW, v, vo.data_ptr())
            assert m > 0
            vo = vo[:2 * m]
        elif zoom:
            assert f.execute_zoom_dev(x_ptr, N, frames, rows.data_ptr(), z.data_ptr(), ZW) == frames
        else:
            assert f.execute_dev(x_ptr, N, frames, rows.data_ptr()) == frames
        torch.cuda.synchronize()
        res.append(tuple(None if a is None else a.cpu().numpy().view(np.uint32) for a in (rows, z, vo)))
    return res


def _equal(got, ref, what):
    for c in range(2):
        for name, a, b in zip(("rows", "zoom rows", "VFO output"), got[c], ref[c]):
            assert (a is None) == (b is None)
            if a is not None:
                assert not np.any(a == 0x7FC00000) or name == "VFO output", f"call {c}: {name} not all written"
                np.testing.assert_array_equal(a, b, err_msg=f"call {c}: {name}, {what}")


# frames = 9 at the default grid: one item per workgroup, 14 padding items; frames = 24 at 16 workgroups: three
# items each (every slot reused across items, the prefetched first row sets); frames = 67 at 16: nine items each.
@pytest.mark.parametrize("frames,grid,zoom,vfo", [(9, None, z, v) for z, v in VARIANTS] + [(24, 16, z, v) for z, v in VARIANTS] +
                         [(67, 16, True, True)])
def test_ring_equals_register_path(frames, grid, zoom, vfo, monkeypatch):
    _env(monkeypatch, grid)
    (_, aligned), (_, shifted) = _buffers(frames)
    f = dsp.FFTSpectrum(N, N, 6)
    ring = _calls(f, aligned, frames, zoom, vfo)
    regs = _calls(f, shifted, frames, zoom, vfo)
    _equal(ring, regs, "LDS-DMA ring vs range-checked register loads")


@pytest.mark.parametrize("zoom,vfo", VARIANTS)
def test_ring_deterministic(zoom, vfo, monkeypatch):
    _env(monkeypatch, 16)
    (_, aligned), _ = _buffers(24)
    f = dsp.FFTSpectrum(N, N, 6)
    first = _calls(f, aligned, 24, zoom, vfo)
    for k in (1, 2):
        _equal(_calls(f, aligned, 24, zoom, vfo), first, f"run {k} vs run 0 on one plan")
