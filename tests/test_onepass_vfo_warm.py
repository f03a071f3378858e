"""The one-pass 64k kernel's fused VFO half along the persistent walk (fft_1p_kernel, round 20): the segments'
coarse NCO phasors come from a table the workgroup fills once per launch (items of a walk beyond the table form
them in place). That may not change a bit:
rows, zoom rows and the VFO's output are compared, as uint32 patterns, with one item per workgroup
(SDRGPU_FFT_1P_GRID=0), and the VFO's output with RxVFO.process_dev on the same input, over two consecutive
calls behind a ragged pre-call (a history and a non-zero decimation phase). Walks at 16 workgroups of two,
three and nine items and of more items than the table holds; the default grid (the first-item path); and
pre-call lengths / VFO offsets at which a coarse-index boundary lies inside a round-0 segment's window and the
first segment reaches back into the history."""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import iq

pytestmark = pytest.mark.gpu

N, ZW = 65536, 2048
FS, OUT_SR, BW = 61.44e6, 240000, 200000
PRE, OFF = 1000, 2.5e6
NCO_LO = 4096                 # input samples per coarse NCO index (nco_value.h)
SEG, ROWS, D = 1024, 36, 32   # a VFO segment: 32 outputs of the 32-fold decimator, 32 + 5 - 1 rows of 32 samples
# the table holds one entry per thread of the prologue (512); an item's 32 segment starts span 31 SEG + 32 samples,
# so they take at most (31 SEG + 31) // NCO_LO + 2 coarse indices
TABLE_ITEMS = 512 // ((31 * SEG + 31) // NCO_LO + 2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"
    yield
    _inputs.clear()   # (the longest walk's input and references are a few hundred MB)
    _refs.clear()


_inputs, _refs = {}, {}


def _input(frames, pre):
    if (frames, pre) not in _inputs:
        import torch
        x = iq(np.random.default_rng(0x2000 + frames + pre), pre + 2 * frames * N)
        _inputs[frames, pre] = torch.from_numpy(x.view(np.float32)).cuda()
        torch.cuda.synchronize()
    return _inputs[frames, pre]


def _run(monkeypatch, grid, frames, zoom, pre=PRE, off=OFF):
    """The pre-call and two consecutive fused calls on one plan under SDRGPU_FFT_1P_GRID=grid (None: unset): per
    call (rows, zoom rows or None, VFO output) as uint32, and the separate VFO's output over the same calls."""
    import torch
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1")
    if grid is None:
        monkeypatch.delenv("SDRGPU_FFT_1P_GRID", raising=False)
    else:
        monkeypatch.setenv("SDRGPU_FFT_1P_GRID", str(grid))
    d_x = _input(frames, pre)
    f = dsp.FFTSpectrum(N, N, 6)
    v, sep = dsp.RxVFO(FS, OUT_SR, BW, off), dsp.RxVFO(FS, OUT_SR, BW, off)
    nout = 2 * (frames * N // 256 + 64)
    scratch = torch.empty(nout, device="cuda")
    bufs = []
    for c in range(2):   # (filled and synchronised before the library, on its own stream, writes them)
        bufs.append((torch.full((frames * N,), float("nan"), device="cuda"),
                     torch.full((frames * ZW,), float("nan"), device="cuda") if zoom else None,
                     torch.zeros(nout, device="cuda"), torch.zeros(nout, device="cuda")))
    torch.cuda.synchronize()
    v.process_dev(d_x.data_ptr(), pre, scratch.data_ptr())
    sep.process_dev(d_x.data_ptr(), pre, scratch.data_ptr())
    res, seps = [], []
    for c, (rows, z, vo, so) in enumerate(bufs):
        x_ptr = d_x.data_ptr() + 8 * (pre + c * frames * N)
        m = f.execute_zoom_vfo_dev(x_ptr, frames, rows.data_ptr(), z.data_ptr() if zoom else 0, ZW, v, vo.data_ptr())
        ms = sep.process_dev(x_ptr, frames * N, so.data_ptr())
        assert m == ms and m > 0
        torch.cuda.synchronize()
        seps.append(so[:2 * ms].cpu().numpy().view(np.uint32))
        res.append(tuple(None if a is None else a.cpu().numpy().view(np.uint32) for a in (rows, z, vo[:2 * m])))
    return res, seps


def _check(monkeypatch, grid, frames, zoom, pre=PRE, off=OFF):
    key = (frames, zoom, pre, off)
    if key not in _refs:   # one item per workgroup, computed once per shape
        _refs[key] = _run(monkeypatch, 0, frames, zoom, pre, off)[0]
    ref = _refs[key]
    got, seps = _run(monkeypatch, grid, frames, zoom, pre, off)
    for c in range(2):
        for name, a, b in zip(("rows", "zoom rows", "VFO output"), got[c], ref[c]):
            assert (a is None) == (b is None)
            if a is not None:
                assert not np.any(a == 0x7FC00000) or name == "VFO output", f"call {c}: {name} not all written"
                np.testing.assert_array_equal(a, b, err_msg=f"call {c}: {name} vs one item per workgroup")
        np.testing.assert_array_equal(got[c][2], seps[c], err_msg=f"call {c}: fused VFO vs RxVFO.process_dev")


# At 16 workgroups a workgroup walks ceil(frames / 8) items. frames = 9: two, most second items padding; 24: three;
# 67: nine (the table across eight item changes); 8 TABLE_ITEMS + 3: one more item than the table holds, its last
# real frames on the in-place path (the seam between the two). None: the default grid (one item per workgroup at
# this size on a 256-CU device: the walk's first item, table item 0).
@pytest.mark.parametrize("zoom", [True, False])
@pytest.mark.parametrize("frames,grid", [(9, 16), (24, 16), (67, 16), (8 * TABLE_ITEMS + 3, 16), (67, None)])
def test_vfo_walk_bit_identical(frames, grid, zoom, monkeypatch):
    if grid == 16:
        assert ((frames + 7) // 8 > TABLE_ITEMS) == (frames > 8 * TABLE_ITEMS)
    _check(monkeypatch, grid, frames, zoom)


def _geometry(pre):
    """H of the VFO's first stage and its decimation phase behind a first call of `pre` samples: segment s of
    the next call reads the input indices SEG s + phase - H .. + ROWS D - 1 and takes its coarse index at the
    first 32 of them."""
    d0, taps = dsp.decim_plan(int(round(FS / OUT_SR)))[0]
    assert d0 == D and ROWS == SEG // D + (len(taps) + D - 1) // D - 1, "the fused first stage: 32-fold, 5 taps per phase"
    return len(taps) - 1, -pre % D


@pytest.mark.parametrize("pre,off", [(1000, 2.5e6), (1013, -7.3e6)])
def test_vfo_coarse_index_boundaries(pre, off, monkeypatch):
    """A 4096-sample coarse-index boundary inside a round-0 segment of the first frame (the segment's phasor is
    the one of its first samples, below the boundary), and the first segment's window reaching back into the
    history (a negative input index: coarse index -1, the floor of i / 4096)."""
    H, phase = _geometry(pre)
    c = phase - H                                            # input index of segment 0's first sample
    round0 = [s for half in (0, 32) for s in range(half, half + 16)]   # the segments of the two items' round 0
    crossing = [s for s in round0 if (SEG * s + c) // NCO_LO != (SEG * s + c + ROWS * D - 1) // NCO_LO]
    assert crossing, "no round-0 segment of the first frame spans a coarse-index boundary"
    assert c < 0 and (c + D - 1) // NCO_LO == -1, "the first segment does not start inside the history"
    _check(monkeypatch, 16, 9, True, pre, off)
