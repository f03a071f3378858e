"""The one-pass 64k kernel's persistent walk (fft_1p_kernel, SDRGPU_FFT_1P_GRID): G item workgroups walk
the 2 x 8 x ceil(frames / 8) items with a stride of G, the tables staged once per workgroup and each next
item's first ring row sets issued under the current item's store burst. The per-item arithmetic is that
of one item per workgroup (SDRGPU_FFT_1P_GRID=0), so every output is compared bit for bit with that launch:
rows, zoom rows and the fused VFO's output, over walks of two, three and nine items, uneven walks, padding
items in the middle and at the end of a walk, the default (co-resident) grid, the range-checked (PAD)
instantiations, and two consecutive calls on one plan. The fused VFO starts from a ragged 1,000-sample
call, so it carries a history and a non-zero decimation phase into the walk, and its output also equals
RxVFO.process_dev's on the same input."""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import iq

pytestmark = pytest.mark.gpu

N, ZW, PRE = 65536, 2048, 1000
FS, OFF = 61.44e6, 2.5e6
VARIANTS = [(zoom, vfo) for zoom in (True, False) for vfo in (True, False)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


_inputs, _refs = {}, {}


def _input(frames):
    """The ragged VFO pre-call, then two calls of `frames` frames (+ 1 sample: the offset-base case)."""
    if frames not in _inputs:
        import torch
        x = iq(np.random.default_rng(0x1F00 + frames), PRE + 2 * frames * N + 1)
        _inputs[frames] = torch.from_numpy(x.view(np.float32)).cuda()
        torch.cuda.synchronize()
    return _inputs[frames]


def _run(monkeypatch, grid, frames, zoom, vfo, nz=N, shift=0):
    """Two consecutive calls on one plan under SDRGPU_FFT_1P_GRID=grid (None: unset, the default grid):
    per call the rows, the zoom rows (or None) and the VFO's output (or None), as uint32 bit patterns. With
    the VFO, its separate form (RxVFO.process_dev over the same three calls) comes back as well."""
    import torch
    monkeypatch.setenv("SDRGPU_TUNING", "1")
    monkeypatch.setenv("SDRGPU_FFT_1P", "1")
    if grid is None:
        monkeypatch.delenv("SDRGPU_FFT_1P_GRID", raising=False)
    else:
        monkeypatch.setenv("SDRGPU_FFT_1P_GRID", str(grid))
    d_x = _input(frames)
    base = d_x.data_ptr() + 8 * (PRE + shift)
    f = dsp.FFTSpectrum(N, nz, 6)
    v = dsp.RxVFO(FS, 240000, 200000, OFF) if vfo else None
    sep = dsp.RxVFO(FS, 240000, 200000, OFF) if vfo else None
    scratch = torch.empty(2 * (frames * N // 256 + 64), device="cuda")
    # The library launches on its own stream, torch fills and copies on its default one: every buffer is
    # filled and synchronised before the library's calls write it, and read only after a synchronise
    # (a fill that runs after the library's kernel would leave zeros in place of its output).
    bufs = []
    for c in range(2):
        rows = torch.full((frames * N,), float("nan"), device="cuda")
        z = torch.full((frames * ZW,), float("nan"), device="cuda") if zoom else None
        vo = torch.zeros(2 * (frames * N // 256 + 64), device="cuda") if vfo else None
        so = torch.zeros_like(vo) if vfo else None
        bufs.append((rows, z, vo, so))
    torch.cuda.synchronize()
    if vfo:
        v.process_dev(d_x.data_ptr(), PRE, scratch.data_ptr())
        sep.process_dev(d_x.data_ptr(), PRE, scratch.data_ptr())
    res, seps = [], []
    for c, (rows, z, vo, so) in enumerate(bufs):
        x_ptr = base + 8 * c * frames * N
        if vfo:
            m = f.execute_zoom_vfo_dev(x_ptr, frames, rows.data_ptr(), z.data_ptr() if zoom else 0, ZW, v, vo.data_ptr())
            ms = sep.process_dev(x_ptr, frames * N, so.data_ptr())
            assert m == ms and m > 0
            torch.cuda.synchronize()
            seps.append(so[:2 * ms].cpu().numpy().view(np.uint32))
            vo = vo[:2 * m]
        elif zoom:
            assert f.execute_zoom_dev(x_ptr, N, frames, rows.data_ptr(), z.data_ptr(), ZW) == frames
        else:
            assert f.execute_dev(x_ptr, N, frames, rows.data_ptr()) == frames
        torch.cuda.synchronize()
        res.append(tuple(None if a is None else a.cpu().numpy().view(np.uint32) for a in (rows, z, vo)))
    return res, seps


def _reference(monkeypatch, frames, zoom, vfo, nz=N, shift=0):
    """The same calls with one item per workgroup (SDRGPU_FFT_1P_GRID=0), computed once per shape."""
    key = (frames, zoom, vfo, nz, shift)
    if key not in _refs:
        _refs[key] = _run(monkeypatch, 0, frames, zoom, vfo, nz, shift)[0]
    return _refs[key]


def _check(monkeypatch, grid, frames, zoom, vfo, nz=N, shift=0):
    ref = _reference(monkeypatch, frames, zoom, vfo, nz, shift)
    got, seps = _run(monkeypatch, grid, frames, zoom, vfo, nz, shift)
    for c in range(2):
        for name, a, b in zip(("rows", "zoom rows", "VFO output"), got[c], ref[c]):
            assert (a is None) == (b is None)
            if a is not None:
                assert not np.any(a == 0x7FC00000) or name == "VFO output", f"call {c}: {name} not all written"
                np.testing.assert_array_equal(a, b, err_msg=f"call {c}: {name} vs one item per workgroup")
        if vfo:
            np.testing.assert_array_equal(got[c][2], seps[c], err_msg=f"call {c}: fused VFO vs RxVFO.process_dev")
    if not vfo:   # (stateless: the second call ran on the next frames; the first call's frames again give its bits)
        again, _ = _run(monkeypatch, grid, frames, zoom, vfo, nz, shift)
        for a, b in zip(again[0], got[0]):
            if a is not None:
                np.testing.assert_array_equal(a, b)


# frames = 9: 32 items, 14 of them padding; 16 workgroups walk two items each, most second items padding.
# frames = 24: 48 items; three items per workgroup at 16, an uneven 2 / 1 split at 32.
# frames = 67: 144 items, 10 of them padding; nine items per workgroup at 16 (the staged tables and stale ring
# slots survive eight item changes), three at 48. None: the default grid (one item per workgroup at these sizes
# on a 256-CU device, the walk's first-item path).
@pytest.mark.parametrize("zoom,vfo", VARIANTS)
@pytest.mark.parametrize("frames,grid", [(9, 16), (9, None), (24, 16), (24, 32), (24, None), (67, 16), (67, 48),
                                         (67, None)])
def test_walk_bit_identical(frames, grid, zoom, vfo, monkeypatch):
    _check(monkeypatch, grid, frames, zoom, vfo)


@pytest.mark.parametrize("zoom,vfo,nz,shift", [(True, False, 60000, 0), (False, False, 60000, 0), (True, True, N, 1),
                                               (False, True, N, 1), (True, False, N, 1)])
@pytest.mark.parametrize("frames,grid", [(24, 16), (67, 16), (67, None)])
def test_walk_padded_bit_identical(frames, grid, zoom, vfo, nz, shift, monkeypatch):
    """The range-checked instantiations: zero-padded frames (nz = 60,000) and a frame base offset by one
    sample (not 16-byte aligned)."""
    _check(monkeypatch, grid, frames, zoom, vfo, nz, shift)
