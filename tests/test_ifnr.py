"""IF noise reduction on the device: noise_reduction::FMIF, NoiseBlanker and Squelch (libsdrgpu,
HIP) against numpy restatements of fm_if.h:45-77, noise_blanker.h:38-57 and squelch.h:33-63
(tests/_restated.py). The restatements and the FMIF bar are themselves held to the reference's own
headers, compiled over scalar stand-ins for VOLK and FFTW (oracle/ref_blocks.cpp), by
tests/test_ref_blocks.py.

Bars:
* FMIF -- the FIR bar of tests/_util.py: atol = 8 eps32 sqrt(B) sum|w| max|x| against an fp64
  restatement (sliding windows x the f32 window values, np.fft.fft in complex128). The block keeps
  ONE bin per sample, the largest; when the two largest magnitudes are closer than 2 atol (each may
  move by atol) the choice is not decidable in fp32 and the output is then held to the reference
  value of SOME bin within 2 atol of the maximum. That gate may cover at most 1 % of a case.
  Outputs are bit-identical however the stream is cut into calls.
* NoiseBlanker -- bit-exact (the reference recurrence in the reference's operation order).
* Squelch -- every block is bit-identical to its input or to zeros as the restated state machine
  says; the levels keep >= 0.05 dB from both thresholds so f32 summation order cannot flip one.
"""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32, iq
from _restated import (fmif_cuts, fm_two_tone, fmif_inputs, fmif_atol, fmif_check, bursty, NoiseBlankerRef, SquelchRef,
                       noise_at, SQ_SEQUENCE)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


# ------------------------------------------------------------------ FMIF
def run_cut(blk, x, cuts):
    outs, i = [], 0
    for c in cuts:
        outs.append(blk.process(x[i:i + c]))
        assert outs[-1].shape == (c,)
        i += c
    assert i == len(x)
    return np.concatenate(outs)


@pytest.mark.parametrize("kind", ["fm", "uniform"])
@pytest.mark.parametrize("B", [3, 9, 15, 16, 31, 32])
def test_fmif_vs_fp64(B, kind):
    x = fmif_inputs(kind)
    cut = run_cut(dsp.FMIF(B), x, fmif_cuts(B))
    share = fmif_check(cut, x, B, f"B={B} {kind}")
    # cut-independence: bit-identical to one call on a fresh handle
    whole = dsp.FMIF(B).process(x)
    assert np.array_equal(cut.view(np.uint32), whole.view(np.uint32)), "output depends on how the stream is cut"
    assert share <= 0.01, f"undecidable share {share:.4%} > 1 %"


def test_fmif_set_bins_and_reset():
    x = fmif_inputs("uniform")[:3000]
    fresh15 = dsp.FMIF(15).process(x)
    f = dsp.FMIF(32)
    f.process(x[:1500])
    f.set_bins(15)
    assert np.array_equal(f.process(x).view(np.uint32), fresh15.view(np.uint32)), "set_bins must clear the history"
    f.process(x[:777])
    f.reset()
    assert np.array_equal(f.process(x).view(np.uint32), fresh15.view(np.uint32)), "reset must clear the history"
    with pytest.raises(sdrpp_amd.SdrGpuError):
        f.set_bins(33)
    assert np.array_equal(f.process(x[:100]).view(np.uint32), dsp.FMIF(15).process(np.concatenate([x, x[:100]]))[-100:].view(np.uint32))


def test_fmif_passes_an_on_bin_tone():
    """What the block is for: a clean tone on bin 5 of 32 comes out as sum(w) x the delayed input, once
    the window is full. Window i covers x[i - 31 .. i] and the output is sample B/2 = 16 of the peak
    bin's back transform, i.e. x[i - 31 + 16] = x[i - 15]: X_i[5] = sum(w) e^{j 2 pi 5 (i - 31) / 32}
    and the factor e^{j 2 pi 5 16 / 32} advances it by 16."""
    B, n = 32, 2000
    t = np.arange(n)
    x = np.exp(2j * np.pi * 5 * t / B).astype(np.complex64)
    y = dsp.FMIF(B).process(x)
    sw = dsp.fmif_window(B).astype(np.float64).sum()
    want = sw * x[B - 1 - 15:n - 15].astype(np.complex128)
    err = np.abs(y[B - 1:].astype(np.complex128) - want).max()
    print(f"on-bin tone: max err {err:.3e}, atol {fmif_atol(B, x):.3e}")
    assert err <= fmif_atol(B, x)


# ------------------------------------------------------------------ NoiseBlanker
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("rate,level", [(500.0 / 24000.0, 10.0), (500.0 / 250000.0, 2.0)])
def test_noise_blanker_bit_exact(rate, level):
    n = 20000
    x = bursty(np.random.default_rng(77), n)
    g, r = dsp.NoiseBlanker(rate, level), NoiseBlankerRef(rate, level)
    cuts = [1, 1023, 1024, 1025, 0, 37]
    i, blanked = 0, 0
    for c in cuts + [n - sum(cuts)]:
        a, b = g.process(x[i:i + c]), r.process(x[i:i + c])
        assert same_bits(a, b), f"block at {i}: max diff {np.abs(a - b).max()}"
        blanked += int(np.sum(a != x[i:i + c]))
        i += c
    assert blanked > 0, "the input never tripped the blanker"


def test_noise_blanker_set_keeps_amp_and_reset_restores_it():
    x = bursty(np.random.default_rng(78), 6000)
    g, r = dsp.NoiseBlanker(500.0 / 24000.0, 10.0), NoiseBlankerRef(500.0 / 24000.0, 10.0)
    assert same_bits(g.process(x[:2000]), r.process(x[:2000]))
    for o in (g, r):
        o.set(500.0 / 250000.0, 2.0)                        # setRate / setLevel: amp is kept
    assert same_bits(g.process(x[2000:4000]), r.process(x[2000:4000]))
    assert r.amp != np.float32(1.0)
    for o in (g, r):
        o.reset()
    assert same_bits(g.process(x[4000:]), r.process(x[4000:]))
    # after reset the block is a fresh one with the current settings
    assert same_bits(dsp.NoiseBlanker(500.0 / 250000.0, 2.0).process(x[4000:]),
                     NoiseBlankerRef(500.0 / 250000.0, 2.0).process(x[4000:]))


# ------------------------------------------------------------------ Squelch
def squelch_run(g, r, blocks):
    for j, x in enumerate(blocks):
        a, b = g.process(x), r.process(x)
        level, L = r.levels[-1]
        # precondition: f32 summation order cannot flip a decision
        assert min(abs(level - L), abs(level - (L - 1.0))) >= 0.05, (j, level, L)
        assert same_bits(a, b), f"block {j} (level {level:.2f} dB): expected {'zeros' if r.muted else 'the input'}"
        assert g.is_muted() == r.muted, j


def test_squelch_sequence():
    rng = np.random.default_rng(99)
    blocks = [noise_at(rng, db) for db in SQ_SEQUENCE]
    g, r = dsp.Squelch(-30.0), SquelchRef(-30.0)
    squelch_run(g, r, blocks)
    ref = SquelchRef(-30.0)
    trace = [bool(np.any(ref.process(b) != 0)) for b in blocks]
    # open; -45 mutes (cnt = 0); the first -20 sets cnt = 10, so the 11th passes; -30.5 is inside the
    # hysteresis; -45 mutes; 3 x -20 count to 8; -40 sets cnt = 10 again, so the 10th -20 after it passes
    want = [True, False] + [False] * 10 + [True, True, False] + [False] * 3 + [False] + [False] * 9 + [True, True]
    assert trace == want                                   # the sequence exercises what it is meant to
    assert g.process(blocks[0][:0]).shape == (0,)          # count == 0 is a no-op
    assert g.is_muted() == r.muted
    g.reset()
    assert not g.is_muted()
    assert same_bits(g.process(blocks[0]), blocks[0])


def test_squelch_set_level_and_per_handle_count():
    rng = np.random.default_rng(100)
    g, r = dsp.Squelch(-30.0), SquelchRef(-30.0)
    x25 = noise_at(rng, -25.0)
    squelch_run(g, r, [x25])
    assert not r.muted
    for o in (g, r):
        o.set_level(-20.0)                                  # takes effect at the next call
    squelch_run(g, r, [x25])
    assert r.muted
    # g is now muted and counting; a second handle runs its own count, interleaved call by call
    for o in (g, r):
        o.set_level(-30.0)
    g2, r2 = dsp.Squelch(-30.0), SquelchRef(-30.0)
    seq2 = [-45.0] + [-20.0] * 11
    for j, db in enumerate(seq2):
        xa, xb = noise_at(rng, -20.0), noise_at(rng, db)
        squelch_run(g, r, [xa])
        squelch_run(g2, r2, [xb])
    assert not r.muted and not r2.muted


# ------------------------------------------------------------------ composition
def test_chain_on_one_stream_matches_block_by_block():
    """NoiseBlanker -> Squelch -> FMIF(32) -> BroadcastFM with process_dev on one stream, 3 blocks of
    4096 with no host synchronise in between, against the same blocks through process()."""
    import torch
    n, nb = 4096, 3
    rng = np.random.default_rng(5)
    x = fm_two_tone(rng, n * nb)

    def chain():
        return [dsp.NoiseBlanker(500.0 / 250000.0, 10.0), dsp.Squelch(-30.0), dsp.FMIF(32),
                dsp.BroadcastFM(75e3, 250e3)]
    host = []
    blocks = chain()
    for j in range(nb):
        y = x[j * n:(j + 1) * n]
        for b in blocks:
            y = b.process(y)
        host.append(y)
    host = np.concatenate(host)
    assert host.shape == (n * nb,) and np.any(host["l"] != 0)

    blocks = chain()
    s = torch.cuda.Stream()
    d_in = torch.from_numpy(x.view(np.float32).copy()).cuda()
    tmp = [torch.zeros(2 * n, dtype=torch.float32, device="cuda") for _ in range(3)]
    d_out = torch.zeros(2 * n * nb, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for j in range(nb):
        src = d_in.data_ptr() + 8 * n * j
        for b, dst in zip(blocks, [t.data_ptr() for t in tmp] + [d_out.data_ptr() + 8 * n * j]):
            assert b.process_dev(src, n, dst, s.cuda_stream) == n
            src = dst
    s.synchronize()
    dev = d_out.cpu().numpy().view(dsp.STEREO)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
