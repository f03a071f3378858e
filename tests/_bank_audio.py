"""Inputs and the event counter of tests/test_bank_audio.py (no GPU code here).

agc_bank: the AGC signal of every stream. With AM's AGC parameters (attack 50 / 48000, decay 5 / 48000, max
output 10) the running amplitude falls by a tenth over a 1024-row call at most, and a look-ahead event
sets it to the largest amplitude of the REST OF THE CALL: a call holds one event per stream at most (nothing
later in the call is ten times above it), and a later call has one only where a sample is ten times above
everything the earlier calls held. So the signal RISES: level steps of 26, 8 and 26 dB (60 dB in all), x50
spikes on top, and the events of the run in CUTS sit where the calls' ends put them. agc_events counts them.
"""
import numpy as np

f32 = np.float32
FRAMES = 4200
SMAX = 130
TILE = 32
AGC_ARGS = (1.0, 50.0 / 48000.0, 5.0 / 48000.0, 10e6, 10.0, float("inf"))     # am.h:27-49
# level steps: rows [from, to) at LEVELS; the step at row 3140 lies between the spikes at rows 32 * 98 and
# 32 * 98 + 20 = 3156, the last row (tile row 31) of the 32-row call of CUTS
STEPS = [0, 600, 2100, 3140, FRAMES]
LEVELS = [1e-3, 2e-2, 5e-2, 1.0]
ZEROS = (500, 540)                                                            # a run of exact zeros
SPIKE_TILES = [1, 20, 40, 70, 97, 98, 110, 130, 131]                          # a: spikes at rows 32a, 32a + 31, 32a + (k mod 32)


def spike_rows(k):
    rows = set()
    for a in SPIKE_TILES:
        rows |= {r for r in (TILE * a, TILE * a + TILE - 1, TILE * a + k % TILE) if r < FRAMES}
    return sorted(rows)


def agc_column(k, cplx):
    """Stream k: noise of magnitude 0.5..1 (seed 400 + k) times the level of its row and 0.5 + 0.25 (k mod 8); exact
    zeros over ZEROS; spikes of 50 times the row's level (x the stream's scale), signs alternating."""
    rng = np.random.default_rng(400 + k)
    mag = rng.uniform(0.5, 1.0, FRAMES)
    x = mag * np.exp(2j * np.pi * rng.uniform(0, 1, FRAMES)) if cplx else mag * rng.choice([-1.0, 1.0], FRAMES)
    level = np.empty(FRAMES)
    for lo, hi, L in zip(STEPS[:-1], STEPS[1:], LEVELS):
        level[lo:hi] = L
    x = x * level
    for j, r in enumerate(spike_rows(k)):
        x[r] = 50.0 * level[r] * (-1) ** j * ((1j if j % 3 == 0 else 1) if cplx else 1)
    x[ZEROS[0]:ZEROS[1]] = 0
    return (x * (0.5 + 0.25 * (k % 8))).astype(np.complex64 if cplx else f32)


def agc_bank(cplx):
    return np.ascontiguousarray(np.stack([agc_column(k, cplx) for k in range(SMAX)], axis=1))


def amplitude(X):
    """complex_t::amplitude() (types.h:79) / fabsf in float32"""
    if np.iscomplexobj(X):
        re, im = X.real.astype(f32), X.imag.astype(f32)
        return np.sqrt(re * re + im * im, dtype=f32)
    return np.abs(X).astype(f32)


def agc_events(X, cuts, set_point, attack, decay, max_gain, max_out, init_gain):
    """agc.h:88-147 (the enabled branch) restated in numpy float32 over all columns at once, to COUNT the
    clip look-ahead events of a fresh AGC fed X in calls of `cuts` rows: a list of (stream, call, row of the
    call, rows of the call). It checks no output."""
    A = amplitude(X)
    sp, att, dec, mg, mo = f32(set_point), f32(attack), f32(decay), f32(max_gain), f32(max_out)
    inv_att, inv_dec = f32(1) - att, f32(1) - dec
    events, i = [], 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        amp = np.full(A.shape[1], sp / f32(init_gain), f32)
        for c, n in enumerate(cuts):
            a = A[i:i + n]
            suffix = np.maximum.accumulate(a[::-1], axis=0)[::-1]
            for r in range(n):
                x = a[r]
                moved = np.where(x > amp, amp * inv_att + x * att, amp * inv_dec + x * dec).astype(f32)
                amp = np.where(x != 0, moved, amp)
                gain = np.where(x != 0, np.minimum(mg, sp / amp), f32(1)).astype(f32)
                fire = x * gain > mo
                amp = np.where(fire, suffix[r], amp)
                events += [(int(k), c, r, n) for k in np.nonzero(fire)[0]]
            i += n
    return events


# ------------------------------------------------------------------- squelch
SQ_LEVEL = -30.0
SQ_CALLS = [480] * 4 + [1] + [480] * 6 + [31] + [480] * 5 + [0] + [480] * 8 + [33] + [480] * 9 + [1, 480]


def squelch_loud(k, c):
    """Is call c of stream k loud? Five schedules, shifted by (k // 5) mod 4 calls:
    0 always loud; 1 quiet for two calls, then loud for good (muted, then the unmute count runs out once: after
    the call that starts the count, exactly 10 loud calls); 2 as 1 with one quiet call in the middle of the count
    (the count restarts); 3 quiet from the start, loud from call 2; 4 alternating blocks of 3 quiet and 12 loud."""
    kind, c = k % 5, c - (k // 5) % 4
    if kind == 0:
        return True
    if kind == 1:
        return not 3 <= c < 5
    if kind == 2:
        return not (3 <= c < 5 or c == 10)
    if kind == 3:
        return c >= 2
    return c % 15 >= 3


def squelch_calls(S=SMAX):
    """The calls' (frames, S) blocks. Every sample of stream k in call c has the magnitude of a level 6..7.75 dB above
    SQ_LEVEL (loud) or 8..9.75 dB below it (quiet), by k mod 8, and a random phase: the call's mean magnitude is that
    level within rounding, at least 1 dB from SQ_LEVEL and from SQ_LEVEL - 1."""
    rng = np.random.default_rng(77)
    calls = []
    for c, n in enumerate(SQ_CALLS):
        db = np.array([SQ_LEVEL + (6.0 + 0.25 * (k % 8) if squelch_loud(k, c) else -8.0 - 0.25 * (k % 8)) for k in range(S)])
        x = 10.0 ** (db / 20.0) * np.exp(2j * np.pi * rng.uniform(0, 1, (n, S)))
        calls.append(x.astype(np.complex64))
    return calls


# ---------------------------------------------------------------- composites
def fm_tone_bank(S, n, fs, tone_of, dev_hz, seed=9):
    """FM at deviation dev_hz by a tone of tone_of(k) Hz per stream, phase and amplitude per stream"""
    t = np.arange(n)
    X = np.empty((n, S), np.complex64)
    for k in range(S):
        msg = np.sin(2 * np.pi * tone_of(k) * t / fs + 0.37 * k)
        X[:, k] = ((0.3 + 0.1 * (k % 5)) * np.exp(1j * (2 * np.pi * dev_hz / fs * np.cumsum(msg) + 0.1 * k))).astype(np.complex64)
    return X


def am_burst_bank(S, n, fs, seed=11):
    """The signal of test_am_vs_oracle per stream: a carrier at 300 Hz, 60 % modulated by a tone of 500 + 40 k Hz,
    noise from seed + k, and a burst over rows 2000..2100 scaled x40 (the carrier AGC's look-ahead fires there: the
    burst is 40 times above what the AGC has seen)."""
    t = np.arange(n)
    X = np.empty((n, S), np.complex64)
    for k in range(S):
        rng = np.random.default_rng(seed + k)
        carrier = (1.0 + 0.6 * np.sin(2 * np.pi * (500 + 40 * k) * t / fs)) * np.exp(1j * (2 * np.pi * 300 * t / fs + 0.3 + 0.2 * k))
        x = (0.05 + 0.01 * (k % 4)) * carrier + 0.001 * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))
        x[2000:2100] *= 40
        X[:, k] = x.astype(np.complex64)
    return X
