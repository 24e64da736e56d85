"""Float64 numpy yardstick of the resampler and the silence trim, written from the definitions.

Resampler: g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g; Z = 32 zero crossings, beta = 14.769656459379492,
rolloff = 0.945; fc = min(1, up / down) * rolloff; W = ceil(Z / fc);
h(t) = fc sinc(fc t) I0(beta sqrt(1 - (t fc / Z)^2)) / I0(beta) for |t| <= Z / fc, else 0 (numpy's normalised sinc);
y[n] = sum_{j=-W..W} x[i0 + j] h(j - p / up), i0 = floor(n down / up), p = (n down) mod up, x zero outside [0, L),
n < ceil(L up / down).

Trim (librosa 0.10 effects.trim): T = 1 + L // hop frames, frame t covers [t hop - frame/2, t hop + frame/2) with zero
padding, ms[t] its mean square; non-silent when max(ms[t], 1e-10) > max(max_t ms, 1e-10) * 10^(-top_db / 10);
(hop * first, min(L, hop * (last + 1))), (0, 0) when no frame passes.  An item whose loudest frame is at or below
the 1e-10 floor has no frame above the floor and is (0, 0) too (all-zero input).
"""
import math

import numpy as np

Z, BETA, ROLLOFF = 32, 14.769656459379492, 0.945


def ratio(sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def h(t, fc):
    """The filter at real positions t (input-sample units)."""
    t = np.asarray(t, dtype=np.float64)
    u = t * fc / Z
    w = np.i0(BETA * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(BETA)
    return np.where(np.abs(t) <= Z / fc, fc * np.sinc(fc * t) * w, 0.0)


def taps(sr_in, sr_out):
    """(up, down, W, table [up, 2W+1]) with table[p, j + W] = h(j - p / up)."""
    up, down = ratio(sr_in, sr_out)
    fc = min(1.0, up / down) * ROLLOFF
    W = int(math.ceil(Z / fc))
    table = np.empty((up, 2 * W + 1))
    for p in range(up):
        table[p] = h(np.arange(-W, W + 1) - p / up, fc)
    return up, down, W, table


def n_out(L, up, down):
    return -(-L * up // down)


def resample_at(x, sr_in, sr_out, ns):
    """The direct sum at output positions ns (python ints, any size) of the 1-D signal x."""
    up, down, W, table = taps(sr_in, sr_out)
    L = len(x)
    out = np.empty(len(ns))
    for k, n in enumerate(ns):
        n = int(n)
        i0, p = divmod(n * down, up)
        lo, hi = max(i0 - W, 0), min(i0 + W + 1, L)
        seg = np.asarray(x[lo:hi], dtype=np.float64)
        out[k] = np.dot(seg, table[p, lo - (i0 - W):hi - (i0 - W)]) if hi > lo else 0.0
    return out


def resample(x, sr_in, sr_out):
    """x [..., L] -> [..., ceil(L up / down)], float64."""
    x = np.asarray(x, dtype=np.float64)
    up, down = ratio(sr_in, sr_out)
    if up == down:
        return x.copy()
    flat = x.reshape(-1, x.shape[-1])
    ns = range(n_out(x.shape[-1], up, down))
    return np.stack([resample_at(row, sr_in, sr_out, ns) for row in flat]).reshape(x.shape[:-1] + (len(ns),))


def frame_ms(y, frame_length=2048, hop_length=512):
    y = np.asarray(y, dtype=np.float64)
    L = len(y)
    T = 1 + L // hop_length
    pad = np.concatenate([np.zeros(frame_length // 2), y, np.zeros(frame_length + T * hop_length)])
    return np.array([np.mean(pad[t * hop_length:t * hop_length + frame_length] ** 2) for t in range(T)])


def trim_db(y, frame_length=2048, hop_length=512):
    """Each frame's level in dB relative to the loudest (floored at 1e-10 either side), as trim compares them."""
    ms = frame_ms(y, frame_length, hop_length)
    return 10.0 * np.log10(np.maximum(ms, 1e-10)) - 10.0 * np.log10(max(ms.max(), 1e-10))


def trim(y, top_db=20, frame_length=2048, hop_length=512):
    """(start, end) of the 1-D signal y."""
    ms = frame_ms(y, frame_length, hop_length)
    mx = ms.max()
    if mx <= 1e-10:
        return 0, 0
    keep = np.flatnonzero(np.maximum(ms, 1e-10) > max(mx, 1e-10) * 10.0 ** (-top_db / 10.0))
    if keep.size == 0:
        return 0, 0
    return int(hop_length * keep[0]), int(min(len(y), hop_length * (keep[-1] + 1)))


# ---- signals shared by the CPU and GPU tests (built once per call, float64) ---------------------------------------
def trim_signal(sr=22050):
    """4096 zeros, 8192 samples of a 0.5-amplitude 441 Hz tone, 4096 samples of it at 1e-3: every edge on a multiple of
    512.  By the definition the frames that touch the loud part are 7 .. 25: bounds (3584, 13312)."""
    tone = np.sin(2.0 * np.pi * 441.0 * np.arange(8192 + 4096) / sr)
    return np.concatenate([np.zeros(4096), 0.5 * tone[:8192], 1e-3 * tone[8192:]])


TRIM_BOUNDS = (3584, 13312)


def dataset_signals():
    """The two recordings of the end-to-end test as int16 PCM: (stereo [L, 2] at 44100 Hz, mono [L] at 22050 Hz).
    Leading digital silence, then 7 s of tones.  The onset sits 256 samples past a multiple of 512 at 22050 Hz, so a
    trim frame overlaps the tones by nothing or by at least 256 of its 2048 samples (-9 dB): none is near -20 dB."""
    on = 512 * 21 + 256                       # 11008 samples of silence at 22050 Hz
    t2 = np.arange(7 * 22050) / 22050.0
    mono = np.concatenate([np.zeros(on), 0.5 * np.sin(2 * np.pi * 330.0 * t2) + 0.2 * np.sin(2 * np.pi * 2500.0 * t2)])
    t4 = np.arange(7 * 44100) / 44100.0
    left = np.concatenate([np.zeros(2 * on), 0.6 * np.sin(2 * np.pi * 440.0 * t4)])
    right = np.concatenate([np.zeros(2 * on), 0.4 * np.sin(2 * np.pi * 1320.0 * t4) + 0.1 * np.sin(2 * np.pi * 6000.0 * t4)])
    q = lambda v: np.round(v * 32767.0).astype(np.int16)   # noqa: E731
    return np.stack([q(left), q(right)], axis=1), q(mono)


def pcm_to_mono(pcm):
    """read_wav followed by .mean(axis=1): float32 mono of int16 PCM [L, ch] (or [L])."""
    x = np.asarray(pcm).reshape(len(pcm), -1).astype(np.float32) / np.float32(32768.0)
    return x.mean(axis=1, dtype=np.float32)
