"""Float64 numpy / scipy yardstick of the loudness unit, written from the definitions.

Meter (ITU-R BS.1770-4, mono): the K-weighting is a high-shelf and a high-pass, each the bilinear transform of its
analogue prototype (coefficients); the weighted signal goes through scipy.signal.sosfilt; hop = round(0.1 sr) samples;
hop_sums[h] = sum of squares over hop h; a block is 4 consecutive hops, z_j its mean square, l_j = -0.691 + 10 log10 z_j;
absolute gate l_j > -70, relative gate l_j > -0.691 + 10 log10(mean of the absolutely gated z) - 10; the integrated
loudness is -0.691 + 10 log10(mean of the z passing both), -inf when none does.

True peak: max(|x|, |the four phases of the project's 4x polyphase oversampler|) (resample_ref.taps(sr, 4 sr)).

Limiter: p[n] the true-peak envelope (the maximum above at sample n, x = 0 outside [0, L)); r = min(1, c / p), 1 outside
[0, L); m = the running minimum of r over |j| <= Lh on the extended range [-Lh, L - 1 + Lh]
(scipy.ndimage.minimum_filter1d on r padded with ones); g[n] = 1 - sum_{|j| <= Lh} w_j (1 - m[n + j]), w the 2 Lh + 1
non-zero points of a Hann window normalised to sum 1; y = g x.
"""
import math

import numpy as np
from scipy import ndimage, signal

import resample_ref as RR

TABLE_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285),
             "shelf_a": (-1.69065929318241, 0.73248077421585),
             "highpass_a": (-1.99004745483398, 0.99007225036621)}


def _biquad_a(f0, Q, sr):
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return K, a0, [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def coefficients(sr):
    """float64 [2, 5]: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K, a0, a = _biquad_a(f0, Q, sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0] + a
    _, _, a = _biquad_a(38.13547087602444, 0.5003270373238773, sr)
    return np.array([shelf, [1.0, -2.0, 1.0] + a], dtype=np.float64)


def hop_of(sr):
    return int(round(0.1 * sr))


def k_weight(x, sr):
    c = coefficients(sr)
    sos = np.array([[c[0, 0], c[0, 1], c[0, 2], 1.0, c[0, 3], c[0, 4]], [c[1, 0], c[1, 1], c[1, 2], 1.0, c[1, 3], c[1, 4]]])
    return signal.sosfilt(sos, np.asarray(x, dtype=np.float64), axis=-1)


def hop_sums(x, sr):
    """x [..., L] -> float64 [..., L // hop]."""
    x = np.asarray(x, dtype=np.float64)
    hop = hop_of(sr)
    nh = x.shape[-1] // hop
    if nh == 0:
        return np.zeros(x.shape[:-1] + (0,))
    y = k_weight(x, sr)[..., :nh * hop]
    return (y * y).reshape(x.shape[:-1] + (nh, hop)).sum(axis=-1)


def block_loudness(hs, sr):
    """(z, l) of the 400 ms blocks of one row's hop sums."""
    hs = np.asarray(hs, dtype=np.float64)
    if hs.size < 4:
        return np.zeros(0), np.zeros(0)
    z = (hs[:-3] + hs[1:-2] + hs[2:-1] + hs[3:]) / (4.0 * hop_of(sr))
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def gate(hs, sr):
    """{integrated LUFS, blocks passing both gates, relative threshold, blocks in all} of one row, plus the block
    loudnesses (for the distance of each block from the thresholds)."""
    z, l = block_loudness(hs, sr)
    a = l > -70.0
    if not a.any():
        return (-np.inf, 0, -np.inf, z.size), l
    thr = -0.691 + 10.0 * np.log10(z[a].mean()) - 10.0
    keep = a & (l > thr)
    integ = -0.691 + 10.0 * np.log10(z[keep].mean()) if keep.any() else -np.inf
    return (integ, int(keep.sum()), thr, z.size), l


def integrated_loudness(x, sr):
    return gate(hop_sums(x, sr), sr)[0][0]


def envelope(x, sr):
    """p[n] on [0, L): max(|x[n]|, |phase k of the 4x oversampler at n|), x zero outside."""
    x = np.asarray(x, dtype=np.float64)
    up, down, W, table = RR.taps(sr, 4 * sr)
    assert (up, down) == (4, 1)
    xp = np.concatenate([np.zeros(W), x, np.zeros(W)])
    p = np.abs(x)
    for k in range(4):
        p = np.maximum(p, np.abs(np.correlate(xp, table[k], mode="valid")))
    return p


def true_peak(x, sr):
    x = np.asarray(x, dtype=np.float64)
    return float(envelope(x, sr).max()) if x.size else 0.0


def hann_weights(Lh):
    """The 2 Lh + 1 non-zero points of a Hann window of 2 Lh + 3 points, normalised to sum 1."""
    w = np.hanning(2 * Lh + 3)[1:-1]
    return w / w.sum()


def limiter_gain(x, sr, ceiling, Lh):
    """(g, r) on [0, L) of the look-ahead limiter with the linear ceiling and a look-ahead of Lh samples."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    p = envelope(x, sr)
    with np.errstate(divide="ignore"):
        r = np.minimum(1.0, ceiling / p)
    rp = np.concatenate([np.ones(2 * Lh), r, np.ones(2 * Lh)])          # r on [-2 Lh, L - 1 + 2 Lh]
    m = ndimage.minimum_filter1d(rp, 2 * Lh + 1, mode="constant", cval=1.0)[Lh:Lh + L + 2 * Lh]   # m on [-Lh, L - 1 + Lh]
    g = 1.0 - np.correlate(1.0 - m, hann_weights(Lh), mode="valid")
    assert g.shape == (L,)
    return g, r


def limit(x, sr, ceiling, Lh):
    g, _ = limiter_gain(x, sr, ceiling, Lh)
    return g * np.asarray(x, dtype=np.float64), g


# ---- signals shared by the CPU and GPU tests ------------------------------------------------------------------------
def sine(freq, seconds, sr, amp=1.0, phase=0.0):
    return amp * np.sin(2.0 * np.pi * freq * np.arange(int(round(seconds * sr))) / sr + phase)


def intersample_sine(sr, amp, seconds=0.2, ramp=0.02):
    """A sine at sr / 4 with phase 45 degrees, faded in and out over `ramp` seconds (an abrupt end rings above amp):
    its samples are +-amp / sqrt(2) in the flat part, its true peak is amp."""
    x = sine(sr / 4.0, seconds, sr, amp=amp, phase=np.pi / 4.0)
    n = int(round(ramp * sr))
    fade = 0.5 - 0.5 * np.cos(np.pi * np.arange(n) / n)
    x[:n] *= fade
    x[-n:] *= fade[::-1]
    return x


def gated_signal(sr, loud=0.25, drop_db=35.0, seconds=(0.9, 0.7, 0.4)):
    """A loud 997 Hz section, one drop_db quieter, then digital silence."""
    a, b, c = (int(round(s * sr)) for s in seconds)
    t = sine(997.0, seconds[0] + seconds[1], sr)
    quiet = loud * 10.0 ** (-drop_db / 20.0)
    return np.concatenate([loud * t[:a], quiet * t[a:a + b], np.zeros(c)])


def threshold_margin(l, thr):
    """The smallest distance in LU of a finite block loudness from -70 and from the relative threshold."""
    f = l[np.isfinite(l)]
    return float(min(np.abs(f + 70.0).min(), np.abs(f - thr).min())) if f.size else np.inf
