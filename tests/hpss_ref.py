"""The yardstick of the harmonic / percussive separation: scipy's median filter and float64 numpy
restatements of librosa's softmask and of the mel energy share, with the synthetic sine-plus-clicks signal and the
seeded inputs the CPU and GPU tests share."""
import numpy as np
import scipy.ndimage

import audio_ref as R

SR, N_FFT, HOP = 22050, 2048, 512
TINY = float(np.finfo(np.float32).tiny)


def median_filter_direct(x, win, axis):
    """scipy.ndimage.median_filter(mode="reflect") as it stands, along frequency (axis 0) or time (axis 1) of every
    item of x [B, F, T] (or [F, T])."""
    x = np.asarray(x)
    size = [1] * x.ndim
    size[x.ndim - 2 + axis] = int(win)
    return scipy.ndimage.median_filter(x, size=tuple(size), mode="reflect")


def scipy_reflect_is_sound(n, win):
    """Whether scipy's own reflection can be trusted for an axis of n samples and this window.  scipy 1.15 folds a
    window position p < -2n as p += 2n (-p // 2n) and then takes -p - 1 for -n <= p <= 0: a position that is a
    multiple of the period 2n (below -2n) lands on index -1, one sample in front of the array, and the "median"
    then depends on memory that is not the input.  That needs win // 2 >= 4n; every shorter window is sound."""
    return int(win) // 2 < 4 * int(n)


def median_filter(x, win, axis):
    """scipy.ndimage.median_filter's median with mode="reflect" as scipy documents it (d c b a | a b c d | d c b a),
    along frequency (axis 0) or time (axis 1) of every item of x [B, F, T] (or [F, T]); x's dtype is kept, so a float32
    input gives the float32 sample scipy selects.  The axis is continued explicitly (numpy's "symmetric" padding is
    that definition, reflecting as often as the halo needs) and scipy filters the padded array, so its reflection
    bug for windows of 8 axis lengths or more (scipy_reflect_is_sound) is not part of the yardstick; wherever scipy's
    own reflection is sound the two are the same call (tests/test_hpss_cpu.py holds them to array_equal)."""
    x = np.asarray(x)
    ax = x.ndim - 2 + axis
    h = int(win) // 2
    pad = [(0, 0)] * x.ndim
    pad[ax] = (h, h)
    out = median_filter_direct(np.pad(x, pad, mode="symmetric"), win, axis)
    return np.ascontiguousarray(np.take(out, np.arange(h, h + x.shape[ax]), axis=ax))


def softmask(X, Xref, power):
    """(X/Z)^p / ((X/Z)^p + (Xref/Z)^p) with Z = max(X, Xref), 0.5 where Z is below the smallest normal fp32."""
    X, Xref = np.asarray(X, dtype=np.float64), np.asarray(Xref, dtype=np.float64)
    Z = np.maximum(X, Xref)
    bad = Z < TINY
    Zs = np.where(bad, 1.0, Z)
    a, r = (X / Zs) ** power, (Xref / Zs) ** power
    den = np.where(bad, 1.0, a + r)
    return np.where(bad, 0.5, a / den)


def masks_from_medians(harm, perc, power=2.0, margin_h=1.0, margin_p=1.0):
    """(mask_h, mask_p) float64 of the two median-filtered spectrograms; the margins multiply the float32 medians the
    way the device does (one fp32 rounding), everything after it is float64."""
    harm32, perc32 = np.asarray(harm, dtype=np.float32), np.asarray(perc, dtype=np.float32)
    rp = (np.float32(margin_h) * perc32).astype(np.float64)
    rh = (np.float32(margin_p) * harm32).astype(np.float64)
    return softmask(harm32, rp, power), softmask(perc32, rh, power)


def hpss_masks(S, kernel_size=31, power=2.0, margin=1.0):
    """(mask_h, mask_p) float64 of a magnitude spectrogram S (float32 [.., F, T]): harmonic median along time,
    percussive along frequency."""
    wins = kernel_size if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    mar = margin if isinstance(margin, (tuple, list)) else (margin, margin)
    S = np.asarray(S, dtype=np.float32)
    return masks_from_medians(median_filter(S, wins[0], 1), median_filter(S, wins[1], 0), power, mar[0], mar[1])


def mel_lohi(M):
    """Each filter's bin range [lo, hi) (int32 [n_mels, 2]), as ldm_amd.audio._mel_host's."""
    lohi = np.zeros((M.shape[0], 2), dtype=np.int32)
    for m in range(M.shape[0]):
        nz = np.flatnonzero(M[m])
        if nz.size:
            lohi[m] = (nz[0], nz[-1] + 1)
    return lohi


def mask_mel_share(P, mask, M):
    """(M (mask P)) / (M P) per [.., n_mels, T] in float64 from the float32 operands; 0.5 where the denominator is
    below the smallest normal fp32."""
    P, mask, M = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (P, mask, M))
    num, den = M @ (mask * P), M @ P
    bad = den < TINY
    return np.where(bad, 0.5, num / np.where(bad, 1.0, den))


# ---- the sine plus clicks ------------------------------------------------------------------------------------
CLICK_SECONDS = (0.4, 0.9, 1.5, 2.1, 2.6)
SINE_HZ, SINE_AMP = 440.0, 0.5


def sine_clicks(seconds=3.0):
    """(y float32 [L], click frames): a 440 Hz sine at 0.5 plus five unit clicks, each placed on a frame centre."""
    L = int(seconds * SR)
    y = SINE_AMP * np.sin(2.0 * np.pi * SINE_HZ * np.arange(L) / SR)
    frames = [int(round(s * SR / HOP)) for s in CLICK_SECONDS]
    for f in frames:
        y[f * HOP] += 1.0
    return y.astype(np.float32), np.asarray(frames)


def sine_bin():
    return int(round(SINE_HZ * N_FFT / SR))


def sine_clicks_regions(T, frames):
    """(frames more than 4 away from every click, the click frames) as index arrays."""
    t = np.arange(T)
    far = np.all(np.abs(t[:, None] - frames[None, :]) > 4, axis=1)
    return np.flatnonzero(far), frames


def check_sine_clicks_masks(mask_h, mask_p, frames):
    """The two separation conditions of the sine plus clicks; returns the two measured minima."""
    mask_h, mask_p = np.asarray(mask_h, dtype=np.float64), np.asarray(mask_p, dtype=np.float64)
    far, clicks = sine_clicks_regions(mask_h.shape[-1], frames)
    h_min = float(mask_h[sine_bin(), far].min())
    p_min = float(mask_p[100:1001][:, clicks].min())
    return h_min, p_min


def sine_clicks_magnitude():
    """(|STFT| float32 [1025, T], click frames) of the sine plus clicks through the float64 STFT of audio_ref."""
    y, frames = sine_clicks()
    C = R.stft(y.astype(np.float64), n_fft=N_FFT)
    return np.abs(C).astype(np.float32), frames
