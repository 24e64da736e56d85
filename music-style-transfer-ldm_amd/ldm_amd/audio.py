"""Audio front and back end on the GPU (csrc/audio.hip): STFT / ISTFT, mel spectrogram, dB, mel inversion and
Griffin-Lim with the defaults the reference relies on (librosa's): sr 22050, n_fft 2048, hop n_fft/4, periodic Hann,
centre reflect padding, Slaney mel scale with Slaney normalisation, power 2, power_to_db(ref=max, amin=1e-10,
top_db=80).

Every function takes batched CUDA tensors ([B, L] waveforms, [B, F, T] spectra, [B, n_mels, T] mels) and runs on the
current stream.  The filterbank, its pseudo-inverse and the step size of the mel inversion are float64 host
computations, cached.  The mel inversion is this project's own: librosa's L-BFGS-B NNLS of an
underdetermined system is not reproducible by another solver.

In front of the transforms (csrc/resample.hip): resample / resample_pcm16, a rational polyphase
Kaiser-windowed-sinc resampler that is this project's own definition (librosa's default, soxr_hq, cannot be
reproduced offline), trim, librosa.effects.trim's algorithm, and chunk_mel_images, the dataset builder's batch of
8-bit log-mel images.

Harmonic / percussive separation (csrc/hpss.hip): median_filter, hpss_masks, hpss (librosa's
decompose.hpss: medians along time and frequency, soft masks) and hpss_keep, the mel-domain keep mask of a component.

Loudness (csrc/loudness.hip): k_weighting, loudness_stats / integrated_loudness (ITU-R BS.1770-4),
true_peak (4x oversampled), limit (a look-ahead true-peak limiter) and loudness_normalize, which chains them.
"""
import functools
import math

import numpy as np
import torch

from . import ops

SR, N_FFT = 22050, 2048


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def _mel_points(sr, n_mels):
    """The n_mels + 2 corner frequencies in Hz of the filterbank's triangles (triangle m: points m, m + 1, m + 2)."""
    return _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))


def mel_centre_frequencies(sr=SR, n_mels=128):
    """The centre frequency in Hz of each of mel_filterbank's n_mels triangles (float64 [n_mels], ascending)."""
    return _mel_points(sr, n_mels)[1:-1].copy()


@functools.lru_cache(maxsize=None)
def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=128):
    """The Slaney mel filterbank [n_mels, n_fft/2 + 1] (fmin 0, fmax sr/2, area-normalised), float64, read-only."""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_points(sr, n_mels)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    M = np.maximum(0.0, np.minimum(lower, upper))
    M *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _mel_host(sr, n_fft, n_mels):
    """(M fp32, M^T, pinv(M) fp32, [lo, hi) per row, 1 / lambda_max(M M^T)) from the float64 filterbank."""
    M = mel_filterbank(sr, n_fft, n_mels)
    lohi = np.zeros((n_mels, 2), dtype=np.int32)
    for m in range(n_mels):
        nz = np.flatnonzero(M[m])
        if nz.size:
            lohi[m] = (nz[0], nz[-1] + 1)
    lam = float(np.linalg.eigvalsh(M @ M.T)[-1])
    return (M.astype(np.float32), np.ascontiguousarray(M.T).astype(np.float32),
            np.linalg.pinv(M).astype(np.float32), lohi, 1.0 / lam)


_MEL_DEV = {}


def _mel_device(sr, n_fft, n_mels, device):
    key = (sr, n_fft, n_mels, torch.device(device).index)
    v = _MEL_DEV.get(key)
    if v is None:
        M, Mt, Minv, lohi, inv_lam = _mel_host(sr, n_fft, n_mels)
        v = _MEL_DEV[key] = tuple(torch.from_numpy(a).to(device) for a in (M, Mt, Minv, lohi)) + (inv_lam,)
    return v


def _batched(x, nd):
    """x with a leading batch axis added when it has nd - 1 dims; (tensor, whether it was added)."""
    return (x.unsqueeze(0), True) if x.dim() == nd - 1 else (x, False)


def stft(y, n_fft=N_FFT, hop_length=None):
    """Complex STFT [B, n_fft/2 + 1, 1 + L // hop] of y [B, L] (or [L])."""
    y, one = _batched(y, 2)
    S = ops.stft(y, n_fft, hop_length, "complex")
    return S[0] if one else S


def istft(S, length=None, n_fft=None, hop_length=None):
    S, one = _batched(S, 3)
    n_fft = 2 * (S.shape[-2] - 1) if n_fft is None else n_fft
    y = ops.istft(S, length, n_fft, hop_length)
    return y[0] if one else y


def spectrogram(y, n_fft=N_FFT, hop_length=None, power=2):
    """|STFT|^power (power 1 or 2), written directly by the transform kernel."""
    y, one = _batched(y, 2)
    P = ops.stft(y, n_fft, hop_length, {1: "mag", 2: "power"}[power])
    return P[0] if one else P


def melspectrogram(y, sr=SR, n_fft=N_FFT, hop_length=None, n_mels=128):
    """Mel power spectrogram [B, n_mels, T]."""
    y, one = _batched(y, 2)
    M, _, _, lohi, _ = _mel_device(sr, n_fft, n_mels, y.device)
    mel = ops.mel_project(ops.stft(y, n_fft, hop_length, "power"), M, lohi)
    return mel[0] if one else mel


def power_to_db(x, amin=1e-10, top_db=80.0):
    """librosa.power_to_db(ref=np.max) per batch item of x [B, ...] (a 2-D x is one item)."""
    x, one = _batched(x, 3)
    out = ops.power_to_db(x, amin, top_db)
    return out[0] if one else out


def db_to_power(db):
    return ops.db_to_power(db)


def mel_to_stft(mel, sr=SR, n_fft=N_FFT, nnls_iters=32, power=2.0, sqrt=True):
    """Approximate |STFT| [B, F, T] of a mel power spectrogram: x0 = max(pinv(M) mel, 0), then nnls_iters
    projected-gradient steps x <- max(x - M^T (M x - mel) / lambda_max(M M^T), 0), then x^(1/power)
    (sqrt=False returns x itself)."""
    mel, one = _batched(mel, 3)
    M, Mt, Minv, lohi, inv_lam = _mel_device(sr, n_fft, mel.shape[-2], mel.device)
    if power != 2.0 and sqrt:
        raise ValueError("mel_to_stft: only power=2 mel spectrograms are inverted")
    x = ops.mel_invert(ops.f32c(mel), M, Mt, Minv, lohi, inv_lam, nnls_iters, sqrt)
    return x[0] if one else x


def random_phase(shape, seed=None, device="cuda"):
    """exp(2 pi i u) as complex64, u uniform from a generator of `device` seeded with `seed` (None: a fresh seed)."""
    g = torch.Generator(device=device)
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed))
    u = torch.rand(tuple(shape), generator=g, dtype=torch.float32, device=device) * (2.0 * np.pi)
    return torch.complex(torch.cos(u), torch.sin(u))


def griffinlim(mag, n_iter=32, momentum=0.99, seed=None, length=None, n_fft=None, hop_length=None, init_phase=None,
               anchor_phase=None, anchor=None):
    """Fast Griffin-Lim (librosa's recurrence) on |STFT| mag [B, F, T]: y [B, length]; length defaults to
    (T - 1) * hop and must give T frames.  The initial phase is init_phase [B, F, T] complex64 when given, else
    drawn from a generator seeded with `seed`.

    anchor_phase [B, F, T] complex64 (unit modulus) with anchor [B, F, T] in [0, 1], both or neither: every
    iteration's phase becomes unit(a anchor_phase + (1 - a) angles): the plain recurrence where a == 0, anchor_phase
    held where a == 1.  Neither: the call it always was."""
    if (anchor_phase is None) != (anchor is None):
        raise ValueError("griffinlim: anchor_phase and anchor go together (both or neither)")
    mag, one = _batched(mag, 3)
    mag = ops.f32c(mag)
    n_fft = 2 * (mag.shape[-2] - 1) if n_fft is None else n_fft
    hop = n_fft // 4 if hop_length is None else hop_length
    length = (mag.shape[-1] - 1) * hop if length is None else length
    if init_phase is None:
        init_phase = random_phase(mag.shape, seed, mag.device)
    elif init_phase.dim() == 2:
        init_phase = init_phase.unsqueeze(0)
    if anchor is not None:
        anchor_phase, anchor = _batched(anchor_phase, 3)[0], ops.f32c(_batched(anchor, 3)[0])
    y = ops.griffinlim(mag, init_phase, n_iter, momentum, length, n_fft, hop, anchor_phase, anchor)
    return y[0] if one else y


def mel_to_audio(mel, sr=SR, n_fft=N_FFT, n_iter=32, nnls_iters=32, momentum=0.99, seed=None, length=None):
    """Waveform [B, (T - 1) * hop] of a mel power spectrogram [B, n_mels, T]: mel_to_stft, then griffinlim."""
    return griffinlim(mel_to_stft(mel, sr, n_fft, nnls_iters), n_iter, momentum, seed, length, n_fft)


# ---- content-anchored vocoder (csrc/vocoder.hip) ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _gain_host(sr, n_fft, n_mels):
    """(Wn fp32 [n_mels, F], mlohi int32 [F, 2]): the filterbank divided by its column sums (a column no filter covers
    stays 0) and each bin's run [m_lo, m_hi) of filters with a non-zero weight, the transpose of _mel_host's lohi."""
    M = mel_filterbank(sr, n_fft, n_mels)
    col = M.sum(axis=0)
    Wn = np.divide(M, col[None, :], out=np.zeros_like(M), where=col[None, :] > 0)
    mlohi = np.zeros((M.shape[1], 2), dtype=np.int32)
    for f in range(M.shape[1]):
        nz = np.flatnonzero(M[:, f])
        if nz.size:
            mlohi[f] = (nz[0], nz[-1] + 1)
    return Wn.astype(np.float32), mlohi


_GAIN_DEV = {}


def _gain_device(sr, n_fft, n_mels, device):
    key = (sr, n_fft, n_mels, torch.device(device).index)
    v = _GAIN_DEV.get(key)
    if v is None:
        v = _GAIN_DEV[key] = tuple(torch.from_numpy(a).to(device) for a in _gain_host(sr, n_fft, n_mels))
    return v


def check_vocoder_args(max_gain_db, anchor_db, what="mel_gain_target"):
    """ValueError for a non-finite or negative max_gain_db or a non-finite anchor_db."""
    if not math.isfinite(float(max_gain_db)) or float(max_gain_db) < 0:
        raise ValueError(f"{what}: max_gain_db must be finite and non-negative, got {max_gain_db}")
    if not math.isfinite(float(anchor_db)):
        raise ValueError(f"{what}: anchor_db must be finite, got {anchor_db}")


def _eps_device(eps, B, device, what):
    """eps as float32 [B] on the device: a positive number, or one per item (a device tensor is taken as it is)."""
    if torch.is_tensor(eps) and eps.is_cuda:
        e = ops.f32c(eps).reshape(-1)
    else:
        e = torch.as_tensor(eps, dtype=torch.float64).reshape(-1)
        if not bool(torch.isfinite(e).all()) or bool((e <= 0).any()):
            raise ValueError(f"{what}: eps must be positive and finite, got {eps}")
        e = e.to(torch.float32).to(device)
    if e.numel() == 1 and B != 1:
        e = e.expand(B).contiguous()
    if e.numel() != B:
        raise ValueError(f"{what}: eps must be one number or one per item ({B}), got {e.numel()}")
    return e


def _gain_inputs(what, C, mel_out, mel_content, eps, max_gain_db, anchor_db, sr):
    check_vocoder_args(max_gain_db, anchor_db, what)
    C, one = _batched(C, 3)
    mel_out, mel_content = ops.f32c(_batched(mel_out, 3)[0]), ops.f32c(_batched(mel_content, 3)[0])
    n_fft = 2 * (C.shape[-2] - 1)
    Wn, mlohi = _gain_device(sr, n_fft, mel_out.shape[-2], C.device)
    e = _eps_device(eps, C.shape[0], C.device, what)
    return C, mel_out, mel_content, Wn, mlohi, e, 10.0 ** (float(max_gain_db) / 10.0), one


def mel_gain_power(C, mel_out, mel_content, eps, max_gain_db=40.0, sr=SR):
    """The content's power under the transfer's gain, Pm = g |C|^2 [B, F, T] (see mel_gain_target)."""
    C, mel_out, mel_content, Wn, mlohi, e, mg, one = _gain_inputs("mel_gain_power", C, mel_out, mel_content, eps,
                                                                  max_gain_db, 0.0, sr)
    Pm = ops.mel_gain_power(C, mel_out, mel_content, Wn, mlohi, e, mg)
    return Pm[0] if one else Pm


def mel_gain_target(C, mel_out, mel_content, eps, max_gain_db=40.0, anchor_db=6.0, residual=None, sr=SR):
    """The transfer as an edit of the content's STFT C [B, F, T] complex64 -> (mag, phase0, anchor), each [B, F, T].
    mel_out, mel_content [B, n_mels, T] mel power: the output's and the content's after the same round trip; eps: a
    positive floor, one number or one per item.  G = (mel_out + eps) / (mel_content + eps) is carried to the bins by
    the filterbank normalised per bin, g = clamp(sum_m Wn[m, f] G[m, t], 0, 10^(max_gain_db / 10)) (1 where no filter
    covers the bin), and mag = sqrt(g |C|^2 + residual), phase0 = C / |C| ((1, 0) where C vanishes), anchor =
    clamp(1 - |10 log10((mag^2 + eps) / (|C|^2 + eps))| / anchor_db, 0, 1), 0 everywhere when anchor_db <= 0.
    residual [B, F, T]: power added to the masked power (None: 0).  Where the mel did not change mag is |C| and anchor 1."""
    C, mel_out, mel_content, Wn, mlohi, e, mg, one = _gain_inputs("mel_gain_target", C, mel_out, mel_content, eps,
                                                                  max_gain_db, anchor_db, sr)
    if residual is not None:
        residual = ops.f32c(_batched(residual, 3)[0])
    out = ops.mel_gain_target(C, mel_out, mel_content, Wn, mlohi, e, mg, anchor_db, residual)
    return tuple(t[0] for t in out) if one else out


def mel_to_audio_content(mel_out, content_wave, mel_content=None, sr=SR, n_fft=N_FFT, n_iter=32, momentum=0.99,
                         max_gain_db=40.0, anchor_db=6.0, residual=True, nnls_iters=32, max_db=80, length=None):
    """Waveform [B, length] of the mel power mel_out [B, n_mels, T] read as an edit of content_wave [B, L] (T = 1 +
    L // hop): the content's STFT scaled by the mel-domain gain (mel_gain_target), then Griffin-Lim started from the
    content's phase and anchored to it where the gain is near unity.  mel_content: the content's mel after the same
    round trip as mel_out (None: melspectrogram(content_wave)); eps = max(mel_content) 10^(-max_db / 10) per item.
    residual: add R = mel_to_stft(max((mel_out - mel_content) - (M Pm - M |C|^2), 0), sqrt=False), the energy a gain
    cannot create: max(mel_out - M Pm, 0) when mel_content is the content's plain mel M |C|^2.
    length defaults to (T - 1) * hop.  mel_out == mel_content returns istft(stft(content_wave))."""
    check_vocoder_args(max_gain_db, anchor_db, "mel_to_audio_content")
    y, one = _batched(content_wave, 2)
    mel_out = ops.f32c(_batched(mel_out, 3)[0])
    n_mels = mel_out.shape[-2]
    M, _, _, lohi, _ = _mel_device(sr, n_fft, n_mels, y.device)
    C, P = ops.stft(y, n_fft, None, "both")
    mel_plain = ops.mel_project(P, M, lohi)
    mel_content = mel_plain if mel_content is None else ops.f32c(_batched(mel_content, 3)[0])
    if mel_out.shape != mel_content.shape or mel_out.shape[0] != C.shape[0] or mel_out.shape[-1] != C.shape[-1]:
        raise ValueError(f"mel_to_audio_content: mel_out {tuple(mel_out.shape)}, mel_content "
                         f"{tuple(mel_content.shape)} and the content's {C.shape[-1]} frames ({C.shape[0]} items) do "
                         "not match")
    tiny = float(np.finfo(np.float32).tiny)
    eps = (mel_content.amax(dim=(1, 2)) * 10.0 ** (-float(max_db) / 10.0)).clamp_min(tiny)
    R = None
    if residual:
        Pm = mel_gain_power(C, mel_out, mel_content, eps, max_gain_db, sr)
        # what the output gained over the content, less what the gain delivered: both differences are taken within
        # one representation, so the round trip's own error (mel_content against M |C|^2) is not read as added energy
        D = ((mel_out - mel_content) - (ops.mel_project(Pm, M, lohi) - mel_plain)).clamp_min(0.0)
        R = mel_to_stft(D, sr, n_fft, nnls_iters, sqrt=False)
    mag, phase0, anchor = mel_gain_target(C, mel_out, mel_content, eps, max_gain_db, anchor_db, R, sr)
    out = griffinlim(mag, n_iter, momentum, None, length, n_fft, None, phase0, phase0, anchor)
    return out[0] if one else out


# ---- harmonic / percussive separation (csrc/hpss.hip) -----------------------------------------
HPSS_COMPONENTS = ("percussive", "harmonic")


def _pair(v, what):
    """A number or a (harmonic, percussive) pair -> the pair."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be a number or a (harmonic, percussive) pair, got {v!r}")
        return v[0], v[1]
    return v, v


def check_hpss_args(kernel_size=31, power=2.0, margin=1.0, what="hpss"):
    """ValueError for a bad kernel_size, power or margin (ops.check_median_args / check_softmask_args); returns
    ((win_harmonic, win_percussive), (margin_harmonic, margin_percussive))."""
    wins, margins = _pair(kernel_size, f"{what}: kernel_size"), _pair(margin, f"{what}: margin")
    for w in wins:
        ops.check_median_args(w, 1, what)
    ops.check_softmask_args(power, margins[0], margins[1], what)
    return (int(wins[0]), int(wins[1])), (float(margins[0]), float(margins[1]))


def median_filter(S, win, axis):
    """The running median of S [B, F, T] (or [F, T]) along frequency (axis 0) or time (axis 1) of each item: window
    win (odd, 1..63), the ends reflected with the edge sample repeated; bitwise
    scipy.ndimage.median_filter(mode="reflect") along that axis.  NaN inputs give an unspecified sample."""
    ops.check_median_args(win, axis)
    S, one = _batched(S, 3)
    out = ops.median_filter(ops.f32c(S), win, axis)
    return out[0] if one else out


def hpss_masks(S, kernel_size=31, power=2.0, margin=1.0):
    """(mask_h, mask_p) of a magnitude spectrogram S [B, F, T] (or [F, T]), librosa.decompose.hpss(mask=True): the
    harmonic enhancement is the median along time, the percussive one the median along frequency, and
    mask_h = softmask(harm, margin_h perc, power), mask_p = softmask(perc, margin_p harm, power), except that a bin
    where both medians vanish gets 0.5 in both whatever the margins.  kernel_size and margin: a number or a (harmonic,
    percussive) pair."""
    wins, margins = check_hpss_args(kernel_size, power, margin, "hpss_masks")
    S, one = _batched(S, 3)
    S = ops.f32c(S)
    harm, perc = ops.median_filter(S, wins[0], 1), ops.median_filter(S, wins[1], 0)
    mh, mp = ops.hpss_masks(harm, perc, power, margins[0], margins[1])
    return (mh[0], mp[0]) if one else (mh, mp)


def hpss(y, kernel_size=31, power=2.0, margin=1.0, n_fft=N_FFT):
    """(y_harm, y_perc) of a waveform y [B, L] (or [L]): hpss_masks of |STFT| applied to the complex STFT, each
    component back through istft at y's length."""
    wins, margins = check_hpss_args(kernel_size, power, margin, "hpss")
    y, one = _batched(y, 2)
    C, S = ops.stft(y, n_fft, None, "both_mag")
    mh, mp = hpss_masks(S, wins, power, margins)
    out = tuple(ops.istft(C, y.shape[-1], n_fft, None, mag=m) for m in (mh, mp))
    return tuple(t[0] for t in out) if one else out


def hpss_keep(y, component, kernel_size=31, power=2.0, margin=1.0, sr=SR, n_mels=128, n_fft=N_FFT):
    """The mel-domain keep mask [n_mels, T] (T = 1 + L // hop) of the "percussive" or "harmonic" component of the
    waveform y [L]: hpss_masks of |STFT|, carried to the mel grid as the share of each filter's energy the component
    holds (ops.mask_mel_share on y's own power spectrogram; 0.5 where a filter sees no energy).  In [0, 1], on y's
    device: what transfer_recording's keep= takes."""
    if component not in HPSS_COMPONENTS:
        raise ValueError(f"hpss_keep: component must be \"percussive\" or \"harmonic\", got {component!r}")
    wins, margins = check_hpss_args(kernel_size, power, margin, "hpss_keep")
    if y.dim() != 1:
        raise ValueError(f"hpss_keep: y must be a mono waveform [L], got shape {tuple(y.shape)}")
    y = y.unsqueeze(0)
    M, _, _, lohi, _ = _mel_device(sr, n_fft, n_mels, y.device)
    mh, mp = hpss_masks(ops.stft(y, n_fft, None, "mag"), wins, power, margins)
    share = ops.mask_mel_share(ops.stft(y, n_fft, None, "power"), mp if component == "percussive" else mh, M, lohi)
    return share[0]


# ---- resampling, silence trim, chunk images (csrc/resample.hip) -------------------------------
RESAMPLE_ZEROS, RESAMPLE_BETA, RESAMPLE_ROLLOFF = 32, 14.769656459379492, 0.945


@functools.lru_cache(maxsize=None)
def resample_taps(sr_in, sr_out):
    """(up, down, W, table): the polyphase filter of sr_in -> sr_out as a read-only float64 table [up, 2W+1],
    table[p, j + W] = h(j - p / up) with h(t) = fc sinc(fc t) I0(beta sqrt(1 - (t fc / Z)^2)) / I0(beta) on
    |t| <= Z / fc (0 outside), fc = min(1, up / down) * rolloff, W = ceil(Z / fc), up / down = sr_out / sr_in reduced."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample_taps: sample rates must be positive ({sr_in}, {sr_out})")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    Z, fc = RESAMPLE_ZEROS, min(1.0, up / down) * RESAMPLE_ROLLOFF
    W = int(math.ceil(Z / fc))
    t = np.arange(-W, W + 1, dtype=np.float64)[None, :] - np.arange(up, dtype=np.float64)[:, None] / up
    u = t * fc / Z
    inside = np.abs(t) <= Z / fc
    win = np.i0(RESAMPLE_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(RESAMPLE_BETA)
    table = np.where(inside, fc * np.sinc(fc * t) * win, 0.0)
    table.setflags(write=False)
    return up, down, W, table


_TAPS_DEV = {}


def _taps_device(sr_in, sr_out, device):
    key = (int(sr_in), int(sr_out), torch.device(device).index)
    v = _TAPS_DEV.get(key)
    if v is None:
        up, down, W, table = resample_taps(sr_in, sr_out)
        v = _TAPS_DEV[key] = (up, down, W, torch.from_numpy(table.astype(np.float32)).to(device))
    return v


def resample(y, sr_in, sr_out):
    """y [B, L] (or [L]) at sr_in -> [B, ceil(L up / down)] at sr_out; equal rates return y unchanged."""
    if int(sr_in) == int(sr_out):
        return y
    y, one = _batched(y, 2)
    ops.require_device(y, dtype=None, what="resample")
    up, down, W, taps = _taps_device(sr_in, sr_out, y.device)
    out = ops.resample(ops.f32c(y), taps, up, down, W)
    return out[0] if one else out


def resample_pcm16(pcm, sr_in, sr_out):
    """Interleaved int16 PCM [L, ch] (or mono [L]) at sr_in -> mono float32 [ceil(L up / down)] at sr_out: each frame is
    the mean over channels of s / 32768 (read_wav followed by .mean(axis=1)), decoded inside the resampler's load."""
    if pcm.dim() == 1:
        pcm = pcm.unsqueeze(1)
    up, down, W, taps = _taps_device(sr_in, sr_out, pcm.device)
    return ops.resample_pcm16(pcm, taps, up, down, W)


def trim(y, top_db=20, frame_length=2048, hop_length=512):
    """librosa.effects.trim: (y[start:end], (start, end)) for y [L] (one host read of the bounds, to slice); for
    y [B, L] the int64 bounds tensor [B, 2] on the device, without a host synchronisation.  A row whose loudest frame
    has a mean square <= 1e-10 (digital silence) is (0, 0)."""
    if y.dim() == 2:
        return ops.trim_bounds(y, top_db, frame_length, hop_length)
    start, end = (int(v) for v in ops.trim_bounds(y.unsqueeze(0), top_db, frame_length, hop_length)[0].tolist())
    return y[start:end], (start, end)


def chunk_mel_images(y, sr, chunk_size, n_mels=128, max_db=80):
    """uint8 [ceil(L / chunk_size), n_mels, 1 + chunk_size // 512]: y [L] cut into chunks of chunk_size samples (the
    last zero-padded), each chunk's log-mel (power_to_db referred to the chunk's own maximum) as 8-bit pixels; one
    batch through melspectrogram, power_to_db and ops.mel_quantize."""
    ops.require_device(y, dtype=None, what="chunk_mel_images")
    chunk_size = int(chunk_size)
    if y.dim() != 1 or y.numel() == 0 or chunk_size < 1:
        raise ValueError("chunk_mel_images: y must be a non-empty [L] waveform and chunk_size positive")
    n = -(-y.numel() // chunk_size)
    y = torch.nn.functional.pad(ops.f32c(y), (0, n * chunk_size - y.numel())).reshape(n, chunk_size)
    return ops.mel_quantize(power_to_db(melspectrogram(y, sr=sr, n_mels=n_mels)), max_db)


# ---- loudness: BS.1770 meter, true peak, look-ahead limiter (csrc/loudness.hip) ---------------
LOUDNESS_INFO_KEYS = ("input_lufs", "gain_db", "output_lufs", "true_peak_db", "max_reduction_db")


@functools.lru_cache(maxsize=None)
def k_weighting(sr=SR):
    """The K-weighting of ITU-R BS.1770-4 at sample rate sr: float64 [2, 5], rows {b0, b1, b2, a1, a2} (a0 = 1) of the
    high-shelf and of the high-pass, each the bilinear transform of its analogue prototype (at 48 kHz the standard's
    table to 1e-15).  Read-only."""
    sr = float(sr)
    if not math.isfinite(sr) or sr <= 0:
        raise ValueError(f"k_weighting: the sample rate must be positive, got {sr}")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    highpass = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    out = np.array([shelf, highpass], dtype=np.float64)
    out.setflags(write=False)
    return out


def loudness_hop(sr=SR):
    """The meter's hop in samples: 100 ms, round(0.1 sr)."""
    return int(round(0.1 * sr))


def check_loudness_args(target_lufs=None, ceiling_db=-1.0, lookahead_ms=5.0, what="loudness_normalize"):
    """ValueError for a non-finite target (None: not checked), a ceiling that is not finite or above 0 dB, or a
    look-ahead that is negative or not finite."""
    if target_lufs is not None and not math.isfinite(float(target_lufs)):
        raise ValueError(f"{what}: the target loudness must be finite, got {target_lufs}")
    if not math.isfinite(float(ceiling_db)) or float(ceiling_db) > 0:
        raise ValueError(f"{what}: the true-peak ceiling must be finite and at most 0 dB, got {ceiling_db}")
    if not math.isfinite(float(lookahead_ms)) or float(lookahead_ms) < 0:
        raise ValueError(f"{what}: the look-ahead must be finite and not negative, got {lookahead_ms}")


def limiter_lookahead(lookahead_ms=5.0, sr=SR):
    """The limiter's look-ahead in samples, round(lookahead_ms sr / 1000); ValueError beyond what one tile's halo holds
    (ops.LIMIT_MAX_LOOKAHEAD samples)."""
    Lh = int(round(float(lookahead_ms) * sr / 1000.0))
    if Lh > ops.LIMIT_MAX_LOOKAHEAD:
        raise ValueError(f"limit: a look-ahead of {lookahead_ms} ms is {Lh} samples at {sr} Hz; at most "
                         f"{ops.LIMIT_MAX_LOOKAHEAD} fit one tile's halo")
    return Lh


def loudness_stats(y, sr=SR):
    """float64 [B, 4] on the device for y [B, L] (or [4] for [L]): {integrated loudness in LUFS, blocks passing both
    gates, the relative threshold in LUFS, blocks in all} of ITU-R BS.1770-4 (mono; 400 ms blocks every 100 ms, gates at
    -70 LUFS and 10 LU under the gated mean).  -inf when no block passes (silence, or less than 400 ms).  No host
    synchronisation."""
    y, one = _batched(y, 2)
    ops.require_device(y, dtype=None, what="loudness_stats")
    hop = loudness_hop(sr)
    out = ops.loudness_gate(ops.loudness_hop_sums(ops.f32c(y), hop, k_weighting(sr).reshape(-1)), hop)
    return out[0] if one else out


def integrated_loudness(y, sr=SR):
    """The integrated loudness in LUFS of each row of y [B, L]: float64 [B] on the device (a 0-dim tensor for [L])."""
    return loudness_stats(y, sr)[..., 0]


def true_peak(y, sr=SR):
    """float32 [B] on the device: max(|y|, |y oversampled 4x|) per row of y [B, L] (a 0-dim tensor for [L]); the
    oversampler is resample(y, sr, 4 sr)'s, fused with the maximum."""
    y, one = _batched(y, 2)
    ops.require_device(y, dtype=None, what="true_peak")
    up, _, W, taps = _taps_device(sr, 4 * int(sr), y.device)
    out = ops.true_peak(ops.f32c(y), taps, up, W)
    return out[0] if one else out


def _limit(y, ceiling_db, lookahead_ms, sr, want_gain=False):
    """(out, gain, min_gain, trim) of the limiter and its trim on y [B, L] fp32 contiguous."""
    Lh = limiter_lookahead(lookahead_ms, sr)
    c = np.float32(10.0 ** (float(ceiling_db) / 20.0))
    if float(c) > 10.0 ** (float(ceiling_db) / 20.0):     # the fp32 ceiling the kernels hold never exceeds the asked one
        c = np.nextafter(c, np.float32(0.0))
    c = float(c)
    up, _, W, taps = _taps_device(sr, 4 * int(sr), y.device)
    out, gain, mn = ops.limit(y, taps, up, W, Lh, c, return_gain=want_gain, return_min=True)
    trim = ops.peak_trim_(out, ops.true_peak(out, taps, up, W), c)
    return out, gain, mn, trim


def limit(y, ceiling_db=-1.0, lookahead_ms=5.0, sr=SR, return_gain=False):
    """The look-ahead true-peak limiter on y [B, L] (or [L]): the gain g = 1 - hann * (1 - min_{|j| <= Lh} r) with r =
    min(1, c / p) and p the 4x true-peak envelope (ldm_limit), then one scalar trim per row that puts
    the measured true peak of g y under the ceiling c = 10^(ceiling_db / 20) (g <= r only in exact arithmetic, and the
    inter-sample peaks of g y can pass c by a hair).  A row wholly under the ceiling comes back bitwise.  No host
    synchronisation.  return_gain: also the gain curve [B, L] (before the trim)."""
    check_loudness_args(None, ceiling_db, lookahead_ms, "limit")
    limiter_lookahead(lookahead_ms, sr)
    y, one = _batched(y, 2)
    ops.require_device(y, dtype=None, what="limit")
    out, gain, _, _ = _limit(ops.f32c(y), ceiling_db, lookahead_ms, sr, return_gain)
    if return_gain:
        return (out[0], gain[0]) if one else (out, gain)
    return out[0] if one else out


def loudness_normalize(y, target_lufs, ceiling_db=-1.0, lookahead_ms=5.0, sr=SR):
    """(out, info): y [B, L] (or [L]) brought to target_lufs (a number, or a float64 device tensor [B] of one target
    per row) and limited under ceiling_db of true peak: measure, gain, limit, measure again.  info: input_lufs,
    gain_db, output_lufs, true_peak_db, max_reduction_db (the limiter's deepest gain reduction, trim included; 0 when it
    did not engage), each a list of B floats (a float for [L]), from one host read at the end.  A row without a finite
    loudness (silence) gets 0 dB of gain."""
    per_row = torch.is_tensor(target_lufs)
    check_loudness_args(None if per_row else target_lufs, ceiling_db, lookahead_ms)
    limiter_lookahead(lookahead_ms, sr)
    y, one = _batched(y, 2)
    ops.require_device(y, dtype=None, what="loudness_normalize")
    y = ops.f32c(y)
    stats = loudness_stats(y, sr)
    in_lufs = stats[:, 0]
    if per_row:     # the targets subtracted from the readings, so that one target of 0 serves every row; a target of
        rel = stats.clone()                                     # -inf (a silent reference) leaves its row at 0 dB
        rel[:, 0] -= target_lufs.to(stats).reshape(-1)
        scaled, gain_db = ops.loudness_gain(y, rel, 0.0)
    else:
        scaled, gain_db = ops.loudness_gain(y, stats, float(target_lufs))
    out, _, mn, trim = _limit(scaled, ceiling_db, lookahead_ms, sr)
    tp = true_peak(out, sr)
    table = torch.stack([in_lufs, gain_db, integrated_loudness(out, sr), 20.0 * torch.log10(tp.double()),
                         -20.0 * torch.log10((mn * trim).double()) + 0.0]).cpu().tolist()    # the one host read
    info = {k: (v[0] if one else v) for k, v in zip(LOUDNESS_INFO_KEYS, table)}
    return (out[0] if one else out), info
