"""Audio front and back end on the GPU (csrc/audio.hip): STFT / ISTFT, mel spectrogram, dB, mel inversion and
Griffin-Lim with the defaults the reference relies on (librosa's): sr 22050, n_fft 2048, hop n_fft/4, periodic Hann,
centre reflect padding, Slaney mel scale with Slaney normalisation, power 2, power_to_db(ref=max, amin=1e-10,
top_db=80).

Every function takes batched CUDA tensors ([B, L] waveforms, [B, F, T] spectra, [B, n_mels, T] mels) and runs on the
current stream.  The filterbank, its pseudo-inverse and the step size of the mel inversion are float64 host
computations, cached.  The mel inversion is this project's own: librosa's L-BFGS-B NNLS of an
underdetermined system is not reproducible by another solver.
"""
import functools

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


@functools.lru_cache(maxsize=None)
def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=128):
    """The Slaney mel filterbank [n_mels, n_fft/2 + 1] (fmin 0, fmax sr/2, area-normalised), float64, read-only."""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
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


def griffinlim(mag, n_iter=32, momentum=0.99, seed=None, length=None, n_fft=None, hop_length=None, init_phase=None):
    """Fast Griffin-Lim (librosa's recurrence) on |STFT| mag [B, F, T]: y [B, length]; length defaults to
    (T - 1) * hop and must give T frames.  The initial phase is init_phase [B, F, T] complex64 when given, else
    drawn from a generator seeded with `seed`."""
    mag, one = _batched(mag, 3)
    mag = ops.f32c(mag)
    n_fft = 2 * (mag.shape[-2] - 1) if n_fft is None else n_fft
    hop = n_fft // 4 if hop_length is None else hop_length
    length = (mag.shape[-1] - 1) * hop if length is None else length
    if init_phase is None:
        init_phase = random_phase(mag.shape, seed, mag.device)
    elif init_phase.dim() == 2:
        init_phase = init_phase.unsqueeze(0)
    y = ops.griffinlim(mag, init_phase, n_iter, momentum, length, n_fft, hop)
    return y[0] if one else y


def mel_to_audio(mel, sr=SR, n_fft=N_FFT, n_iter=32, nnls_iters=32, momentum=0.99, seed=None, length=None):
    """Waveform [B, (T - 1) * hop] of a mel power spectrogram [B, n_mels, T]: mel_to_stft, then griffinlim."""
    return griffinlim(mel_to_stft(mel, sr, n_fft, nnls_iters), n_iter, momentum, seed, length, n_fft)
