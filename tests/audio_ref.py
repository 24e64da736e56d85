"""The float64 yardstick of the audio path: a numpy restatement (numpy.fft) of the definitions ldm_amd/audio.py
implements, librosa's defaults throughout.  Not a test file; tests/test_audio_host.py pins it on the CPU (against
torch.stft / torch.istft and recorded filterbank values) and tests/test_gpu_audio.py compares the kernels to it.
Written from the definitions, independently of ldm_amd: periodic Hann, hop = n_fft / 4, centre reflect padding,
Slaney mel scale and normalisation, power_to_db(ref=max, amin=1e-10, top_db=80)."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def stft(y, n_fft=2048):
    """y [..., L] float64 -> complex [..., n_fft/2+1, 1 + L // hop]."""
    y = np.asarray(y, dtype=np.float64)
    hop = n_fft // 4
    pad = [(0, 0)] * (y.ndim - 1) + [(n_fft // 2, n_fft // 2)]
    yp = np.pad(y, pad, mode="reflect")
    T = 1 + y.shape[-1] // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = yp[..., idx] * hann(n_fft)                      # [..., T, n_fft]
    return np.swapaxes(np.fft.rfft(frames, axis=-1), -1, -2)


def istft(S, length=None, n_fft=None):
    """complex [..., F, T] -> y [..., length]: overlap-add / window sum-of-squares, centre padding trimmed."""
    S = np.asarray(S, dtype=np.complex128)
    n_fft = 2 * (S.shape[-2] - 1) if n_fft is None else n_fft
    hop, T = n_fft // 4, S.shape[-1]
    w = hann(n_fft)
    frames = np.fft.irfft(np.swapaxes(S, -1, -2), n=n_fft, axis=-1) * w   # [..., T, n_fft]
    total = n_fft + hop * (T - 1)
    y = np.zeros(S.shape[:-2] + (total,))
    env = np.zeros(total)
    for t in range(T):
        y[..., t * hop:t * hop + n_fft] += frames[..., t, :]
        env[t * hop:t * hop + n_fft] += w * w
    ok = env > TINY32
    y[..., ok] /= env[ok]
    length = (T - 1) * hop if length is None else length
    y = y[..., n_fft // 2:n_fft // 2 + length]
    if y.shape[-1] < length:
        y = np.pad(y, [(0, 0)] * (y.ndim - 1) + [(0, length - y.shape[-1])])
    return y


def hz_to_mel(f):
    f = np.atleast_1d(np.asarray(f, dtype=np.float64))
    out = f / (200.0 / 3)
    big = f >= 1000.0
    out[big] = 15.0 + np.log(f[big] / 1000.0) / (np.log(6.4) / 27.0)
    return out


def mel_to_hz(m):
    m = np.atleast_1d(np.asarray(m, dtype=np.float64))
    out = m * (200.0 / 3)
    big = m >= 15.0
    out[big] = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m[big] - 15.0))
    return out


def mel_filterbank(sr=22050, n_fft=2048, n_mels=128):
    F = n_fft // 2 + 1
    freqs = np.arange(F) * (sr / n_fft)
    edges = mel_to_hz(np.linspace(hz_to_mel(0.0)[0], hz_to_mel(sr / 2.0)[0], n_mels + 2))
    M = np.zeros((n_mels, F))
    for m in range(n_mels):
        lo, c, hi = edges[m], edges[m + 1], edges[m + 2]
        up = (freqs - lo) / (c - lo)
        down = (hi - freqs) / (hi - c)
        M[m] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (hi - lo))
    return M


def melspectrogram(y, sr=22050, n_fft=2048, n_mels=128):
    return np.einsum("mf,...ft->...mt", mel_filterbank(sr, n_fft, n_mels), np.abs(stft(y, n_fft)) ** 2)


def power_to_db(x, amin=1e-10, top_db=80.0):
    """One item (the reference is the array's own maximum)."""
    x = np.asarray(x, dtype=np.float64)
    db = 10.0 * np.log10(np.maximum(amin, x)) - 10.0 * np.log10(max(amin, x.max()))
    return np.maximum(db, db.max() - top_db) if top_db is not None else db


def db_to_power(db):
    return 10.0 ** (0.1 * np.asarray(db, dtype=np.float64))


def quantize(db, max_db=80.0):
    return (np.clip((np.asarray(db, dtype=np.float64) + max_db) * (255.0 / max_db), 0, 255) + 0.5).astype(np.uint8)


def mel_invert(mel, M, iters, pinv=None):
    """x (before the square root) of the stated NNLS: x0 = max(pinv(M) mel, 0), then projected-gradient steps with
    step 1 / lambda_max(M M^T).  mel [..., n_mels, T]."""
    mel = np.asarray(mel, dtype=np.float64)
    pinv = np.linalg.pinv(M) if pinv is None else pinv
    lam = np.linalg.eigvalsh(M @ M.T)[-1]
    x = np.maximum(pinv @ mel, 0.0)
    for _ in range(iters):
        x = np.maximum(x - M.T @ (M @ x - mel) / lam, 0.0)
    return x


def griffinlim(mag, init_angles, n_iter, momentum=0.99, n_fft=None):
    """librosa's fast Griffin-Lim recurrence from the given initial phase (complex, unit modulus)."""
    mag = np.asarray(mag, dtype=np.float64)
    n_fft = 2 * (mag.shape[-2] - 1) if n_fft is None else n_fft
    angles = np.asarray(init_angles, dtype=np.complex128)
    prev = np.zeros_like(angles)
    for _ in range(n_iter):
        r = stft(istft(mag * angles, n_fft=n_fft), n_fft)
        angles = r - (momentum / (1.0 + momentum)) * prev
        angles = angles / (np.abs(angles) + TINY32)
        prev = r
    return istft(mag * angles, n_fft=n_fft)


def spectral_convergence(y, mag, n_fft):
    d = np.abs(stft(y, n_fft)) - mag
    return float(np.linalg.norm(d) / np.linalg.norm(mag))


def test_signal(L, seed=5, variant=0):
    """Sines at 440 Hz and a 1-1.8 kHz chirp plus 0.05 Gaussian noise from PCG64(seed); `variant` shifts the
    pitches so that batch items differ."""
    rng = np.random.Generator(np.random.PCG64(seed + variant))
    t = np.arange(L) / 22050.0
    dur = max(L / 22050.0, 1e-9)
    f0 = 440.0 * (1.0 + 0.37 * variant)
    chirp = np.sin(2 * np.pi * ((1000.0 + 200.0 * variant) * t + 0.5 * (800.0 / dur) * t * t))
    return 0.5 * np.sin(2 * np.pi * f0 * t) + 0.3 * chirp + 0.05 * rng.standard_normal(L)
