"""Transfer report (csrc/metrics.hip): what a style transfer kept of the content and how far it moved
towards the style, as numbers.

Features on the device: onset_strength (rhythm), chroma (harmony), mfcc_moments (timbre: the first two moments of the
MFCC frames, which never leave the chip) and pair_stats (the seven sums behind Pearson correlation, cosine similarity
and weighted RMS difference).  Host tables (chroma_filterbank, dct_basis) are float64 and cached per device; the scores
are formed on the host in float64 (PairStats, frechet).  transfer_report puts them together.

The chroma is this project's own definition (linear split of a bin between the two nearest pitch classes), not
librosa's.  Mono only.  The scores describe spectra, not perceived quality.
"""
import functools
import math

import numpy as np
import torch

from . import audio, ops

AMIN, TOP_DB, ACTIVE_REL = 1e-10, 80.0, 1e-6
PAIR_KEYS = ("w", "wa", "wb", "waa", "wbb", "wab", "wdd")


# ---- host tables ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chroma_filterbank(sr, n_fft, fmin=55.0, fmax=5000.0):
    """(cls int32 [F], wt float64 [F]), F = n_fft / 2 + 1: a bin at v = f sr / n_fft Hz inside [fmin, fmax] has the
    fractional MIDI pitch p = 69 + 12 log2(v / 440) and gives wt = 1 - (p - floor(p)) of its power to pitch class
    cls = floor(p) mod 12 (0 = C) and 1 - wt to the next class; a bin outside the band has cls = -1 and wt = 0."""
    v = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    band = (v >= fmin) & (v <= fmax) & (v > 0)
    p = 69.0 + 12.0 * np.log2(np.where(band, v, 440.0) / 440.0)
    lo = np.floor(p)
    cls = np.where(band, np.mod(lo, 12.0), -1.0).astype(np.int32)
    wt = np.where(band, 1.0 - (p - lo), 0.0)
    cls.setflags(write=False)
    wt.setflags(write=False)
    return cls, wt


@functools.lru_cache(maxsize=None)
def dct_basis(n_mfcc, n_mels):
    """The first n_mfcc rows of the orthonormal DCT-II of length n_mels, float64 [n_mfcc, n_mels]: row 0 is
    sqrt(1 / n), row k sqrt(2 / n) cos(pi k (2 m + 1) / (2 n))."""
    n_mfcc, n = int(n_mfcc), int(n_mels)
    if not 1 <= n_mfcc <= n:
        raise ValueError(f"dct_basis: need 1 <= n_mfcc <= n_mels, got {n_mfcc}, {n}")
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    m = np.arange(n, dtype=np.float64)[None, :]
    D = math.sqrt(2.0 / n) * np.cos(math.pi * k * (2.0 * m + 1.0) / (2.0 * n))
    D[0] = math.sqrt(1.0 / n)
    D.setflags(write=False)
    return D


_TABLES = {}


def _chroma_device(sr, n_fft, device):
    key = ("chroma", sr, n_fft, torch.device(device).index)
    v = _TABLES.get(key)
    if v is None:
        cls, wt = chroma_filterbank(sr, n_fft)
        v = _TABLES[key] = (torch.from_numpy(cls.copy()).to(device), torch.from_numpy(wt.astype(np.float32)).to(device))
    return v


def _dct_device(n_mfcc, n_mels, device):
    key = ("dct", n_mfcc, n_mels, torch.device(device).index)
    v = _TABLES.get(key)
    if v is None:
        v = _TABLES[key] = torch.from_numpy(dct_basis(n_mfcc, n_mels).copy()).to(device)
    return v


# ---- features -------------------------------------------------------------------------------------------------
def onset_strength(db, lag=1):
    """The onset envelope [B, T] (or [T]) of a log-mel db [B, n_mels, T] (or [n_mels, T]) in dB: the mean over the mel
    bins of max(0, db[t] - db[t - lag]), 0 for t < lag (librosa's onset_strength with max_size 1 and mean aggregation,
    without its centring shift)."""
    db, one = audio._batched(db, 3)
    env = ops.onset_strength(ops.f32c(db), lag)
    return env[0] if one else env


def chroma(P, sr=audio.SR, n_fft=audio.N_FFT):
    """The chroma [B, 12, T] (or [12, T]) of a power spectrogram P [B, F, T] (or [F, T]) under chroma_filterbank(sr,
    n_fft): class 0 is C; every frame has unit L2 norm, or is exactly 0 where the band holds no power."""
    P, one = audio._batched(P, 3)
    cls, wt = _chroma_device(sr, n_fft, P.device)
    out = ops.chroma(ops.f32c(P), cls, wt)
    return out[0] if one else out


def moments_from_sums(sums, n):
    """(count, mean [n], cov [n, n]) in float64 from { sum w, sum w c_k, sum w c_j c_k (j <= k) } (one row, or several
    rows that are pooled); the covariance is the weighted population covariance.  A zero count gives nan."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 1 + n + n * (n + 1) // 2).sum(axis=0)
    count = float(s[0])
    if not count > 0:
        return count, np.full(n, np.nan), np.full((n, n), np.nan)
    mean = s[1:1 + n] / count
    second = np.zeros((n, n))
    second[np.triu_indices(n)] = s[1 + n:]
    second = second + np.triu(second, 1).T
    return count, mean, second / count - np.outer(mean, mean)


def mfcc_moments(db, n_mfcc=20, weight=None):
    """(count, mean [n_mfcc], cov [n_mfcc, n_mfcc]) as host float64 of the MFCC frames c = dct_basis(n_mfcc, n_mels) db
    of a log-mel db [B, n_mels, T] (or [n_mels, T]), frames weighted by weight [B, T] (or [T]; None: 1) and the items
    of a batch pooled.  A zero count gives nan.  One host read."""
    db, _ = audio._batched(db, 3)
    if weight is not None:
        weight = ops.f32c(audio._batched(weight, 2)[0])
    D = _dct_device(int(n_mfcc), db.shape[-2], db.device)
    return moments_from_sums(ops.mfcc_moments(ops.f32c(db), D, weight).cpu().numpy(), int(n_mfcc))


class PairStats:
    """The seven weighted sums of two signals a and b (float64: sum w, sum w a, sum w b, sum w a^2, sum w b^2,
    sum w a b, sum w (a - b)^2) and the scores they give.  A zero count or a zero variance / norm gives nan."""

    def __init__(self, sums):
        self.sums = tuple(float(v) for v in sums)
        if len(self.sums) != 7:
            raise ValueError(f"PairStats: seven sums expected, got {len(self.sums)}")
        for k, v in zip(PAIR_KEYS, self.sums):
            setattr(self, k, v)

    @property
    def pearson(self):
        num = self.w * self.wab - self.wa * self.wb
        va, vb = self.w * self.waa - self.wa * self.wa, self.w * self.wbb - self.wb * self.wb
        if not (self.w > 0 and va > 0 and vb > 0):
            return math.nan
        return num / math.sqrt(va * vb) if va != vb else num / va

    @property
    def cosine(self):
        if not (self.waa > 0 and self.wbb > 0):
            return math.nan
        return self.wab / math.sqrt(self.waa * self.wbb) if self.waa != self.wbb else self.wab / self.waa

    @property
    def rms_diff(self):
        return math.sqrt(max(self.wdd, 0.0) / self.w) if self.w > 0 else math.nan

    def __repr__(self):
        return "PairStats(" + ", ".join(f"{k}={v:.6g}" for k, v in zip(PAIR_KEYS, self.sums)) + ")"


def pair_stats(a, b, weight=None):
    """PairStats of two device tensors of one shape (weight likewise, None: 1), every element one sample."""
    if a.shape != b.shape or (weight is not None and weight.shape != a.shape):
        raise ValueError(f"pair_stats: a, b and weight must have one shape, got {tuple(a.shape)}, {tuple(b.shape)}"
                         + ("" if weight is None else f", {tuple(weight.shape)}"))
    w = None if weight is None else ops.f32c(weight).reshape(1, -1)
    return PairStats(ops.pair_stats(ops.f32c(a).reshape(1, -1), ops.f32c(b).reshape(1, -1), w)[0].tolist())


# ---- host scores ----------------------------------------------------------------------------------------------
def _sym_sqrt(C):
    lam, V = np.linalg.eigh((C + C.T) * 0.5)
    return (V * np.sqrt(np.clip(lam, 0.0, None))) @ V.T


def frechet(mean1, cov1, mean2, cov2):
    """The Fréchet distance between two Gaussians, |m1 - m2|^2 + tr(C1 + C2 - 2 (C1^(1/2) C2 C1^(1/2))^(1/2)), by two
    symmetric eigendecompositions in float64; negative eigenvalues and a negative result are clamped at 0.  nan when
    an input holds a nan."""
    m1, m2 = np.asarray(mean1, dtype=np.float64), np.asarray(mean2, dtype=np.float64)
    C1, C2 = np.asarray(cov1, dtype=np.float64), np.asarray(cov2, dtype=np.float64)
    if not all(np.isfinite(x).all() for x in (m1, m2, C1, C2)):
        return math.nan
    S = _sym_sqrt(C1)
    M = S @ C2 @ S
    lam = np.linalg.eigvalsh((M + M.T) * 0.5)
    d = m1 - m2
    return float(max(d @ d + np.trace(C1) + np.trace(C2) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum(), 0.0))


# ---- the report -----------------------------------------------------------------------------------------------
def _analyse(y, sr, n_fft, n_mels):
    """(P [1, F, T], mel dB before the floor [1, n_mels, T], active frames [1, T] as 0 / 1) of a waveform [L]."""
    M, _, _, lohi, _ = audio._mel_device(sr, n_fft, n_mels, y.device)
    P = ops.stft(y.unsqueeze(0), n_fft, None, "power")
    mel = ops.mel_project(P, M, lohi)
    power = mel.sum(dim=1)                             # the frame's power on the mel grid
    active = (power >= ACTIVE_REL * power.amax()).to(torch.float32)
    return P, 10.0 * torch.log10(mel.clamp_min(AMIN)), active


def transfer_report(content, output, style, sr=audio.SR, keep=None, n_mfcc=20, n_fft=audio.N_FFT, n_mels=128,
                    loudness=False):
    """Scores of a transfer as a dict of Python floats; content, output: mono device waveforms [L] of one length,
    style: one waveform or a list (their MFCC moments are pooled).  keep: the mask [n_mels, 1 + L // hop] in [0, 1] the
    transfer used, or None.

    Log-mels are absolute dB, 10 log10(max(mel, 1e-10)), floored 80 dB below the louder of content and output.  A frame
    is active when its power (the mel power summed over the bins) is at least 1e-6 of its signal's maximum; the paired
    scores need it of both signals.

      onset_corr          Pearson correlation of the two onset envelopes, content against output (rhythm kept)
      chroma_sim          mean over the active frames of the cosine between content and output chroma (harmony kept)
      timbre_out_style, timbre_out_content, timbre_content_style
                          Fréchet distances between the distributions of MFCC 1 .. n_mfcc - 1 (c0 is level) over each
                          signal's active frames
      timbre_shift        (timbre_content_style - timbre_out_style) / timbre_content_style: 0 nothing moved, 1 arrived
      kept_rms_db, changed_rms_db   (with keep) RMS of the log-mel difference weighted by keep and by 1 - keep
      content_lufs, output_lufs, style_lufs, output_true_peak_db
                          (with loudness) ITU-R BS.1770-4 integrated loudness (audio.integrated_loudness; several
                          styles: the loudness of their mean gated power) and the output's 4x true peak in dB relative
                          to full scale; -inf for silence

    A score that has no value (no active frame, a constant envelope) is nan.  One host read at the end."""
    styles = list(style) if isinstance(style, (list, tuple)) else [style]
    if not styles:
        raise ValueError("transfer_report: no style recording")
    for name, y in [("content", content), ("output", output)] + [("style", s) for s in styles]:
        ops.require_device(y, dtype=None, what="transfer_report")
        if y.dim() != 1 or y.numel() < n_fft // 2 + 1:
            raise ValueError(f"transfer_report: {name} must be a mono waveform [L] of at least {n_fft // 2 + 1} "
                             f"samples, got shape {tuple(y.shape)}")
    if content.shape != output.shape:
        raise ValueError(f"transfer_report: content and output must have one length, got {content.numel()} and "
                         f"{output.numel()} samples")
    if not 2 <= int(n_mfcc) <= ops.MFCC_MAX:
        raise ValueError(f"transfer_report: n_mfcc must lie in 2..{ops.MFCC_MAX}, got {n_mfcc}")
    n_mfcc = int(n_mfcc)
    dev = content.device
    Pc, dbc, act_c = _analyse(content, sr, n_fft, n_mels)
    Po, dbo, act_o = _analyse(output, sr, n_fft, n_mels)
    T = dbc.shape[-1]
    if keep is not None:
        keep = torch.as_tensor(keep, dtype=torch.float32).to(dev)
        if tuple(keep.shape) != (n_mels, T):
            raise ValueError(f"transfer_report: keep must be [{n_mels}, {T}], got {tuple(keep.shape)}")
    floor = torch.maximum(dbc.amax(), dbo.amax()) - TOP_DB
    dbc, dbo = torch.maximum(dbc, floor), torch.maximum(dbo, floor)
    both = act_c * act_o

    rows = [ops.pair_stats(ops.onset_strength(dbc), ops.onset_strength(dbo))]
    cls, wt = _chroma_device(sr, n_fft, dev)
    w12 = both.unsqueeze(1).expand(1, 12, T).reshape(1, -1)
    rows.append(ops.pair_stats(ops.chroma(Pc, cls, wt).reshape(1, -1), ops.chroma(Po, cls, wt).reshape(1, -1), w12))
    if keep is not None:
        flat = keep.reshape(1, -1)
        rows.append(ops.pair_stats(dbc.reshape(1, -1), dbo.reshape(1, -1), flat))
        rows.append(ops.pair_stats(dbc.reshape(1, -1), dbo.reshape(1, -1), 1.0 - flat))
    D = _dct_device(n_mfcc, n_mels, dev)
    moms = [ops.mfcc_moments(dbc, D, act_c), ops.mfcc_moments(dbo, D, act_o)]
    for s in styles:
        _, dbs, act_s = _analyse(s, sr, n_fft, n_mels)
        moms.append(ops.mfcc_moments(torch.maximum(dbs, floor), D, act_s))
    parts = [torch.cat(rows).reshape(-1), torch.cat(moms).reshape(-1)]
    if loudness:
        parts.append(torch.stack([audio.integrated_loudness(y, sr) for y in [content, output] + styles]))
        parts.append(audio.true_peak(output, sr).double().reshape(1))
    host = torch.cat(parts).cpu().numpy()   # the one host read
    if loudness:
        host, loud = host[:-(3 + len(styles))], host[-(3 + len(styles)):]

    pairs = [PairStats(host[7 * i:7 * i + 7]) for i in range(len(rows))]
    sums = host[7 * len(rows):].reshape(len(moms), -1)
    dist = {}
    for name, s in (("content", sums[0:1]), ("out", sums[1:2]), ("style", sums[2:])):
        _, mean, cov = moments_from_sums(s, n_mfcc)
        dist[name] = (mean[1:], cov[1:, 1:])
    out_style = frechet(*dist["out"], *dist["style"])
    out_content = frechet(*dist["out"], *dist["content"])
    content_style = frechet(*dist["content"], *dist["style"])
    rep = {
        "onset_corr": pairs[0].pearson,
        "chroma_sim": 12.0 * pairs[1].wab / pairs[1].w if pairs[1].w > 0 else math.nan,
        "timbre_out_style": out_style,
        "timbre_out_content": out_content,
        "timbre_content_style": content_style,
        "timbre_shift": (content_style - out_style) / content_style if content_style > 0 else math.nan,
    }
    if keep is not None:
        rep["kept_rms_db"], rep["changed_rms_db"] = pairs[2].rms_diff, pairs[3].rms_diff
    if loudness:
        gated = [10.0 ** (v / 10.0) for v in loud[2:-1] if np.isfinite(v)]
        rep["content_lufs"], rep["output_lufs"] = loud[0], loud[1]
        rep["style_lufs"] = 10.0 * math.log10(sum(gated) / len(gated)) if gated else -math.inf
        rep["output_true_peak_db"] = 20.0 * math.log10(loud[-1]) if loud[-1] > 0 else -math.inf
    return {k: float(v) for k, v in rep.items()}
