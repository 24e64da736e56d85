"""Float64 numpy restatement of the transfer report's definitions: the yardstick of
tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.  It takes nothing from the code under test; audio_ref.py
supplies the STFT and the mel filterbank."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R         # noqa: E402

SR, N_FFT, HOP, N_MELS = 22050, 2048, 512, 128
AMIN, TOP_DB, ACTIVE_REL = 1e-10, 80.0, 1e-6
FLT_MIN = float(np.finfo(np.float32).tiny)


# ---- tables -----------------------------------------------------------------------------------------------------
def chroma_filterbank(sr, n_fft, fmin=55.0, fmax=5000.0):
    """(cls [F] int, wt [F] float64); cls = -1 outside [fmin, fmax]."""
    F = n_fft // 2 + 1
    cls, wt = np.full(F, -1, dtype=np.int64), np.zeros(F)
    for f in range(F):
        v = f * sr / n_fft
        if v <= 0 or v < fmin or v > fmax:
            continue
        p = 69.0 + 12.0 * math.log2(v / 440.0)
        cls[f] = int(math.floor(p)) % 12
        wt[f] = 1.0 - (p - math.floor(p))
    return cls, wt


def dct_basis(n_mfcc, n_mels):
    D = np.zeros((n_mfcc, n_mels))
    for k in range(n_mfcc):
        for m in range(n_mels):
            D[k, m] = math.sqrt(1.0 / n_mels) if k == 0 else \
                math.sqrt(2.0 / n_mels) * math.cos(math.pi * k * (2 * m + 1) / (2 * n_mels))
    return D


# ---- features ---------------------------------------------------------------------------------------------------
def onset_strength(db, lag=1):
    """db [B, n_mels, T] -> env [B, T]"""
    db = np.asarray(db, dtype=np.float64)
    B, n_mels, T = db.shape
    env = np.zeros((B, T))
    if T > lag:
        env[:, lag:] = np.maximum(db[:, :, lag:] - db[:, :, :-lag], 0.0).sum(axis=1) / n_mels
    return env


def chroma_raw(P, cls, wt):
    """The 12 class sums [B, 12, T] before the normalisation."""
    P = np.asarray(P, dtype=np.float64)
    B, F, T = P.shape
    acc = np.zeros((B, 12, T))
    for f in range(F):
        if cls[f] < 0:
            continue
        acc[:, cls[f]] += wt[f] * P[:, f]
        acc[:, (cls[f] + 1) % 12] += (1.0 - wt[f]) * P[:, f]
    return acc


def chroma(P, cls, wt):
    acc = chroma_raw(P, cls, wt)
    n = np.sqrt((acc * acc).sum(axis=1, keepdims=True))
    return np.where(n >= FLT_MIN, acc / np.where(n >= FLT_MIN, n, 1.0), 0.0)


def mfcc_sums(db, D, w=None):
    """(sums [B, E], abs [B, E]): { sum w, sum w c_k, sum w c_j c_k (j <= k) } per item and the sums of the absolute
    terms of each entry, the coefficients' own terms taken absolutely too (what an error bound scales with)."""
    db = np.asarray(db, dtype=np.float64)
    B, n_mels, T = db.shape
    n = D.shape[0]
    w = np.ones((B, T)) if w is None else np.asarray(w, dtype=np.float64)
    c = np.einsum("km,bmt->bkt", D, db)
    ca = np.einsum("km,bmt->bkt", np.abs(D), np.abs(db))
    iu = np.triu_indices(n)
    sums = np.concatenate([w.sum(1, keepdims=True), np.einsum("bt,bkt->bk", w, c),
                           np.einsum("bt,bjt,bkt->bjk", w, c, c)[:, iu[0], iu[1]]], axis=1)
    absw = np.abs(w)
    mags = np.concatenate([absw.sum(1, keepdims=True), np.einsum("bt,bkt->bk", absw, ca),
                           np.einsum("bt,bjt,bkt->bjk", absw, ca, ca)[:, iu[0], iu[1]]], axis=1)
    return sums, mags


def moments_from_sums(s, n):
    s = np.asarray(s, dtype=np.float64).reshape(-1, 1 + n + n * (n + 1) // 2).sum(axis=0)
    count = s[0]
    mean = s[1:1 + n] / count
    second = np.zeros((n, n))
    second[np.triu_indices(n)] = s[1 + n:]
    second = second + np.triu(second, 1).T
    return count, mean, second / count - np.outer(mean, mean)


def pair_sums(a, b, w=None):
    """(sums [B, 7], abs [B, 7]) of a, b, w [B, n]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = np.ones_like(a) if w is None else np.asarray(w, dtype=np.float64)
    terms = [w, w * a, w * b, w * a * a, w * b * b, w * a * b, w * (a - b) ** 2]
    return np.stack([t.sum(1) for t in terms], 1), np.stack([np.abs(t).sum(1) for t in terms], 1)


def pearson(s):
    w, wa, wb, waa, wbb, wab = s[:6]
    va, vb = w * waa - wa * wa, w * wbb - wb * wb
    return (w * wab - wa * wb) / math.sqrt(va * vb) if w > 0 and va > 0 and vb > 0 else math.nan


def frechet_sqrtm(m1, C1, m2, C2):
    """The same distance through scipy.linalg.sqrtm"""
    from scipy.linalg import sqrtm
    S = np.real(sqrtm(C1))
    d = np.asarray(m1) - np.asarray(m2)
    return float(d @ d + np.trace(C1) + np.trace(C2) - 2.0 * np.trace(np.real(sqrtm(S @ C2 @ S))))


# ---- the report -------------------------------------------------------------------------------------------------
def analyse(y):
    P = np.abs(R.stft(np.asarray(y, dtype=np.float64))) ** 2                 # [F, T]
    mel = R.mel_filterbank(SR, N_FFT, N_MELS) @ P
    power = mel.sum(axis=0)
    return P, 10.0 * np.log10(np.maximum(mel, AMIN)), (power >= ACTIVE_REL * power.max()).astype(np.float64)


def transfer_report(content, output, styles, keep=None, n_mfcc=20):
    Pc, dbc, ac = analyse(content)
    Po, dbo, ao = analyse(output)
    floor = max(dbc.max(), dbo.max()) - TOP_DB
    dbc, dbo = np.maximum(dbc, floor), np.maximum(dbo, floor)
    both = ac * ao
    rep = {"onset_corr": pearson(pair_sums(onset_strength(dbc[None]), onset_strength(dbo[None]))[0][0])}
    cls, wt = chroma_filterbank(SR, N_FFT)
    cc, co = chroma(Pc[None], cls, wt)[0], chroma(Po[None], cls, wt)[0]
    rep["chroma_sim"] = float(((cc * co).sum(axis=0) * both).sum() / both.sum()) if both.sum() > 0 else math.nan
    D = dct_basis(n_mfcc, N_MELS)

    def dist(dbs, acts):
        s = np.concatenate([mfcc_sums(d[None], D, a[None])[0] for d, a in zip(dbs, acts)])
        _, mean, cov = moments_from_sums(s, n_mfcc)
        return mean[1:], cov[1:, 1:]
    st = [analyse(s) for s in styles]
    d_c, d_o = dist([dbc], [ac]), dist([dbo], [ao])
    d_s = dist([np.maximum(s[1], floor) for s in st], [s[2] for s in st])
    rep["timbre_out_style"] = max(frechet_sqrtm(*d_o, *d_s), 0.0)
    rep["timbre_out_content"] = max(frechet_sqrtm(*d_o, *d_c), 0.0)
    rep["timbre_content_style"] = max(frechet_sqrtm(*d_c, *d_s), 0.0)
    rep["timbre_shift"] = (rep["timbre_content_style"] - rep["timbre_out_style"]) / rep["timbre_content_style"]
    if keep is not None:
        keep = np.asarray(keep, dtype=np.float64)
        d2 = (dbc - dbo) ** 2
        rep["kept_rms_db"] = math.sqrt((keep * d2).sum() / keep.sum()) if keep.sum() > 0 else math.nan
        rep["changed_rms_db"] = math.sqrt(((1 - keep) * d2).sum() / (1 - keep).sum()) if (1 - keep).sum() > 0 \
            else math.nan
    return rep, (d_c, d_o, d_s)


# ---- two-second synthetic signals of the behaviour tests ---------------------------------------------------------
L2S = 2 * SR


def tone(hz, amp=0.5, L=L2S):
    return amp * np.sin(2.0 * np.pi * hz * np.arange(L) / SR)


def click_train(period=5512, offset=1000, L=L2S, width=64):
    """Short decaying noise bursts every `period` samples from `offset` on."""
    y = np.zeros(L)
    burst = np.random.default_rng(3).standard_normal(width) * np.exp(-np.arange(width) / 16.0)
    for s in range(offset, L - width, period):
        y[s:s + width] += 0.8 * burst
    return y


def noise(seed, lowpass=None, L=L2S):
    """White noise; lowpass: a one-pole smoothing coefficient applied forwards (None: white)."""
    x = 0.1 * np.random.default_rng(seed).standard_normal(L)
    if lowpass is None:
        return x
    from scipy.signal import lfilter
    return lfilter([1.0 - lowpass], [1.0, -lowpass], x) * 3.0
