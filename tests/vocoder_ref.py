"""The float64 yardstick of the content-anchored vocoder: a numpy restatement of the definitions
csrc/vocoder.hip and the anchored Griffin-Lim epilogue of csrc/audio.hip implement.  Not a test file;
tests/test_vocoder_host.py pins it on the CPU and tests/test_gpu_vocoder.py compares the kernels to it.  STFT, ISTFT,
filterbank and the plain Griffin-Lim recurrence come from tests/audio_ref.py.  Written from the definitions,
independently of ldm_amd.

    G[m, t]  = (Mo[m, t] + eps) / (Mc[m, t] + eps)
    Wn[m, f] = M[m, f] / sum_m' M[m', f]           for bins whose column sum is positive
    g[f, t]  = clamp(sum_m Wn[m, f] G[m, t], 0, 10^(max_gain_db / 10)),   1 for a bin no filter covers
    Pm = g |C|^2,   A = sqrt(Pm + R),   P0 = C / |C|  ((1, 0) where |C| < TINY32)
    a  = clamp(1 - |10 log10((A^2 + eps) / (|C|^2 + eps))| / anchor_db, 0, 1),   0 everywhere when anchor_db <= 0
"""
import numpy as np

import audio_ref as R

TINY32 = R.TINY32


def _eps(eps, B):
    e = np.asarray(eps, dtype=np.float64).reshape(-1)
    assert (e > 0).all() and e.size in (1, B)
    return np.broadcast_to(e, (B,)).reshape(B, 1, 1)


def bin_gain(Mo, Mc, M, eps, max_gain_db):
    """g [B, F, T] from the mels [B, n_mels, T] and the filterbank M [n_mels, F]."""
    Mo, Mc, M = (np.asarray(v, dtype=np.float64) for v in (Mo, Mc, M))
    e = _eps(eps, Mo.shape[0])
    G = (Mo + e) / (Mc + e)
    col = M.sum(axis=0)
    covered = col > 0
    Wn = np.zeros_like(M)
    Wn[:, covered] = M[:, covered] / col[covered]
    g = np.einsum("mf,bmt->bft", Wn, G)
    g[:, ~covered, :] = 1.0
    return np.clip(g, 0.0, 10.0 ** (max_gain_db / 10.0))


def masked_power(C, Mo, Mc, M, eps, max_gain_db):
    return bin_gain(Mo, Mc, M, eps, max_gain_db) * np.abs(np.asarray(C, dtype=np.complex128)) ** 2


def unit_phase(C):
    C = np.asarray(C, dtype=np.complex128)
    mod = np.abs(C)
    small = mod < TINY32
    return np.where(small, 1.0 + 0.0j, C / np.where(small, 1.0, mod))


def anchor_weight(A2, P2, eps, anchor_db):
    """(a, the value before the clamp to [0, 1]); anchor_db <= 0: a = 0 (and the pre-clamp value -inf)."""
    if anchor_db <= 0:
        return np.zeros_like(A2), np.full_like(A2, -np.inf)
    e = _eps(eps, A2.shape[0])
    pre = 1.0 - np.abs(10.0 * np.log10((A2 + e) / (P2 + e))) / anchor_db
    return np.clip(pre, 0.0, 1.0), pre


def mel_gain_target(C, Mo, Mc, M, eps, max_gain_db=40.0, anchor_db=6.0, residual=None):
    """(A, P0, a, pre): target magnitude, unit phase, anchor weight and the weight before its clamp, each [B, F, T]."""
    C = np.asarray(C, dtype=np.complex128)
    P2 = np.abs(C) ** 2
    A2 = masked_power(C, Mo, Mc, M, eps, max_gain_db)
    if residual is not None:
        A2 = A2 + np.asarray(residual, dtype=np.float64)
    a, pre = anchor_weight(A2, P2, eps, anchor_db)
    return np.sqrt(A2), unit_phase(C), a, pre


def griffinlim_anchored(mag, P0, a, n_iter, momentum=0.99, n_fft=None, init_angles=None, return_min_blend=False):
    """audio_ref.griffinlim's recurrence with every iteration's phase replaced by unit(a P0 + (1 - a) angles): angles
    itself where a == 0, P0 itself where a == 1.  Starts from init_angles (default P0).  With return_min_blend also the
    smallest |a P0 + (1 - a) angles| met over the bins with 0 < a < 1 in any iteration (inf when there is none)."""
    mag = np.asarray(mag, dtype=np.float64)
    P0 = np.asarray(P0, dtype=np.complex128)
    a = np.asarray(a, dtype=np.float64)
    n_fft = 2 * (mag.shape[-2] - 1) if n_fft is None else n_fft
    angles = P0.copy() if init_angles is None else np.asarray(init_angles, dtype=np.complex128)
    prev = np.zeros_like(angles)
    mid = (a > 0) & (a < 1)
    min_blend = np.inf
    for _ in range(n_iter):
        r = R.stft(R.istft(mag * angles, n_fft=n_fft), n_fft)
        ang = r - (momentum / (1.0 + momentum)) * prev
        ang = ang / (np.abs(ang) + TINY32)
        prev = r
        blend = a * P0 + (1.0 - a) * ang
        if mid.any():
            min_blend = min(min_blend, float(np.abs(blend[mid]).min()))
        mixed = blend / (np.abs(blend) + TINY32)
        angles = np.where(a <= 0, ang, np.where(a >= 1, P0, mixed))
    y = R.istft(mag * angles, n_fft=n_fft)
    return (y, min_blend) if return_min_blend else y


def smooth_gain_db(shape, span_db, seed):
    """A smooth random field over the last two axes of `shape` spanning [-span_db, span_db] dB exactly: white noise
    from PCG64(seed) smoothed by a 5 x 3 box and rescaled per item."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(shape)
    for ax, k in ((-2, 5), (-1, 3)):
        x = sum(np.roll(x, s, axis=ax) for s in range(-(k // 2), k // 2 + 1)) / k
    lo = x.min(axis=(-2, -1), keepdims=True)
    hi = x.max(axis=(-2, -1), keepdims=True)
    return (2.0 * (x - lo) / (hi - lo) - 1.0) * span_db


# ---- the test inputs (shared by the CPU and the GPU tests, so the seeds' properties are asserted where they are used) --
CASES = {"n2048": (2048, 4096, 2), "n512": (512, 2048 + 37, 3)}   # n_fft, L, B: 9 frames; 17 frames, ragged tail
N_MELS, MAX_GAIN_DB, SPAN_DB = 128, 20.0, 30.0


def f32(x):
    """x rounded to float32 (complex: to complex64) and back: the tests' inputs are exact in both precisions."""
    x = np.asarray(x)
    return x.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float32).astype(np.float64)


def gain_case(name, seed=11):
    """One case's inputs, all float32-exact: C [B, F, T] (B different items, |C| exactly 0 in a few bins), the
    filterbank M, Mc = M |C|^2, Mo = Mc times a smooth gain spanning +-SPAN_DB dB (beyond the MAX_GAIN_DB clamp on
    some bins), eps [B] = max(Mc) 1e-8 and a residual power R [B, F, T]."""
    n_fft, L, B = CASES[name]
    y = np.stack([R.test_signal(L, variant=v) for v in range(B)])
    C = f32(R.stft(y, n_fft))
    rng = np.random.Generator(np.random.PCG64(seed))
    zero = rng.random(C.shape) < 0.003
    zero[:, 7, 2] = True
    C[zero] = 0.0
    M = R.mel_filterbank(22050, n_fft, N_MELS)
    Mc = f32(np.einsum("mf,bft->bmt", M, np.abs(C) ** 2))
    Mo = f32(Mc * 10.0 ** (smooth_gain_db(Mc.shape, SPAN_DB, seed + 1) / 10.0))
    eps = f32(Mc.max(axis=(1, 2)) * 1e-8)
    Rres = f32(rng.random(C.shape) ** 4 * 0.5 * (np.abs(C) ** 2).mean())
    return dict(n_fft=n_fft, L=L, B=B, C=C, zero=zero, M=M, Mc=Mc, Mo=Mo, eps=eps, R=Rres)
