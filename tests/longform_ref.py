"""The float64 yardstick of the whole-recording path (ldm_amd/longform.py, csrc/longform.hip): the window plan, the
windowed log-mel front end and the crossfade stitch, in numpy, written from their definitions and
independently of ldm_amd.  Not a test file: tests/test_longform_host.py pins it on the CPU and
tests/test_gpu_longform.py compares the kernels to it."""
import math

import numpy as np


def window_plan(T_total, frames=512, overlap=64):
    if frames % 64 or frames < 64 or not 0 <= overlap <= frames // 2 or T_total < 1:
        raise ValueError("bad plan")
    stride = frames - overlap
    return max(1, math.ceil((T_total - overlap) / stride)), stride


def cut(A, frames, overlap, fill=0.0):
    """[n_mels, T_total] -> [N, n_mels, frames]: window n is columns [n stride, n stride + frames), `fill` beyond."""
    A = np.asarray(A, dtype=np.float64)
    N, stride = window_plan(A.shape[1], frames, overlap)
    pad = np.full((A.shape[0], (N - 1) * stride + frames), fill)
    pad[:, :A.shape[1]] = A
    return np.stack([pad[:, n * stride:n * stride + frames] for n in range(N)])


def window_db(P, frames, overlap, amin=1e-10, top_db=80.0):
    """(db [N, n_mels, frames] relative to each window's own maximum and clamped at -top_db, ref_db [N])."""
    W = cut(P, frames, overlap)
    ref = 10.0 * np.log10(np.maximum(amin, W.max(axis=(1, 2))))
    db = 10.0 * np.log10(np.maximum(amin, W)) - ref[:, None, None]
    return np.maximum(db, -top_db), ref


def mel_windows(P, frames, overlap, max_db=80.0, amin=1e-10, top_db=80.0):
    """(x [N, 1, n_mels, frames] = 8-bit levels / 255, ref_db [N])."""
    db, ref = window_db(P, frames, overlap, amin, top_db)
    px = np.floor(np.clip((db + max_db) * (255.0 / max_db), 0.0, 255.0) + 0.5)
    return (px / 255.0)[:, None], ref


def stitch_db(d, overlap, T_total):
    """Absolute dB maps d [N, n_mels, frames] of the windows -> [n_mels, T_total] with the linear crossfade."""
    d = np.asarray(d, dtype=np.float64)
    N, n_mels, frames = d.shape
    want, stride = window_plan(T_total, frames, overlap)
    assert N == want, (N, want)
    out = np.empty((n_mels, T_total))
    for t in range(T_total):
        n1 = min(N - 1, t // stride)
        j1 = t - n1 * stride
        if n1 >= 1 and j1 < overlap:
            out[:, t] = ((overlap - j1) / (overlap + 1.0)) * d[n1 - 1, :, j1 + stride] \
                + ((j1 + 1) / (overlap + 1.0)) * d[n1, :, j1]
        else:
            out[:, t] = d[n1, :, j1]
    return out


def stitch(y, ref_db, overlap, T_total, max_db=80.0):
    """Decoded windows y [N, 1, n_mels, frames] -> (power [n_mels, T_total], db [n_mels, T_total])."""
    y = np.asarray(y, dtype=np.float64)[:, 0]
    d = np.clip(y, 0.0, 1.0) * max_db - max_db + np.asarray(ref_db, dtype=np.float64)[:, None, None]
    db = stitch_db(d, overlap, T_total)
    return 10.0 ** (0.1 * db), db


def in_overlap(T_total, frames, overlap):
    """bool [T_total]: the frames that two windows cover."""
    N, stride = window_plan(T_total, frames, overlap)
    t = np.arange(T_total)
    n1 = np.minimum(N - 1, t // stride)
    return (n1 >= 1) & (t - n1 * stride < overlap)


def random_power(n_mels, T, seed, decades=12.0):
    """Power spanning `decades` decades around 1, log-uniform, from PCG64(seed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return 10.0 ** (decades * (rng.random((n_mels, T)) - 0.5))
