"""Whole recordings through a model that takes one window (csrc/longform.hip): the window plan, the
windowed log-mel front end and the crossfade stitch that puts the decoded windows back into one mel power map.

A recording of T_total mel frames is covered by N windows of `frames` frames that start every stride = frames -
overlap frames.  Each window is referred to its own maximum, exactly as the training images are
(audio.chunk_mel_images); the stitch undoes that per window and crossfades linearly in dB where two windows overlap.
overlap <= frames / 2, so no frame lies in more than two windows.
"""
from . import ops


def window_plan(T_total, frames=512, overlap=64):
    """(N, stride): N = max(1, ceil((T_total - overlap) / stride)) windows, stride = frames - overlap; window n covers
    mel frames [n * stride, n * stride + frames), frames at or beyond T_total hold zero power."""
    T_total, frames, overlap = int(T_total), int(frames), int(overlap)
    if frames < 64 or frames % 64 != 0:
        raise ValueError(f"window_plan: frames must be a positive multiple of 64 (the model's /64 geometry), got {frames}")
    if not 0 <= overlap <= frames // 2:
        raise ValueError(f"window_plan: overlap must lie in [0, frames / 2], got {overlap} for frames {frames}")
    if T_total < 1:
        raise ValueError(f"window_plan: T_total must be at least 1, got {T_total}")
    stride = frames - overlap
    return max(1, -(-(T_total - overlap) // stride)), stride


def mel_windows(P, frames=512, overlap=64, max_db=80):
    """Mel power P [n_mels, T_total] (CUDA) -> (x [N, 1, n_mels, frames], ref_db [N]): the model's [0,1] input of every
    window and each window's reference level 10 log10(max(1e-10, window max)), which stitch_windows needs back."""
    window_plan(P.shape[-1], frames, overlap)
    return ops.mel_windows(P, frames, overlap, max_db)


def stitch_windows(y, ref_db, overlap, T_total, max_db=80, return_db=False):
    """Decoded windows y [N, 1, n_mels, frames] (the decoder's [0,1] output, clamped, not re-quantised) -> mel power
    [n_mels, T_total].  Inside an overlap the two windows' dB values are mixed with weights (overlap - j) / (overlap +
    1) and (j + 1) / (overlap + 1), j the frame's index in the later window; overlap = 0 is plain concatenation."""
    N, stride = window_plan(T_total, y.shape[-1], overlap)
    if y.shape[0] != N:
        raise ValueError(f"stitch_windows: {y.shape[0]} windows given, the plan of T_total {T_total} has {N}")
    return ops.mel_stitch(y, ref_db, overlap, T_total, max_db, return_db)
