"""Whole recordings through a model that takes one window (csrc/longform.hip): the window plan, the
windowed log-mel front end and the crossfade stitch that puts the decoded windows back into one mel power map.

A recording of T_total mel frames is covered by N windows of `frames` frames that start every stride = frames -
overlap frames.  Each window is referred to its own maximum, exactly as the training images are
(audio.chunk_mel_images); the stitch undoes that per window and crossfades linearly in dB where two windows overlap.
overlap <= frames / 2, so no frame lies in more than two windows.
"""
import numpy as np
import torch

from . import audio, ops


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


def noise_windows(N, C, H, W, ov, seed):
    """The q_sample noise of N neighbouring latent windows [N, C, H, W] that share `ov` latent columns (0 <= ov <=
    W / 2), cut from one canvas: one CPU draw [C, H, (N - 1)(W - ov) + W] from torch.Generator().manual_seed(seed),
    window n holding its columns [n (W - ov), n (W - ov) + W).  Neighbours therefore share their overlap's noise,
    noise[n, :, :, W-ov:] == noise[n+1, :, :, :ov], whatever batch size the windows are later grouped by (joint
    sampling).  CPU fp32."""
    N, C, H, W, ov = int(N), int(C), int(H), int(W), int(ov)
    if N < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError(f"noise_windows: need N, C, H, W >= 1, got {N}, {C}, {H}, {W}")
    if not 0 <= ov <= W // 2:
        raise ValueError(f"noise_windows: ov must lie in [0, W / 2], got {ov} for W {W}")
    stride = W - ov
    canvas = torch.randn((C, H, (N - 1) * stride + W), generator=torch.Generator().manual_seed(int(seed)))
    return torch.stack([canvas[:, :, n * stride:n * stride + W] for n in range(N)]).contiguous()


def _keep_profile(n, lo, hi, feather):
    """[n] float64: 1 on indices [lo, hi] (clipped to the axis), 0 elsewhere, with a linear ramp over the `feather`
    outermost indices inside each edge, (d + 1) / (feather + 1) at distance d from the edge.  An edge that is the
    axis' own end gets no ramp."""
    p = np.zeros(n, dtype=np.float64)
    lo, hi = max(int(lo), 0), min(int(hi), n - 1)
    if hi < lo:
        return p
    idx = np.arange(lo, hi + 1)
    w = np.ones(idx.shape[0], dtype=np.float64)
    if feather > 0:
        if lo > 0:
            w = np.minimum(w, (idx - lo + 1) / (feather + 1.0))
        if hi < n - 1:
            w = np.minimum(w, (hi - idx + 1) / (feather + 1.0))
    p[lo:hi + 1] = w
    return p


def keep_mask(T_total, n_mels=128, sr=audio.SR, times=(), bands=(), feather=0):
    """The keep mask [n_mels, T_total] in [0, 1] (CPU fp32) of a recording of T_total mel frames: 1 where the content
    is to stay as it is.  times: (t0, t1) spans in seconds, covering the frames whose time f * hop / sr lies in
    [t0, t1]; bands: (f_lo, f_hi) in Hz, covering the mel bins whose centre frequency (audio.mel_centre_frequencies)
    lies in [f_lo, f_hi].  feather: a linear ramp of that many frames (bins) inside each edge of a region, except at
    the ends of the recording (of the mel axis).  The result is the union (max) of all regions; none gives zeros."""
    T_total, n_mels, feather = int(T_total), int(n_mels), int(feather)
    if T_total < 1 or n_mels < 1 or feather < 0:
        raise ValueError(f"keep_mask: need T_total >= 1, n_mels >= 1, feather >= 0; got {T_total}, {n_mels}, {feather}")
    hop = audio.N_FFT // 4
    m = np.zeros((n_mels, T_total), dtype=np.float64)
    ft = np.arange(T_total) * (hop / float(sr))
    for t0, t1 in times:
        if not t0 <= t1:
            raise ValueError(f"keep_mask: a time span needs t0 <= t1, got ({t0}, {t1})")
        inside = np.nonzero((ft >= t0) & (ft <= t1))[0]
        if inside.size:
            m = np.maximum(m, _keep_profile(T_total, inside[0], inside[-1], feather)[None, :])
    fc = audio.mel_centre_frequencies(sr, n_mels)
    for f0, f1 in bands:
        if not f0 <= f1:
            raise ValueError(f"keep_mask: a band needs f_lo <= f_hi, got ({f0}, {f1})")
        inside = np.nonzero((fc >= f0) & (fc <= f1))[0]
        if inside.size:
            m = np.maximum(m, _keep_profile(n_mels, inside[0], inside[-1], feather)[:, None])
    return torch.from_numpy(m.astype(np.float32))


def mask_windows(mask, frames=512, overlap=64):
    """A keep mask [n_mels, T_total] cut by window_plan exactly as the content is cut: [N, 1, n_mels, frames], window n
    holding frames [n * stride, n * stride + frames); frames at or beyond T_total (a padded tail) get 0."""
    if mask.dim() != 2:
        raise ValueError(f"mask_windows: the mask must be [n_mels, T_total], got {tuple(mask.shape)}")
    n_mels, T_total = mask.shape
    N, stride = window_plan(T_total, frames, overlap)
    out = torch.zeros((N, 1, n_mels, frames), dtype=mask.dtype, device=mask.device)
    for n in range(N):
        t0 = n * stride
        t1 = min(t0 + frames, T_total)
        if t1 > t0:
            out[n, 0, :, :t1 - t0] = mask[:, t0:t1]
    return out


def style_map_windows(style_map, frames=512, overlap=64, n_mels=128):
    """A recording's style map cut by window_plan exactly as the content is cut.  style_map [R, n_mels, T_total] (or
    [R, T_total], broadcast over the n_mels mel bins): the non-negative weight of each of R style references at every
    bin and frame.  Returns [N, R, n_mels, frames], window n holding frames [n * stride, n * stride + frames); frames at
    or beyond T_total (a padded tail) repeat the last real frame: zeros there would leave a position without any
    reference (LDM.style_map_bias wants a positive sum everywhere)."""
    if not isinstance(style_map, torch.Tensor) or style_map.dim() not in (2, 3):
        raise ValueError("style_map_windows: the map must be a tensor [R, n_mels, T_total] or [R, T_total]")
    if style_map.dim() == 2:
        style_map = style_map[:, None, :].expand(style_map.shape[0], int(n_mels), style_map.shape[1])
    R, M, T_total = style_map.shape
    if R < 1:
        raise ValueError("style_map_windows: the map needs at least one reference")
    N, stride = window_plan(T_total, frames, overlap)
    t = torch.arange(N, device=style_map.device)[:, None] * stride + torch.arange(frames, device=style_map.device)[None, :]
    t = t.clamp_(max=T_total - 1)                                # [N, frames]: the tail repeats the last real frame
    return style_map[:, :, t].permute(2, 0, 1, 3).contiguous()   # [R, M, N, frames] -> [N, R, M, frames]


def morph_map(R, T_total):
    """[R, T_total] float64: a morph from the first of R references to the last along a recording of T_total frames.
    Piecewise-linear triangular weights max(0, 1 - |u - r|) at u = t (R - 1) / (T_total - 1): frame 0 is all the first
    reference, the last frame all the last, reference r peaks at its own knot, and every frame's weights sum to 1."""
    R, T_total = int(R), int(T_total)
    if R < 1 or T_total < 1:
        raise ValueError(f"morph_map: need R >= 1 and T_total >= 1, got {R}, {T_total}")
    if R == 1:
        return torch.ones((1, T_total), dtype=torch.float64)
    # t (R - 1) is an exact integer, and its quotient by T_total - 1 at the last frame is exactly R - 1
    u = (torch.arange(T_total, dtype=torch.float64) * (R - 1)) / max(T_total - 1, 1)
    w = (1.0 - (u[None, :] - torch.arange(R, dtype=torch.float64)[:, None]).abs()).clamp_(min=0.0)
    return w / w.sum(0, keepdim=True)
