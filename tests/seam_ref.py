"""Float64 yardstick for the joint sampling of overlapping windows.

Written from the definition.  The rows of x [B, C, H, W] are neighbouring windows that share `ov` latent columns,
1 <= ov <= W / 2.  One seam fuse replaces, for every b < B - 1 and j in [0, ov),
    a = x[b, :, :, W-ov+j];  q = x[b+1, :, :, j];  w_j = (j + 1) / (ov + 1);  m = a + w_j (q - a)
in both places by m.  A joint loop fuses once before step 0 and after every step's update (after the keep blend when
there is one); the logs and the solver's history are the model's own x0 / eps, unfused.  Guided, target and base are
evaluated on the same fused state (the engine's doubled state: two equal halves fused separately).  numpy only,
except sample(), which calls the oracle's UNet in float64 through guidance_ref.unet_eps_fn.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as GR    # noqa: E402
import regional_ref as RR    # noqa: E402
import solver_ref as SR      # noqa: E402


def weights(ov):
    """[ov] float64: the later window's weight at each seam column."""
    return (np.arange(ov, dtype=np.float64) + 1.0) / (ov + 1.0)


def fuse(x, ov):
    """A fused copy of x [B, C, H, W] (float64); x itself is left alone."""
    x = np.array(x, dtype=np.float64)
    B, _, _, W = x.shape
    ov = int(ov)
    if not 1 <= ov <= W // 2:
        raise ValueError(f"fuse: ov must lie in [1, W / 2], got {ov} for W {W}")
    w = weights(ov)
    for b in range(B - 1):
        a, q = x[b, :, :, W - ov:].copy(), x[b + 1, :, :, :ov].copy()
        m = a + w * (q - a)
        x[b, :, :, W - ov:] = m
        x[b + 1, :, :, :ov] = m
    return x


def solve(ab, times, x, eps_fn, ov, solver="dpmpp2m", eta=0.0, keep=None, eps_b_fn=None, s=None):
    """regional_ref.solve with a fuse before step 0 and after each step.  keep = (z0, n0, w, coefs) or None;
    eps_b_fn / s: guided as in guidance_ref.solve.  Returns (x_final, [x0_i], [eps_i]), the logs unfused."""
    order = {"ddim": 0, "dpmpp1": 1, "dpmpp2m": 2}[solver]
    x = fuse(x, ov)
    x0s, epss, prev = [], [], None
    for i in range(len(times) - 1):
        e = np.asarray(eps_fn(x, i), dtype=np.float64)
        if eps_b_fn is not None:
            e = GR.guide(e, eps_b_fn(x, i), s)
        if order:
            xu, x0 = SR.step(ab, times, i, x, e, prev, order)
        else:
            xu, x0 = GR.ddim_step(ab, times, i, x, e, eta)
        if keep is not None:
            xu = RR.keep_blend(xu, keep[0], keep[1], keep[2], keep[3][i][0], keep[3][i][1])
        x = fuse(xu, ov)
        x0s.append(x0)
        epss.append(e)
        prev = x0
    return x, x0s, epss


def sample(sd64, ab, times, x, maps, ov, solver="dpmpp2m", eta=0.0, keep=None, base=None, s=None, exact_last=True):
    """maps / base: (s5, s6) as in guidance_ref.sample; keep = (z0, n0, w) or None."""
    B = x.shape[0]
    fb = None if base is None else GR.unet_eps_fn(sd64, times, B, *base)
    kp = None if keep is None else tuple(keep) + (RR.keep_coefs(ab, times, exact_last),)
    return solve(ab, times, x, GR.unet_eps_fn(sd64, times, B, *maps), ov, solver, eta, kp, fb, s)


def noise_windows(N, C, H, W, ov, seed):
    """longform.noise_windows restated: window n is columns [n (W - ov), n (W - ov) + W) of one canvas draw
    [C, H, (N - 1)(W - ov) + W] from torch.Generator().manual_seed(seed).  Returns (windows [N, C, H, W], canvas)."""
    import torch
    stride = W - ov
    canvas = torch.randn((C, H, (N - 1) * stride + W), generator=torch.Generator().manual_seed(int(seed)))
    return torch.stack([canvas[:, :, n * stride:n * stride + W] for n in range(N)]), canvas
