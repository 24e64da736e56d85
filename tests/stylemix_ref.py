"""Float64 yardstick for style mixing: cross-attention over several weighted style references.

Written from the definition: for a query q of one head, keys k_{r,j} / values v_{r,j} of reference r, weights w_r,

    out(q) = sum_r sum_j w_r exp(q.k_rj) v_rj / sum_r sum_j w_r exp(q.k_rj)

evaluated literally as weighted sums of exponentials (shifted by the row maximum of q.k over keys of positive weight),
not as a softmax with a bias, so that the product's "bias = log w" form is checked against something else.  A key bias
b is the weight exp(b); -inf is weight 0.  The UNet is the oracle's (oracle/ldm_torch_cpu.py) with this attention in
place of its own; the samplers are tests/solver_ref.py's recursion and the oracle's DDIM step.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import solver_ref as SR
from oracle import ldm_torch_cpu as TC


def stack(maps):
    """[B,R,C,h,w] -> [B,C,R*h,w]: reference r owns the rows [r*h, (r+1)*h), i.e. the tokens [r*h*w, (r+1)*h*w)."""
    B, R, C, h, w = maps.shape
    return maps.permute(0, 2, 1, 3, 4).reshape(B, C, R * h, w)


def key_weights(weights, B, R, L):
    """Per-key weights [B, R*L] (float64) from [R] or [B,R] reference weights, normalised to sum 1 per sample."""
    w = torch.as_tensor(weights, dtype=torch.float64)
    w = w.view(1, R).expand(B, R) if w.dim() == 1 else w
    w = w / w.sum(-1, keepdim=True)
    return w.repeat_interleave(L, dim=1)


def drop_reference(maps, r):
    """[B,R,...] without reference r."""
    keep = [i for i in range(maps.shape[1]) if i != r]
    return maps[:, keep]


def attention(q, k, v, kw=None):
    """q [B,h,L,d] (already scaled), k, v [B,h,S,d], kw [B,S] key weights >= 0 or None -> [B,h,L,d], float64."""
    s = torch.einsum("bhld,bhsd->bhls", q, k)
    if kw is None:
        kw = torch.ones(q.shape[0], k.shape[2], dtype=q.dtype)
    kw = kw.to(q.dtype)[:, None, None, :]
    live = (kw > 0).expand_as(s)
    m = torch.where(live, s, torch.full_like(s, -math.inf)).amax(-1, keepdim=True)
    e = torch.where(live, kw * torch.exp(torch.where(live, s - m, torch.zeros_like(s))), torch.zeros_like(s))
    return torch.einsum("bhls,bhsd->bhld", e, v) / e.sum(-1, keepdim=True)


def cross_attention(sd, p, x, s, kw=None, heads=4):
    """CrossAttention of the UNet map x [B,C,h,w] over the style tokens of s [B,C,Hs,Ws] (any token count)."""
    B, C, h, w = x.shape
    W = TC._g(sd, p + "multihead_attn.in_proj_weight")
    b = TC._g(sd, p + "multihead_attn.in_proj_bias")
    d = C // heads
    xq = x.reshape(B, C, h * w).transpose(1, 2)                       # [B,L,C]
    xs = s.reshape(B, C, -1).transpose(1, 2)                          # [B,S,C]
    q = (xq @ W[:C].T + b[:C]) * math.sqrt(1.0 / d)
    k = xs @ W[C:2 * C].T + b[C:2 * C]
    v = xs @ W[2 * C:].T + b[2 * C:]
    split = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)  # noqa: E731
    o = attention(split(q), split(k), split(v), kw).permute(0, 2, 1, 3).reshape(B, h * w, C)
    o = o @ TC._g(sd, p + "multihead_attn.out_proj.weight").T + TC._g(sd, p + "multihead_attn.out_proj.bias")
    return o.transpose(1, 2).reshape(B, C, h, w)


def unet(sd, z, t, s5, s6, kw5=None, kw6=None, p="unet."):
    """The UNet with stacked style maps s5 [B,256,R*H/4,W/4], s6 [B,512,R*H/8,W/8] and per-key weights."""
    def cv(name, x, stride=1):
        return F.conv2d(x, TC._g(sd, p + name + ".weight"), TC._g(sd, p + name + ".bias"), stride=stride, padding=1)

    def ct(name, x):
        return F.conv_transpose2d(x, TC._g(sd, p + name + ".weight"), TC._g(sd, p + name + ".bias"), stride=2,
                                  padding=1, output_padding=1)

    temb = TC.time_mlp(sd, p, t)[:, :, None, None]
    z1 = F.relu(cv("enc1", z))
    z2 = F.relu(cv("enc2", z1, 2)) + temb
    z3 = F.relu(cv("enc3", z2, 2))
    z4 = F.relu(cv("enc4", cross_attention(sd, p + "cross_attention2.", z3, s5, kw5), 2))
    zb = F.relu(cv("bottleneck", cross_attention(sd, p + "cross_attention1.", z4, s6, kw6)))
    d4 = F.relu(ct("dec4", zb)) + z3
    d3 = F.relu(ct("dec3", d4)) + z2
    d2 = F.relu(ct("dec2", d3)) + z1
    return cv("dec1", d2)


def sample(sd64, ab, times, x, s5, s6, kw5=None, kw6=None, order=2):
    """The multistep sampler (solver_ref.solve) on this UNet.  Returns (x_final, [x0_i], [eps_i]) as numpy."""
    B = x.shape[0]
    s5, s6 = torch.as_tensor(s5).double(), torch.as_tensor(s6).double()

    def eps_fn(xv, i):
        with torch.no_grad():
            t = torch.full((B,), int(times[i]), dtype=torch.long)
            return unet(sd64, torch.from_numpy(np.ascontiguousarray(xv)), t, s5, s6, kw5, kw6).numpy()

    return SR.solve(ab, times, x, eps_fn, order)


def ddim(sd64, ab, times, x, s5, s6, kw5=None, kw6=None, eta=0.0):
    """The DDIM-style sampler (the oracle's update) on this UNet; ab numpy float64.  Returns x_final as numpy."""
    abt = torch.from_numpy(np.asarray(ab, dtype=np.float64))
    x = torch.as_tensor(x).double()
    s5, s6 = torch.as_tensor(s5).double(), torch.as_tensor(s6).double()
    B = x.shape[0]
    with torch.no_grad():
        for i in range(len(times) - 1):
            t = torch.full((B,), int(times[i]), dtype=torch.long)
            tn = torch.full((B,), int(times[i + 1]), dtype=torch.long)
            x, _ = TC.ddim_step(abt, x, unet(sd64, x, t, s5, s6, kw5, kw6), t, tn, eta)
    return x.numpy()
