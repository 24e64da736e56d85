"""Float64 yardstick for the style map: cross-attention whose reference weights depend on the query position.

Written from the definition: for query l of one head, keys k_s / values v_s and weights W[l, s] >= 0,

    out(q_l) = sum_s W[l, s] exp(q_l.k_s) v_s / sum_s W[l, s] exp(q_l.k_s)

evaluated literally as weighted sums of exponentials (shifted by the row maximum of q.k over keys of positive weight);
weight 0 means the key is removed for that query, and a query whose weights are all 0 gives 0.  The product's form, a
bias log W inside a streaming softmax, is checked against this.  W is the product of a key weight (style mixing) and
the map's weight of the key's reference at the query's position.  The UNet is tests/stylemix_ref.py's with this
attention in place; the samplers are those of tests/solver_ref.py, guidance_ref.py and regional_ref.py.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as GR    # noqa: E402
import regional_ref as RR    # noqa: E402
from oracle import ldm_torch_cpu as TC   # noqa: E402


def pair_weights(B, L, S, key_w=None, ref_w=None):
    """W [B,L,S] float64 = key_w [B,S] (None: 1) times ref_w [B,L,R] (None: 1) of each key's reference s // (S / R)."""
    W = torch.ones(B, L, S, dtype=torch.float64)
    if key_w is not None:
        W = W * torch.as_tensor(key_w, dtype=torch.float64)[:, None, :]
    if ref_w is not None:
        ref_w = torch.as_tensor(ref_w, dtype=torch.float64)
        R = ref_w.shape[2]
        assert S % R == 0 and tuple(ref_w.shape[:2]) == (B, L)
        W = W * ref_w.repeat_interleave(S // R, dim=2)
    return W


def attention(q, k, v, W=None):
    """q [B,h,L,d] (already scaled), k, v [B,h,S,d], W [B,L,S] pair weights >= 0 or None -> [B,h,L,d], float64."""
    s = torch.einsum("bhld,bhsd->bhls", q, k)
    if W is None:
        W = torch.ones(q.shape[0], q.shape[2], k.shape[2], dtype=q.dtype)
    W = W.to(q.dtype)[:, None].expand_as(s)
    live = W > 0
    m = torch.where(live, s, torch.full_like(s, -math.inf)).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))          # a query without any key
    e = torch.where(live, W * torch.exp(torch.where(live, s - m, torch.zeros_like(s))), torch.zeros_like(s))
    den = e.sum(-1, keepdim=True)
    num = torch.einsum("bhls,bhsd->bhld", e, v)
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))


def cross_attention(sd, p, x, s, W=None, heads=4):
    """CrossAttention of the UNet map x [B,C,h,w] over the style tokens of s [B,C,Hs,Ws] with pair weights W."""
    B, C, h, w = x.shape
    Wi = TC._g(sd, p + "multihead_attn.in_proj_weight")
    b = TC._g(sd, p + "multihead_attn.in_proj_bias")
    d = C // heads
    xq = x.reshape(B, C, h * w).transpose(1, 2)
    xs = s.reshape(B, C, -1).transpose(1, 2)
    q = (xq @ Wi[:C].T + b[:C]) * math.sqrt(1.0 / d)
    k = xs @ Wi[C:2 * C].T + b[C:2 * C]
    v = xs @ Wi[2 * C:].T + b[2 * C:]
    split = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)  # noqa: E731
    o = attention(split(q), split(k), split(v), W).permute(0, 2, 1, 3).reshape(B, h * w, C)
    o = o @ TC._g(sd, p + "multihead_attn.out_proj.weight").T + TC._g(sd, p + "multihead_attn.out_proj.bias")
    return o.transpose(1, 2).reshape(B, C, h, w)


def unet(sd, z, t, s5, s6, W5=None, W6=None, p="unet."):
    """The UNet with stacked style maps and pair weights W5 [B,H*W/16,S5] / W6 [B,H*W/64,S6]."""
    def cv(name, x, stride=1):
        return F.conv2d(x, TC._g(sd, p + name + ".weight"), TC._g(sd, p + name + ".bias"), stride=stride, padding=1)

    def ct(name, x):
        return F.conv_transpose2d(x, TC._g(sd, p + name + ".weight"), TC._g(sd, p + name + ".bias"), stride=2,
                                  padding=1, output_padding=1)

    temb = TC.time_mlp(sd, p, t)[:, :, None, None]
    z1 = F.relu(cv("enc1", z))
    z2 = F.relu(cv("enc2", z1, 2)) + temb
    z3 = F.relu(cv("enc3", z2, 2))
    z4 = F.relu(cv("enc4", cross_attention(sd, p + "cross_attention2.", z3, s5, W5), 2))
    zb = F.relu(cv("bottleneck", cross_attention(sd, p + "cross_attention1.", z4, s6, W6)))
    d4 = F.relu(ct("dec4", zb)) + z3
    d3 = F.relu(ct("dec3", d4)) + z2
    d2 = F.relu(ct("dec2", d3)) + z1
    return cv("dec1", d2)


def eps_fn(sd64, times, B, s5, s6, W5=None, W6=None):
    """eps(x, i) of this UNet in float64."""
    s5, s6 = torch.as_tensor(s5).double(), torch.as_tensor(s6).double()

    def fn(xv, i):
        with torch.no_grad():
            t = torch.full((B,), int(times[i]), dtype=torch.long)
            return unet(sd64, torch.from_numpy(np.ascontiguousarray(xv)), t, s5, s6, W5, W6).numpy()

    return fn


def sample(sd64, ab, times, x, s5, s6, W5, W6, solver="dpmpp2m", eta=0.0, base=None, s=None, keep=None):
    """The sampler under a style map.  base = (s5_base, s6_base) with s [B]: guided, the base half without a map.
    keep = (z0, n0, w, coefs): the regional keep.  Returns (x_final, [x0_i], [eps_i]) as numpy."""
    B = x.shape[0]
    ft = eps_fn(sd64, times, B, s5, s6, W5, W6)
    fb = None if base is None else eps_fn(sd64, times, B, base[0], base[1])
    if keep is not None:
        z0, n0, w, coefs = keep
        return RR.solve(ab, times, x, ft, z0, n0, w, coefs, solver, eta, fb, s)
    if fb is not None:
        return GR.solve(ab, times, x, ft, fb, s, solver, eta)
    return GR.plain(ab, times, x, ft, solver, eta)
