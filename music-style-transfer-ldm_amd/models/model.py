"""Drop-in for the reference's models/model.py: same classes, constructor signatures and defaults,
parameter names and shapes (state_dicts interchange), forward semantics and return values — with every
tensor operation of the path executed by libldm_amd.so (hand-written HIP for gfx950).

Deliberate, documented deviations:
  * style_conditioned_ddim_sample / content_style_ddim_sample log timesteps as int(t[0]) instead of
    t.item(), which raises for batch > 1 in the reference (model.py:461, :555).  Numerics unchanged.
  * ForwardDiffusion.forward and LDM.forward accept an optional `noise=` to inject epsilon (parity
    tests); without it epsilon is drawn on the device exactly like torch.randn_like.
  * SpectrogramDecoder.forward(z, rescale=True) fuses the reference's `(decoder(z) + 1) / 2`
    (model.py:371, :405, :498) into the final Tanh epilogue with the same fp32 op order.
  * The sampling loops are inference-only: they build no autograd graph.
No tensor op falls back to the CPU: a CPU tensor on the hot path raises.
"""
import math
import weakref
from typing import Dict, List, Optional, Tuple  # noqa: F401  (API-compat with the reference imports)

import torch
import torch.nn as nn

try:
    from .config import config
except ImportError:
    from config import config

try:
    from . import _pathfix  # noqa: F401
except ImportError:
    import _pathfix  # noqa: F401

try:
    from .loss import VGGishFeatureLoss
except ImportError:
    from loss import VGGishFeatureLoss

from ldm_amd import functional as HF
from ldm_amd import graphs as hgraphs
from ldm_amd import nn as hnn
from ldm_amd import ops
from ldm_amd.engine import LoopOptions, UNetEngine


# ------------------------------------------------------------------------------------------------
# fused helpers
# ------------------------------------------------------------------------------------------------
def _bn_is_eval(bn):
    return not (bn.training or not bn.track_running_stats)


def _conv_bn_act(conv, bn, act, x, transposed=False):
    """conv -> BatchNorm2d -> activation, reference op order.  Eval-mode BN (with frozen affine) is folded
    into the conv epilogue; train-mode BN runs the batch-statistics kernel after the conv."""
    kw = dict(stride=conv.stride[0], padding=conv.padding[0], transposed=transposed,
              output_padding=conv.output_padding[0] if transposed else 0)
    if bn is not None and _bn_is_eval(bn) and not HF._needs_grad(bn.weight, bn.bias):
        return HF.conv(x, conv.weight, conv.bias, act=act,
                       bn_eval=(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps), **kw)
    if bn is None:
        return HF.conv(x, conv.weight, conv.bias, act=act, **kw)
    y = HF.conv(x, conv.weight, conv.bias, act="none", **kw)
    return HF.batchnorm(y, bn, act)


# ------------------------------------------------------------------------------------------------
# VAE
# ------------------------------------------------------------------------------------------------
class SpectrogramEncoder(nn.Module):
    """[B,1,H,W] -> [B,latent_dim,H/8,W/8]: 3 x (conv3x3 s2 + BN) with ReLU after the first two
    (reference model.py:10-28)."""

    def __init__(self, latent_dim=4):
        super(SpectrogramEncoder, self).__init__()
        self.encoder = nn.Sequential(
            hnn.Conv2d(1, 64, kernel_size=3, stride=2, padding=1),
            hnn.BatchNorm2d(64),
            hnn.ReLU(),
            hnn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1),
            hnn.BatchNorm2d(128),
            hnn.ReLU(),
            hnn.Conv2d(128, latent_dim, kernel_size=3, stride=2, padding=1),
            hnn.BatchNorm2d(latent_dim),
        )

    def forward(self, x):
        e = self.encoder
        h = _conv_bn_act(e[0], e[1], "relu", x)
        h = _conv_bn_act(e[3], e[4], "relu", h)
        return _conv_bn_act(e[6], e[7], "none", h)


class SpectrogramDecoder(nn.Module):
    """[B,latent_dim,h,w] -> [B,1,8h,8w]: 3 x convT k4 s2 p1 (+BN+ReLU, last Tanh) (reference
    model.py:31-49).  rescale=True returns (tanh(.)+1)/2 in the same fused epilogue."""

    def __init__(self, latent_dim=4):
        super(SpectrogramDecoder, self).__init__()
        self.decoder = nn.Sequential(
            hnn.ConvTranspose2d(latent_dim, 128, kernel_size=4, stride=2, padding=1),
            hnn.BatchNorm2d(128),
            hnn.ReLU(),
            hnn.ConvTranspose2d(128, 64, kernel_size=4, stride=2, padding=1),
            hnn.BatchNorm2d(64),
            hnn.ReLU(),
            hnn.ConvTranspose2d(64, 1, kernel_size=4, stride=2, padding=1),
            hnn.Tanh(),
        )

    def forward(self, z, rescale=False):
        d = self.decoder
        h = _conv_bn_act(d[0], d[1], "relu", z, transposed=True)
        h = _conv_bn_act(d[3], d[4], "relu", h, transposed=True)
        return _conv_bn_act(d[6], None, "tanh_half" if rescale else "tanh", h, transposed=True)


class StyleEncoder(nn.Module):
    """6 x (conv3x3 s2 + ReLU) -> {'s1'..'s6'} (reference model.py:51-88)."""

    def __init__(self, in_channels=1, num_filters=64):
        super().__init__()
        nf = num_filters
        self.enc1 = hnn.Conv2d(in_channels, nf, kernel_size=3, stride=2, padding=1)
        self.enc2 = hnn.Conv2d(nf, nf * 2, kernel_size=3, stride=2, padding=1)
        self.enc3 = hnn.Conv2d(nf * 2, nf * 4, kernel_size=3, stride=2, padding=1)
        self.enc4 = hnn.Conv2d(nf * 4, nf * 4, kernel_size=3, stride=2, padding=1)
        self.enc5 = hnn.Conv2d(nf * 4, nf * 4, kernel_size=3, stride=2, padding=1)
        self.enc6 = hnn.Conv2d(nf * 4, nf * 8, kernel_size=3, stride=2, padding=1)

    def forward(self, style_spectrogram):
        out = {}
        h = style_spectrogram
        for i in range(1, 7):
            h = getattr(self, f"enc{i}")(h, act="relu")
            out[f"s{i}"] = h
        return out


# ------------------------------------------------------------------------------------------------
# DDPM schedule
# ------------------------------------------------------------------------------------------------
class ForwardDiffusion(nn.Module):
    """beta = linspace(1e-4, 0.02, T); alpha = 1 - beta; alpha_bar = cumprod(alpha) (reference
    model.py:90-124).  The tables are host constants computed with the reference's own torch calls;
    q_sample / predict_start_from_noise run on the device with per-sample gathers of {sqrt(ab),
    sqrt(1-ab)}."""

    def __init__(self, num_timesteps=config["forward_diffusion_num_timesteps"]):
        super().__init__()
        self.num_timesteps = num_timesteps
        beta_start, beta_end = 0.0001, 0.02
        self.register_buffer("beta_t", torch.linspace(beta_start, beta_end, num_timesteps))
        self.register_buffer("alpha_t", 1 - self.beta_t)
        self.register_buffer("alpha_bar_t", torch.cumprod(self.alpha_t, dim=0))

    def _check_t(self, t):
        if not t.is_cuda:
            T = self.alpha_bar_t.shape[0]
            bad = (t >= T) | (t < -T)
            if bool(bad.any()):
                raise IndexError(f"index {int(t[bad][0])} is out of bounds for dimension 0 with size {T}")
            t = torch.where(t < 0, t + T, t)
        return t

    def coef_table(self, device):
        return ops.alpha_bar_coef_table(self.alpha_bar_t, device)

    def forward(self, x_0, t, noise=None):
        device = x_0.device
        t = self._check_t(t).to(device)
        self.alpha_bar_t = self.alpha_bar_t.to(device)   # reference side effect (model.py:106)
        eps = torch.randn_like(x_0, device=device) if noise is None else noise.to(device)
        z_t = HF.q_sample(x_0, eps, self.coef_table(device), t)
        return z_t, eps

    def predict_start_from_noise(self, z_t, t, noise_pred):
        device = z_t.device
        t = self._check_t(t).to(device)
        self.alpha_bar_t = self.alpha_bar_t.to(device)   # reference side effect (model.py:121)
        return HF.predict_start(z_t, noise_pred, self.coef_table(device), t)

    def reverse_coefs(self, times):
        """[n,4] {sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_next), sqrt(1-ab_next)} for consecutive `times`."""
        ab = self.alpha_bar_t.detach().to("cpu", torch.float32)
        T = ab.shape[0]
        if times.numel() and (int(times.max()) >= T or int(times.min()) < -T):
            bad = int(times.max()) if int(times.max()) >= T else int(times.min())
            raise IndexError(f"index {bad} is out of bounds for dimension 0 with size {T}")
        a_t, a_n = ab[times[:-1]], ab[times[1:]]
        return torch.stack([torch.sqrt(a_t), torch.sqrt(1 - a_t), torch.sqrt(a_n), torch.sqrt(1 - a_n)], 1).contiguous()

    def keep_coefs(self, times, exact_last=True):
        """fp32 [n,2] {sqrt(ab_next), sqrt(1-ab_next)} for consecutive `times` (columns 2 and 3 of reverse_coefs): where
        the content's own noising trajectory a z0 + b noise stands after step i, for every solver (the regional keep,
        keep_blend).  exact_last: the last row is (1, 0), so a fully kept pixel ends as z0 itself and not as z0 at
        the last index's noise level."""
        c = self.reverse_coefs(times)[:, 2:4].contiguous()
        if exact_last and c.shape[0]:
            c[-1, 0], c[-1, 1] = 1.0, 0.0
        return c

    def multistep_coefs(self, times, order=2):
        """fp32 [n,8] rows {alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0} of the multistep solver (DPM-Solver++ in its
        data-prediction form) for consecutive `times`, n = len(times) - 1:
            x0 = (x - sigma_t eps) / alpha_t;   x_next = c_x x + c_0 x0 + c_1 x0_prev.
        Computed in float64 from alpha_bar_t: alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = ln(ab / (1 - ab)) / 2,
        h_i = lambda(t_i+1) - lambda(t_i), phi_i = -expm1(-h_i), c_x = sigma_next / sigma_t.  First order:
        c_0 = alpha_next phi_i, c_1 = 0.  Second order (2M), r = h_i-1 / h_i: c_0 = alpha_next phi_i (1 + 1/(2r)),
        c_1 = -alpha_next phi_i / (2r).  Rows 0 and n-1 are always first order (there is no history for the
        first; the last jumps to index 0, where lambda grows too fast for the extrapolation); order=1 makes
        every row first order (DDIM with eta = 0)."""
        if order not in (1, 2):
            raise ValueError(f"multistep_coefs: order must be 1 or 2, got {order}")
        ab = self.alpha_bar_t.detach().to("cpu", torch.float64)
        T = ab.shape[0]
        times = torch.as_tensor(times).long().cpu()
        if times.numel() and (int(times.max()) >= T or int(times.min()) < -T):
            bad = int(times.max()) if int(times.max()) >= T else int(times.min())
            raise IndexError(f"index {bad} is out of bounds for dimension 0 with size {T}")
        n = max(int(times.numel()) - 1, 0)
        out = torch.zeros((n, 8), dtype=torch.float64)
        if n == 0:
            return out.float()
        a = ab[times]
        alpha, sigma = torch.sqrt(a), torch.sqrt(1 - a)
        lam = 0.5 * torch.log(a / (1 - a))
        h = lam[1:] - lam[:-1]
        phi = -torch.expm1(-h)
        out[:, 0], out[:, 1] = alpha[:-1], sigma[:-1]
        out[:, 2] = sigma[1:] / sigma[:-1]
        out[:, 3] = alpha[1:] * phi
        if order == 2 and n > 2:
            r = h[:-1] / h[1:]                      # r_i for rows 1..n-1
            k = 1.0 / (2.0 * r[:-1])                # rows 1..n-2 are second order
            out[1:n - 1, 3] = alpha[2:n] * phi[1:n - 1] * (1.0 + k)
            out[1:n - 1, 4] = -alpha[2:n] * phi[1:n - 1] * k
        return out.float().contiguous()


# ------------------------------------------------------------------------------------------------
# UNet
# ------------------------------------------------------------------------------------------------
class CrossAttention(nn.Module):
    """nn.MultiheadAttention(E, heads) over the H*W tokens of two NCHW maps, no residual (reference
    model.py:126-160).  Runs on the channel-major maps directly: the reference's permute/reshape pairs
    are folded into the projection GEMMs' addressing."""

    def __init__(self, embed_dim, num_heads=4):
        super().__init__()
        self.multihead_attn = hnn.MultiheadAttention(embed_dim, num_heads)
        self.embed_dim = embed_dim

    def forward(self, unet_features, style_embedding):
        B, c, h, w = unet_features.shape
        if style_embedding.shape[0] != B or style_embedding.shape[1] != c or \
                style_embedding.shape[2] * style_embedding.shape[3] != h * w:
            raise RuntimeError(f"CrossAttention: style map {tuple(style_embedding.shape)} cannot be viewed as "
                               f"[{h * w}, {B}, {c}] (reference model.py:150)")
        kv = style_embedding.reshape(B, c, h, w) if tuple(style_embedding.shape[2:]) != (h, w) else style_embedding
        return hnn.attention_nchw(self.multihead_attn, unet_features, kv)


class SinusoidalPositionEmbeddings(nn.Module):
    """[sin(t f_i), cos(t f_i)], f_i = exp(-i ln(1e4)/(dim/2-1)) (reference model.py:234-246)."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, time):
        if not time.is_cuda:
            raise RuntimeError("SinusoidalPositionEmbeddings: time must be a GPU tensor (no CPU fallback)")
        return ops.sinusoid_embed(time, self.dim, time.device)


class _TimeMLP(nn.Sequential):
    """nn.Sequential(Sinusoid, Linear, GELU, Linear) whose inference forward is one fused kernel."""

    def forward(self, t):
        lin1, lin2 = self[1], self[3]
        if HF._needs_grad(lin1.weight, lin1.bias, lin2.weight, lin2.bias):
            emb = ops.sinusoid_embed(t, self[0].dim, lin1.weight.device)
            h = HF.activation(HF.linear(emb, lin1.weight, lin1.bias), "gelu")
            return HF.linear(h, lin2.weight, lin2.bias)
        return ops.time_mlp(t, lin1.weight, lin1.bias, lin2.weight, lin2.bias)


_ENGINES = weakref.WeakKeyDictionary()


def engine_for(unet):
    eng = _ENGINES.get(unet)
    if eng is None:
        eng = UNetEngine(unet)
        _ENGINES[unet] = eng
    return eng


class UNet(nn.Module):
    """Style-conditioned denoiser (reference model.py:163-231): conv encoder, two cross-attentions,
    bottleneck, transposed-conv decoder with additive skips, sinusoid time MLP added after enc2."""

    def __init__(self, in_channels=1, out_channels=1, num_filters=64):
        super(UNet, self).__init__()
        time_emb_dim = 128
        self.num_filters = num_filters
        self.time_mlp = _TimeMLP(
            SinusoidalPositionEmbeddings(time_emb_dim),
            hnn.Linear(time_emb_dim, time_emb_dim),
            hnn.GELU(),
            hnn.Linear(time_emb_dim, time_emb_dim),
        )
        nf = num_filters
        self.enc1 = hnn.Conv2d(in_channels, nf, kernel_size=3, stride=1, padding=1)
        self.enc2 = hnn.Conv2d(nf, nf * 2, kernel_size=3, stride=2, padding=1)
        self.enc3 = hnn.Conv2d(nf * 2, nf * 4, kernel_size=3, stride=2, padding=1)
        self.enc4 = hnn.Conv2d(nf * 4, nf * 8, kernel_size=3, stride=2, padding=1)
        self.cross_attention1 = CrossAttention(embed_dim=512, num_heads=4)
        self.cross_attention2 = CrossAttention(embed_dim=256, num_heads=4)
        self.bottleneck = hnn.Conv2d(nf * 8, nf * 8, kernel_size=3, stride=1, padding=1)
        self.dec4 = hnn.ConvTranspose2d(nf * 8, nf * 4, kernel_size=3, stride=2, padding=1, output_padding=1)
        self.dec3 = hnn.ConvTranspose2d(nf * 4, nf * 2, kernel_size=3, stride=2, padding=1, output_padding=1)
        self.dec2 = hnn.ConvTranspose2d(nf * 2, nf, kernel_size=3, stride=2, padding=1, output_padding=1)
        self.dec1 = hnn.Conv2d(nf, out_channels, kernel_size=3, stride=1, padding=1)

    def _layerwise(self, z, t, s5, s6):
        """Same kernels and plans as the fused engine, one autograd node per layer (training)."""
        temb = self.time_mlp(t)
        z1 = self.enc1(z, act="relu")
        z2 = self.enc2(z1, act="relu", bcast=temb)            # relu(enc2(z1)) + t_emb   (model.py:206)
        z3 = self.enc3(z2, act="relu")
        z3a = self.cross_attention2(z3, s5)
        z4 = self.enc4(z3a, act="relu")
        z4a = self.cross_attention1(z4, s6)
        zb = self.bottleneck(z4a, act="relu")
        d4 = self.dec4(zb, act="relu", skip=z3)                 # relu(dec4(.)) + z3_original  (model.py:220-221)
        d3 = self.dec3(d4, act="relu", skip=z2)
        d2 = self.dec2(d3, act="relu", skip=z1)
        return self.dec1(d2)

    def forward(self, z, t, style_embedding: dict = None):
        s5, s6 = style_embedding["s5"], style_embedding["s6"]
        if style_embedding.get("refs", 1) > 1 or style_embedding.get("key_bias5") is not None or \
                style_embedding.get("key_bias6") is not None:
            raise RuntimeError("UNet.forward: a style embedding of several references (LDM.encode_styles) is attended "
                               "over in the samplers' fused reverse loop only; the single forward, the per-layer path "
                               "and training take one style map per sample")
        if HF._needs_grad(z, s5, s6, *self.parameters()) or not UNetEngine.supports(z.shape[1]):
            return self._layerwise(z, t, s5, s6)
        return engine_for(self).forward(z, t, s5, s6)


# ------------------------------------------------------------------------------------------------
# LDM
# ------------------------------------------------------------------------------------------------
class LDM(nn.Module):
    """VAE + style encoder + DDPM schedule + UNet (reference model.py:249-559)."""

    def __init__(self, latent_dim, pretrained_path: str = "models/pretrained/", pretraind_filename: str = "ldm.pth",
                 num_timesteps=config["forward_diffusion_num_timesteps"], load_full_model=False):
        super(LDM, self).__init__()
        self.encoder = SpectrogramEncoder(latent_dim=latent_dim)
        self.decoder = SpectrogramDecoder(latent_dim=latent_dim)
        self.unet = UNet(in_channels=latent_dim, out_channels=latent_dim, num_filters=64)
        self.noise_scheduler = ForwardDiffusion(num_timesteps=num_timesteps)
        self.style_encoder = StyleEncoder(in_channels=1, num_filters=64)
        self.num_timesteps = num_timesteps
        self.feature_loss_net = VGGishFeatureLoss()

        if pretrained_path:
            if load_full_model:
                try:
                    sd = torch.load(pretrained_path + pretraind_filename, map_location="cpu", weights_only=True)
                    for prefix, mod in (("encoder.", self.encoder), ("decoder.", self.decoder), ("unet.", self.unet),
                                        ("style_encoder.", self.style_encoder),
                                        ("noise_scheduler.", self.noise_scheduler)):
                        mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
                    print(f"Loaded full pretrained LDM components from {pretrained_path + 'ldm.pth'}")
                    self.encoder.eval()
                    self.decoder.train()
                    self.unet.train()
                    self.style_encoder.train()
                    for p in self.encoder.parameters():
                        p.requires_grad = False
                    for p in self.decoder.parameters():
                        p.requires_grad = True
                    return
                except (FileNotFoundError, RuntimeError) as e:
                    print(f"Could not load full LDM model: {e}")
                    print("Falling back to loading just encoder/decoder weights")
            self.encoder.load_state_dict(torch.load(pretrained_path + "encoder.pth", map_location="cpu",
                                                    weights_only=True))
            self.decoder.load_state_dict(torch.load(pretrained_path + "decoder.pth", map_location="cpu",
                                                    weights_only=True))
            print("Loaded pretrained weights from", pretrained_path)
            for p in self.encoder.parameters():
                p.requires_grad = False
            for p in self.decoder.parameters():
                p.requires_grad = True
            self.encoder.eval()
            self.decoder.train()
            self.style_encoder.train()

        # The reference rebuilds these three after loading (model.py:350-353); mirrored so that the
        # parameter-init RNG draws match it.
        self.unet = UNet(in_channels=latent_dim, out_channels=latent_dim, num_filters=64)
        self.noise_scheduler = ForwardDiffusion(num_timesteps=num_timesteps)
        self.style_encoder = StyleEncoder(in_channels=1, num_filters=64)
        self.num_timesteps = num_timesteps

    # -------------------------------------------------------------------------------------------
    def forward(self, x, style, t, noise=None):
        x = x.float()
        style = style.float()
        # the style encoder depends on nothing the VAE encoder / scheduler compute: on a side stream it overlaps
        # them (and, through the autograd engine's stream semantics, its backward overlaps theirs)
        with hgraphs.branch(style.device, "style_encoder") as side:
            style_embedding = self.style_encoder(style)
        z_0 = self.encoder(x)
        z_t, noise = self.noise_scheduler(z_0, t, noise=noise)
        hgraphs.join(side, style.device)
        noise_pred = self.unet(z_t, t, style_embedding)
        z_0_pred = self.noise_scheduler.predict_start_from_noise(z_t, t, noise_pred)
        reconstructed = self.decoder(z_0_pred, rescale=True)       # (decoder(.) + 1) / 2  (model.py:369-371)
        return {
            "z_t": z_t,
            "noise": noise,
            "noise_pred": noise_pred,
            "z_0": z_0,
            "reconstructed": reconstructed,
        }

    # -------------------------------------------------------------------------------------------
    def _reverse(self, z_t, style_embedding, times, eta, order=0, base_embedding=None, guidance_scale=1.0, keep=None,
                 ref_bias=None, seam_cols=0):
        """The shared body of the samplers: len(times)-1 UNet + update steps in one C call.  order 0: the
        reference's DDIM-style update with eta; 1 / 2: the multistep solver of that order (eta unused).

        base_embedding / guidance_scale (a finite float or one per sample, [B]): style guidance.  Each step
        evaluates the denoiser under both embeddings on the same x and t and steps on eps = e_b + s (e_t - e_b)
        (fp32, one rounding per operation); the logs hold the guided x0 / eps.  Without a base and at scale 1 the
        loop below is the unguided one.

        keep = (z0, n0, w, coefs): the regional keep (UNetEngine.ddim_loop).  After each step's update the state is
        blended with coefs[i][0] z0 + coefs[i][1] n0 under the weights w [B,H,W]; the logs stay unblended.

        ref_bias = (ref_bias5, ref_bias6): the style map's biases (style_map_bias; UNetEngine.ddim_loop).

        seam_cols: joint sampling (UNetEngine.ddim_loop): the rows of z_t are neighbouring windows sharing that many
        latent columns, fused before step 0 and after every step.  The engine is called without a split."""
        n = int(times.numel()) - 1
        logs = {"timesteps": [], "pred_x0": [], "noise_pred": []}
        dev = z_t.device
        emb_b = base_embedding
        # the checks, before anything runs: ValueError on a bad scale, base, mask or seam width
        opts = LoopOptions(z_t, max(n, 0), style_embedding["s5"], style_embedding["s6"],
                           key_bias5=style_embedding.get("key_bias5"), key_bias6=style_embedding.get("key_bias6"),
                           base=emb_b and (emb_b["s5"], emb_b["s6"], emb_b.get("key_bias5"), emb_b.get("key_bias6")),
                           guidance_scale=guidance_scale, keep=keep, ref_bias5=ref_bias and ref_bias[0].to(dev),
                           ref_bias6=ref_bias and ref_bias[1].to(dev), seam_cols=seam_cols)
        opts.base_check()
        if n <= 0:
            return z_t, logs
        x = ops.f32c(z_t).clone()
        if order:
            coefs = self.noise_scheduler.multistep_coefs(times, order=order)
        else:
            coefs = self.noise_scheduler.reverse_coefs(times)
        B = x.shape[0]
        t_table = times[:-1].view(n, 1).expand(n, B).contiguous().to(dev)
        x0_logs = torch.empty((n,) + tuple(x.shape), device=dev, dtype=torch.float32)
        eps_logs = torch.empty_like(x0_logs)
        coefs = coefs.to(dev)
        with torch.no_grad():
            if UNetEngine.supports(x.shape[1]):
                eng = engine_for(self.unet)
                if order:
                    eng.msolver_loop(x, opts.s5, opts.s6, t_table, coefs, x0_logs, eps_logs, **opts.public())
                else:
                    eng.ddim_loop(x, opts.s5, opts.s6, t_table, coefs, float(eta), x0_logs, eps_logs, **opts.public())
            else:   # latent widths the fused engine does not take: per-layer UNet + the update kernel
                if opts.is_mix(x):
                    raise RuntimeError(f"style mix: latent width {x.shape[1]} runs the per-layer path, which takes one "
                                       "style map per sample (the fused engine needs a multiple of 8, at least 16)")
                emb = {"s5": opts.s5, "s6": opts.s6}
                emb_b = {"s5": opts.s5_base, "s6": opts.s6_base} if opts.guided else None
                seam = opts.seam_cols if B > 1 else 0
                if seam:     # the stand-alone fuse: before step 0, then after every step
                    ops.seam_fuse_(x, seam)
                for i in range(n):
                    eps = self.unet(x, t_table[i], emb)
                    if opts.guided:      # the second UNet call of the step, then the guidance kernel
                        eps = ops.guide_eps(ops.f32c(eps), ops.f32c(self.unet(x, t_table[i], emb_b)), opts.scale)
                    if order:
                        ops.msolver_step_(x, eps, coefs[i].contiguous(), x0_logs[i], x0_logs[i - 1] if i else None,
                                          eps_logs[i])
                    else:
                        ops.ddim_step_(x, eps, coefs[i].contiguous(), float(eta), x0_logs[i], eps_logs[i])
                    if opts.z0 is not None:    # the stand-alone blend, after the update kernel
                        ops.keep_blend_(x, opts.z0, opts.n0, opts.keep_w, opts.keep_coef[i])
                    if seam:
                        ops.seam_fuse_(x, seam)
        logs["timesteps"] = [int(v) for v in times[:-1]]
        logs["pred_x0"] = list(x0_logs.unbind(0))
        logs["noise_pred"] = list(eps_logs.unbind(0))
        return x, logs

    @staticmethod
    def tile_embedding(emb, R):
        """A single-style embedding as R stacked copies of itself along the maps' height, without key biases: the base
        of a guided sampler whose target is a mix of R references (R equally weighted copies of one style attend
        like that style)."""
        R = int(R)
        if R < 1:
            raise ValueError(f"tile_embedding: R must be at least 1, got {R}")
        if emb.get("key_bias5") is not None or emb.get("key_bias6") is not None or int(emb.get("refs", 1)) != 1:
            raise ValueError("tile_embedding: a single-style embedding is expected (no references, no key bias)")
        out = {"refs": R, "key_bias5": None, "key_bias6": None}
        for k in ("s5", "s6"):
            out[k] = emb[k].repeat(1, 1, R, 1).contiguous() if R > 1 else emb[k]
        return out

    MAX_STYLE_REFS = 8

    @staticmethod
    def style_map_bias(style_map, H, W):
        """A style map (which style where) as the reverse loop's reference biases for a latent of H x W.

        style_map [B,R,n_mels,F] at spectrogram resolution (n_mels = 8 H, F = 8 W) or [B,R,H,W] at latent resolution:
        the non-negative weight of each of R references at every position, with a positive sum over R everywhere
        (ValueError otherwise, and for NaN / inf).  In float64 on the host: normalised per position to sum 1, averaged
        over the cells of the two cross-attentions' token grids (CA2: H/4 x W/4, cells of 4 x 4 latent or 32 x 32
        spectrogram positions; CA1: H/8 x W/8), then the log (0 becomes -inf: the reference is removed there).  The
        average is taken by halving one axis at a time, (a + b) / 2, so a map that is constant over a cell keeps its
        value exactly.  Returns (ref_bias5 [B,H*W/16,R], ref_bias6 [B,H*W/64,R]), fp32 on style_map's device, tokens
        row-major as the UNet flattens its maps."""
        H, W = int(H), int(W)
        if H < 8 or W < 8 or H % 8 or W % 8:
            raise ValueError(f"style_map_bias: the latent must be H x W with multiples of 8, got {H} x {W}")
        if not isinstance(style_map, torch.Tensor) or style_map.dim() != 4 or style_map.shape[1] < 1 or \
                tuple(style_map.shape[2:]) not in ((H, W), (8 * H, 8 * W)):
            got = tuple(style_map.shape) if isinstance(style_map, torch.Tensor) else type(style_map).__name__
            raise ValueError(f"style_map_bias: style_map must be [B,R,{8 * H},{8 * W}] (spectrogram) or [B,R,{H},{W}] "
                             f"(latent), got {got}")
        m = style_map.detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(m).all()) or bool((m < 0).any()):
            raise ValueError("style_map_bias: style_map must be finite and non-negative")
        tot = m.sum(1, keepdim=True)
        if bool((tot <= 0).any()):
            raise ValueError("style_map_bias: every position needs at least one reference of positive weight")
        m = m / tot

        def halve(t):     # 2 x 2 cells -> their mean, one axis at a time
            t = (t[:, :, 0::2] + t[:, :, 1::2]) * 0.5
            return (t[:, :, :, 0::2] + t[:, :, :, 1::2]) * 0.5

        while m.shape[2] > H // 4:
            m = halve(m)
        out = []
        for g in (m, halve(m)):
            B, R, h, w = g.shape
            out.append(torch.log(g).to(torch.float32).permute(0, 2, 3, 1).reshape(B, h * w, R).contiguous()
                       .to(style_map.device))
        return out[0], out[1]

    def _map_biases(self, style_map, style_embedding, z_t):
        """style_map_bias of a sampler call, after the checks against its embedding and latent."""
        R = int(style_embedding.get("refs", 1)) if isinstance(style_embedding, dict) else 1
        B, _, H, W = z_t.shape
        if not isinstance(style_map, torch.Tensor) or style_map.dim() != 4 or style_map.shape[0] != B or \
                style_map.shape[1] != R:
            got = tuple(style_map.shape) if isinstance(style_map, torch.Tensor) else type(style_map).__name__
            raise ValueError(f"style_map: need one map per sample and reference of the embedding, [{B},{R},...], got {got}")
        rb5, rb6 = self.style_map_bias(style_map, H, W)
        return rb5.to(z_t.device), rb6.to(z_t.device)

    @staticmethod
    def normalise_style_weights(weights, R, B=None):
        """Host-side checks of style weights: a float64 CPU tensor [R] or [B,R], each row non-negative with a
        positive sum, scaled to sum 1.  ValueError otherwise."""
        w = torch.as_tensor(weights, dtype=torch.float64).detach().cpu()
        if w.dim() not in (1, 2) or w.shape[-1] != R or (w.dim() == 2 and B is not None and w.shape[0] != B):
            raise ValueError(f"style weights must be [{R}] or [B,{R}] for {R} references, got {tuple(w.shape)}")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("style weights must be finite and non-negative")
        tot = w.sum(-1, keepdim=True)
        if bool((tot <= 0).any()):
            raise ValueError("style weights: every sample needs at least one positive weight")
        return w / tot

    def encode_styles(self, style_specs, weights=None):
        """Style embedding of R weighted references per sample: style_specs [B,R,1,n_mels,F], weights [R] or [B,R]
        (default equal; normalised to sum 1).  The style encoder runs once on the B*R maps; the result's s5 / s6
        hold the references stacked along the map's height (reference r owns the keys [r*L, (r+1)*L)) and
        key_bias5 / key_bias6 [B,R*L] the log of each key's reference weight (None for equal weights), which the
        samplers add to the cross-attentions' scores: softmax over all references' keys, reference r scaled by w_r.
        A zero column of an [R] weight vector is dropped before anything runs; a zero in [B,R] weights becomes a
        -inf bias (that sample ignores the reference).  R = 1 is the plain embedding."""
        if style_specs.dim() != 5:
            raise ValueError(f"encode_styles: style_specs must be [B,R,1,n_mels,F], got {tuple(style_specs.shape)}")
        B, R = style_specs.shape[:2]
        if not 1 <= R <= self.MAX_STYLE_REFS:
            raise ValueError(f"encode_styles: 1 to {self.MAX_STYLE_REFS} style references, got {R}")
        w = None
        if weights is not None:
            w = self.normalise_style_weights(weights, R, B)
            if w.dim() == 1:
                keep = torch.nonzero(w > 0).flatten()
                if keep.numel() < R:
                    style_specs = style_specs[:, keep.to(style_specs.device)]
                    w, R = w[keep], int(keep.numel())
        specs = style_specs.float().reshape((B * R,) + tuple(style_specs.shape[2:]))
        emb = self.style_encoder(specs)
        out = {"refs": R, "key_bias5": None, "key_bias6": None}
        for k in ("s5", "s6"):
            m = emb[k]
            if R == 1:
                out[k] = m
                continue
            c, h, wd = m.shape[1:]
            out[k] = m.reshape(B, R, c, h, wd).permute(0, 2, 1, 3, 4).reshape(B, c, R * h, wd).contiguous()
        if w is not None and R > 1:
            logw = torch.log(w if w.dim() == 2 else w.view(1, R).expand(B, R)).float()   # log 0 = -inf
            for k, name in (("s5", "key_bias5"), ("s6", "key_bias6")):
                L = out[k].shape[2] * out[k].shape[3] // R
                out[name] = logw.repeat_interleave(L, dim=1).contiguous().to(out[k].device)
        return out

    def _style_embedding(self, style_spec, style_weights=None):
        """The style embedding of a 4-D map (today's) or of 5-D stacked references with optional weights."""
        if style_spec.dim() == 5:
            return self.encode_styles(style_spec, style_weights)
        if style_weights is not None:
            raise ValueError("style_weights needs a 5-D style_spec [B,R,1,n_mels,F]")
        return self.style_encoder(style_spec)

    def style_ddim_sample_wrapper(self, z_shape, style_spec, timesteps=100, eta=0.0):
        z_t = torch.randn(z_shape).to(style_spec.device)            # CPU generator (model.py:394)
        style_embedding = self.style_encoder(style_spec)
        sampled, _ = self.style_conditioned_ddim_sample(z_t, style_embedding, timesteps, eta)
        return self.decoder(sampled, rescale=True)

    def style_conditioned_ddim_sample(self, z_t, style_embedding, timesteps=100, eta=0.0):
        times = torch.linspace(self.num_timesteps - 1, 0, timesteps).long()    # (model.py:420)
        return self._reverse(z_t, style_embedding, times, eta)

    def content_style_transfer_wrapper(self, content_spec, style_spec, num_timesteps=250, eta=0.0, noise=None,
                                       style_weights=None):
        """Encode content, q_sample it at T'-1, run the T'-step content/style loop, decode (reference
        model.py:468-501).  `noise` (optional, [B, latent, H/8, W/8]) injects the q_sample epsilon that
        the reference draws with randn_like (parity tests); by default it is drawn on the device."""
        content_spec = content_spec.float()
        style_spec = style_spec.float()
        z_0 = self.encoder(content_spec)
        t = torch.full((content_spec.shape[0],), num_timesteps - 1, dtype=torch.long)
        self.noise_scheduler._check_t(t)                                        # IndexError like model.py:107
        z_t, noise = self.noise_scheduler(z_0, t.to(content_spec.device), noise=noise)
        style_embedding = self._style_embedding(style_spec, style_weights)   # 5-D: several references (encode_styles)
        sampled, _ = self.content_style_ddim_sample(z_t, style_embedding, num_timesteps, eta)
        decoded = self.decoder(sampled, rescale=True)
        z_t_decoded = self.decoder(z_t)
        return decoded, z_t_decoded

    def content_style_ddim_sample(self, z_t, style_embedding, timesteps=250, eta=0.0):
        times = torch.linspace(timesteps - 1, 0, timesteps).long()              # (model.py:514)
        return self._reverse(z_t, style_embedding, times, eta)

    # -------------------------------------------------------------------------------------------
    # Samplers with a separate noise level (t_start) and step count, and a choice of solver.  The reference has
    # no counterpart; its methods above are untouched.
    _SOLVERS = {"ddim": 0, "dpmpp1": 1, "dpmpp2m": 2}

    def sample_times(self, t_start, steps):
        """The steps + 1 schedule indices linspace(t_start, 0) of a `steps`-step sampler from t_start."""
        t_start, steps = int(t_start), int(steps)
        if not 1 <= steps <= t_start <= self.num_timesteps - 1:
            raise ValueError(f"sample_times: need 1 <= steps <= t_start <= {self.num_timesteps - 1}, got steps "
                             f"{steps}, t_start {t_start} (with more steps than indices two times coincide)")
        return torch.linspace(t_start, 0, steps + 1).long()

    def _solve(self, z_t, style_embedding, times, solver, eta, base_embedding=None, guidance_scale=1.0, keep=None,
               style_map=None, seam_cols=0):
        if solver not in self._SOLVERS:
            raise ValueError(f"unknown solver {solver!r}: one of {sorted(self._SOLVERS)}")
        rb = None if style_map is None else self._map_biases(style_map, style_embedding, z_t)
        return self._reverse(z_t, style_embedding, times, eta, self._SOLVERS[solver], base_embedding, guidance_scale,
                             keep=keep, ref_bias=rb, seam_cols=seam_cols)

    @classmethod
    def _seam_cols(cls, seam_overlap, frames, solver):
        """A joint call's seam width in latent columns from the overlap in mel frames, after the checks."""
        ov = int(seam_overlap)
        if ov != seam_overlap or ov < 0:
            raise ValueError(f"seam_overlap must be a non-negative whole number of mel frames, got {seam_overlap!r}")
        if ov == 0:
            return 0
        if solver not in cls._SOLVERS:
            raise ValueError(f"seam_overlap needs a solver, one of {sorted(cls._SOLVERS)} (got {solver!r})")
        if ov % 8:
            raise ValueError(f"seam_overlap must be a multiple of 8 mel frames (one latent column), got {ov}")
        if ov > int(frames) // 2:
            raise ValueError(f"seam_overlap must be at most frames / 2 = {int(frames) // 2}, got {ov}")
        return ov // 8

    @staticmethod
    def latent_keep(mask):
        """A keep mask at spectrogram resolution [B,1,n_mels,F] reduced to latent resolution [B,H,W] = [B,n_mels/8,F/8]
        by the mean over each 8 x 8 cell (the VAE's downsampling factor)."""
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] % 8 or mask.shape[3] % 8:
            raise ValueError(f"latent_keep: the mask must be [B,1,n_mels,F] with n_mels and F multiples of 8, got "
                             f"{tuple(mask.shape)}")
        B, _, M, F = mask.shape
        return mask.float().reshape(B, M // 8, 8, F // 8, 8).mean(dim=(2, 4))

    def _keep_tuple(self, keep, z0, noise, times, exact_last):
        if z0 is None or noise is None:
            raise ValueError("keep needs z0 and noise: the clean latent and the q_sample noise that produced z_t")
        return (z0, noise, keep, self.noise_scheduler.keep_coefs(times, exact_last))

    def style_conditioned_sample(self, z_t, style_embedding, steps=20, solver="dpmpp2m", t_start=None, eta=0.0,
                                 guidance_scale=1.0, base_embedding=None, keep=None, z0=None, noise=None, exact_last=True,
                                 style_map=None, seam_cols=0):
        """z_t at index t_start (default num_timesteps - 1) denoised in `steps` UNet passes over
        sample_times(t_start, steps).  solver: "dpmpp2m" (DPM-Solver++(2M), first-order first and last step),
        "dpmpp1" (its first-order form) or "ddim" (the reference's update, with eta, on this time grid).
        Returns (x, logs) like style_conditioned_ddim_sample.

        base_embedding (a style embedding with the target's key counts) and guidance_scale (a finite float or [B]):
        every step steers the noise prediction from the base style towards the target, e_b + s (e_t - e_b): s = 1
        samples the target, s > 1 exaggerates it, 0 < s < 1 applies it partly.  A scale other than 1 without a
        base raises ValueError; scale 1 without a base is the unguided sampler.

        keep [B,H,W] in [0,1] with z0 and noise (z_t = q_sample(z0, t_start, noise)): the regional keep.  Where keep is
        1 the state is held on the content's own noising trajectory and ends as z0 (exact_last) or as z0 at index
        0's noise level; where it is 0 the sampler runs free; values between blend the two after every step.

        style_map [B,R,n_mels,F] or [B,R,H,W] (style_map_bias) with an embedding of R references (encode_styles): which
        style where.  Reference r's weight at a query position is its map value there (normalised over R, averaged
        over the attention's token cell), on top of the embedding's own weights; under guidance it applies to the
        target only.  The fused engine only (RuntimeError on the per-layer path, as for a mix).

        seam_cols (latent columns, 0 = off, at most W / 2): joint sampling of overlapping windows.  The rows of z_t are
        neighbouring windows of one recording, row b + 1 starting seam_cols columns before row b ends; the columns two
        rows share are replaced in both by one weighted average before step 0 and after every step
        (UNetEngine.ddim_loop), so the returned x agrees bitwise across every seam.  The logs stay each window's own."""
        t_start = self.num_timesteps - 1 if t_start is None else t_start
        times = self.sample_times(t_start, steps)
        kp = None if keep is None else self._keep_tuple(keep, z0, noise, times, exact_last)
        return self._solve(z_t, style_embedding, times, solver, eta, base_embedding, guidance_scale, keep=kp,
                           style_map=style_map, seam_cols=seam_cols)

    def content_style_transfer(self, content_spec, style_spec, t_start=99, steps=10, solver="dpmpp2m", noise=None,
                               eta=0.0, style_weights=None, guidance_scale=1.0, base_style=None, keep=None,
                               composite=True, style_map=None, seam_overlap=0):
        """Encode content, q_sample it at index t_start (the strength), denoise over sample_times(t_start, steps)
        with `solver`, decode.  Returns (decoded, z_t_decoded) like content_style_transfer_wrapper.

        No equivalence with content_style_transfer_wrapper is promised, solver="ddim" included: the wrapper ties
        noise level and step count together (its time grid is linspace(T' - 1, 0, T')), here they are separate
        arguments and `steps` counts UNet passes, so the grids differ by design.

        style_spec [B,R,1,n_mels,F] with style_weights ([R] or [B,R], default equal) attends over R weighted
        style references (encode_styles).

        guidance_scale / base_style: style guidance (style_conditioned_sample).  base_style is a spectrogram
        [B,1,n_mels,F] passed through the style encoder; None with a scale other than 1 takes the content
        spectrogram itself ("away from how it sounds now, towards the target").  Against a mix of R references the
        base is tiled R times (tile_embedding).

        keep: a mask in [0,1] of what to leave as it is, [B,1,n_mels,F] at spectrogram resolution (reduced by
        latent_keep) or [B,H,W] at latent resolution: the regional keep with this call's own z_0 and noise.  composite
        (spectrogram-resolution masks): the decoded window becomes (1 - M) decoded + M content_spec, since the VAE is
        lossy and a kept region should come back as it went in.

        style_map [B,R,n_mels,F] (or [B,R,H,W] at latent resolution) with a 5-D style_spec of R references: which
        style where (style_conditioned_sample).  It composes with style_weights (the weights multiply); a reference
        that a zero of an [R] weight vector drops is dropped from the map too.

        seam_overlap (mel frames, 0 = off): joint sampling.  The rows of content_spec are neighbouring windows of one
        recording that share seam_overlap frames (longform.window_plan's overlap); the sampler fuses the seam_overlap / 8
        latent columns they share after every step (style_conditioned_sample's seam_cols).  A multiple of 8, at most
        frames / 2, and it needs a solver (ValueError otherwise).  For the windows to describe one canvas from the
        start, pass `noise` from longform.noise_windows."""
        seam_cols = self._seam_cols(seam_overlap, content_spec.shape[3], solver)
        if style_weights is not None and style_spec.dim() != 5:
            raise ValueError("style_weights needs a 5-D style_spec [B,R,1,n_mels,F]")
        if style_map is not None:      # the checks, before anything runs
            if style_spec.dim() != 5:
                raise ValueError("style_map needs a 5-D style_spec [B,R,1,n_mels,F]")
            B, R = style_spec.shape[:2]
            if not isinstance(style_map, torch.Tensor) or style_map.dim() != 4 or tuple(style_map.shape[:2]) != (B, R):
                got = tuple(style_map.shape) if isinstance(style_map, torch.Tensor) else type(style_map).__name__
                raise ValueError(f"style_map: need one map per sample and reference, [{B},{R},...], got {got}")
            if style_weights is not None:
                w = self.normalise_style_weights(style_weights, R, B)
                if w.dim() == 1 and bool((w <= 0).any()):    # encode_styles drops these references: so does the map
                    style_map = style_map[:, torch.nonzero(w > 0).flatten().to(style_map.device)]
            self.style_map_bias(style_map, content_spec.shape[2] // 8, content_spec.shape[3] // 8)   # ValueError early
        content_spec = content_spec.float()
        style_spec = style_spec.float()
        times = self.sample_times(t_start, steps)
        mask = None
        if keep is not None:      # the checks, before anything runs
            B = content_spec.shape[0]
            if keep.dim() == 4:
                if tuple(keep.shape) != (B, 1) + tuple(content_spec.shape[2:]):
                    raise ValueError(f"keep: a spectrogram-resolution mask must be [B,1,n_mels,F] like the content "
                                     f"{tuple(content_spec.shape)}, got {tuple(keep.shape)}")
            elif tuple(keep.shape) != (B, content_spec.shape[2] // 8, content_spec.shape[3] // 8):
                raise ValueError(f"keep: a latent-resolution mask must be [B,H,W] = [B,n_mels/8,F/8] for the content "
                                 f"{tuple(content_spec.shape)}, got {tuple(keep.shape)}")
            keep = keep.detach().to(content_spec.device, torch.float32)
            if not bool(torch.isfinite(keep).all()):
                raise ValueError("keep: the mask must be finite (NaN / inf given)")
            if not (bool((keep >= 0).all()) and bool((keep <= 1).all())):
                raise ValueError("keep: mask values must lie in [0, 1]")
            if keep.dim() == 4:
                mask, keep = keep, self.latent_keep(keep)
        z_0 = self.encoder(content_spec)
        t = torch.full((content_spec.shape[0],), int(t_start), dtype=torch.long)
        z_t, noise = self.noise_scheduler(z_0, t.to(content_spec.device), noise=noise)
        kp = None
        if keep is not None:
            kp = UNetEngine.keep_operands(self._keep_tuple(keep, z_0, noise, times, True), z_t.shape, len(times) - 1,
                                          z_t.device)
        style_embedding = self._style_embedding(style_spec, style_weights)
        if UNetEngine.is_unguided(base_style, guidance_scale):
            sampled, _ = self._solve(z_t, style_embedding, times, solver, eta, keep=kp, style_map=style_map,
                                     seam_cols=seam_cols)
        else:
            UNetEngine.guidance_scale(guidance_scale, content_spec.shape[0])   # (validated before anything runs)
            base_spec = content_spec if base_style is None else base_style.float()
            base_embedding = self.style_encoder(base_spec)
            R = int(style_embedding.get("refs", 1)) if isinstance(style_embedding, dict) else 1
            if R > 1:
                base_embedding = self.tile_embedding(base_embedding, R)
            sampled, _ = self._solve(z_t, style_embedding, times, solver, eta, base_embedding, guidance_scale, keep=kp,
                                     style_map=style_map, seam_cols=seam_cols)
        decoded = self.decoder(sampled, rescale=True)
        if mask is not None and composite:
            decoded = (1 - mask) * decoded + mask * content_spec
        z_t_decoded = self.decoder(z_t)
        return decoded, z_t_decoded
