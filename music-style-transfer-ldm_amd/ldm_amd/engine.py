"""UNet engine: binds a UNet module's parameters to the C ABI's ldm_unet_weights and runs the whole
denoiser (ldm_unet_forward) or the whole reverse loop (ldm_sample) in one C call each; the
reverse loop is replayed from a captured hipGraph (torch.cuda.CUDAGraph on the same stream).

Host side only: it owns workspaces (torch allocations) and caches, never computes.
"""
import ctypes
import os
import weakref

import torch

from . import _lib as L
from . import ops
from .graphs import capture

byref = ctypes.byref

def prepared_key(operands, weight_version, extra=()):
    """The host-side key of a prepared reverse-loop workspace (ldm_sample_prepare): (data_ptr, _version, shape) of
    every tensor the prepare phase reads (None for an absent one), the engine's weight version, and whatever else
    the prepared state depends on.  Equal keys mean the same storage with no in-place write through torch since;
    writes through raw pointers do not move a version, so they need an explicit invalidation (GraphedDDIM.invalidate).
    The key says nothing about a tensor that has been freed (another may live at its address with the same version):
    it is only compared for tensors that its holder keeps alive (GraphedDDIM's static buffers)."""
    ops_key = tuple(None if t is None else (t.data_ptr(), t._version, tuple(t.shape)) for t in operands)
    return ops_key + (weight_version,) + tuple(extra)


_CONV_NAMES = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec4", "dec3", "dec2", "dec1")


class UNetEngine:
    """Runs `unet` (a models.model.UNet: reference parameter names / shapes) through libldm_amd."""

    def __init__(self, unet, fold=None, step=None, dtype=None):
        self.unet = unet
        # Operand precision of the step kernels (ldm_capi.h LDM_DT_*): None follows the caller's
        # torch.autocast("cuda") region (fp16 / bf16 operands, fp32 accumulation and sampler state) or
        # LDM_AMD_STEP_DTYPE; "fp32" / "fp16" / "bf16" pins it.
        self.dtype = dtype
        # Re-associated cross-attentions in the reverse loop (ldm_capi.h use_fold); LDM_AMD_FOLD=0 turns
        # it off (A/B timing, parity of the literal form).
        self.fold = (os.environ.get("LDM_AMD_FOLD", "1") != "0") if fold is None else bool(fold)
        # Step kernels for the folded reverse loop (ldm_capi.h use_step): 1 or 2 (default, or True) the
        # register-direct kernels (uconv.hip; 2 selected the LDS-staged kernels of rounds 2-5, removed in round 6);
        # 0 conv.hip's general kernel (LDM_AMD_STEP, A/B timing).  Built for the LDM's latent 32 / 64 filters.
        if step is None:
            step = int(os.environ.get("LDM_AMD_STEP", "2"))
        self.step = 2 if step is True else (0 if step is False else int(step))
        if self.step not in (0, 1, 2):
            raise ValueError(f"step must be 0, 1 or 2, got {step!r}")
        self._bound = {}      # shape key -> (key of param versions, UNetWeights, keepalive)
        self._ws = {}         # (shape key, device) -> workspace tensor
        self._graphs = {}

    _DT = {"fp32": 0, "f32": 0, "float32": 0, "fp16": 1, "f16": 1, "float16": 1, "bf16": 2, "bfloat16": 2}

    def step_dtype(self):
        """LDM_DT_* the reverse loop's step kernels run at (see __init__)."""
        if self.dtype is not None:
            return self._DT[str(self.dtype).replace("torch.", "")]
        env = os.environ.get("LDM_AMD_STEP_DTYPE")
        if env:
            return self._DT[env]
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            return 1 if dt == torch.float16 else (2 if dt == torch.bfloat16 else 0)
        return 0

    # -------------------------------------------------------------------------------------------
    def shape(self, B, C, H, W):
        return L.UNetShape(B, C, H, W, self.unet.num_filters)

    def _params(self):
        u = self.unet
        ps = []
        for n in _CONV_NAMES:
            m = getattr(u, n)
            ps += [m.weight, m.bias]
        for ca in (u.cross_attention2, u.cross_attention1):
            a = ca.multihead_attn
            ps += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias]
        tm = u.time_mlp
        ps += [tm[1].weight, tm[1].bias, tm[3].weight, tm[3].bias]
        return ps

    @staticmethod
    def supports(channels):
        """The fused engine keeps the UNet's activations NHWC, which its MFMA conv instances need 8-aligned
        channel counts for (enc1's input, dec1's output); other latent widths (UNet(1, 1) on a raw mel, the
        VAE's default latent_dim=4) run the per-layer path (UNet._layerwise, NCHW kernels)."""
        return channels % 8 == 0 and channels >= 16

    @staticmethod
    def fold_applies(shape):
        """The folded cross-attentions re-associate the scores' contraction from d to E per head: that pays
        while the key count S stays below ~E/3 (the saved Q projection is L*E*E, the extra score work
        (heads-1)*L*S*E), and its LDS-resident instances cover S <= 64 (CA2) / 32 (CA1).  Wider latents (mels
        beyond 512 frames) run the literal loop with the KV-tiled attention (flash.hip)."""
        return shape.H * shape.W <= 1024

    def weight_version(self):
        """What the bound weights depend on besides the shape: every parameter's (_version, data_ptr), the forced
        plans and the engine's fold / step / dtype settings.  Host only."""
        params = self._params()
        return tuple(p._version for p in params) + tuple(p.data_ptr() for p in params) + \
            tuple(sorted(ops._PLAN_OVERRIDE.items())) + (self.fold, self.step, self.step_dtype() if self.step else 0)

    def weights(self, shape):
        """UNetWeights for this shape, re-packing only the parameters whose _version moved."""
        skey = (shape.B, shape.C, shape.H, shape.W, shape.nf)
        params = self._params()
        for p in params:
            ops.require_device(p, what="UNet parameter")
            if not p.is_contiguous():
                raise RuntimeError("UNet parameters must be contiguous")
        vkey = self.weight_version()
        hit = self._bound.get(skey)
        if hit is not None and hit[0] == vkey:
            return hit[1]
        w = L.UNetWeights()
        L.call("ldm_unet_make_plans", byref(shape), byref(w))
        keep = []
        u = self.unet

        def desc(layer):
            d = L.ConvDesc()
            L.call("ldm_unet_layer_desc", byref(shape), layer, byref(d))
            return d

        def bind(layer, weight4d, owner, tag, plan_slot):
            d = desc(layer)
            forced = ops._PLAN_OVERRIDE.get(d.key())
            if forced is not None:
                plan = ops.get_plan(d)
                plan_slot[0] = plan
            else:
                plan = plan_slot[0]
            buf = ops.packed_weight(weight4d, d, plan, owner=owner, tag=tag)
            keep.append(buf)
            return buf.data_ptr()

        for i, n in enumerate(_CONV_NAMES):
            m = getattr(u, n)
            slot = [w.conv_plan[i]]
            w.conv_w[i] = bind(i, m.weight, m.weight, None, slot)
            w.conv_plan[i] = slot[0]
            w.conv_b[i] = m.bias.data_ptr()
        for j, ca in enumerate((u.cross_attention2, u.cross_attention1)):
            a = ca.multihead_attn
            E = a.embed_dim
            ipw, ipb = a.in_proj_weight, a.in_proj_bias
            base = 9 + 3 * j
            slot = [w.ca_plan_q[j]]
            w.ca_wq[j] = bind(base, ipw[:E].view(E, E, 1, 1), ipw, "q", slot)
            w.ca_plan_q[j] = slot[0]
            slot = [w.ca_plan_kv[j]]
            w.ca_wkv[j] = bind(base + 1, ipw[E:].view(2 * E, E, 1, 1), ipw, "kv", slot)
            w.ca_plan_kv[j] = slot[0]
            slot = [w.ca_plan_o[j]]
            w.ca_wo[j] = bind(base + 2, a.out_proj.weight.view(E, E, 1, 1), a.out_proj.weight, "o", slot)
            w.ca_plan_o[j] = slot[0]
            w.ca_bq[j] = ipb.data_ptr()
            w.ca_bkv[j] = ipb.data_ptr() + E * 4
            w.ca_bo[j] = a.out_proj.bias.data_ptr()
        folded = {}
        if self.fold and self.fold_applies(shape):
            # enc4 o out_proj(CA2) and bottleneck o out_proj(CA1), packed with those layers' plans
            for j, (layer, conv, ca) in enumerate(((3, u.enc4, u.cross_attention2), (4, u.bottleneck, u.cross_attention1))):
                a = ca.multihead_attn
                d = desc(layer)
                wf = torch.empty_like(conv.weight)
                pb = torch.empty((d.Cout, d.Hout, d.Wout), device=conv.weight.device, dtype=torch.float32)
                L.call("ldm_fold_conv_proj", byref(d), conv.weight.data_ptr(), conv.bias.data_ptr(),
                       a.out_proj.weight.data_ptr(), a.out_proj.bias.data_ptr(), a.embed_dim, wf.data_ptr(),
                       pb.data_ptr(), ops.stream_handle())
                buf = ops.packed_weight(wf, d, w.conv_plan[layer])
                keep += [wf, pb, buf]
                w.fold_w[j] = buf.data_ptr()
                w.fold_pb[j] = pb.data_ptr()
                w.ca_wq_raw[j] = a.in_proj_weight.data_ptr()
                folded[layer] = (wf, pb)
            w.use_fold = 1
            if self.step and shape.C == 32 and shape.nf == 64:
                lib = L.load()
                sdt = self.step_dtype()
                for i, n in enumerate(_CONV_NAMES):
                    src = folded[i][0] if i in folded else getattr(u, n).weight.detach()
                    src = ops.f32c(src)
                    # 16-bit operands read a 16-bit pack (half the floats of storage)
                    nfl = int(lib.ldm_step_packed_floats(i)) // (2 if sdt else 1)
                    buf = torch.empty(nfl, device=src.device, dtype=torch.float32)
                    L.call("ldm_step_pack_weight_dt", i, sdt, src.data_ptr(), buf.data_ptr(), ops.stream_handle())
                    keep += [src, buf]
                    w.step_w[i] = buf.data_ptr()
                for j, layer in enumerate((3, 4)):
                    pbt = folded[layer][1].permute(1, 2, 0).contiguous()     # [Hout, Wout, Cout]
                    keep.append(pbt)
                    w.step_pb[j] = pbt.data_ptr()
                w.use_step = self.step
                w.step_dtype = sdt
                # the bottleneck's fold unpacked: U (CA1's values folded into it) is formed from it once per loop
                w.step_bneck_w = folded[4][0].data_ptr()
        tm = u.time_mlp
        freqs = ops.sinusoid_freqs(tm[1].weight.shape[0], tm[1].weight.device)
        keep.append(freqs)
        w.t_freqs = freqs.data_ptr()
        w.t_w1, w.t_b1 = tm[1].weight.data_ptr(), tm[1].bias.data_ptr()
        w.t_w2, w.t_b2 = tm[3].weight.data_ptr(), tm[3].bias.data_ptr()
        w._keep = keep
        self._bound[skey] = (vkey, w)
        return w

    def workspace(self, shape, device, nsteps=0, slot=0, keys=None, guided=False, plan_batch=None, keep=False):
        """Workspace for this shape and its bound plans; `slot` separates concurrently running sub-batch
        chains.  Zero-filled on allocation: it carries the split-K tile counters (ldm_capi.h).
        keys = (S5, S6): the style-mixing loops' key counts (None or 0 = the maps' own).
        guided: the guided loops' workspace for the caller's `shape` (sized for the doubled batch the body runs at;
        plan_batch as in _guided_weights).
        keep: with the regional keep's region.
        One buffer per configuration (ldm_sample_workspace_floats of it) and slot."""
        own = ((shape.H // 4) * (shape.W // 4), (shape.H // 8) * (shape.W // 8))
        keys = tuple(0 if int(k) == o else int(k) for k, o in zip(keys, own)) if keys else (0, 0)
        plan_batch = (plan_batch or 0) if guided else 0
        w = self._guided_weights(shape.B, shape.C, shape.H, shape.W, plan_batch) if guided else self.weights(shape)
        a = L.SampleArgs(nsteps=int(nsteps), S5=keys[0], S6=keys[1])
        if guided:   # (the size function reads only whether an option's pointers are set)
            a.s5_base = a.s6_base = a.guide_scale = 1
        if keep:
            a.z0 = a.n0 = a.keep = a.keep_coef = 1
        n = L.load().ldm_sample_workspace_floats(byref(shape), byref(w), byref(a))
        if n <= 0:
            raise RuntimeError("ldm_sample_workspace_floats failed")
        key = (shape.B, shape.C, shape.H, shape.W, shape.nf, str(device), slot, keys, bool(guided), plan_batch, bool(keep))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < n:
            ws = torch.zeros(int(n), device=device, dtype=torch.float32)
            self._ws[key] = ws
        return ws

    def release_workspaces(self, slot_prefix):
        """Drops the workspaces whose slot is a tuple starting with slot_prefix (a GraphedDDIM's private ones)."""
        for key in [k for k in self._ws if isinstance(k[6], tuple) and k[6][:len(slot_prefix)] == slot_prefix]:
            del self._ws[key]

    def side_streams(self, device, k):
        key = ("streams", str(device))
        ss = self._graphs.get(key, [])
        while len(ss) < k:
            ss.append(torch.cuda.Stream(device=device))
        self._graphs[key] = ss
        return ss[:k]

    @staticmethod
    def split_plan(t_table, B, split):
        """[(lo, hi, t_sub)] for `split` contiguous sub-batches; t_sub = t_table[:, lo:hi] made contiguous
        (prepared once, outside any timed / captured region, by GraphedDDIM)."""
        split = max(1, min(int(split), B))
        out = []
        for k in range(split):
            lo, hi = B * k // split, B * (k + 1) // split
            out.append((lo, hi, t_table[:, lo:hi].contiguous()))
        return out

    # -------------------------------------------------------------------------------------------
    def forward(self, z, t, s5, s6, out=None):
        ops.require_device(z, s5, s6)
        z, s5, s6 = ops.f32c(z), ops.f32c(s5), ops.f32c(s6)
        B, C, H, W = z.shape
        shape = self.shape(B, C, H, W)
        if self.mix_keys(z, s5, s6) is not None:
            raise RuntimeError("UNetEngine.forward: several style references (stacked style maps) are attended over in "
                               "the reverse loop only (ddim_loop / msolver_loop with the folded cross-attentions)")
        if tuple(s5.shape) != (B, 256, H // 4, W // 4) or tuple(s6.shape) != (B, 512, H // 8, W // 8):
            raise RuntimeError(f"UNet: style maps must be s5 [B,256,H/4,W/4], s6 [B,512,H/8,W/8] for z {tuple(z.shape)}; "
                               f"got {tuple(s5.shape)}, {tuple(s6.shape)}")
        if t.numel() == 1 and B > 1:
            t = t.reshape(1).expand(B)
        t_dev, t_is_float = ops._t_arg(t, z.device)
        if t_dev.shape[0] != B:
            raise RuntimeError("UNet: t must have one entry per sample")
        w = self.weights(shape)
        ws = self.workspace(shape, z.device)
        y = out if out is not None else torch.empty_like(z)
        L.call("ldm_unet_forward", byref(shape), byref(w), z.data_ptr(), t_dev.data_ptr(), t_is_float, s5.data_ptr(),
               s6.data_ptr(), y.data_ptr(), ws.data_ptr(), ops.stream_handle())
        return y

    @staticmethod
    def mix_keys(x, s5, s6, key_bias5=None, key_bias6=None):
        """(S5, S6), the key counts of a style mix: style maps holding R references stacked along the height (s5
        [B,256,R*H/4,W/4], s6 [B,512,R*H/8,W/8]) and / or a key bias.  None for today's single maps."""
        B, C, H, W = x.shape
        if s5.dim() != 4 or s6.dim() != 4:
            return None
        S5, S6 = s5.shape[2] * s5.shape[3], s6.shape[2] * s6.shape[3]
        if key_bias5 is None and key_bias6 is None and S5 == (H // 4) * (W // 4) and S6 == (H // 8) * (W // 8):
            return None
        return S5, S6

    def _mix_check(self, x, s5, s6, key_bias5, key_bias6):
        """Validates a style mix's operands and returns (S5, S6, bias pointers); raises where no mixing path exists."""
        B, C, H, W = x.shape
        S5, S6 = s5.shape[2] * s5.shape[3], s6.shape[2] * s6.shape[3]   # (= mix_keys where that is not None)
        L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
        if tuple(s5.shape[:2]) != (B, 256) or tuple(s6.shape[:2]) != (B, 512) or S5 % L2 or S6 % L1 or \
                S5 // L2 != S6 // L1 or s5.shape[3] != W // 4 or s6.shape[3] != W // 8:
            raise RuntimeError(f"style mix: style maps must be s5 [B,256,R*H/4,W/4], s6 [B,512,R*H/8,W/8] with one R for "
                               f"z {tuple(x.shape)}; got {tuple(s5.shape)}, {tuple(s6.shape)}")
        if not (self.fold and self.fold_applies(self.shape(B, C, H, W))):
            raise RuntimeError("style mix: several style references need the folded cross-attentions (fold=True, "
                               "latent planes up to 1024 positions); the unfolded engine has no kernel for them")
        ptrs = []
        for kb, S, name in ((key_bias5, S5, "key_bias5"), (key_bias6, S6, "key_bias6")):
            if kb is None:
                ptrs.append(None)
                continue
            ops.require_device(kb, what=name)
            if kb.dtype != torch.float32 or tuple(kb.shape) != (B, S) or not kb.is_contiguous():
                raise RuntimeError(f"style mix: {name} must be a contiguous fp32 [{B},{S}] tensor, got "
                                   f"{kb.dtype} {tuple(kb.shape)}")
            ptrs.append(kb.data_ptr())
        return S5, S6, ptrs[0], ptrs[1]

    @staticmethod
    def map_refs(x, s5, s6):
        """R of stacked style maps (s5 [B,256,R*H/4,W/4]): the reference count a style map's biases must have."""
        L2 = (x.shape[2] // 4) * (x.shape[3] // 4)
        return (s5.shape[2] * s5.shape[3]) // L2 if s5.dim() == 4 and L2 else 0

    @staticmethod
    def map_layout_check(xshape, R, ref_bias5, ref_bias6):
        """A style map's biases for a state of xshape and R references, checked on the host without device work: both
        given, contiguous fp32 ref_bias5 [B,H*W/16,R] / ref_bias6 [B,H*W/64,R] (ValueError), on the GPU (RuntimeError)."""
        if ref_bias5 is None or ref_bias6 is None:
            raise ValueError("style map: ref_bias5 and ref_bias6 go together (one is None)")
        B, C, H, W = xshape
        if R < 1:
            raise ValueError("style map: the biases need stacked style maps of R >= 1 references (LDM.encode_styles)")
        for rb, Lq, name in ((ref_bias5, (H // 4) * (W // 4), "ref_bias5"), (ref_bias6, (H // 8) * (W // 8), "ref_bias6")):
            if not isinstance(rb, torch.Tensor):
                raise ValueError(f"style map: {name} must be a tensor")
            if rb.dtype != torch.float32 or tuple(rb.shape) != (B, Lq, R) or not rb.is_contiguous():
                raise ValueError(f"style map: {name} must be a contiguous fp32 [{B},{Lq},{R}] tensor (one log-weight per "
                                 f"sample, query position and reference), got {rb.dtype} {tuple(rb.shape)}")
        ops.require_device(ref_bias5, ref_bias6, what="style map bias")

    def _map_check(self, x, s5, s6, ref_bias5, ref_bias6):
        """A style map's operands checked against the loop's (no device work).  Returns (R, S5, S6, pointers)."""
        if ref_bias5 is None or ref_bias6 is None:
            raise ValueError("style map: ref_bias5 and ref_bias6 go together (one is None)")
        S5, S6, _, _ = self._mix_check(x, s5, s6, None, None)    # stacked maps of one R, the folded engine
        R = self.map_refs(x, s5, s6)
        self.map_layout_check(tuple(x.shape), R, ref_bias5, ref_bias6)
        return R, S5, S6, ref_bias5.data_ptr(), ref_bias6.data_ptr()

    @staticmethod
    def map_values_check(ref_bias5, ref_bias6):
        """The biases' values (a device reduction and a host read): finite or -inf; NaN and +inf are refused."""
        for rb, name in ((ref_bias5, "ref_bias5"), (ref_bias6, "ref_bias6")):
            if bool(torch.isnan(rb).any()) or bool((rb == float("inf")).any()):
                raise ValueError(f"style map: {name} must be finite or -inf (NaN / +inf given)")

    @staticmethod
    def guidance_scale(scale, B, device=None):
        """The per-sample guidance strengths as a contiguous fp32 [B] tensor (on `device` when given): a Python
        number is broadcast, a tensor must hold B entries.  Finite values only (negative allowed): ValueError
        otherwise."""
        if isinstance(scale, torch.Tensor):
            t = scale.detach().to(torch.float32).reshape(-1)
            if t.numel() == 1 and B != 1:
                t = t.expand(B)
            if t.numel() != B:
                raise ValueError(f"guidance_scale: need one strength per sample ([{B}]), got {tuple(scale.shape)}")
        else:
            v = float(scale)
            t = torch.full((B,), v, dtype=torch.float32)
        if not bool(torch.isfinite(t).all()):
            raise ValueError("guidance_scale must be finite (NaN / inf given)")
        t = t.contiguous()
        return t.to(device) if device is not None else t

    @staticmethod
    def is_unguided(base, guidance_scale):
        """True where the arguments select today's samplers: no base and a scale of exactly 1 (every entry)."""
        if base is not None:
            return False
        if isinstance(guidance_scale, torch.Tensor):
            return bool((guidance_scale.detach() == 1).all())
        return float(guidance_scale) == 1.0

    def _guided_keys(self, x, s5, s6, key_bias5, key_bias6, base):
        """(S5, S6) of a guided loop: the key counts where either side is a mix (stacked maps or a bias), else (0, 0)."""
        if self.mix_keys(x, s5, s6, key_bias5, key_bias6) is None and base[2] is None and base[3] is None:
            return 0, 0
        return s5.shape[2] * s5.shape[3], s6.shape[2] * s6.shape[3]

    def _guided_weights(self, B, C, H, W, plan_batch=None):
        """The weights a guided loop of caller batch B binds: those of the doubled batch 2B the body runs at.
        plan_batch (a sub-batch chain of a split loop: the whole loop's batch): the chain runs the plans chosen for the
        whole loop's doubled batch instead of its own, so that a sample's arithmetic does not depend on how the batch
        is split (ldm_conv_make_plan picks the K/V projections' kernel kind and K split by the column count).  Only on
        the step-kernel path, whose sole planned launches are those two projections, and only where their plans need
        no split-K workspace (its size is per batch); otherwise the chain's own plans, as for the unguided loops."""
        if plan_batch and plan_batch != B:
            wf = self.weights(self.shape(2 * plan_batch, C, H, W))
            if wf.use_step and wf.ca_plan_kv[0].ws_floats == 0 and wf.ca_plan_kv[1].ws_floats == 0:
                return wf
        return self.weights(self.shape(2 * B, C, H, W))

    class KeepOperands(tuple):
        """(z0, n0, w, coefs) as keep_operands() returns them: checked, contiguous fp32 on the device."""

    @classmethod
    def keep_operands(cls, keep, xshape, n, device):
        """The regional keep's operands checked and made contiguous fp32 on `device`: keep is a dict or tuple of z0, n0
        ([B,C,H,W] like x), w ([B,H,W] keep weights: 1 keeps the content, 0 is free) and coefs ([n,2],
        ForwardDiffusion.keep_coefs).  ValueError for wrong shapes and for a w that is not finite or lies outside
        [0, 1].  A KeepOperands is returned as it is (a captured loop's static buffers)."""
        if isinstance(keep, cls.KeepOperands):
            return keep
        if isinstance(keep, dict):
            try:
                keep = (keep["z0"], keep["n0"], keep["w"], keep["coefs"])
            except KeyError as e:
                raise ValueError(f"keep: missing entry {e} (need z0, n0, w, coefs)") from None
        if len(keep) != 4 or any(not isinstance(v, torch.Tensor) for v in keep):
            raise ValueError("keep must hold the four tensors z0, n0, w, coefs")
        z0, n0, w, coefs = keep
        B, C, H, W = xshape
        if tuple(z0.shape) != tuple(xshape) or tuple(n0.shape) != tuple(xshape):
            raise ValueError(f"keep: z0 / n0 must be shaped like x {tuple(xshape)}, got {tuple(z0.shape)}, {tuple(n0.shape)}")
        if tuple(w.shape) != (B, H, W):
            raise ValueError(f"keep: w must be [B,H,W] = {(B, H, W)}, got {tuple(w.shape)}")
        if tuple(coefs.shape) != (n, 2):
            raise ValueError(f"keep: coefs must be [n,2] for n = {n} steps, got {tuple(coefs.shape)}")
        wf = w.detach().to(torch.float32)
        if not bool(torch.isfinite(wf).all()):
            raise ValueError("keep: w must be finite (NaN / inf given)")
        if not (bool((wf >= 0).all()) and bool((wf <= 1).all())):
            raise ValueError("keep: w must lie in [0, 1]")
        return cls.KeepOperands(v.detach().to(device, torch.float32).contiguous() for v in (z0, n0, wf, coefs))

    def _guided_operands(self, x, s5, s6, key_bias5, key_bias6, base, scale):
        """The guided loop's operands checked: its SampleArgs fields (the key counts, and the biases, the base maps and
        the scale as pointers)."""
        B, C, H, W = x.shape
        s5b, s6b, kb5b, kb6b = base
        ops.require_device(s5b, s6b, scale, what="guidance operand")
        if tuple(s5b.shape) != tuple(s5.shape) or tuple(s6b.shape) != tuple(s6.shape):
            raise ValueError(f"guidance: the base style maps must have the target's shapes (same key counts): target "
                             f"{tuple(s5.shape)}, {tuple(s6.shape)}; base {tuple(s5b.shape)}, {tuple(s6b.shape)} "
                             "(LDM.tile_embedding repeats a single style for a mix of R references)")
        if scale.dtype != torch.float32 or tuple(scale.shape) != (B,) or not scale.is_contiguous():
            raise ValueError(f"guidance: scale must be a contiguous fp32 [{B}] device tensor, got {scale.dtype} "
                             f"{tuple(scale.shape)}")
        S5, S6 = self._guided_keys(x, s5, s6, key_bias5, key_bias6, base)
        p5 = p6 = p5b = p6b = None
        if S5:
            S5, S6, p5, p6 = self._mix_check(x, s5, s6, key_bias5, key_bias6)
            _, _, p5b, p6b = self._mix_check(x, s5b, s6b, kb5b, kb6b)
        else:
            self._single_maps_check(x, s5, s6)
        return dict(S5=S5, S6=S6, key_bias5=p5, key_bias6=p6, s5_base=s5b.data_ptr(), s6_base=s6b.data_ptr(),
                    key_bias5_base=p5b, key_bias6_base=p6b, guide_scale=scale.data_ptr())

    @staticmethod
    def seam_check(seam_cols, W):
        """The joint loop's seam width as an int: 0 (off) or latent columns in [1, W / 2].  ValueError otherwise."""
        ov = int(seam_cols)
        if ov != seam_cols or not 0 <= ov <= int(W) // 2:
            raise ValueError(f"seam_cols must be a whole number of latent columns in [0, W / 2] = [0, {int(W) // 2}], "
                             f"got {seam_cols!r}")
        return ov

    @staticmethod
    def _single_maps_check(x, s5, s6):
        B, C, H, W = x.shape
        if tuple(s5.shape) != (B, 256, H // 4, W // 4) or tuple(s6.shape) != (B, 512, H // 8, W // 8):
            raise RuntimeError(f"UNet: style maps must be s5 [B,256,H/4,W/4], s6 [B,512,H/8,W/8] for z {tuple(x.shape)}; "
                               f"got {tuple(s5.shape)}, {tuple(s6.shape)}")

    def _sample_call(self, solver, x, s5, s6, t_table, coef_table, eta, x0_logs, eps_logs, log_stride, slot,
                     key_bias5=None, key_bias6=None, base=None, scale=None, plan_batch=None, keep=None, phase=None,
                     ref_bias5=None, ref_bias6=None, seam_cols=0):
        """One C loop (ldm_sample) of solver "ddim" / "msolver" on x, with whichever options are given: a mix (stacked
        s5 / s6, key biases), guidance (base = (s5_base, s6_base, key_bias5_base, key_bias6_base) with the target's key
        counts, scale a device fp32 [B] tensor (guidance_scale()); plan_batch: see _guided_weights) and the regional
        keep (keep_operands()).  ref_bias5 / ref_bias6: the style map's biases (ddim_loop); their layout is checked here,
        their values by the callers (no device work in this function: it runs under capture).  seam_cols: the joint
        loop's seam width (ddim_loop; checked by seam_check).

        phase None: the whole loop (ldm_sample).  phase "prepare" / "run": that C entry alone (GraphedDDIM, on
        workspaces of its own: the engine's shared ones are also written by forward() and by captured graphs' replays,
        so nothing prepared in them is trusted from one call to the next)."""
        B, C, H, W = x.shape
        shape = self.shape(B, C, H, W)
        n = t_table.shape[0]
        a = L.SampleArgs(solver=L.SOLVER[solver], nsteps=n, eta=float(eta), x=x.data_ptr(), s5=s5.data_ptr(),
                         s6=s6.data_ptr(), t_table=t_table.data_ptr(), coef_table=coef_table.data_ptr(),
                         x0_logs=ops._p(x0_logs), eps_logs=ops._p(eps_logs), log_step_stride=int(log_stride),
                         stream=ops.stream_handle(), seam_cols=self.seam_check(seam_cols, W))
        if base is not None:
            for f, v in self._guided_operands(x, s5, s6, key_bias5, key_bias6, base, scale).items():
                setattr(a, f, v)
            w = self._guided_weights(B, C, H, W, plan_batch)   # the body runs at the doubled batch: targets, then bases
        else:
            if self.mix_keys(x, s5, s6, key_bias5, key_bias6) is not None:
                a.S5, a.S6, a.key_bias5, a.key_bias6 = self._mix_check(x, s5, s6, key_bias5, key_bias6)
            else:
                self._single_maps_check(x, s5, s6)
            w = self.weights(shape)
        if keep is not None:
            keep = self.keep_operands(keep, x.shape, n, x.device)
            a.z0, a.n0, a.keep, a.keep_coef = (v.data_ptr() for v in keep)
        if ref_bias5 is not None or ref_bias6 is not None:
            a.refs, S5, S6, a.ref_bias5, a.ref_bias6 = self._map_check(x, s5, s6, ref_bias5, ref_bias6)
            if not a.S5:    # one reference without a key bias: the maps' own counts, stated
                a.S5, a.S6 = S5, S6
        a.workspace = self.workspace(shape, x.device, n, slot, keys=(a.S5, a.S6), guided=base is not None,
                                     plan_batch=plan_batch, keep=keep is not None).data_ptr()
        entry = {None: "ldm_sample", "prepare": "ldm_sample_prepare", "run": "ldm_sample_run"}[phase]
        L.call(entry, byref(shape), byref(w), byref(a))

    def msolver_loop(self, x, s5, s6, t_table, coef_table, x0_logs, eps_logs=None, split=1, plan=None, key_bias5=None,
                     key_bias6=None, base=None, guidance_scale=1.0, keep=None, ref_bias5=None, ref_bias6=None,
                     seam_cols=0):
        """ddim_loop's twin for the multistep solver (DPM-Solver++(2M) or its first-order form): coef_table
        [n,8] from ForwardDiffusion.multistep_coefs (device), no eta.  x0_logs [n,B,C,H,W] is required: step i
        reads step i-1's slot as its history.  Same sub-batch chains, base=, guidance_scale=, keep=, style map
        (ref_bias5= / ref_bias6=) and seam_cols= as ddim_loop."""
        if x0_logs is None:
            raise ValueError("msolver_loop: x0_logs is required (it is the solver's history)")
        if coef_table.dim() != 2 or coef_table.shape[1] != 8 or coef_table.shape[0] != t_table.shape[0]:
            raise ValueError(f"msolver_loop: coef_table must be [n,8] for n = {t_table.shape[0]} steps, "
                             f"got {tuple(coef_table.shape)}")
        return self._loop("msolver", x, s5, s6, t_table, coef_table, 0.0, x0_logs, eps_logs, split, plan, key_bias5,
                          key_bias6, base, guidance_scale, keep, ref_bias5, ref_bias6, seam_cols)

    def ddim_loop(self, x, s5, s6, t_table, coef_table, eta, x0_logs=None, eps_logs=None, split=1, plan=None,
                  key_bias5=None, key_bias6=None, base=None, guidance_scale=1.0, keep=None, ref_bias5=None,
                  ref_bias6=None, seam_cols=0):
        """In-place reverse loop on x ([B,C,H,W] contiguous fp32).  t_table [n,B] int64, coef [n,4] (device).

        Style mixing: s5 / s6 may hold R style references stacked along the map's height (s5 [B,256,R*H/4,W/4],
        s6 [B,512,R*H/8,W/8]; reference r owns keys [r*L, (r+1)*L)), with key_bias5 [B,R*H*W/16] / key_bias6
        [B,R*H*W/64] (fp32, the log of each key's reference weight, -inf allowed; None = equal weights).  Needs the
        folded engine; the sub-batch split slices the biases with the maps.

        Style guidance: base = (s5_base, s6_base, key_bias5_base, key_bias6_base) (maps shaped like the target's, the
        biases None or as above) makes every step evaluate the denoiser under both styles and step on
        e_b + guidance_scale * (e_t - e_b); guidance_scale is a float or a [B] tensor (finite).  With base=None the
        call is the unguided one, argument for argument (a scale other than 1 then has nothing to guide against:
        ValueError).

        Regional keep: keep = a dict or tuple of z0, n0 ([B,C,H,W]: the clean latent and the q_sample noise), w
        ([B,H,W] in [0,1]: 1 keeps the content, 0 is free) and coefs ([n,2], ForwardDiffusion.keep_coefs).  After every
        step's update the state becomes (1 - w) x + w (coefs[i][0] z0 + coefs[i][1] n0), fused into dec1's epilogue;
        the logs stay the model's own prediction.  Composes with the mix, the guidance and the split (each chain gets
        its slice).  ValueError for a w outside [0, 1] or not finite, and for wrong shapes.

        Style map: ref_bias5 [B,H*W/16,R] / ref_bias6 [B,H*W/64,R] (contiguous fp32 on the device, finite or -inf; both
        or neither) give the log-weight of each of the R stacked references at every query position of the two
        cross-attentions (tokens row-major as the UNet flattens its maps; LDM.style_map_bias builds them).  They add
        to the key biases, apply to the target half only under guidance, and are read by every step's attentions, not
        folded before the loop.  ValueError for a wrong shape, dtype or device and for NaN / +inf.

        Joint sampling: seam_cols (latent columns, 0 = off, at most W / 2) declares the batch rows neighbouring windows
        of one recording, row b + 1 starting seam_cols columns before row b ends.  Before step 0 and after every
        step's update (after the keep blend) the columns two rows share are replaced in both by one weighted average,
        a + w_j (q - a) with w_j = (j + 1) / (seam_cols + 1) the later window's weight (ldm_capi.h), so all rows carry
        one consistent latent canvas and the returned x agrees bitwise across every seam.  The logs stay each
        window's own prediction; under guidance the two halves are fused separately.  The rows are then not
        independent: split > 1 or a multi-chain plan with seam_cols > 0 is a ValueError.  B = 1 is the plain loop.

        split > 1 runs the batch as that many independent sub-batch chains, each on its own stream
        (forked from and joined back into the current stream, so it also works under graph capture).
        The path is per-sample, so the result is the same up to fp32 summation order (a sub-batch
        size may get a conv plan that splits K differently); the chains' launch and memory latencies
        overlap each other's work."""
        return self._loop("ddim", x, s5, s6, t_table, coef_table, eta, x0_logs, eps_logs, split, plan, key_bias5,
                          key_bias6, base, guidance_scale, keep, ref_bias5, ref_bias6, seam_cols)

    def _loop(self, solver, x, s5, s6, t_table, coef_table, eta, x0_logs, eps_logs, split, plan, key_bias5=None,
              key_bias6=None, base=None, guidance_scale=1.0, keep=None, ref_bias5=None, ref_bias6=None, seam_cols=0):
        """The whole batch in one _sample_call, or one per sub-batch chain with every per-sample operand (the maps, the
        biases, the base, the scales, the keep operands, the logs) sliced with the batch.
        Guided, on the step-kernel path, the chains run the whole batch's plans (_guided_weights), so split > 1 gives
        each sample bitwise what split = 1 gives it while both select the same per-batch forms (the bottleneck value
        fold applies up to a doubled batch of 8)."""
        B, n = x.shape[0], t_table.shape[0]
        guided = base is not None
        seam_cols = self.seam_check(seam_cols, x.shape[3])
        if seam_cols and (split > 1 or (plan and len(plan) > 1)):
            raise ValueError("seam_cols: the rows of a joint loop are fused across their seams after every step, so the "
                             "batch cannot run as independent sub-batch chains (split > 1 or a multi-chain plan)")
        if keep is not None:
            keep = self.keep_operands(keep, x.shape, n, x.device)
        if ref_bias5 is not None or ref_bias6 is not None:
            self._map_check(x, s5, s6, ref_bias5, ref_bias6)
            if not torch.cuda.is_current_stream_capturing():    # (a captured loop's static buffers were checked)
                self.map_values_check(ref_bias5, ref_bias6)
        scale = None
        if guided:
            if len(base) != 4:
                raise ValueError("base must be (s5_base, s6_base, key_bias5_base, key_bias6_base)")
            scale = guidance_scale
            if not (isinstance(scale, torch.Tensor) and scale.is_cuda and scale.dtype == torch.float32 and
                    tuple(scale.shape) == (B,) and scale.is_contiguous()):   # (a graph's static buffer is passed as it is)
                scale = self.guidance_scale(scale, B, x.device)
            base = (ops.f32c(base[0]), ops.f32c(base[1]), base[2], base[3])
        else:
            if not self.is_unguided(None, guidance_scale):
                raise ValueError("guidance_scale other than 1 needs a base style to guide against (base=)")
            if self.mix_keys(x, s5, s6, key_bias5, key_bias6) is not None:
                self._mix_check(x, s5, s6, key_bias5, key_bias6)
        if plan is None:
            plan = self.split_plan(t_table, B, split) if split > 1 else None
        if not plan or len(plan) == 1:
            self._sample_call(solver, x, s5, s6, t_table, coef_table, eta, x0_logs, eps_logs, 0, 0, key_bias5, key_bias6,
                              base, scale, None, keep, ref_bias5=ref_bias5, ref_bias6=ref_bias6, seam_cols=seam_cols)
            return x
        per_step = x[0].numel() * B
        main = torch.cuda.current_stream(x.device)
        streams = self.side_streams(x.device, len(plan))
        C, H, W = x.shape[1:]
        keys = self._guided_keys(x, s5, s6, key_bias5, key_bias6, base) if guided else \
            self.mix_keys(x, s5, s6, key_bias5, key_bias6)
        for k, (lo, hi, t_sub) in enumerate(plan):   # bind / pack / allocate on the main stream first
            self.workspace(self.shape(hi - lo, C, H, W), x.device, n, k, keys=keys, guided=guided,
                           plan_batch=B if guided else None, keep=keep is not None)

        def cut(lo, hi):
            """(x, s5, s6, x0_logs, eps_logs, key_bias5, key_bias6, base, scale, keep) of samples [lo, hi)"""
            def c(v):
                return None if v is None else v[lo:hi]
            return (x[lo:hi], s5[lo:hi], s6[lo:hi], None if x0_logs is None else x0_logs[0, lo:hi],
                    None if eps_logs is None else eps_logs[0, lo:hi], c(key_bias5), c(key_bias6),
                    tuple(c(v) for v in base) if guided else None, c(scale), self._keep_cut(keep, lo, hi))

        for k, (lo, hi, t_sub) in enumerate(plan):
            st = streams[k]
            st.wait_stream(main)
            if not torch.cuda.is_current_stream_capturing():
                t_sub.record_stream(st)
            with torch.cuda.stream(st):
                xs, a5, a6, x0l, epl, b5, b6, gb, gs, kc = cut(lo, hi)
                c5, c6 = (None if v is None else v[lo:hi] for v in (ref_bias5, ref_bias6))   # the chain's maps
                self._sample_call(solver, xs, a5, a6, t_sub, coef_table, eta, x0l, epl, per_step, k, b5, b6, gb, gs,
                                  B if guided else None, kc, ref_bias5=c5, ref_bias6=c6)
        for st in streams:
            main.wait_stream(st)
        return x

    @classmethod
    def _keep_cut(cls, kp, lo, hi):
        """A sub-batch chain's slice of the keep operands (the coefficient table is shared)."""
        return None if kp is None else cls.KeepOperands((kp[0][lo:hi], kp[1][lo:hi], kp[2][lo:hi], kp[3]))


class GraphedDDIM:
    """A captured reverse loop with static buffers: replay() re-runs all n steps from x_init."""

    def __init__(self, engine, x_init, s5, s6, t_table, coef_table, eta, logs=True, split=1, solver="ddim",
                 key_bias5=None, key_bias6=None, base=None, guidance_scale=1.0, keep=None, ref_bias5=None,
                 ref_bias6=None, seam_cols=0):
        """solver="ddim": coef_table [n,4] and eta, the reference's update; solver="msolver": coef_table [n,8]
        (ForwardDiffusion.multistep_coefs), eta unused and the x0 logs always kept (the solver's history).
        s5 / s6 may be stacked style references with key_bias5 / key_bias6 (UNetEngine.ddim_loop).
        base / guidance_scale: style guidance as in UNetEngine.ddim_loop; the strengths live in the static device
        buffer `scale` ([B] fp32), which set_guidance_scale() rewrites between replays without a new capture.
        keep: the regional keep as in UNetEngine.ddim_loop; its operands are cloned into static buffers, and
        set_keep() rewrites the weights between replays without a new capture.
        ref_bias5 / ref_bias6: the style map as in UNetEngine.ddim_loop, cloned into static buffers that the captured
        loop's attentions read; set_style_map() rewrites them between replays without a new capture and without a
        prepare launch (the prepare phase does not read them).
        seam_cols: joint sampling as in UNetEngine.ddim_loop (the fuses are captured with the loop; not with split > 1)."""
        if solver not in ("ddim", "msolver"):
            raise ValueError(f"GraphedDDIM: unknown solver {solver!r}")
        self.seam_cols = engine.seam_check(seam_cols, x_init.shape[3])
        if self.seam_cols and split > 1:
            raise ValueError("GraphedDDIM: seam_cols needs split = 1 (the rows of a joint loop are not independent)")
        self.solver = solver
        logs = logs or solver == "msolver"
        self.engine = engine
        self.split = split
        dev = x_init.device
        self.x_init = x_init.contiguous().clone()
        self.x = torch.empty_like(self.x_init)
        self.s5 = s5.contiguous().clone()
        self.s6 = s6.contiguous().clone()
        self.kb5 = None if key_bias5 is None else key_bias5.contiguous().clone()
        self.kb6 = None if key_bias6 is None else key_bias6.contiguous().clone()
        self.rb5 = self.rb6 = None
        if ref_bias5 is not None or ref_bias6 is not None:
            engine._map_check(self.x, self.s5, self.s6, ref_bias5, ref_bias6)
            engine.map_values_check(ref_bias5, ref_bias6)
            self.rb5, self.rb6 = ref_bias5.clone(), ref_bias6.clone()
        self.base = self.scale = None
        if base is not None:
            self.base = tuple(None if v is None else ops.f32c(v).clone() for v in base)
            self.scale = engine.guidance_scale(guidance_scale, x_init.shape[0], dev)
        elif not engine.is_unguided(None, guidance_scale):
            raise ValueError("guidance_scale other than 1 needs a base style to guide against (base=)")
        self.t_table = t_table.to(dev).contiguous()
        self.coef = coef_table.to(dev).contiguous()
        n = self.t_table.shape[0]
        self.keep = None
        if keep is not None:
            kp = engine.keep_operands(keep, x_init.shape, n, dev)
            self.keep = engine.KeepOperands(v.clone() for v in kp)
        self.x0_logs = torch.empty((n,) + tuple(x_init.shape), device=dev) if logs else None
        self.eps_logs = torch.empty((n,) + tuple(x_init.shape), device=dev) if logs else None
        self.eta = float(eta)
        # static sub-batch timestep tables, made once outside the captured region
        self.plan = engine.split_plan(self.t_table, x_init.shape[0], split) if split > 1 else None
        # Workspaces of this object's own (a slot no other caller names): between two replays nothing else writes the
        # prepared regions, which is what lets a replay skip the prepare graph.
        self._slot = ("graph", id(self))
        weakref.finalize(self, engine.release_workspaces, self._slot)
        self.prepare_launches = 0     # replays that launched the prepare graphs first
        self._build()

    def _chains(self):
        """(k, lo, hi, t_sub) per sub-batch chain; the whole batch as one chain without a split."""
        if not self.plan:
            return [(0, 0, self.x.shape[0], self.t_table)]
        return [(k, lo, hi, t_sub) for k, (lo, hi, t_sub) in enumerate(self.plan)]

    def _chain_call(self, k, lo, hi, t_sub, phase):
        """One phase (ldm_sample_prepare / ldm_sample_run) of chain k on its own workspace."""
        def c(v):
            return None if v is None else v[lo:hi]
        split = bool(self.plan)
        gb = None if self.base is None else tuple(c(v) for v in self.base)
        x0l = None if self.x0_logs is None else (self.x0_logs[0, lo:hi] if split else self.x0_logs)
        epl = None if self.eps_logs is None else (self.eps_logs[0, lo:hi] if split else self.eps_logs)
        per_step = self.x[0].numel() * self.x.shape[0] if split else 0
        self.engine._sample_call(self.solver, self.x[lo:hi], self.s5[lo:hi], self.s6[lo:hi], t_sub, self.coef, self.eta,
                                 x0l, epl, per_step, self._slot + (k,), c(self.kb5), c(self.kb6), gb, c(self.scale),
                                 self.x.shape[0] if (split and gb is not None) else None,
                                 self.engine._keep_cut(self.keep, lo, hi), phase=phase, ref_bias5=c(self.rb5),
                                 ref_bias6=c(self.rb6), seam_cols=self.seam_cols)

    def _operands(self):
        """The static tensors the prepare phase reads."""
        return (self.s5, self.s6, self.kb5, self.kb6) + (self.base if self.base is not None else (None,) * 4) + \
            (self.t_table,)

    def prepared_key(self, weight_version=None):
        """prepared_key of the static buffers and the engine's weights as they stand (host only, no device work)."""
        wv = self.engine.weight_version() if weight_version is None else weight_version
        return prepared_key(self._operands(), wv)

    def _build(self):
        """Warm-up, then two captured graphs per chain: the prepare (style and time state) and the loop.  Run again
        when the engine's weight version moves: a capture holds the addresses of the packed weights."""
        self.graphs = self.prep_graphs = None
        self._prepared_key = None
        self._weight_version = self.engine.weight_version()
        # warm-up (packs weights, allocates workspaces, runs the entries' eager-only workspace check) outside capture
        self.x.copy_(self.x_init)
        for ch in self._chains():
            self._chain_call(*ch, phase="prepare")
            self._chain_call(*ch, phase="run")
        torch.cuda.synchronize()
        # Without a split one chain on the capture stream.  With one, a pair of graphs per sub-batch chain, each chain
        # replayed on its own stream: a single graph's parallel branches are executed one after another, separate
        # graphs on separate streams (hardware queues) run concurrently.
        self.streams = self.engine.side_streams(self.x.device, len(self.plan)) if self.plan else None
        self.graphs, self.prep_graphs = [], []
        for k, lo, hi, t_sub in self._chains():
            st = None if self.streams is None else self.streams[k]
            gp, gl = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with capture(gp, stream=st):
                self._chain_call(k, lo, hi, t_sub, "prepare")
            with capture(gl, stream=st):
                self.x[lo:hi].copy_(self.x_init[lo:hi])
                self._chain_call(k, lo, hi, t_sub, "run")
            self.prep_graphs.append(gp)
            self.graphs.append(gl)

    def invalidate(self):
        """The next replay launches the prepare graphs first.  For callers that write the static style buffers, key
        biases or t_table through raw pointers, which moves no tensor version (writes through torch are seen)."""
        self._prepared_key = None

    def set_guidance_scale(self, guidance_scale):
        """Writes new strengths (float or [B]) into the static buffer the captured loop reads: the next replay runs
        at them.  Only for a graph captured with a base style."""
        if self.scale is None:
            raise ValueError("set_guidance_scale: this loop was captured without a base style")
        self.scale.copy_(self.engine.guidance_scale(guidance_scale, self.scale.shape[0]), non_blocking=False)

    def set_keep(self, w):
        """Writes new keep weights ([B,H,W] in [0,1]) into the static buffer the captured loop reads: the next replay
        runs under the new mask.  Only for a graph captured with keep=."""
        if self.keep is None:
            raise ValueError("set_keep: this loop was captured without keep=")
        kp = self.engine.keep_operands((self.keep[0], self.keep[1], w, self.keep[3]), self.x.shape, self.keep[3].shape[0],
                                       self.x.device)
        self.keep[2].copy_(kp[2], non_blocking=False)

    def set_style_map(self, ref_bias5, ref_bias6):
        """Writes a new style map (UNetEngine.ddim_loop's ref_bias5 / ref_bias6) into the static buffers the captured
        loop reads: the next replay runs under it.  No new capture and no prepare launch: the biases are not among the
        prepare phase's operands.  Only for a graph captured with a style map."""
        if self.rb5 is None:
            raise ValueError("set_style_map: this loop was captured without a style map (ref_bias5= / ref_bias6=)")
        self.engine._map_check(self.x, self.s5, self.s6, ref_bias5, ref_bias6)
        self.engine.map_values_check(ref_bias5, ref_bias6)
        self.rb5.copy_(ref_bias5, non_blocking=False)
        self.rb6.copy_(ref_bias6, non_blocking=False)

    def replay(self):
        """Launches the loop graphs; the prepare graphs first when a static buffer the prepare phase reads (s5, s6,
        the key biases, the base maps and biases, t_table) or a UNet weight has been written through torch since the
        last prepare (compared by tensor version on the host), or after invalidate().  x_init, the coefficient
        table, the guidance scale, the keep operands and the style map are read by the loop graphs: no prepare for them."""
        wv = self.engine.weight_version()
        if wv != self._weight_version:
            self._build()
        key = self.prepared_key(wv)
        prepare = key != self._prepared_key
        if prepare:
            if self.plan:     # the chains read their own contiguous column blocks of t_table
                for lo, hi, t_sub in self.plan:
                    t_sub.copy_(self.t_table[:, lo:hi])
            self._prepared_key = key
            self.prepare_launches += 1
        if self.streams is None:
            if prepare:
                self.prep_graphs[0].replay()
            self.graphs[0].replay()
            return self.x
        main = torch.cuda.current_stream()
        for st, gp, g in zip(self.streams, self.prep_graphs, self.graphs):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                if prepare:
                    gp.replay()
                g.replay()
        for st in self.streams:
            main.wait_stream(st)
        return self.x
