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
        keys = keys or (0, 0)
        # no operands here: a set flag stands for its option's pointers (the size function reads only whether they are set)
        a = L.SampleArgs(nsteps=int(nsteps), S5=int(keys[0]), S6=int(keys[1]), guide_scale=int(bool(guided)),
                         keep=int(bool(keep)))
        w = self._guided_weights(shape.B, shape.C, shape.H, shape.W, plan_batch) if guided else self.weights(shape)
        return self._workspace(shape, w, a, device, slot, plan_batch)

    def _workspace(self, shape, w, a, device, slot, plan_batch):
        """The workspace of the call that passes the argument struct `a` (LoopOptions.fill) with the weights w."""
        own = ((shape.H // 4) * (shape.W // 4), (shape.H // 8) * (shape.W // 8))
        keys = tuple(0 if k == o else k for k, o in zip((a.S5, a.S6), own))
        guided, keep = bool(a.s5_base or a.guide_scale), bool(a.z0 or a.keep)
        n = L.load().ldm_sample_workspace_floats(byref(shape), byref(w), byref(a))
        if n <= 0:
            raise RuntimeError("ldm_sample_workspace_floats failed")
        key = (shape.B, shape.C, shape.H, shape.W, shape.nf, str(device), slot, keys, guided,
               (plan_batch or 0) if guided else 0, keep)
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

    @staticmethod
    def seam_check(seam_cols, W):
        """The joint loop's seam width as an int: 0 (off) or latent columns in [1, W / 2].  ValueError otherwise."""
        ov = int(seam_cols)
        if ov != seam_cols or not 0 <= ov <= int(W) // 2:
            raise ValueError(f"seam_cols must be a whole number of latent columns in [0, W / 2] = [0, {int(W) // 2}], "
                             f"got {seam_cols!r}")
        return ov

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
        opts = LoopOptions(x, t_table.shape[0], s5, s6, key_bias5=key_bias5, key_bias6=key_bias6, base=base,
                           guidance_scale=guidance_scale, keep=keep, ref_bias5=ref_bias5, ref_bias6=ref_bias6,
                           seam_cols=seam_cols)
        return self._loop("msolver", x, opts, t_table, coef_table, 0.0, x0_logs, eps_logs, split, plan)

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
        opts = LoopOptions(x, t_table.shape[0], s5, s6, key_bias5=key_bias5, key_bias6=key_bias6, base=base,
                           guidance_scale=guidance_scale, keep=keep, ref_bias5=ref_bias5, ref_bias6=ref_bias6,
                           seam_cols=seam_cols)
        return self._loop("ddim", x, opts, t_table, coef_table, eta, x0_logs, eps_logs, split, plan)

    def _sample_call(self, solver, x, opts, t_table, coef_table, eta, x0_logs, eps_logs, log_stride, slot,
                     plan_batch=None, phase=None):
        """One C loop (ldm_sample) of solver "ddim" / "msolver" on x under opts, a checked LoopOptions (or a cut of one)
        for x's samples.  No checks and no device work here: it runs under capture.  plan_batch: see _guided_weights.

        phase None: the whole loop (ldm_sample).  phase "prepare" / "run": that C entry alone (GraphedDDIM, on
        workspaces of its own: the engine's shared ones are also written by forward() and by captured graphs' replays,
        so nothing prepared in them is trusted from one call to the next)."""
        a = L.SampleArgs(solver=L.SOLVER[solver], nsteps=t_table.shape[0], eta=float(eta), x=x.data_ptr(),
                         t_table=t_table.data_ptr(), coef_table=coef_table.data_ptr(), x0_logs=ops._p(x0_logs),
                         eps_logs=ops._p(eps_logs), log_step_stride=int(log_stride), stream=ops.stream_handle())
        shape, w = self._bind(x, opts, a, slot, plan_batch)
        entry = {None: "ldm_sample", "prepare": "ldm_sample_prepare", "run": "ldm_sample_run"}[phase]
        L.call(entry, byref(shape), byref(w), byref(a))

    def _bind(self, x, opts, a, slot, plan_batch):
        """Fills the SampleArgs a's option fields from opts and its workspace, sized by the very struct the call
        passes; returns the call's (shape, weights).  Guided, the weights of the doubled batch the body runs at."""
        B, C, H, W = x.shape
        shape = self.shape(B, C, H, W)
        opts.fill(a)
        w = self._guided_weights(B, C, H, W, plan_batch) if opts.guided else self.weights(shape)
        a.workspace = self._workspace(shape, w, a, x.device, slot, plan_batch).data_ptr()
        return shape, w

    def _loop(self, solver, x, opts, t_table, coef_table, eta, x0_logs, eps_logs, split, plan):
        """The whole batch in one _sample_call, or one per sub-batch chain on that chain's cut of the options and of
        the logs.  The options are checked once, here, for the whole batch.
        Guided, on the step-kernel path, the chains run the whole batch's plans (_guided_weights), so split > 1 gives
        each sample bitwise what split = 1 gives it while both select the same per-batch forms (the bottleneck value
        fold applies up to a doubled batch of 8)."""
        B, n = x.shape[0], t_table.shape[0]
        if opts.seam_cols and (split > 1 or (plan and len(plan) > 1)):
            raise ValueError("seam_cols: the rows of a joint loop are fused across their seams after every step, so the "
                             "batch cannot run as independent sub-batch chains (split > 1 or a multi-chain plan)")
        opts.check(self, x, n)
        if not torch.cuda.is_current_stream_capturing():    # (a captured loop's static buffers were checked)
            opts.check_values()
        if plan is None:
            plan = self.split_plan(t_table, B, split) if split > 1 else None
        if not plan or len(plan) == 1:
            self._sample_call(solver, x, opts, t_table, coef_table, eta, x0_logs, eps_logs, 0, 0)
            return x
        per_step = x[0].numel() * B
        main = torch.cuda.current_stream(x.device)
        streams = self.side_streams(x.device, len(plan))
        plan_batch = B if opts.guided else None
        chains = [(st, x[lo:hi], opts.cut(lo, hi), t_sub, None if x0_logs is None else x0_logs[0, lo:hi],
                   None if eps_logs is None else eps_logs[0, lo:hi]) for st, (lo, hi, t_sub) in zip(streams, plan)]
        for k, (st, xs, oc, t_sub, x0l, epl) in enumerate(chains):   # bind / pack / allocate on the main stream first
            self._bind(xs, oc, L.SampleArgs(nsteps=n), k, plan_batch)
        for k, (st, xs, oc, t_sub, x0l, epl) in enumerate(chains):
            st.wait_stream(main)
            if not torch.cuda.is_current_stream_capturing():
                t_sub.record_stream(st)
            with torch.cuda.stream(st):
                self._sample_call(solver, xs, oc, t_sub, coef_table, eta, x0l, epl, per_step, k, plan_batch)
        for st in streams:
            main.wait_stream(st)
        return x


class LoopOptions:
    """Everything a reverse loop takes besides the state, the tables and the logs (UNetEngine.ddim_loop documents the
    options): the style maps, the mix's key biases, the guidance base and scale, the regional keep's operands, the style
    map's reference biases and the joint loop's seam width.  Built from the public arguments, checked once for the whole
    batch (check), cut per sub-batch chain (cut) and written into the C argument struct (fill)."""
    # field -> the ldm_sample_args pointer it fills.  Every one is per-sample ([B, ...]) unless listed in SHARED.
    POINTERS = {"s5": "s5", "s6": "s6", "key_bias5": "key_bias5", "key_bias6": "key_bias6", "ref_bias5": "ref_bias5",
                "ref_bias6": "ref_bias6", "s5_base": "s5_base", "s6_base": "s6_base", "key_bias5_base": "key_bias5_base",
                "key_bias6_base": "key_bias6_base", "scale": "guide_scale", "z0": "z0", "n0": "n0", "keep_w": "keep",
                "keep_coef": "keep_coef"}
    SHARED = ("keep_coef", "seam_cols", "S5", "S6", "refs")   # cut() carries these over as they are
    __slots__ = tuple(POINTERS) + ("seam_cols", "S5", "S6", "refs")

    def __init__(self, x, n, s5, s6, key_bias5=None, key_bias6=None, base=None, guidance_scale=1.0, keep=None,
                 ref_bias5=None, ref_bias6=None, seam_cols=0):
        """The public arguments of a loop of n steps on x (read for its shape and device), normalised: the maps
        contiguous fp32, the scale a contiguous fp32 [B] tensor on x's device (a graph's static buffer is taken as it
        is), the keep as keep_operands() gives it.  ValueError for a bad scale, keep or seam width."""
        B = x.shape[0]
        self.s5, self.s6 = ops.f32c(s5), ops.f32c(s6)
        self.key_bias5, self.key_bias6, self.ref_bias5, self.ref_bias6 = key_bias5, key_bias6, ref_bias5, ref_bias6
        self.seam_cols = UNetEngine.seam_check(seam_cols, x.shape[3])
        self.s5_base = self.s6_base = self.key_bias5_base = self.key_bias6_base = self.scale = None
        if base is not None:
            if len(base) != 4:
                raise ValueError("base must be (s5_base, s6_base, key_bias5_base, key_bias6_base)")
            self.s5_base, self.s6_base, self.key_bias5_base, self.key_bias6_base = \
                ops.f32c(base[0]), ops.f32c(base[1]), base[2], base[3]
            sc = guidance_scale
            if not (isinstance(sc, torch.Tensor) and sc.is_cuda and sc.dtype == torch.float32 and
                    tuple(sc.shape) == (B,) and sc.is_contiguous()):
                sc = UNetEngine.guidance_scale(sc, B, x.device)
            self.scale = sc
        elif not UNetEngine.is_unguided(None, guidance_scale):
            raise ValueError("guidance_scale other than 1 needs a base style to guide against (base=)")
        self.z0, self.n0, self.keep_w, self.keep_coef = \
            (None,) * 4 if keep is None else UNetEngine.keep_operands(keep, x.shape, n, x.device)
        self.S5 = self.S6 = self.refs = None     # the key counts and the reference count: check() derives them

    guided = property(lambda self: self.s5_base is not None)
    mapped = property(lambda self: self.ref_bias5 is not None or self.ref_bias6 is not None)

    def _key_biases(self):
        return self.key_bias5, self.key_bias6, self.key_bias5_base, self.key_bias6_base

    def is_mix(self, x):
        """True where the loop on x needs the mixing attention (UNetEngine.mix_keys, or a key bias of the base, or a
        style map): 4-D maps that are stacked references, or come with a key bias or reference biases."""
        return self.s5.dim() == 4 and self.s6.dim() == 4 and (
            self.mapped or any(b is not None for b in self._key_biases()) or
            UNetEngine.mix_keys(x, self.s5, self.s6) is not None)

    def base_check(self):
        """ValueError unless the base style maps have the target's shapes (no device work, on any device)."""
        s5, s6, s5b, s6b = self.s5, self.s6, self.s5_base, self.s6_base
        if self.guided and (tuple(s5b.shape) != tuple(s5.shape) or tuple(s6b.shape) != tuple(s6.shape)):
            raise ValueError(f"guidance: the base style maps must have the target's shapes (same key counts): target "
                             f"{tuple(s5.shape)}, {tuple(s6.shape)}; base {tuple(s5b.shape)}, {tuple(s6b.shape)} "
                             "(LDM.tile_embedding repeats a single style for a mix of R references)")

    def public(self):
        """The keyword arguments of UNetEngine.ddim_loop / msolver_loop that give these options again; none for the
        plain loop, which stays the positional call."""
        kw = {}
        if self.guided:
            kw.update(base=self.prepare_operands()[4:], guidance_scale=self.scale)
        if self.z0 is not None:
            kw["keep"] = UNetEngine.KeepOperands((self.z0, self.n0, self.keep_w, self.keep_coef))
        if self.mapped:
            kw.update(ref_bias5=self.ref_bias5, ref_bias6=self.ref_bias6)
        if self.seam_cols:
            kw["seam_cols"] = self.seam_cols
        if kw or self.key_bias5 is not None or self.key_bias6 is not None:
            kw.update(key_bias5=self.key_bias5, key_bias6=self.key_bias6)
        return kw

    def check(self, engine, x, n):
        """The operands' layouts against a loop of `engine` on x (no device work; the constructor has checked the keep
        against n), and the key counts (S5, S6) and reference count they give.  RuntimeError where no kernel exists or
        an operand is not on the GPU, ValueError for the guidance's and the style map's operands."""
        B, C, H, W = x.shape
        L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
        s5, s6 = self.s5, self.s6
        if self.mapped and (self.ref_bias5 is None or self.ref_bias6 is None):
            raise ValueError("style map: ref_bias5 and ref_bias6 go together (one is None)")
        self.base_check()
        if self.guided:
            ops.require_device(self.s5_base, self.s6_base, self.scale, what="guidance operand")
            sc = self.scale
            if sc.dtype != torch.float32 or tuple(sc.shape) != (B,) or not sc.is_contiguous():
                raise ValueError(f"guidance: scale must be a contiguous fp32 [{B}] device tensor, got {sc.dtype} "
                                 f"{tuple(sc.shape)}")
        if not self.is_mix(x):
            if tuple(s5.shape) != (B, 256, H // 4, W // 4) or tuple(s6.shape) != (B, 512, H // 8, W // 8):
                raise RuntimeError(f"UNet: style maps must be s5 [B,256,H/4,W/4], s6 [B,512,H/8,W/8] for z "
                                   f"{tuple(x.shape)}; got {tuple(s5.shape)}, {tuple(s6.shape)}")
            self.S5 = self.S6 = self.refs = 0      # today's single maps: the maps' own counts
            return
        S5, S6 = s5.shape[2] * s5.shape[3], s6.shape[2] * s6.shape[3]
        if tuple(s5.shape[:2]) != (B, 256) or tuple(s6.shape[:2]) != (B, 512) or S5 % L2 or S6 % L1 or \
                S5 // L2 != S6 // L1 or s5.shape[3] != W // 4 or s6.shape[3] != W // 8:
            raise RuntimeError(f"style mix: style maps must be s5 [B,256,R*H/4,W/4], s6 [B,512,R*H/8,W/8] with one R for "
                               f"z {tuple(x.shape)}; got {tuple(s5.shape)}, {tuple(s6.shape)}")
        if not (engine.fold and engine.fold_applies(engine.shape(B, C, H, W))):
            raise RuntimeError("style mix: several style references need the folded cross-attentions (fold=True, "
                               "latent planes up to 1024 positions); the unfolded engine has no kernel for them")
        for kb, S, name in zip(self._key_biases(), (S5, S6, S5, S6), ("key_bias5", "key_bias6") * 2):
            if kb is None:
                continue
            ops.require_device(kb, what=name)
            if kb.dtype != torch.float32 or tuple(kb.shape) != (B, S) or not kb.is_contiguous():
                raise RuntimeError(f"style mix: {name} must be a contiguous fp32 [{B},{S}] tensor, got "
                                   f"{kb.dtype} {tuple(kb.shape)}")
        if self.mapped:
            UNetEngine.map_layout_check(tuple(x.shape), S5 // L2, self.ref_bias5, self.ref_bias6)
        self.S5, self.S6, self.refs = S5, S6, (S5 // L2 if self.mapped else 0)

    def check_values(self):
        """The checks that read device values on the host (skipped under capture): the style map's biases.  The keep
        weights' range is read where keep_operands() first sees them."""
        if self.mapped:
            UNetEngine.map_values_check(self.ref_bias5, self.ref_bias6)

    def _copy(self, per_sample):
        o = object.__new__(LoopOptions)
        for f in self.__slots__:
            v = getattr(self, f)
            setattr(o, f, v if v is None or f in self.SHARED else per_sample(v))
        return o

    def cut(self, lo, hi):
        """The options of samples [lo, hi): every per-sample operand sliced, the SHARED ones carried over.  A cut of a
        checked record is a checked record."""
        return self._copy(lambda v: v[lo:hi])

    def clone(self):
        """The same options on tensors of their own (GraphedDDIM's static buffers; the keep's coefficients included)."""
        o = self._copy(lambda v: v.contiguous().clone())
        o.keep_coef = None if self.keep_coef is None else self.keep_coef.clone()
        return o

    def fill(self, a):
        """Sets the option fields of the SampleArgs a: the key counts, the reference count, the seam width and every
        operand's pointer (NULL for an absent one).  Only from a checked record."""
        if self.S5 is None:
            raise RuntimeError("LoopOptions.fill: check() the options first (it derives the key counts)")
        a.S5, a.S6, a.refs, a.seam_cols = self.S5, self.S6, self.refs, self.seam_cols
        for f, arg in self.POINTERS.items():
            setattr(a, arg, ops._p(getattr(self, f)))

    def prepare_operands(self):
        """The tensors the prepare phase reads (GraphedDDIM.replay), None for an absent one: the maps, the key biases
        and the base.  Not the scale, the keep's operands or the style map: the run phase reads those."""
        return (self.s5, self.s6, self.key_bias5, self.key_bias6, self.s5_base, self.s6_base, self.key_bias5_base,
                self.key_bias6_base)


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
        self.solver = solver
        logs = logs or solver == "msolver"
        self.engine = engine
        self.split = split
        dev = x_init.device
        self.x_init = x_init.contiguous().clone()
        self.x = torch.empty_like(self.x_init)
        self.t_table = t_table.to(dev).contiguous()
        self.coef = coef_table.to(dev).contiguous()
        n = self.t_table.shape[0]
        opts = LoopOptions(self.x, n, s5, s6, key_bias5=key_bias5, key_bias6=key_bias6, base=base,
                           guidance_scale=guidance_scale, keep=keep, ref_bias5=ref_bias5, ref_bias6=ref_bias6,
                           seam_cols=seam_cols)
        if opts.seam_cols and split > 1:
            raise ValueError("GraphedDDIM: seam_cols needs split = 1 (the rows of a joint loop are not independent)")
        opts.check(engine, self.x, n)
        opts.check_values()
        self.opts = opts.clone()      # the static buffers of every operand: the captured loops read these
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

    s5, s6 = property(lambda self: self.opts.s5), property(lambda self: self.opts.s6)
    kb5, kb6 = property(lambda self: self.opts.key_bias5), property(lambda self: self.opts.key_bias6)

    def _chain_call(self, k, lo, hi, t_sub, phase):
        """One phase (ldm_sample_prepare / ldm_sample_run) of chain k on its own workspace."""
        split, B = bool(self.plan), self.x.shape[0]
        x0l = None if self.x0_logs is None else (self.x0_logs[0, lo:hi] if split else self.x0_logs)
        epl = None if self.eps_logs is None else (self.eps_logs[0, lo:hi] if split else self.eps_logs)
        self.engine._sample_call(self.solver, self.x[lo:hi], self.opts.cut(lo, hi), t_sub, self.coef, self.eta, x0l, epl,
                                 self.x[0].numel() * B if split else 0, self._slot + (k,),
                                 B if (split and self.opts.guided) else None, phase)

    def prepared_key(self, weight_version=None):
        """prepared_key of the static buffers and the engine's weights as they stand (host only, no device work)."""
        wv = self.engine.weight_version() if weight_version is None else weight_version
        return prepared_key(self.opts.prepare_operands() + (self.t_table,), wv)

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
        scale = self.opts.scale
        if scale is None:
            raise ValueError("set_guidance_scale: this loop was captured without a base style")
        scale.copy_(self.engine.guidance_scale(guidance_scale, scale.shape[0]), non_blocking=False)

    def set_keep(self, w):
        """Writes new keep weights ([B,H,W] in [0,1]) into the static buffer the captured loop reads: the next replay
        runs under the new mask.  Only for a graph captured with keep=."""
        o = self.opts
        if o.keep_w is None:
            raise ValueError("set_keep: this loop was captured without keep=")
        kp = self.engine.keep_operands((o.z0, o.n0, w, o.keep_coef), self.x.shape, o.keep_coef.shape[0], self.x.device)
        o.keep_w.copy_(kp[2], non_blocking=False)

    def set_style_map(self, ref_bias5, ref_bias6):
        """Writes a new style map (UNetEngine.ddim_loop's ref_bias5 / ref_bias6) into the static buffers the captured
        loop reads: the next replay runs under it.  No new capture and no prepare launch: the biases are not among the
        prepare phase's operands.  Only for a graph captured with a style map."""
        o = self.opts
        if not o.mapped:
            raise ValueError("set_style_map: this loop was captured without a style map (ref_bias5= / ref_bias6=)")
        self.engine.map_layout_check(tuple(self.x.shape), o.refs, ref_bias5, ref_bias6)
        self.engine.map_values_check(ref_bias5, ref_bias6)
        o.ref_bias5.copy_(ref_bias5, non_blocking=False)
        o.ref_bias6.copy_(ref_bias6, non_blocking=False)

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
