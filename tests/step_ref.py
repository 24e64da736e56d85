"""One step layer (csrc/uconv.hip) against float64 torch: the comparison test_gpu_step_kernels.py and
test_gpu_step_forms.py share.  Reference: model.py:178-194 (layers), :205-229 (epilogue order: ReLU, then + t_emb /
+ skip)."""
import torch
import torch.nn.functional as F

from conftest import rel_err

# (Cin, Cout, mode) of the nine layers; mode 0 conv s1, 1 conv s2, 2 convT k3 s2 p1 op1
LAYERS = [(32, 64, 0), (64, 128, 1), (128, 256, 1), (256, 512, 1), (512, 512, 0), (512, 256, 2), (256, 128, 2),
          (128, 64, 2), (64, 32, 0)]
DIV = [1, 1, 2, 4, 8, 8, 4, 2, 1]
LAYER_TOL = 1e-5


def npy(t):
    return t.detach().double().cpu().numpy()


def check_step_layer(cuda, variant, layer, shape, dtype=0, tol=LAYER_TOL):
    """uconv: ldm_step_conv (register-direct, any latent with H, W multiples of 8); ksplit: ldm_step_conv_ws
    (the forms the LDM_UCONV_* variables select, on a zeroed workspace).  The workspace form runs twice on one
    workspace: bitwise-equal results (the split-K sum is in slot order) and the counters left zero.
    dtype 1 (fp16 operands): the float64 reference takes the operands rounded to fp16 and rounds where the kernel
    does (the conv output + bias, then each add), as the autocast convs of the reference return 16-bit tensors."""
    from ldm_amd import _lib as L
    B, H, W = shape
    Cin, Cout, mode = LAYERS[layer]
    Hin, Win = H // DIV[layer], W // DIV[layer]
    Hout, Wout = (Hin, Win) if mode == 0 else ((Hin // 2, Win // 2) if mode == 1 else (2 * Hin, 2 * Win))
    g = torch.Generator().manual_seed(100 * layer + B)
    x = torch.randn(B, Cin, Hin, Win, generator=g)
    wshape = (Cin, Cout, 3, 3) if mode == 2 else (Cout, Cin, 3, 3)
    w = torch.randn(wshape, generator=g) * (1.0 / (Cin * 9) ** 0.5)
    posb = layer in (3, 4)
    bias = torch.randn((Hout, Wout, Cout) if posb else (Cout,), generator=g) * 0.1
    bc = torch.randn(B, Cout, generator=g) if layer == 1 else None
    sk = torch.randn(B, Cout, Hout, Wout, generator=g) if mode == 2 else None
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(int(lib.ldm_step_packed_floats(layer)), device=cuda)
    wd = w.to(cuda).contiguous()
    if dtype == 0:
        L.call("ldm_step_pack_weight", layer, wd.data_ptr(), packed.data_ptr(), st)
    else:
        L.call("ldm_step_pack_weight_dt", layer, dtype, wd.data_ptr(), packed.data_ptr(), st)
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    y = torch.full((B, Hout, Wout, Cout), float("nan"), device=cuda)
    bd = bias.contiguous().to(cuda)
    bcd = bc.to(cuda) if bc is not None else None
    skd = sk.permute(0, 2, 3, 1).contiguous().to(cuda) if sk is not None else None
    bcp = None if bcd is None else bcd.data_ptr()
    skp = None if skd is None else skd.data_ptr()
    if variant == "uconv" and dtype == 0:
        L.call("ldm_step_conv", layer, B, H, W, xd.data_ptr(), packed.data_ptr(), bd.data_ptr(), bcp, skp,
               y.data_ptr(), st)
    elif variant == "uconv":
        L.call("ldm_step_conv_dt", layer, B, H, W, xd.data_ptr(), packed.data_ptr(), bd.data_ptr(), bcp, skp,
               y.data_ptr(), dtype, st)
    elif variant == "ksplit":   # the K-split form (32x32 tiles, K over 2-8 blocks, last arriver sums)
        nws = int(lib.ldm_step_workspace_floats(B, H, W))
        assert nws > 0
        ws = torch.zeros(nws, device=cuda)
        for yy in (y, y2 := torch.full_like(y, float("nan"))):
            L.call("ldm_step_conv_ws", layer, B, H, W, xd.data_ptr(), packed.data_ptr(), bd.data_ptr(), bcp, skp,
                   yy.data_ptr(), dtype, ws.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(y, y2)
        ncnt = int(lib.ldm_step_workspace_counter_floats(B, H, W))
        assert 64 <= ncnt < nws
        # every tile counter is back to zero
        assert int(ws[:ncnt].view(torch.int32).abs().sum()) == 0
    else:
        raise ValueError(variant)
    torch.cuda.synchronize()
    rnd = (lambda t: t.half().double()) if dtype == 1 else (lambda t: t)
    x64, w64 = rnd(x.double()), rnd(w.double())
    if mode == 2:
        ref = F.conv_transpose2d(x64, w64, None, stride=2, padding=1, output_padding=1)
    else:
        ref = F.conv2d(x64, w64, None, stride=1 if mode == 0 else 2, padding=1)
    ref = rnd(ref + (bias.double().permute(2, 0, 1)[None] if posb else bias.double()[None, :, None, None]))
    ref = ref.clamp_min(0)
    if bc is not None:
        ref = rnd(ref + bc.double()[:, :, None, None])
    if sk is not None:
        ref = rnd(ref + sk.double())
    got = y.permute(0, 3, 1, 2)
    err = rel_err(npy(got), ref.numpy())
    print(f"layer {layer} {variant} {shape} dtype {dtype}: rel_err {err:.2e}")
    assert err < tol
