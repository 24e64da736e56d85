"""Argument marshalling of the reverse loop's kernels (csrc/uconv_kernel.h: the head record UHead passed as plain
leading parameters in front of UArgs; csrc/bfold.hip and the folded attention, whose plain parameters are preloaded).

A field in the wrong slot, or the shift decode of the block order used at a shape it does not fit, gives wrong numbers
at once, so every case is the comparison the existing tests make, at the smallest shapes that reach every form:
  * (1, 16, 64) and (3, 16, 64): the canonical latent's window and plane forms; B = 3 leaves the plane layers' Nq no
    multiple of the block's columns (the cval / out-of-range path) and some tile counts no multiple of 8 (the general
    decode next to the XCD-grid one);
  * (2, 16, 16): the register-direct forms the window and plane forms do not take.
Step layers: step_ref.check_step_layer (float64, rel_err < 1e-5, run twice bitwise).  Stale slots: a layer's output
is bitwise what it was after a call at another shape.  Loop: captured == eager bitwise at B = 1, three steps, both
logs, for the plain, guided and keep instances of dec1.  ca1_probs / bneck_pv / attention_folded: float64 of
test_gpu_bfold.py's operands, its bound 1e-5.
"""
import ctypes

import pytest
import torch

import recipe
from conftest import rel_err
from step_ref import DIV, LAYERS, check_step_layer
from test_gpu_bfold import _operands, _ptr, _reference64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 64), (3, 16, 64), (2, 16, 16)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layer", range(8))
def test_step_layer_vs_float64(cuda, layer, shape):
    check_step_layer(cuda, "ksplit", layer, shape)


def _layer_call(cuda, layer, shape, seed):
    """One ldm_step_conv_ws call on fixed random operands; returns a closure that reruns it into a fresh y."""
    from ldm_amd import _lib as L
    B, H, W = shape
    Cin, Cout, mode = LAYERS[layer]
    Hin, Win = H // DIV[layer], W // DIV[layer]
    Hout, Wout = (Hin, Win) if mode == 0 else ((Hin // 2, Win // 2) if mode == 1 else (2 * Hin, 2 * Win))
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hin, Win, Cin, generator=g).to(cuda)
    w = (torch.randn((Cin, Cout, 3, 3) if mode == 2 else (Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5).to(cuda)
    packed = torch.empty(int(lib.ldm_step_packed_floats(layer)), device=cuda)
    L.call("ldm_step_pack_weight", layer, w.data_ptr(), packed.data_ptr(), st)
    bias = (torch.randn((Hout * Wout * Cout) if layer in (3, 4) else Cout, generator=g) * 0.1).to(cuda)
    bc = torch.randn(B, Cout, generator=g).to(cuda)
    sk = torch.randn(B, Hout, Wout, Cout, generator=g).to(cuda)
    ws = torch.zeros(int(lib.ldm_step_workspace_floats(B, H, W)), device=cuda)
    keep = (x, w, packed, bias, bc, sk, ws)

    def run():
        y = torch.full((B, Hout, Wout, Cout), float("nan"), device=cuda)
        L.call("ldm_step_conv_ws", layer, B, H, W, x.data_ptr(), packed.data_ptr(), bias.data_ptr(),
               bc.data_ptr() if layer == 1 else None, sk.data_ptr() if mode == 2 else None, y.data_ptr(), 0,
               ws.data_ptr(), st)
        torch.cuda.synchronize()
        assert keep is not None and not torch.isnan(y).any()
        return y
    return run


@pytest.mark.parametrize("layer", range(8))
def test_no_stale_argument_slots(cuda, layer):
    """Every launch carries its own head record: a layer's result at one shape is bitwise the same after launches of
    the same layer at the two other shapes (another block order, other divisors, other tile counts)."""
    runs = [_layer_call(cuda, layer, s, 900 + 10 * layer + i) for i, s in enumerate(SHAPES)]
    first = [r() for r in runs]
    for i, r in enumerate(runs):
        assert torch.equal(r(), first[i])            # twice
    for i in (2, 0, 1):                              # and once more, each after a call at a different shape
        assert torch.equal(runs[i](), first[i])


@pytest.fixture(scope="module")
def loop_ctx(cuda):
    import models.model as M
    unet = M.UNet(32, 32, 64)
    recipe.fill_module(unet, seed=100)
    unet = unet.to(cuda)
    fd = M.ForwardDiffusion(200)
    times = torch.linspace(199, 0, 4).long()          # three steps
    B, H, W = 1, 16, 64
    g = torch.Generator().manual_seed(17)
    d = dict(x=torch.randn(B, 32, H, W, generator=g), z0=torch.randn(B, 32, H, W, generator=g),
             n0=torch.randn(B, 32, H, W, generator=g), w=torch.rand(B, H, W, generator=g).round(),
             s5=torch.rand(B, 256, H // 4, W // 4, generator=g), s6=torch.rand(B, 512, H // 8, W // 8, generator=g),
             b5=torch.rand(B, 256, H // 4, W // 4, generator=g), b6=torch.rand(B, 512, H // 8, W // 8, generator=g))
    d = {k: v.to(cuda) for k, v in d.items()}
    return dict(M=M, unet=unet, fd=fd, times=times, d=d,
                t_table=times[:-1].view(-1, 1).expand(-1, B).contiguous().to(cuda))


@pytest.mark.parametrize("solver", ["ddim", "msolver"])
@pytest.mark.parametrize("form", ["plain", "guided", "keep", "guided_keep"])
def test_captured_loop_equals_eager_bitwise(loop_ctx, cuda, form, solver):
    """dec1's instances in uconv.hip, uconv_guide.hip and uconv_keep.hip take the head record too."""
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    c, d = loop_ctx, loop_ctx["d"]
    fd, times, t_table = c["fd"], c["times"], c["t_table"]
    coef = (fd.reverse_coefs(times) if solver == "ddim" else fd.multistep_coefs(times)).to(cuda)
    eta = 0.3 if solver == "ddim" else 0.0
    kw = {}
    if "guided" in form:
        kw.update(base=(d["b5"], d["b6"], None, None), guidance_scale=2.5)
    if "keep" in form:
        kw.update(keep=(d["z0"], d["n0"], d["w"], fd.keep_coefs(times)))
    eng = UNetEngine(c["unet"])
    n = t_table.shape[0]
    with torch.no_grad():
        x = d["x"].clone()
        x0l = torch.full((n,) + tuple(x.shape), float("nan"), device=cuda)
        epl = torch.full_like(x0l, float("nan"))
        if solver == "ddim":
            eng.ddim_loop(x, d["s5"], d["s6"], t_table, coef, eta, x0l, epl, **kw)
        else:
            eng.msolver_loop(x, d["s5"], d["s6"], t_table, coef, x0l, epl, **kw)
        gd = GraphedDDIM(eng, d["x"], d["s5"], d["s6"], t_table, coef, eta, logs=True, solver=solver, **kw)
        r = gd.replay().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.isfinite(x0l).all() and torch.isfinite(epl).all()
    assert torch.equal(r, x) and torch.equal(gd.x0_logs, x0l) and torch.equal(gd.eps_logs, epl)


@pytest.mark.parametrize("B", [1, 3])
def test_other_loop_kernels_vs_float64(cuda, B):
    """ca1_probs_kernel, bneck_pv_kernel and the folded attention (CA1's instance) against float64 of the literal
    order on test_gpu_bfold.py's operands."""
    from ldm_amd import _lib as L
    ops = _operands(B, 500 + B)
    p64, y64 = _reference64(*ops)
    v64 = ops[3].double()[:, 512:, :].reshape(B, 4, 128, 16)
    a64 = torch.einsum("bhls,bhds->blhd", p64, v64).reshape(B, 16, 512)
    z4, kf, bf, kv, wf, pb = (t.to(cuda).contiguous() for t in ops)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = torch.full((B, 4, 16, 16), float("nan"), device=cuda)
    u = torch.empty(B, 512, 576, device=cuda)
    y = torch.full((B, 16, 512), float("nan"), device=cuda)
    a = torch.full((B, 16, 512), float("nan"), device=cuda)
    L.call("ldm_ca1_probs", _ptr(z4), _ptr(kf), _ptr(bf), _ptr(p), B, st)
    L.call("ldm_bneck_fold_values", _ptr(wf), _ptr(kv), _ptr(u), B, st)
    L.call("ldm_bneck_pv", _ptr(u), _ptr(p), _ptr(pb), _ptr(y), B, 0, st)
    L.call("ldm_attention_folded", _ptr(z4), _ptr(kv), _ptr(kf), _ptr(bf), _ptr(a), B, 512, 4, 16, 16, st)
    torch.cuda.synchronize()
    errs = (rel_err(p.cpu().numpy(), p64.numpy()), rel_err(y.cpu().numpy(), y64.numpy()),
            rel_err(a.cpu().numpy(), a64.numpy()))
    print(f"B={B}: probs {errs[0]:.2e}, bottleneck {errs[1]:.2e}, attention {errs[2]:.2e}")
    assert max(errs) < 1e-5


@pytest.mark.parametrize("B", [1, 3])
def test_loop_attention_ca2_vs_float64(cuda, B):
    """The loop's second cross-attention (E 256, 64 queries x 64 keys on the 4 x 16 plane), whose instance differs from
    CA1's: float64 of the same literal order, the same bound."""
    from ldm_amd import _lib as L
    E, H, Lq, S = 256, 4, 64, 64
    g = torch.Generator().manual_seed(700 + B)
    z = torch.rand(B, Lq, E, generator=g)
    kf = torch.randn(B, H, S, E, generator=g) * 0.05
    bf = torch.randn(B, H, S, generator=g) * 0.1
    kv = torch.randn(B, 2 * E, S, generator=g)
    p64 = torch.softmax(torch.einsum("ble,bhse->bhls", z.double(), kf.double()) + bf.double()[:, :, None, :], dim=-1)
    a64 = torch.einsum("bhls,bhds->blhd", p64, kv.double()[:, E:, :].reshape(B, H, E // H, S)).reshape(B, Lq, E)
    zd, kfd, bfd, kvd = (t.to(cuda).contiguous() for t in (z, kf, bf, kv))
    out = torch.full((B, Lq, E), float("nan"), device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.call("ldm_attention_folded", _ptr(zd), _ptr(kvd), _ptr(kfd), _ptr(bfd), _ptr(out), B, E, H, Lq, S, st)
    torch.cuda.synchronize()
    err = rel_err(out.cpu().numpy(), a64.numpy())
    print(f"B={B}: CA2 attention {err:.2e}")
    assert err < 1e-5
