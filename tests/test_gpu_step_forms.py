"""The step-kernel instances that the LDM_UCONV_* variables select (csrc/uconv.hip), each against float64.

The variables are read once per process, so every case starts one fresh child process with the setting in its
environment.  The child first asserts through ldm_step_layer_forms that the setting took effect (where the mask of
K-split layers shows it), then runs, at the latent shapes (3, 16, 64) and (3, 8, 24):
  * layers 0..7 through ldm_step_conv_ws on a zeroed workspace: the comparison of
    test_gpu_step_kernels.py::test_step_layer_vs_float64 (step_ref.check_step_layer, rel_err < 1e-5);
  * dec1 through ldm_step_dec1_ddim and ldm_step_dec1_msolver: the float64 updates and the 1e-5 bounds of
    test_gpu_bench_config.py (DDIM, eta 0.3) and test_gpu_solver.py (a second-order row, with and without history).
(3, 16, 64) is the canonical plane that variant 3, EPI_PLANE and the 64-column windows need, B = 3 leaving the 32- and
64-column N tiles of the deeper layers ragged; (3, 8, 24) takes every non-window, non-plane fallback.
The fp16 case (LDM_UCONV_KS_LOWP=0: the bottleneck's single-block form under 16-bit operands) runs layer 4 only,
against float64 of the fp16-rounded operands rounded where the kernel rounds, to test_gpu_amp.py's fp16 bound 1e-3
(one fp16 ulp of a value that lands on a rounding boundary is 4.9e-4 of it).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 64), (3, 8, 24)]
DEC1_TOL = 1e-5          # test_gpu_bench_config.py / test_gpu_solver.py (UPD_TOL)
FP16_TOL = 1e-3          # test_gpu_amp.py TOLS["fp16"]
_SINGLE = {"LDM_UCONV_KS3": "0", "LDM_UCONV_KS": "0"}

# id: (environment, expected ldm_step_layer_forms mask, fp16 bottleneck only)
SETTINGS = {
    "defaults": ({}, 0x10, False),
    "ks3_off": ({"LDM_UCONV_KS3": "0"}, 0x38, False),
    "variant1": ({"LDM_UCONV_KS3": "0", "LDM_UCONV_KS2": "0"}, 0x38, False),
    "every_split_row": ({"LDM_UCONV_KS3": "0", "LDM_UCONV_KS": "0x7c", "LDM_UCONV_KS2": "0x38"}, 0x7c, False),
    "single_block": (_SINGLE, 0, False),
    "single_block_no_window_no_plane": (dict(_SINGLE, LDM_UCONV_WINDOW="0", LDM_UCONV_PLANE="0"), 0, False),
    "single_block_dec1_32row": (dict(_SINGLE, LDM_UCONV_DEC1_THIN="0"), 0, False),
    "single_block_enc2_wide_enc3_thin": (dict(_SINGLE, LDM_UCONV_ENC2_WIDE="1", LDM_UCONV_ENC3_THIN="1"), 0, False),
    "xcd_off": ({"LDM_UCONV_XCD": "0"}, 0x10, False),
    "ks_lowp_off_fp16": ({"LDM_UCONV_KS_LOWP": "0"}, 0x10, True),
}


def _dec1(cuda, shape):
    """dec1 with its fused DDIM and multistep updates against float64."""
    import torch
    import torch.nn.functional as F

    import models.model as M
    import solver_ref as SR
    from conftest import rel_err
    from ldm_amd import _lib as L
    from step_ref import npy
    B, H, W = shape
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(78 + H)
    w = torch.randn(32, 64, 3, 3, generator=g) / (64 * 9) ** 0.5
    bias = torch.randn(32, generator=g) * 0.1
    d2 = torch.randn(B, 64, H, W, generator=g)
    xs = torch.randn(B, 32, H, W, generator=g)
    prev = torch.randn(B, 32, H, W, generator=g)
    packed = torch.empty(int(lib.ldm_step_packed_floats(8)), device=cuda)
    L.call("ldm_step_pack_weight", 8, w.to(cuda).contiguous().data_ptr(), packed.data_ptr(), st)
    bd = bias.to(cuda)
    d2d = d2.permute(0, 2, 3, 1).contiguous().to(cuda)
    eps = F.conv2d(d2.double(), w.double(), bias.double(), padding=1)

    def fresh():
        xsd = xs.permute(0, 2, 3, 1).contiguous().to(cuda)
        x0l = torch.full((B, 32, H, W), float("nan"), device=cuda)
        return xsd, x0l, torch.full_like(x0l, float("nan"))

    # the fused DDIM update (model.py:442-463) with both logs
    coef = torch.tensor([0.6, 0.8, 0.7, 0.71414284], dtype=torch.float32)
    xsd, x0l, epl = fresh()
    L.call("ldm_step_dec1_ddim", B, H, W, d2d.data_ptr(), packed.data_ptr(), bd.data_ptr(), coef.to(cuda).data_ptr(),
           0.3, xsd.data_ptr(), x0l.data_ptr(), epl.data_ptr(), 0, st)
    torch.cuda.synchronize()
    c = coef.double()
    x0 = (xs.double() - c[1] * eps) / c[0]
    xn = c[2] * x0 + c[3] * eps + 0.3 * (c[3] * eps - c[1] * eps)
    errs = (rel_err(npy(epl), eps.numpy()), rel_err(npy(x0l), x0.numpy()),
            rel_err(npy(xsd.permute(0, 3, 1, 2)), xn.numpy()))
    print(f"dec1 ddim {shape}: eps {errs[0]:.2e}, x0 {errs[1]:.2e}, x {errs[2]:.2e}")
    assert max(errs) < DEC1_TOL
    # the multistep update: a second-order row, with and without the history
    row = M.ForwardDiffusion().multistep_coefs(SR.sample_times(99, 10))[4].contiguous()
    assert float(row[4]) != 0.0
    c = row.double().cpu().numpy()
    for with_prev in (True, False):
        xsd, x0l, epl = fresh()
        pd = prev.to(cuda) if with_prev else None
        L.call("ldm_step_dec1_msolver", B, H, W, d2d.data_ptr(), packed.data_ptr(), bd.data_ptr(),
               row.to(cuda).data_ptr(), xsd.data_ptr(), None if pd is None else pd.data_ptr(), x0l.data_ptr(),
               epl.data_ptr(), 0, st)
        torch.cuda.synchronize()
        x0 = (npy(xs) - c[1] * eps.numpy()) / c[0]
        xn = c[2] * npy(xs) + c[3] * x0 + (c[4] * npy(prev) if with_prev else 0.0)
        errs = (rel_err(npy(epl), eps.numpy()), rel_err(npy(x0l), x0), rel_err(npy(xsd.permute(0, 3, 1, 2)), xn))
        print(f"dec1 msolver {shape} with_prev {with_prev}: eps {errs[0]:.2e}, x0 {errs[1]:.2e}, x {errs[2]:.2e}")
        assert max(errs) <= DEC1_TOL


def child(name):
    """Runs in the child process, the setting already in its environment."""
    import torch

    from ldm_amd import _lib as L
    from step_ref import check_step_layer
    env, mask, fp16 = SETTINGS[name]
    assert all(os.environ.get(k) == v for k, v in env.items())
    assert L.step_layer_forms() == mask, hex(L.step_layer_forms())
    cuda = torch.device("cuda:0")
    for shape in SHAPES:
        if fp16:
            check_step_layer(cuda, "ksplit", 4, shape, dtype=1, tol=FP16_TOL)
            continue
        for layer in range(8):
            check_step_layer(cuda, "ksplit", layer, shape)
        _dec1(cuda, shape)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_step_form_vs_float64(cuda, name):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import conftest, test_gpu_step_forms as t; t.child(%r)" % (here, name))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDM_UCONV_")}
    env.update(SETTINGS[name][0])
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=here, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
