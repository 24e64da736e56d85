"""dec4 of the reverse loop on its tap-class form (uconv.hip, kTapClass): at the canonical 16 x 64 latent the wide
instance is split over two blocks per tile by output parity, not by K.  One block carries the four taps of parity
(odd, odd), the other the five taps of the remaining three parities, each over all 512 input channels, so every
output element is finished and written by exactly one block and nothing passes through the split-K workspace.

dec4: ConvTranspose2d(512, 256, k3, s2, p1, op1) + bias, ReLU, + skip; input [B, 2, 8, 512] NHWC, output and skip
[B, 4, 16, 256] NHWC.  B = 1 is one column of tiles, B = 3 an odd count of them; every sample's plane has the edge
rows / columns whose taps fall outside it.

Tolerance: max-norm relative 1e-5 against float64, as test_gpu_bench_config.py holds every step layer to.
  * fp32 operands: seeded normal inputs.
  * fp16 / bf16 operands: the kernel rounds the conv output (+ bias) and the skip add to the 16-bit type (the
    autocast semantics, test_gpu_amp.py), so a float64 reference has to round at the same two places, and a sum that
    lands within fp32 accumulation noise of a rounding boundary would flip by a whole 16-bit ulp (1e-3 of the value),
    which says nothing about the kernel.  The 16-bit cases therefore draw seeded inputs from dyadic grids (x in
    1/4 steps up to 2, weights in 1/8 steps up to 1, bias and skip in 1/32 steps): every product and every partial
    sum (at most 2048 terms, |sum| <= 4096, multiples of 1/32: 17 bits) is exact in fp32 in any order, both
    roundings see the exact value, and the same 1e-5 bound holds (a wrong tap, channel, parity or offset still moves
    an output by whole grid steps).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
H, W = 16, 64
CIN, COUT = 512, 256
DTS = {"fp32": 0, "fp16": 1, "bf16": 2}


def _inputs(B, name):
    """Seeded operands of dec4 (torch layouts, CPU fp32): x, w [CIN, COUT, 3, 3], bias, skip."""
    g = torch.Generator().manual_seed(500 + 10 * B + DTS[name])
    if name == "fp32":
        x = torch.randn(B, CIN, 2, 8, generator=g)
        w = torch.randn(CIN, COUT, 3, 3, generator=g) / (CIN * 9) ** 0.5
        bias = torch.randn(COUT, generator=g) * 0.1
        sk = torch.randn(B, COUT, 4, 16, generator=g)
    else:
        grid = lambda shape, n, step: torch.randint(-n, n + 1, shape, generator=g).float() * step
        x = grid((B, CIN, 2, 8), 8, 0.25)
        w = grid((CIN, COUT, 3, 3), 8, 0.125)
        bias = grid((COUT,), 32, 1 / 32)
        sk = grid((B, COUT, 4, 16), 128, 1 / 32)
    return x, w, bias, sk


def _reference(x, w, bias, sk, name):
    rnd = {"fp32": lambda t: t, "fp16": lambda t: t.half().double(), "bf16": lambda t: t.bfloat16().double()}[name]
    ref = F.conv_transpose2d(rnd(x.double()), rnd(w.double()), stride=2, padding=1, output_padding=1)
    ref = rnd(ref + bias.double()[None, :, None, None]).clamp_min(0)
    return rnd(ref + sk.double()).numpy()


def _run(B, name, ws_fill=0.0, launches=1):
    """dec4 through ldm_step_conv_ws on NaN-filled outputs; returns the outputs (NCHW, numpy) of each launch."""
    from ldm_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    dt = DTS[name]
    x, w, bias, sk = _inputs(B, name)
    packed = torch.empty(int(lib.ldm_step_packed_floats(5)), device=dev)
    L.call("ldm_step_pack_weight_dt", 5, dt, w.to(dev).contiguous().data_ptr(), packed.data_ptr(), st)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    skd = sk.permute(0, 2, 3, 1).contiguous().to(dev)
    bd = bias.to(dev)
    ws = torch.full((int(lib.ldm_step_workspace_floats(B, H, W)),), ws_fill, device=dev)
    outs = []
    for _ in range(launches):
        y = torch.full((B, 4, 16, COUT), float("nan"), device=dev)
        L.call("ldm_step_conv_ws", 5, B, H, W, xd.data_ptr(), packed.data_ptr(), bd.data_ptr(), None, skd.data_ptr(),
               y.data_ptr(), dt, ws.data_ptr(), st)
        torch.cuda.synchronize()
        outs.append(y.permute(0, 3, 1, 2).contiguous().cpu().numpy())
    return outs


def _parity_form_active():
    from ldm_amd import _lib as L
    return (L.step_layer_forms() >> 5) & 1 == 0     # dec4 not on a K-split form


@pytest.fixture(scope="module")
def runs(cuda):
    """Two launches per case on the same buffers, computed once and shared (never modified)."""
    assert _parity_form_active(), "dec4 is expected on its tap-class form by default"
    return {(B, name): _run(B, name, launches=2) for B in (1, 3) for name in DTS}


@pytest.mark.parametrize("name", list(DTS))
@pytest.mark.parametrize("B", [1, 3])
def test_dec4_parity_matches_float64(runs, B, name):
    got = runs[(B, name)][0]
    err = rel_err(got, _reference(*_inputs(B, name), name))
    print(f"dec4 tap-class form B={B} {name}: rel_err {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("name", list(DTS))
@pytest.mark.parametrize("B", [1, 3])
def test_dec4_parity_every_output_written_once(runs, B, name):
    """y starts as NaN: none may remain (each parity has an owner), and a second launch on the same buffers is
    bitwise equal (nothing accumulates into y or depends on what an earlier launch left behind)."""
    first, second = runs[(B, name)]
    assert not np.isnan(first).any()
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


@pytest.mark.parametrize("name", list(DTS))
def test_dec4_parity_ignores_the_workspace(runs, name):
    """Slabs and arrival counters filled with garbage: bitwise the result of the zeroed workspace."""
    got = _run(3, name, ws_fill=-1.7e38)[0]           # (as int32 counters: a large negative number)
    assert np.array_equal(got.view(np.uint32), runs[(3, name)][0].view(np.uint32))


def test_dec4_switch_restores_k_split(runs):
    """LDM_UCONV_DEC4_PAR=0 (read once per process, so in a child): the K-split instance, within the same bound of
    float64 and hence of the tap-class form; not bitwise, the two sum the K halves in different orders."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import conftest, test_gpu_dec4_parity as t; "
            "from ldm_amd import _lib as L; assert (L.step_layer_forms() >> 5) & 1 == 1; "
            "np.save(sys.argv[1], t._run(3, 'fp32')[0])" % here)
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"dec4_ksplit_{os.getpid()}.npy")
    env = dict(os.environ, LDM_UCONV_DEC4_PAR="0")
    r = subprocess.run([sys.executable, "-c", code, out], env=env, cwd=here, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    ksplit = np.load(out)
    os.remove(out)
    ref = _reference(*_inputs(3, "fp32"), "fp32")
    e_ks, e_par = rel_err(ksplit, ref), rel_err(runs[(3, "fp32")][0], ref)
    print(f"dec4 B=3 fp32: K-split {e_ks:.3e}, tap-class {e_par:.3e}, between them {rel_err(ksplit, runs[(3, 'fp32')][0]):.3e}")
    assert e_ks < TOL and e_par < TOL
