"""GPU: style mixing, from the key-tiled folded attention (csrc/stylemix.hip) up to transfer_recording, against the
float64 yardstick tests/stylemix_ref.py (weighted sums of exponentials, written from the definition).

Bars: 1e-5 relative for the attention alone (what tests/test_gpu_fold.py holds ldm_attention_folded to against
float64), PARITY_TOL = 1e-4 for a loop's final x against the yardstick and UPD_TOL = 1e-5 for the float64 replay of
the coefficient table from the logged eps (tests/test_gpu_solver.py's)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR       # noqa: E402
import solver_ref as SR      # noqa: E402
import stylemix_ref as MR    # noqa: E402

pytestmark = pytest.mark.gpu
ATT_TOL, UPD_TOL, PARITY_TOL = 1e-5, 1e-5, 1e-4
NEG = float("-inf")


def npy(t):
    return t.detach().double().cpu().numpy()


# ---- the kernel alone ------------------------------------------------------------------------------------------------
def att_inputs(B, E, L, S):
    g = torch.Generator().manual_seed(7 * E + 13 * L + S)
    z = torch.randn(B, L, E, generator=g)
    kv = torch.randn(B, 2 * E, S, generator=g)
    wq = torch.randn(E, E, generator=g) / E ** 0.5
    bq = torch.randn(E, generator=g) * 0.1
    bias = torch.randn(B, S, generator=g)
    return z, kv, wq, bq, bias


def att_ref(z, kv, wq, bq, kw, keep=None):
    """float64: the unfolded attention with per-key weights kw [B,S] (None: all 1); keep: key indices kept."""
    B, L, E = z.shape
    heads, d = 4, E // 4
    q = (torch.einsum("oe,ble->blo", wq.double(), z.double()) + bq.double()) * float(np.sqrt(1.0 / d))
    qh = q.view(B, L, heads, d).permute(0, 2, 1, 3)
    K = kv.double()[:, :E].reshape(B, heads, d, -1).permute(0, 1, 3, 2)
    V = kv.double()[:, E:].reshape(B, heads, d, -1).permute(0, 1, 3, 2)
    if keep is not None:
        K, V = K[:, :, keep], V[:, :, keep]
        kw = None if kw is None else kw[:, keep]
    return MR.attention(qh, K, V, kw).permute(0, 2, 1, 3).reshape(B, L, E)


def run_att(cuda, z, kv, wq, bq, bias, fold_bias=False):
    """fold the keys, then ldm_attention_folded_keys; fold_bias: the bias goes into bf at the fold instead."""
    from ldm_amd import _lib as L_
    B, L, E = z.shape
    S, heads = kv.shape[2], 4
    st = torch.cuda.current_stream().cuda_stream
    zd, kvd, wqd, bqd = z.to(cuda), kv.to(cuda), wq.to(cuda), bq.to(cuda)
    bd = None if bias is None else bias.to(cuda).contiguous()
    kf = torch.empty((B, heads, S, E), device=cuda)
    bf = torch.empty((B, heads, S), device=cuda)
    out = torch.full((B, L, E), float("nan"), device=cuda)
    scale = float(np.sqrt(1.0 / (E // heads)))
    if fold_bias:
        L_.call("ldm_attention_fold_keys_bias", kvd.data_ptr(), wqd.data_ptr(), bqd.data_ptr(), B, E, heads, S, scale,
                None if bd is None else bd.data_ptr(), kf.data_ptr(), bf.data_ptr(), st)
        arg = None
    else:
        L_.call("ldm_attention_fold_keys", kvd.data_ptr(), wqd.data_ptr(), bqd.data_ptr(), B, E, heads, S, scale,
                kf.data_ptr(), bf.data_ptr(), st)
        arg = None if bd is None else bd.data_ptr()
    L_.call("ldm_attention_folded_keys", zd.data_ptr(), kvd.data_ptr(), kf.data_ptr(), bf.data_ptr(), arg,
            out.data_ptr(), B, E, heads, L, S, st)
    torch.cuda.synchronize()
    return out


ATT_CASES = [(512, 16, 16), (512, 16, 17), (512, 16, 48), (512, 16, 128), (512, 1, 3),
             (256, 64, 64), (256, 64, 65), (256, 64, 192), (256, 64, 512), (256, 4, 12)]


@pytest.mark.parametrize("E,L,S", ATT_CASES)
def test_tiled_attention_vs_float64(cuda, E, L, S):
    B = 2
    z, kv, wq, bq, bias = att_inputs(B, E, L, S)
    # NULL bias
    e0 = rel_err(npy(run_att(cuda, z, kv, wq, bq, None)), att_ref(z, kv, wq, bq, None).numpy())
    # a random finite bias
    e1 = rel_err(npy(run_att(cuda, z, kv, wq, bq, bias)), att_ref(z, kv, wq, bq, torch.exp(bias.double())).numpy())
    # the whole first reference run -inf for sample 1 only (S == L: its first half, so that a key is left)
    run = L if S > L else S // 2
    masked = bias.clone()
    masked[1, :run] = NEG
    out = run_att(cuda, z, kv, wq, bq, masked)
    assert bool(torch.isfinite(out).all())
    e2 = rel_err(npy(out), att_ref(z, kv, wq, bq, torch.exp(masked.double())).numpy())
    gone = att_ref(z[1:], kv[1:], wq, bq, torch.exp(masked[1:].double()), keep=list(range(run, S)))
    e3 = rel_err(npy(out[1:]), gone.numpy())
    print(f"E {E} L {L} S {S}: null {e0:.2e}, finite {e1:.2e}, masked {e2:.2e}, against removal {e3:.2e}")
    assert max(e0, e1, e2, e3) < ATT_TOL


@pytest.mark.parametrize("E,L,S,lo,hi", [(512, 16, 128, 0, 64), (512, 16, 128, 32, 96), (256, 64, 200, 0, 128),
                                         (256, 64, 200, 64, 200)])
def test_tiled_attention_whole_tiles_masked(cuda, E, L, S, lo, hi):
    """Key tiles (32 keys at E 512, 64 at E 256) that are entirely -inf: leading, in the middle, trailing."""
    z, kv, wq, bq, bias = att_inputs(2, E, L, S)
    bias[:, lo:hi] = NEG
    out = run_att(cuda, z, kv, wq, bq, bias)
    assert bool(torch.isfinite(out).all())
    keep = [s for s in range(S) if not lo <= s < hi]
    e = rel_err(npy(out), att_ref(z, kv, wq, bq, torch.exp(bias.double()), keep=keep).numpy())
    print(f"E {E} S {S} keys [{lo},{hi}) masked: {e:.2e}")
    assert e < ATT_TOL


def test_bias_folded_into_bf_is_the_bias_argument_bitwise(cuda):
    for E, L, S in ((512, 16, 48), (256, 64, 130)):
        z, kv, wq, bq, bias = att_inputs(2, E, L, S)
        bias[1, :L] = NEG
        assert torch.equal(run_att(cuda, z, kv, wq, bq, bias), run_att(cuda, z, kv, wq, bq, bias, fold_bias=True))
        # no bias: the new fold entry is the old one
        assert torch.equal(run_att(cuda, z, kv, wq, bq, None), run_att(cuda, z, kv, wq, bq, None, fold_bias=True))


def test_equal_counts_without_bias_run_the_resident_kernel(cuda):
    """S == L and no bias: ldm_attention_folded_keys is ldm_attention_folded, bit for bit."""
    from ldm_amd import _lib as L_
    for E, L in ((512, 16), (256, 64)):
        z, kv, wq, bq, _ = att_inputs(2, E, L, L)
        a = run_att(cuda, z, kv, wq, bq, None)
        st = torch.cuda.current_stream().cuda_stream
        zd, kvd, wqd, bqd = z.to(cuda), kv.to(cuda), wq.to(cuda), bq.to(cuda)
        kf = torch.empty((2, 4, L, E), device=cuda)
        bf = torch.empty((2, 4, L), device=cuda)
        out = torch.empty((2, L, E), device=cuda)
        L_.call("ldm_attention_fold_keys", kvd.data_ptr(), wqd.data_ptr(), bqd.data_ptr(), 2, E, 4, L,
                float(np.sqrt(4.0 / E)), kf.data_ptr(), bf.data_ptr(), st)
        L_.call("ldm_attention_folded", zd.data_ptr(), kvd.data_ptr(), kf.data_ptr(), bf.data_ptr(), out.data_ptr(), 2, E,
                4, L, L, st)
        torch.cuda.synchronize()
        assert torch.equal(a, out)


# ---- the loops -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its float64 state dict and schedule."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm.state_dict().items()}
    return dict(M=M, ldm=ldm, sd64=sd64, ab=SR.alpha_bar(ldm.num_timesteps))


def mix_inputs(B, H, W, R, seed):
    """z, stacked s5 / s6, per-key weights (float64) and their log as fp32 biases."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 32, H, W, generator=g)
    m5 = torch.rand(B, R, 256, H // 4, W // 4, generator=g)
    m6 = torch.rand(B, R, 512, H // 8, W // 8, generator=g)
    w = torch.rand(B, R, generator=g, dtype=torch.float64) + 0.1
    kw5 = MR.key_weights(w, B, R, (H // 4) * (W // 4))
    kw6 = MR.key_weights(w, B, R, (H // 8) * (W // 8))
    return dict(z=z, s5=MR.stack(m5).contiguous(), s6=MR.stack(m6).contiguous(), kw5=kw5, kw6=kw6,
                kb5=torch.log(kw5).float(), kb6=torch.log(kw6).float(), m5=m5, m6=m6)


def run_loop(ctx, cuda, eng, d, times, solver="msolver", split=1, bias=True):
    z = d["z"]
    B, n = z.shape[0], len(times) - 1
    fd = ctx["ldm"].noise_scheduler
    tt = torch.from_numpy(times)
    coef = (fd.multistep_coefs(tt) if solver == "msolver" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(n, 1).expand(n, B).contiguous().to(cuda)
    x = z.to(cuda).clone()
    x0l = torch.full((n,) + tuple(z.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    kb = dict(key_bias5=d["kb5"].to(cuda), key_bias6=d["kb6"].to(cuda)) if bias else {}
    with torch.no_grad():
        if solver == "msolver":
            eng.msolver_loop(x, d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, x0l, epl, split=split, **kb)
        else:
            eng.ddim_loop(x, d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, 0.0, x0l, epl, split=split, **kb)
    torch.cuda.synchronize()
    return x, x0l, epl, coef, t_table


def replay_err(z, x, x0l, epl, coef, times):
    """The float64 replay of the multistep table from the logged eps (tests/test_gpu_solver.py's check)."""
    c = coef.double().cpu().numpy()
    xv, prev, worst = npy(z), None, 0.0
    for i in range(len(times) - 1):
        x0 = (xv - c[i, 1] * npy(epl[i])) / c[i, 0]
        xv = c[i, 2] * xv + c[i, 3] * x0 + (c[i, 4] * prev if prev is not None else 0.0)
        worst = max(worst, rel_err(npy(x0l[i]), x0))
        prev = x0
    return max(worst, rel_err(npy(x), xv))


MIX_CASES = {"B2-16x64-R2": (2, 16, 64, 2), "B2-16x64-R3": (2, 16, 64, 3), "B1-8x8-R3": (1, 8, 8, 3)}


@pytest.fixture(scope="module")
def mix_runs(ctx, cuda):
    """Each 2M case once on the default engine, with its yardstick; shared, never modified."""
    times = SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    out = {}
    for k, (B, H, W, R) in MIX_CASES.items():
        d = mix_inputs(B, H, W, R, 40 + R + H)
        want, _, _ = MR.sample(ctx["sd64"], ctx["ab"], times, npy(d["z"]), d["s5"], d["s6"], d["kw5"], d["kw6"])
        out[k] = (d, times, run_loop(ctx, cuda, eng, d, times), want)
    return out


@pytest.mark.parametrize("case", list(MIX_CASES))
def test_msolver_loop_mix(ctx, mix_runs, case):
    d, times, (x, x0l, epl, coef, _), want = mix_runs[case]
    if case == "B1-8x8-R3":
        assert d["s6"].shape[2] * d["s6"].shape[3] == 3 and d["s5"].shape[2] * d["s5"].shape[3] == 12
    e_replay, e_ref = replay_err(d["z"], x, x0l, epl, coef, times), rel_err(npy(x), want)
    print(f"{case}: replay {e_replay:.2e}, yardstick {e_ref:.2e}")
    assert e_replay <= UPD_TOL
    assert e_ref <= PARITY_TOL


def test_ddim_loop_mix(ctx, cuda):
    d, times = mix_inputs(2, 16, 64, 2, 51), SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x, x0l, epl, coef, _ = run_loop(ctx, cuda, eng, d, times, solver="ddim")
    want = MR.ddim(ctx["sd64"], ctx["ab"], times, d["z"], d["s5"], d["s6"], d["kw5"], d["kw6"], eta=0.0)
    e = rel_err(npy(x), want)
    print(f"ddim eta 0, R 2: {e:.2e}")
    assert e <= PARITY_TOL and bool(torch.isfinite(x0l).all()) and bool(torch.isfinite(epl).all())


def test_msolver_loop_mix_without_step_kernels(ctx, cuda):
    from ldm_amd.engine import UNetEngine
    d, times = mix_inputs(2, 16, 64, 2, 52), SR.sample_times(99, 4)
    eng = UNetEngine(ctx["ldm"].unet, step=0)
    x, x0l, epl, coef, _ = run_loop(ctx, cuda, eng, d, times)
    want, _, _ = MR.sample(ctx["sd64"], ctx["ab"], times, npy(d["z"]), d["s5"], d["s6"], d["kw5"], d["kw6"])
    e_replay, e_ref = replay_err(d["z"], x, x0l, epl, coef, times), rel_err(npy(x), want)
    print(f"step=0, R 2: replay {e_replay:.2e}, yardstick {e_ref:.2e}")
    assert e_replay <= UPD_TOL and e_ref <= PARITY_TOL


def test_fp16_operands(ctx, cuda):
    """The fp16 step kernels with a mix, held to twice the error of the existing single-style fp16 loop against the
    same yardstick on the same inputs (z, times, and reference 0 as the single style).
    Measured on an MI355X: mix 7.47e-5, single style 8.10e-5."""
    from ldm_amd.engine import UNetEngine
    d, times = mix_inputs(2, 16, 64, 2, 53), SR.sample_times(99, 4)
    eng = UNetEngine(ctx["ldm"].unet, dtype="fp16")
    x, _, _, _, _ = run_loop(ctx, cuda, eng, d, times)
    want, _, _ = MR.sample(ctx["sd64"], ctx["ab"], times, npy(d["z"]), d["s5"], d["s6"], d["kw5"], d["kw6"])
    one = dict(d, s5=d["m5"][:, 0].contiguous(), s6=d["m6"][:, 0].contiguous())
    x1, _, _, _, _ = run_loop(ctx, cuda, eng, one, times, bias=False)
    want1, _, _ = SR.sample(ctx["sd64"], ctx["ab"], times, npy(d["z"]), one["s5"], one["s6"])
    e_mix, e_one = rel_err(npy(x), want), rel_err(npy(x1), want1)
    print(f"fp16: mix {e_mix:.3e}, single style {e_one:.3e}")
    assert e_mix <= 2 * e_one


# ---- identities on the device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specs(cuda):
    g = torch.Generator().manual_seed(61)
    return dict(z=torch.randn(2, 32, 16, 64, generator=g).to(cuda), st=torch.rand(2, 3, 1, 128, 512, generator=g).to(cuda))


def sample3(ctx, z, emb):
    with torch.no_grad():
        x, _ = ctx["ldm"].style_conditioned_sample(z, emb, steps=3, t_start=99)
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module")
def plain3(ctx, specs):
    """The plain call on each of the three styles; shared, never modified."""
    with torch.no_grad():
        return [sample3(ctx, specs["z"], ctx["ldm"].style_encoder(specs["st"][:, r])) for r in range(3)]


def test_one_reference_is_the_plain_call_bitwise(ctx, specs, plain3):
    ldm = ctx["ldm"]
    with torch.no_grad():
        emb = ldm.encode_styles(specs["st"][:, :1])
    assert emb["key_bias5"] is None and emb["refs"] == 1
    assert torch.equal(sample3(ctx, specs["z"], emb), plain3[0])


def test_two_copies_are_the_single_style(ctx, specs, plain3):
    ldm = ctx["ldm"]
    with torch.no_grad():
        emb = ldm.encode_styles(specs["st"][:, [1, 1]], [0.3, 0.7])
    assert tuple(emb["s5"].shape) == (2, 256, 8, 16) and tuple(emb["key_bias6"].shape) == (2, 32)
    e = rel_err(npy(sample3(ctx, specs["z"], emb)), npy(plain3[1]))
    print(f"two copies (0.3, 0.7) against the plain call: {e:.2e}")
    assert e <= PARITY_TOL


def test_zero_weight_column_is_dropped_bitwise(ctx, specs):
    ldm = ctx["ldm"]
    with torch.no_grad():
        a = ldm.encode_styles(specs["st"], [0.5, 0.0, 0.5])
        b = ldm.encode_styles(specs["st"][:, [0, 2]], [0.5, 0.5])
    assert a["refs"] == 2 and torch.equal(a["s5"], b["s5"]) and torch.equal(a["key_bias5"], b["key_bias5"])
    assert torch.equal(sample3(ctx, specs["z"], a), sample3(ctx, specs["z"], b))


def test_per_sample_zero_weight_removes_the_reference(ctx, specs, plain3):
    ldm = ctx["ldm"]
    with torch.no_grad():
        emb = ldm.encode_styles(specs["st"][:, :2], [[0.4, 0.6], [1.0, 0.0]])
    assert bool(torch.isinf(emb["key_bias5"][1, 64:]).all()) and bool(torch.isfinite(emb["key_bias5"][0]).all())
    x = sample3(ctx, specs["z"], emb)
    assert bool(torch.isfinite(x).all())
    e = rel_err(npy(x[1]), npy(plain3[0][1]))
    print(f"sample 1 with weights (1, 0) against its plain call: {e:.2e}")
    assert e <= PARITY_TOL


# ---- capture, split, refusals ----------------------------------------------------------------------------------------
def test_capture_and_split(ctx, cuda):
    from ldm_amd.engine import GraphedDDIM
    d, times = mix_inputs(4, 16, 64, 2, 71), SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x1, x0l1, epl1, coef, t_table = run_loop(ctx, cuda, eng, d, times)
    x2, x0l2, epl2, _, _ = run_loop(ctx, cuda, eng, d, times, split=2)
    e = max(rel_err(npy(x2), npy(x1)), rel_err(npy(x0l2), npy(x0l1)), rel_err(npy(epl2), npy(epl1)))
    print(f"mix, split 2 against 1: {e:.2e}")
    assert e <= UPD_TOL
    with torch.no_grad():
        gd = GraphedDDIM(eng, d["z"].to(cuda), d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, 0.0, logs=True,
                         solver="msolver", key_bias5=d["kb5"].to(cuda), key_bias6=d["kb6"].to(cuda))
        a = gd.replay().clone()
        a0 = gd.x0_logs.clone()
        b = gd.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(a, x1) and torch.equal(a0, x0l1)
    assert torch.equal(b, x1) and torch.equal(gd.x0_logs, x0l1) and torch.equal(gd.eps_logs, epl1)


def test_paths_without_a_mixing_kernel_refuse(ctx, cuda):
    from ldm_amd.engine import UNetEngine
    M, ldm = ctx["M"], ctx["ldm"]
    d, times = mix_inputs(2, 16, 64, 2, 81), SR.sample_times(99, 2)
    with pytest.raises(RuntimeError, match="folded"):
        run_loop(ctx, cuda, UNetEngine(ldm.unet, fold=False), d, times)
    emb = {"s5": d["s5"].to(cuda), "s6": d["s6"].to(cuda), "key_bias5": d["kb5"].to(cuda), "key_bias6": d["kb6"].to(cuda),
           "refs": 2}
    t = torch.tensor([17, 150], device=cuda)
    with pytest.raises(RuntimeError, match="reverse loop"):
        ldm.unet(d["z"].to(cuda), t, emb)
    with pytest.raises(RuntimeError, match="reverse loop"):
        M.engine_for(ldm.unet).forward(d["z"].to(cuda), t, emb["s5"], emb["s6"])
    torch.manual_seed(2)
    ldm4 = M.LDM(4, pretrained_path="").eval().to(cuda)      # a latent width the engine does not take
    g = torch.Generator().manual_seed(82)
    z4 = torch.randn(2, 4, 16, 16, generator=g).to(cuda)
    emb4 = {"s5": torch.rand(2, 256, 8, 4, generator=g).to(cuda), "s6": torch.rand(2, 512, 4, 2, generator=g).to(cuda),
            "refs": 2, "key_bias5": None, "key_bias6": None}
    with pytest.raises(RuntimeError, match="per-layer"):
        ldm4.style_conditioned_sample(z4, emb4, steps=2, t_start=99)


# ---- the whole recording ---------------------------------------------------------------------------------------------
def test_transfer_recording_with_several_references(ctx, cuda):
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(100 * 512)).float().to(cuda)     # 101 frames: two windows of 64 / 16
    style = torch.from_numpy(AR.test_signal(200 * 512, variant=1)).float().to(cuda)   # 201 frames: three full windows
    style2 = torch.from_numpy(AR.test_signal(70 * 512, variant=2)).float().to(cuda)   # one full window
    kw = dict(frames=64, overlap=16, n_iter=2, nnls_iters=2, seed=4)
    x, ref = LF.mel_windows(A.melspectrogram(content), 64, 16)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 64, 0)
    xs2, _ = LF.mel_windows(A.melspectrogram(style2), 64, 0)
    noise = torch.randn((2, 32, 16, 8), generator=torch.Generator().manual_seed(4)).to(cuda)

    def check(res, spec, weights):
        assert res.N == 2
        with torch.no_grad():
            want, _ = ldm.content_style_transfer(x, spec.unsqueeze(0).expand(2, -1, -1, -1, -1), t_start=99, steps=4,
                                                 solver="dpmpp2m", noise=noise, style_weights=weights)
        assert torch.equal(res.windows_out, want)
        mel = LF.stitch_windows(want, ref, 16, 101)
        assert torch.equal(res.mel_power, mel)
        assert torch.equal(res.audio, A.mel_to_audio(mel, seed=4, length=100 * 512, n_iter=2, nnls_iters=2))

    # two windows of one recording: the first and the last of its three full windows, equal weights
    check(transfer_recording(ldm, content, style, num_timesteps=4, solver="dpmpp2m", style_refs=2, **kw),
          xs[[0, 2]], None)
    # two recordings at (0.7, 0.3), one window each
    check(transfer_recording(ldm, content, [style, style2], num_timesteps=4, solver="dpmpp2m",
                             style_weights=[0.7, 0.3], **kw),
          torch.cat([xs[:1], xs2[:1]]), [0.7, 0.3])
    with pytest.raises(ValueError):
        transfer_recording(ldm, content, [style, style2], num_timesteps=4, solver="dpmpp2m", style_weights=[1.0], **kw)
    with pytest.raises(ValueError):
        transfer_recording(ldm, content, [style] * 3, num_timesteps=4, solver="dpmpp2m", style_refs=3, **kw)
