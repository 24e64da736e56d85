"""GPU: the whole-recording path (csrc/longform.hip through ldm_amd.longform, and models.transfer).  mel_windows is
held bitwise to the composition of the existing ops it fuses; the stitch and the reference levels are held to the
float64 yardstick tests/longform_ref.py.  Kernel tests run at n_mels = 8, frames = 64 on power spanning 12 decades."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR      # noqa: E402
import longform_ref as R    # noqa: E402

pytestmark = pytest.mark.gpu

N_MELS, FRAMES = 8, 64
OVERLAPS = (0, 1, 5, 32)
T_TOTALS = (1, 63, 64, 65, 200)
CASES = [(ov, T) for ov in OVERLAPS for T in T_TOTALS]
HALF_STEP = 80.0 / 255.0 / 2.0     # dB: half an 8-bit level
DB_TOL = 1e-3                      # dB: test_power_to_db_per_item's bound on the fp32 dB arithmetic


@pytest.fixture(scope="module")
def LF(cuda):
    from ldm_amd import longform
    return longform


def dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(cuda)


def power_case(overlap, T):
    """fp32 power [8, T] over 12 decades (as float64 for the yardstick).  With three or more windows, window 1 holds
    no power at all; every other window spans more than 80 dB."""
    P = R.random_power(N_MELS, T, seed=100 * overlap + T).astype(np.float32)
    N, stride = R.window_plan(T, FRAMES, overlap)
    if N >= 3:
        P[:, stride:stride + FRAMES] = 0.0
    return P, N, stride


def composition(P, overlap):
    """The existing ops on an unfolded copy: zero-pad, unfold, power_to_db, mel_quantize, u8_to_unit."""
    from ldm_amd import ops
    N, stride = R.window_plan(P.shape[1], FRAMES, overlap)
    pad = torch.nn.functional.pad(P, (0, (N - 1) * stride + FRAMES - P.shape[1]))
    W = pad.unfold(1, FRAMES, stride).permute(1, 0, 2).contiguous()           # [N, n_mels, frames]
    db = ops.power_to_db(W, amin=1e-10, top_db=80.0)
    return ops.u8_to_unit(ops.mel_quantize(db, 80)).unsqueeze(1)


# ---- mel_windows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,T", CASES)
def test_mel_windows_bitwise_the_composition(LF, cuda, overlap, T):
    P, N, stride = power_case(overlap, T)
    Pd = dev(P, cuda)
    x, ref = LF.mel_windows(Pd, FRAMES, overlap)
    assert x.shape == (N, 1, N_MELS, FRAMES) and ref.shape == (N,) and x.dtype == torch.float32
    assert torch.equal(x, composition(Pd, overlap))
    _, ref64 = R.window_db(P.astype(np.float64), FRAMES, overlap)
    err = np.abs(ref.cpu().numpy().astype(np.float64) - ref64).max()
    print(f"overlap {overlap} T {T}: N {N}, ref_db max err {err:.2e} dB")
    assert err <= 1e-4
    xs = x.cpu().numpy()
    W = R.cut(P, FRAMES, overlap)
    if N >= 3:
        assert (xs[1] == 1.0).all() and abs(float(ref[1]) + 100.0) <= 1e-4    # the window without power
    if T >= 63:
        far = (W > 0) & (W < W.max(axis=(1, 2), keepdims=True) * 1e-9)         # more than 80 dB under the maximum
        assert far.any() and (xs[:, 0][far] == 0.0).all()
    assert torch.equal(x, LF.mel_windows(Pd, FRAMES, overlap)[0])


def test_mel_windows_of_a_view_and_bad_arguments(LF, cuda):
    P, N, _ = power_case(5, 200)
    buf = torch.zeros(N_MELS, 213, device=cuda)
    buf[:, 13:] = dev(P, cuda)
    x, ref = LF.mel_windows(buf[:, 13:], FRAMES, 5)                            # non-contiguous rows, offset start
    x0, ref0 = LF.mel_windows(dev(P, cuda), FRAMES, 5)
    assert torch.equal(x, x0) and torch.equal(ref, ref0)
    with pytest.raises(ValueError):
        LF.mel_windows(dev(P, cuda), FRAMES, 33)
    with pytest.raises(ValueError):
        LF.mel_windows(dev(P, cuda), 100, 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        LF.mel_windows(torch.from_numpy(P), FRAMES, 5)
    with pytest.raises(ValueError):
        LF.stitch_windows(x0[:-1], ref0[:-1], 5, 200)                          # one window short of the plan


# ---- stitch_windows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,T", CASES)
def test_stitch_matches_float64(LF, cuda, overlap, T):
    N, stride = R.window_plan(T, FRAMES, overlap)                              # T = 1, 63: one window cut short
    rng = np.random.Generator(np.random.PCG64(7 + 100 * overlap + T))
    y = (rng.random((N, 1, N_MELS, FRAMES)) * 1.4 - 0.2).astype(np.float32)    # 1 in 7 outside [0, 1] on each side
    ref = (rng.random(N) * 80.0 - 60.0).astype(np.float32)
    yd, rd = dev(y, cuda), dev(ref, cuda)
    power, db = LF.stitch_windows(yd, rd, overlap, T, return_db=True)
    assert power.shape == (N_MELS, T) and db.shape == (N_MELS, T)
    p64, d64 = R.stitch(y.astype(np.float64), ref.astype(np.float64), overlap, T)
    e_db = np.abs(db.cpu().numpy().astype(np.float64) - d64).max()
    e_p = rel_err(power.cpu().numpy(), p64)
    print(f"overlap {overlap} T {T}: N {N}, dB err {e_db:.2e}, power rel_err {e_p:.2e}")
    assert e_db <= DB_TOL
    assert e_p <= 1e-4
    again = LF.stitch_windows(yd, rd, overlap, T)                              # without the dB map; bitwise repeatable
    assert torch.equal(again, power)
    clamped, cdb = LF.stitch_windows(yd.clamp(0, 1), rd, overlap, T, return_db=True)
    assert torch.equal(clamped, power) and torch.equal(cdb, db)                # inputs outside [0, 1] are clamped
    if overlap == 0:                                                           # plain concatenation
        cat = torch.cat([yd[n, 0].clamp(0, 1) * 80.0 - 80.0 + rd[n] for n in range(N)], dim=1)[:, :T]
        assert torch.equal(db, cat)


# ---- round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,T", CASES)
def test_round_trip_within_half_a_level(LF, cuda, overlap, T):
    """stitch(mel_windows(P)) gives back max(P, floor of the frame's window) to half an 8-bit level, the floor being
    80 dB under the window's maximum (window max * 1e-8; the all-zero window's is amin, where its pixels sit).
    Inside an overlap the target is the yardstick's crossfade of the two windows' own clamped maps."""
    P, N, stride = power_case(overlap, T)
    x, ref = LF.mel_windows(dev(P, cuda), FRAMES, overlap)
    power, db = LF.stitch_windows(x, ref, overlap, T, return_db=True)
    db = db.cpu().numpy().astype(np.float64)
    P64 = P.astype(np.float64)
    own, ref64 = R.window_db(P64, FRAMES, overlap)
    target = R.stitch_db(own + ref64[:, None, None], overlap, T)
    both = R.in_overlap(T, FRAMES, overlap)
    assert both.any() == (N >= 2 and overlap > 0)
    # frames in one window: stated directly, without the yardstick's stitch
    n1 = np.minimum(N - 1, np.arange(T) // stride)
    wmax = R.cut(P64, FRAMES, overlap).max(axis=(1, 2))
    floor = np.maximum(1e-10, wmax[n1] * 1e-8)
    single = 10.0 * np.log10(np.maximum(np.maximum(P64, floor[None, :]), 1e-10))
    e1 = np.abs(db - single)[:, ~both].max()
    e2 = np.abs(db - target)[:, both].max() if both.any() else 0.0
    print(f"overlap {overlap} T {T}: one window {e1:.4f} dB, overlap {e2:.4f} dB (bound {HALF_STEP + DB_TOL:.4f})")
    assert e1 <= HALF_STEP + DB_TOL
    assert e2 <= HALF_STEP + DB_TOL
    back = 10.0 * np.log10(power.cpu().numpy().astype(np.float64))
    assert np.abs(back - db).max() <= DB_TOL


# ---- end to end -------------------------------------------------------------------------------------------------
E2E = dict(frames=128, overlap=32, num_timesteps=3, n_iter=2, nnls_iters=2, seed=4)
L_CONTENT, L_STYLE = 300 * 512, 200 * 512


@pytest.fixture(scope="module")
def e2e(cuda):
    """The model, the two recordings, and transfer_recording's result at batch_size 3 and 1; never modified."""
    import models.model as M
    from models.transfer import transfer_recording
    torch.manual_seed(0)
    model = M.LDM(32, pretrained_path="").eval().to(cuda)
    content = dev(AR.test_signal(L_CONTENT), cuda)
    style = dev(AR.test_signal(L_STYLE, variant=1), cuda)
    res = {b: transfer_recording(model, content, style, batch_size=b, **E2E) for b in (3, 1)}
    torch.cuda.synchronize()
    return model, content, style, res


def test_transfer_shapes_and_finiteness(e2e):
    model, content, style, res = e2e
    for r in res.values():
        assert r.N == 3 and r.audio.shape == (L_CONTENT,) and r.mel_power.shape == (128, 301)
        assert r.windows_out.shape == (3, 1, 128, 128) and r.ref_db.shape == (3,)
        for t in (r.audio, r.mel_power, r.windows_out, r.ref_db):
            assert bool(torch.isfinite(t).all())
        assert float(r.windows_out.min()) >= 0.0 and float(r.windows_out.max()) <= 1.0
    assert not model.training and not model.decoder.training


def test_transfer_windows_are_the_wrapper_on_the_same_inputs(LF, e2e):
    from ldm_amd import audio as A
    model, content, style, res = e2e
    x, ref = LF.mel_windows(A.melspectrogram(content), 128, 32)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 128, 0)
    assert xs.shape[0] == 2                                   # 201 frames: one full window, one padded (dropped)
    noise = torch.randn((3, 32, 16, 16), generator=torch.Generator().manual_seed(E2E["seed"])).to(content.device)
    with torch.no_grad():
        want, _ = model.content_style_transfer_wrapper(x, xs[:1].expand(3, -1, -1, -1).contiguous(), num_timesteps=3,
                                                       eta=0.0, noise=noise)
    assert torch.equal(res[3].windows_out, want)
    assert torch.equal(res[3].ref_db, ref)
    with torch.no_grad():
        one, _ = model.content_style_transfer_wrapper(x[1:2], xs[:1], num_timesteps=3, eta=0.0, noise=noise[1:2])
    assert torch.equal(res[1].windows_out[1:2], one)          # row n of the noise belongs to window n


def test_transfer_is_independent_of_batch_size(e2e):
    res = e2e[3]
    e = rel_err(res[1].windows_out.cpu().numpy(), res[3].windows_out.cpu().numpy())
    print(f"windows_out, batch_size 1 against 3: rel_err {e:.2e}")
    assert e <= 1e-4


def test_transfer_audio_is_one_vocoder_call_over_the_stitched_mel(LF, e2e):
    from ldm_amd import audio as A
    for r in e2e[3].values():
        assert torch.equal(r.mel_power, LF.stitch_windows(r.windows_out, r.ref_db, 32, 301))
        want = A.mel_to_audio(r.mel_power, seed=E2E["seed"], length=L_CONTENT, n_iter=2, nnls_iters=2)
        assert torch.equal(r.audio, want)


def test_transfer_rejects_bad_arguments(e2e, cuda):
    from models.transfer import transfer_recording
    model, content, style, _ = e2e
    with pytest.raises(ValueError, match="samples"):
        transfer_recording(model, content[:100], style, **E2E)
    with pytest.raises(ValueError, match="num_timesteps"):
        transfer_recording(model, content, style, **{**E2E, "num_timesteps": 250})
    with pytest.raises(ValueError, match="overlap"):
        transfer_recording(model, content, style, **{**E2E, "overlap": 65})
