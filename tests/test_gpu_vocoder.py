"""GPU: the content-anchored vocoder (csrc/vocoder.hip, the anchored Griffin-Lim of csrc/audio.hip, through
ldm_amd.audio and models.transfer) against the float64 yardstick tests/vocoder_ref.py.  Bounds: rel_err (max-abs over
max-abs) <= 1e-4, the project's fp32 bar, unless a test states its own."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R          # noqa: E402
import vocoder_ref as V        # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A(cuda):
    from ldm_amd import audio
    return audio


@pytest.fixture(scope="module")
def cases():
    """Per case the float32-exact inputs (vocoder_ref.gain_case); never modified."""
    return {name: V.gain_case(name) for name in V.CASES}


def dev(x, cuda, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(cuda)


def cplx(t):
    return t.cpu().numpy().astype(np.complex128)


def gpu_target(A, cuda, c, anchor_db, res=None, Mo=None):
    return A.mel_gain_target(dev(c["C"], cuda, torch.complex64), dev(c["Mo"] if Mo is None else Mo, cuda),
                             dev(c["Mc"], cuda), dev(c["eps"], cuda), V.MAX_GAIN_DB, anchor_db,
                             None if res is None else dev(res, cuda))


# ---- 1. mel gain -> target ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("anchor_db", [0.0, 6.0])
@pytest.mark.parametrize("case", list(V.CASES))
def test_mel_gain_target_matches_float64(A, cuda, cases, case, anchor_db, with_residual):
    c = cases[case]
    res = c["R"] if with_residual else None
    want_A, want_P0, want_a, pre = V.mel_gain_target(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB,
                                                     anchor_db, res)
    g = V.bin_gain(c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB)
    assert (g == 10.0 ** (V.MAX_GAIN_DB / 10.0)).any() and c["zero"].any()
    mag, p0, a = gpu_target(A, cuda, c, anchor_db, res)
    assert mag.shape == want_A.shape and p0.dtype == torch.complex64 and a.dtype == torch.float32
    e_mag = rel_err(mag.cpu().numpy(), want_A)
    p0n = cplx(p0)
    e_p0 = rel_err(np.stack([p0n.real, p0n.imag], -1), np.stack([want_P0.real, want_P0.imag], -1))
    assert (p0n[c["zero"]] == 1.0).all()                                  # (1, 0) where the content vanishes
    an = a.cpu().numpy().astype(np.float64)
    if anchor_db <= 0:
        assert (an == 0).all()
        e_a, left_out = 0.0, 0.0
    else:
        near = (np.abs(pre) < 1e-3) | (np.abs(pre - 1.0) < 1e-3)          # the kinks of the clamp
        left_out = near.mean()
        assert left_out <= 0.02
        e_a = np.abs(an - want_a)[~near].max()
        assert an.min() >= 0.0 and an.max() <= 1.0
    print(f"mel_gain_target {case} anchor_db {anchor_db} residual {with_residual}: mag {e_mag:.2e} phase0 {e_p0:.2e} "
          f"anchor abs {e_a:.2e} (left out {100 * left_out:.2f} %)")
    assert e_mag <= 1e-4 and e_p0 <= 1e-4 and e_a <= 1e-4
    if not with_residual and anchor_db > 0:
        Pm = A.mel_gain_power(dev(c["C"], cuda, torch.complex64), dev(c["Mo"], cuda), dev(c["Mc"], cuda),
                              dev(c["eps"], cuda), V.MAX_GAIN_DB)
        assert rel_err(Pm.cpu().numpy(), V.masked_power(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB)) <= 1e-4
        one = A.mel_gain_target(dev(c["C"][1], cuda, torch.complex64), dev(c["Mo"][1], cuda), dev(c["Mc"][1], cuda),
                                float(c["eps"][1]), V.MAX_GAIN_DB, anchor_db)                # unbatched, eps a number
        assert all(torch.equal(o, w[1]) for o, w in zip(one, (mag, p0, a)))


@pytest.mark.parametrize("case", list(V.CASES))
def test_unchanged_mel_gives_the_content_bitwise(A, cuda, cases, case):
    c = cases[case]
    mag, p0, a = gpu_target(A, cuda, c, 6.0, Mo=c["Mc"])
    assert torch.equal(a, torch.ones_like(a))                              # g is exactly 1, so the anchor is
    assert rel_err(mag.cpu().numpy(), np.abs(c["C"])) <= 1e-6


# ---- 2. / 3. anchored Griffin-Lim --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gl_ref(cases):
    """Per case: the float64 target (mag, P0, fractional anchors) and the float64 anchored recurrence after 1 and 4
    iterations.  The seed keeps every blended phase's modulus above 1e-3 (asserted), away from the normalisation's
    singularity."""
    out = {}
    for name, c in cases.items():
        mag, P0, a, _ = V.mel_gain_target(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB, 6.0)
        mag, a = V.f32(mag), V.f32(a)
        P0 = V.unit_phase(V.f32(P0))
        assert ((a > 0) & (a < 1)).mean() > 0.1
        ref = {}
        for k in (1, 4):
            ref[k], mb = V.griffinlim_anchored(mag, P0, a, k, n_fft=c["n_fft"], return_min_blend=True)
            assert mb >= 1e-3
        out[name] = (c["n_fft"], mag, P0, a, ref)
    return out


@pytest.mark.parametrize("case", list(V.CASES))
def test_anchored_griffinlim_elementwise(A, cuda, gl_ref, case):
    n_fft, mag, P0, a, ref = gl_ref[case]
    pd = dev(P0, cuda, torch.complex64)
    for k in (1, 4):
        got = A.griffinlim(dev(mag, cuda), n_iter=k, init_phase=pd, n_fft=n_fft, anchor_phase=pd, anchor=dev(a, cuda))
        e = rel_err(got.cpu().numpy(), ref[k])
        print(f"anchored griffinlim {case} iters {k}: rel_err {e:.3e}")
        assert e <= 1e-4


@pytest.mark.parametrize("case", list(V.CASES))
def test_anchor_ends_are_bitwise(A, cuda, gl_ref, case):
    n_fft, mag, P0, a, _ = gl_ref[case]
    md, pd = dev(mag, cuda), dev(P0, cuda, torch.complex64)
    zero, one = torch.zeros_like(md), torch.ones_like(md)
    plain = A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft)
    assert torch.equal(A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft, anchor_phase=pd, anchor=zero), plain)
    held = A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft, anchor_phase=pd, anchor=one)
    assert torch.equal(held, A.griffinlim(md, n_iter=0, init_phase=pd, n_fft=n_fft, anchor_phase=pd, anchor=one))
    assert torch.equal(held, A.griffinlim(md, n_iter=0, init_phase=pd, n_fft=n_fft)) and not torch.equal(held, plain)


def test_anchored_griffinlim_graph_replay(A, cuda, gl_ref):
    n_fft, mag, P0, a, _ = gl_ref["n2048"]
    md, pd, ad = dev(mag, cuda), dev(P0, cuda, torch.complex64), dev(a, cuda)
    kw = dict(n_iter=4, init_phase=pd, n_fft=n_fft, anchor_phase=pd, anchor=ad)
    eager = A.griffinlim(md, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.griffinlim(md, **kw)                                       # tables and caches made outside the capture
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        out = A.griffinlim(md, **kw)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- 4. / 5. identity and locality -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(V.CASES))
def test_identity(A, cuda, cases, case):
    c = cases[case]
    n_fft, hop = c["n_fft"], c["n_fft"] // 4
    y = np.stack([R.test_signal(c["L"], variant=v) for v in range(c["B"])])
    yd = dev(y, cuda)
    mel = A.melspectrogram(yd, n_fft=n_fft)
    n = (mel.shape[-1] - 1) * hop
    for k in (0, 4):
        for res in (True, False):
            got = A.mel_to_audio_content(mel, yd, n_fft=n_fft, n_iter=k, residual=res)
            assert got.shape == (c["B"], n)
            e = np.abs(got.cpu().numpy() - y[:, :n]).max()
            print(f"identity {case} n_iter {k} residual {res}: max abs {e:.2e}")
            assert e <= 1e-4
    one = A.mel_to_audio_content(mel[1], yd[1], n_fft=n_fft, n_iter=0)          # unbatched
    assert one.shape == (n,) and np.abs(one.cpu().numpy() - y[1, :n]).max() <= 1e-4


@pytest.mark.parametrize("case", list(V.CASES))
def test_locality(A, cuda, cases, case):
    """The gain differs from 1 only in frames t >= T / 2: every sample all of whose covering frames lie in t < T / 2
    comes back as the content."""
    c = cases[case]
    n_fft, hop = c["n_fft"], c["n_fft"] // 4
    y = np.stack([R.test_signal(c["L"], variant=v) for v in range(c["B"])])
    yd = dev(y, cuda)
    mel_c = A.melspectrogram(yd, n_fft=n_fft)
    T = mel_c.shape[-1]
    half = T // 2
    gain = 10.0 ** (V.smooth_gain_db((c["B"], V.N_MELS, T), 20.0, 3) / 10.0)
    gain[:, :, :half] = 1.0
    mel_o = mel_c * dev(gain, cuda)
    assert torch.equal(mel_o[:, :, :half], mel_c[:, :, :half]) and not torch.equal(mel_o, mel_c)
    n = (T - 1) * hop
    # sample i is covered by the frames t with t hop - n_fft / 2 <= i < t hop + n_fft / 2: the last is (i + n_fft / 2) // hop
    inside = (np.arange(n) + n_fft // 2) // hop < half
    assert inside.sum() >= hop
    for k in (0, 4):
        got = A.mel_to_audio_content(mel_o, yd, n_fft=n_fft, n_iter=k).cpu().numpy()
        e = np.abs(got - y[:, :n])[:, inside].max()
        print(f"locality {case} n_iter {k}: max abs inside {e:.2e}, outside {np.abs(got - y[:, :n])[:, ~inside].max():.2e}")
        assert e <= 1e-4
        assert np.abs(got - y[:, :n])[:, ~inside].max() > 1e-2            # and is something else where the gain acts


# ---- 7. end to end -----------------------------------------------------------------------------------------------
def test_transfer_recording_content_vocoder(cuda):
    import models.model as M
    from ldm_amd import longform as LF
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    model = M.LDM(32, pretrained_path="").eval().to(cuda)
    frames, overlap, T_total = 128, 32, 224                                 # two windows: [0, 128) and [96, 224)
    L = (T_total - 1) * HOP
    y = R.test_signal(L)
    content = dev(y, cuda)
    style = dev(R.test_signal(150 * HOP, variant=1), cuda)
    assert LF.window_plan(T_total, frames, overlap)[0] == 2
    sr = 22050
    keep = LF.keep_mask(T_total, 128, sr, times=[(0.0, 95 * HOP / sr + 1e-6)])    # the first window's interior
    assert bool((keep[:, :96] == 1).all()) and bool((keep[:, 96:] == 0).all())
    kw = dict(frames=frames, overlap=overlap, num_timesteps=2, solver="dpmpp2m", n_iter=4, nnls_iters=2, seed=4,
              keep=keep, composite=True)
    res = transfer_recording(model, content, style, vocoder="content", **kw)
    assert res.N == 2 and res.audio.shape == (L,) and bool(torch.isfinite(res.audio).all())
    inside = (np.arange(L) + 1024) // HOP < 96                              # every covering frame is a kept one
    d = np.abs(res.audio.cpu().numpy() - y)
    print(f"content vocoder: max abs in the kept region {d[inside].max():.2e}, elsewhere {d[~inside].max():.2e}")
    assert d[inside].max() <= 1e-4
    assert d[~inside].max() > 1e-2
    plain = transfer_recording(model, content, style, **kw)
    named = transfer_recording(model, content, style, vocoder="griffinlim", **kw)
    assert torch.equal(named.audio, plain.audio) and torch.equal(named.mel_power, plain.mel_power)
    assert torch.equal(res.mel_power, plain.mel_power) and not torch.equal(res.audio, plain.audio)
    ref_sampler = transfer_recording(model, content, style, vocoder="content", frames=frames, overlap=overlap,
                                     num_timesteps=2, n_iter=1, nnls_iters=2, seed=4)          # solver=None
    assert ref_sampler.audio.shape == (L,) and bool(torch.isfinite(ref_sampler.audio).all())


# ---- 8. errors ---------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(A, cuda, cases):
    c = cases["n512"]
    Cd, Mo, Mc = dev(c["C"], cuda, torch.complex64), dev(c["Mo"], cuda), dev(c["Mc"], cuda)
    mag, p0, a = A.mel_gain_target(Cd, Mo, Mc, dev(c["eps"], cuda))
    with pytest.raises(ValueError, match="both or neither"):
        A.griffinlim(mag, n_iter=1, init_phase=p0, n_fft=512, anchor=a)
    with pytest.raises(ValueError, match="both or neither"):
        A.griffinlim(mag, n_iter=1, init_phase=p0, n_fft=512, anchor_phase=p0)
    with pytest.raises(ValueError, match="shape"):
        A.griffinlim(mag, n_iter=1, init_phase=p0, n_fft=512, anchor_phase=p0, anchor=a[:, :, :5])
    with pytest.raises(ValueError, match="shape"):
        A.griffinlim(mag, n_iter=1, init_phase=p0, n_fft=512, anchor_phase=p0[:2], anchor=a)
    with pytest.raises(ValueError, match="mel_out"):
        A.mel_gain_target(Cd, Mo[:, :, :5], Mc, 1e-3)
    with pytest.raises(ValueError, match="mel_out"):
        A.mel_gain_target(Cd, Mo, Mc[:2], 1e-3)
    with pytest.raises(ValueError, match="residual"):
        A.mel_gain_target(Cd, Mo, Mc, 1e-3, residual=mag[:, :5])
    for bad in (0.0, -1.0, float("nan"), [1e-3, 1e-3]):
        with pytest.raises(ValueError, match="eps"):
            A.mel_gain_target(Cd, Mo, Mc, bad)
    with pytest.raises(ValueError, match="max_gain_db"):
        A.mel_gain_target(Cd, Mo, Mc, 1e-3, max_gain_db=float("inf"))
    with pytest.raises(ValueError, match="anchor_db"):
        A.mel_gain_target(Cd, Mo, Mc, 1e-3, anchor_db=float("nan"))
    with pytest.raises(ValueError, match="do not match"):
        A.mel_to_audio_content(Mo[:, :, :5], torch.zeros(3, c["L"], device=cuda), n_fft=512)
