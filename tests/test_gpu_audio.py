"""GPU: the audio kernels (csrc/audio.hip through ldm_amd.audio and AudioPreprocessor) against the float64
yardstick tests/audio_ref.py.  Bounds: rel_err (max-abs over max-abs) <= 1e-4, the project's fp32 bar, unless a
test states its own."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"n2048": (2048, 4096), "n512": (512, 2048 + 37)}   # 9 frames (0-1, 7-8 reflected); 17 frames, ragged tail


@pytest.fixture(scope="module")
def A(cuda):
    from ldm_amd import audio
    return audio


@pytest.fixture(scope="module")
def sig():
    """Per case: float64 signals [3, L] (three different items), their float64 STFT; never modified."""
    out = {}
    for name, (n_fft, L) in CASES.items():
        y = np.stack([R.test_signal(L, variant=v) for v in range(3)])
        out[name] = (n_fft, y, R.stft(y, n_fft))
    return out


def dev(x, cuda, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(cuda)


def unit_phase(shape, seed=5):
    u = np.random.Generator(np.random.PCG64(seed)).random(shape)
    return np.exp(2j * np.pi * u)


# ---- STFT -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_stft_matches_float64(A, cuda, sig, case):
    n_fft, y, S = sig[case]
    got = A.stft(dev(y, cuda), n_fft)            # B = 3, different items
    assert got.shape == S.shape and got.dtype == torch.complex64
    assert rel_err(torch.view_as_real(got).cpu().numpy(), np.stack([S.real, S.imag], -1)) <= 1e-4
    one = A.stft(dev(y[1], cuda), n_fft)         # unbatched
    assert torch.equal(one, got[1])
    assert rel_err(A.spectrogram(dev(y, cuda), n_fft, power=1).cpu().numpy(), np.abs(S)) <= 1e-4
    assert rel_err(A.spectrogram(dev(y, cuda), n_fft, power=2).cpu().numpy(), np.abs(S) ** 2) <= 1e-4


def test_stft_of_offset_view(A, cuda, sig):
    n_fft, y, S = sig["n512"]
    buf = torch.zeros(y.shape[1] + 13, device=cuda)
    buf[13:] = dev(y[2], cuda)
    v = buf[13:]
    assert v.storage_offset() == 13
    assert torch.equal(A.stft(v, n_fft), A.stft(dev(y[2], cuda), n_fft))


# ---- ISTFT ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_istft(A, cuda, sig, case):
    n_fft, y, S = sig[case]
    n = (S.shape[-1] - 1) * (n_fft // 4)
    Sd = dev(S, cuda, torch.complex64)
    got = A.istft(Sd, n, n_fft)
    assert rel_err(got.cpu().numpy(), R.istft(S, n)) <= 1e-4
    assert torch.equal(got, A.istft(Sd, n, n_fft))                       # bitwise run to run
    rt = A.istft(A.stft(dev(y, cuda), n_fft), n, n_fft)
    assert rel_err(rt.cpu().numpy(), y[:, :n]) <= 1e-4


# ---- Griffin-Lim ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gl_ref(sig):
    """Per case: mag and initial phase (float64), the float64 recurrence after 1, 4 and 32 iterations."""
    out = {}
    for name, (n_fft, y, S) in sig.items():
        mag = np.abs(S[:1])
        ph = unit_phase(mag.shape)
        out[name] = (n_fft, mag, ph, {k: R.griffinlim(mag, ph, k, n_fft=n_fft) for k in (1, 4, 32)})
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_griffinlim_elementwise(A, cuda, gl_ref, case):
    n_fft, mag, ph, ref = gl_ref[case]
    for k in (1, 4):
        got = A.griffinlim(dev(mag, cuda), n_iter=k, init_phase=dev(ph, cuda, torch.complex64), n_fft=n_fft)
        e = rel_err(got.cpu().numpy(), ref[k])
        print(f"griffinlim {case} iters {k}: rel_err {e:.3e}")
        assert e <= 1e-4


@pytest.mark.parametrize("case", list(CASES))
def test_griffinlim_full_run_converges(A, cuda, gl_ref, case):
    n_fft, mag, ph, ref = gl_ref[case]
    md, pd = dev(mag, cuda), dev(ph, cuda, torch.complex64)
    sc = {k: R.spectral_convergence(A.griffinlim(md, n_iter=k, init_phase=pd, n_fft=n_fft).double().cpu().numpy(),
                                    mag, n_fft) for k in (4, 32)}
    want = R.spectral_convergence(ref[32], mag, n_fft)
    print(f"griffinlim {case}: convergence {sc[32]:.6f} (float64 {want:.6f}), after 4 iterations {sc[4]:.6f}")
    assert abs(sc[32] - want) <= 1e-3 * want
    assert sc[32] < sc[4]


def test_griffinlim_graph_replay_and_seeds(A, cuda, gl_ref):
    n_fft, mag, ph, _ = gl_ref["n2048"]
    md, pd = dev(mag, cuda), dev(ph, cuda, torch.complex64)
    eager = A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft)       # tables and caches made outside the capture
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        out = A.griffinlim(md, n_iter=4, init_phase=pd, n_fft=n_fft)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    a, b, c = (A.griffinlim(md, n_iter=2, seed=s) for s in (7, 7, 8))
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---- mel and dB -------------------------------------------------------------------------------------------------
def test_melspectrogram_matches_float64(A, cuda, sig):
    n_fft, y, S = sig["n2048"]
    got = A.melspectrogram(dev(y, cuda))
    assert got.shape == (3, 128, 9)
    assert rel_err(got.cpu().numpy(), R.melspectrogram(y)) <= 1e-4


def test_power_to_db_per_item(A, cuda, sig):
    mel = R.melspectrogram(sig["n2048"][1][:2])              # two items, different maxima
    x = np.concatenate([mel, np.zeros_like(mel[:1]), mel[:1]])
    x[3, 5, :] *= 1e-12                                      # more than 80 dB under the item's maximum: the clamp
    x[1] *= 37.0
    got = A.power_to_db(dev(x, cuda)).cpu().numpy().astype(np.float64)
    want = np.stack([R.power_to_db(i) for i in x.astype(np.float32).astype(np.float64)])
    assert np.abs(got - want).max() <= 1e-3                  # dB, 1/300 of an 8-bit step
    assert (got[2] == 0).all() and got[3].min() == -80.0 and got[0].max() == 0.0 and got[1].max() == 0.0
    back = A.db_to_power(dev(want, cuda)).cpu().numpy()
    assert rel_err(back, R.db_to_power(want.astype(np.float32).astype(np.float64))) <= 1e-4


# ---- mel inversion ----------------------------------------------------------------------------------------------
def test_mel_to_stft_matches_stated_nnls(A, cuda):
    M = R.mel_filterbank()
    mel = R.melspectrogram(np.stack([R.test_signal(7 * 512, variant=v) for v in range(2)]))   # 8 frames
    res = {}
    for k in (0, 1, 8):
        got = A.mel_to_stft(dev(mel, cuda), nnls_iters=k, sqrt=False).cpu().numpy().astype(np.float64)
        assert (got >= 0).all()
        assert rel_err(got, R.mel_invert(mel, M, k)) <= 1e-4
        res[k] = np.linalg.norm(M @ got - mel) / np.linalg.norm(mel)
    print("nnls residuals", res)
    assert res[0] >= res[1] >= res[8]
    full = A.mel_to_stft(dev(mel, cuda), nnls_iters=8).cpu().numpy()
    assert rel_err(full, np.sqrt(R.mel_invert(mel, M, 8))) <= 1e-4


# ---- end to end -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    y = R.test_signal(512 * 511)
    db = R.power_to_db(R.melspectrogram(y))
    return y, db, R.quantize(db)


def test_audio_to_model_input(cuda, e2e):
    """8-bit pixels against the float64 chain: at most 1 level anywhere, in at most 0.1 % of pixels.
    A torch float32 CPU restatement of the chain (torch.stft, fp32 matmul, log10, the same quantisation) differs
    from float64 on this input in 0.0015 % of the pixels (1 of 65536), by one level: the cap leaves room."""
    from data.audio_processor import AudioPreprocessor
    y, _, px = e2e
    x = AudioPreprocessor().audio_to_model_input(dev(y, cuda))
    assert x.shape == (1, 1, 128, 512) and x.dtype == torch.float32
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    got = np.rint(x[0, 0].cpu().numpy().astype(np.float64) * 255.0).astype(np.int64)
    d = np.abs(got - px.astype(np.int64))
    print(f"pixels off by one: {100.0 * (d > 0).mean():.4f} %")
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_model_output_to_audio(A, cuda, e2e):
    from data.audio_processor import AudioPreprocessor
    y, db, px = e2e
    x = dev(px.astype(np.float32) / 255.0, cuda).reshape(1, 1, 128, 512)
    out = AudioPreprocessor().model_output_to_audio(x, 22050, seed=5)
    assert out.shape == (1, 511 * 512) and bool(torch.isfinite(out).all())
    mel_in = px.astype(np.float64) * (80.0 / 255.0) - 80.0
    back = A.power_to_db(A.melspectrogram(out))[0].cpu().numpy().astype(np.float64)
    corr = np.corrcoef(back.ravel(), mel_in.ravel())[0, 1]
    # the float64 chain's own correlation: the same inversion and Griffin-Lim in float64
    M = R.mel_filterbank()
    mag = np.sqrt(R.mel_invert(R.db_to_power(mel_in), M, 32))
    y64 = R.griffinlim(mag, unit_phase(mag.shape), 32)
    c64 = np.corrcoef(R.power_to_db(R.melspectrogram(y64)).ravel(), mel_in.ravel())[0, 1]
    print(f"log-mel correlation: native {corr:.4f}, float64 {c64:.4f}")
    assert corr > c64 - 0.01


def test_audio_preprocessor_cuda_routes_are_native(cuda, sig):
    from data.audio_processor import AudioPreprocessor
    proc = AudioPreprocessor()
    y = dev(sig["n2048"][1][0], cuda)
    mel = proc.get_mel_spectogram(y, 22050, n_mels=128)
    spec = proc.get_spectogram(y)
    assert mel.is_cuda and mel.shape == (128, 9) and spec.is_cuda and spec.shape == (1025, 9)
    a = proc.grayscale_mel_spectogram_image_to_audio(proc.quantize(mel), 22050, 128, 9)
    b = proc.grayscale_spectogram_image_to_audio(proc.quantize(spec), 1025, 9)
    assert a.is_cuda and b.is_cuda and a.shape == (4096,) and b.shape == (4096,)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert "librosa" not in sys.modules


# ---- errors -----------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(A, cuda):
    from ldm_amd._lib import LDMError
    y = torch.zeros(1, 4096, device=cuda)
    with pytest.raises(LDMError, match="n_fft"):
        A.stft(y, n_fft=1000)
    with pytest.raises(LDMError, match="hop"):
        A.stft(y, n_fft=2048, hop_length=300)
    with pytest.raises(LDMError, match="L "):
        A.stft(torch.zeros(1, 100, device=cuda), n_fft=2048)
