"""CPU: the float64 yardstick of the audio path (tests/audio_ref.py) pinned to torch.stft / torch.istft and to
recorded Slaney filterbank values (a float64 self-consistency pin, not librosa-verified), ldm_amd.audio's host
filterbank pinned to the same, and the .wav reader / writer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R   # noqa: E402


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("n_fft,L", [(2048, 4096), (512, 2048 + 37)])
def test_stft_istft_match_torch(n_fft, L):
    y = np.stack([R.test_signal(L, variant=v) for v in range(2)])
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    St = torch.stft(torch.from_numpy(y), n_fft, hop_length=n_fft // 4, window=w, center=True, pad_mode="reflect",
                    return_complex=True)
    S = R.stft(y, n_fft)
    assert S.shape == tuple(St.shape)
    assert rel(S, St.numpy()) <= 1e-10
    n = (S.shape[-1] - 1) * (n_fft // 4)
    yt = torch.istft(St, n_fft, hop_length=n_fft // 4, window=w, center=True, length=n).numpy()
    assert rel(R.istft(S, n), yt) <= 1e-10
    assert rel(R.istft(S, n), y[:, :n]) <= 1e-10


def test_filterbank_pin():
    from ldm_amd import audio
    for M in (R.mel_filterbank(22050, 2048, 128), audio.mel_filterbank(22050, 2048, 128)):
        assert M.shape == (128, 1025) and M.dtype == np.float64
        assert (M >= 0).all()
        for row in M:
            nz = np.flatnonzero(row)
            assert nz.size and nz[-1] - nz[0] + 1 == nz.size   # one contiguous run
        np.testing.assert_allclose(M[:3].sum(1), [0.09034588, 0.09337388, 0.09372150], rtol=2e-7)
        ev = np.linalg.eigvalsh(M @ M.T)
        np.testing.assert_allclose([ev[0], ev[-1]], [1.2409e-4, 3.6001e-3], rtol=1e-4)
    assert np.abs(R.mel_filterbank() - audio.mel_filterbank()).max() <= 1e-15


def test_power_to_db_definition():
    x = np.array([[1.0, 1e-3, 1e-9, 0.0]])
    np.testing.assert_allclose(R.power_to_db(x), [[0.0, -30.0, -80.0, -80.0]], atol=1e-12)
    assert (R.power_to_db(np.zeros((2, 3))) == 0).all()
    np.testing.assert_allclose(R.db_to_power(R.power_to_db(x))[0, :2], [1.0, 1e-3], rtol=1e-12)


def test_nnls_residual_decreases():
    M = R.mel_filterbank()
    mel = R.melspectrogram(R.test_signal(7 * 512))
    res = [np.linalg.norm(M @ R.mel_invert(mel, M, k) - mel) / np.linalg.norm(mel) for k in (0, 1, 8)]
    assert res[0] >= res[1] >= res[2]
    assert (R.mel_invert(mel, M, 8) >= 0).all()


def test_wav_round_trip_and_rate_mismatch(tmp_path):
    from data.audio_processor import AudioPreprocessor, save_wav
    pcm = (np.random.Generator(np.random.PCG64(5)).integers(-32768, 32768, 3000)).astype(np.int16)
    p = tmp_path / "a.wav"
    save_wav(p, pcm, 22050)
    y, sr = AudioPreprocessor(22050).load_audio(str(p))
    assert sr == 22050 and y.dtype == np.float32 and y.shape == (3000,)
    assert np.array_equal((y * 32768.0).astype(np.int16), pcm)
    with pytest.raises(ValueError, match="resampling"):
        AudioPreprocessor(16000).load_audio(str(p))


def test_wav_float32_stereo_is_mixed_to_mono(tmp_path):
    import struct
    from data.audio_processor import AudioPreprocessor
    x = np.array([[0.5, -0.5], [0.25, 0.75], [-1.0, 0.0]], dtype="<f4")
    body = x.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 2, 22050,
                                                                                       22050 * 8, 8, 32)
    p = tmp_path / "f.wav"
    p.write_bytes(hdr + b"data" + struct.pack("<I", len(body)) + body)
    y, sr = AudioPreprocessor(22050).load_audio(str(p))
    assert sr == 22050 and np.array_equal(y, np.array([0.0, 0.5, -0.5], dtype=np.float32))
