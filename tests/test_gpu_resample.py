"""GPU: the resampler, the silence trim, the chunk images and the dataset builder (csrc/resample.hip through
ldm_amd.audio, AudioPreprocessor and data.build_dataset) against the float64 yardstick tests/resample_ref.py.

Resampler bound: max |y - ref| <= 2e-6 max |ref|.  An fp32 numpy evaluation of the same sum lies 1.0-1.5e-7 from the
float64 one (the kernel's sequential fmaf chain measured 0.3-0.6e-6 on an MI355X); a wrong tap or phase gives >= 1e-3."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR   # noqa: E402

pytestmark = pytest.mark.gpu

RATES = [(44100, 22050), (48000, 22050), (16000, 22050), (22050, 16000)]
LENGTHS = [1, 73, 1000, 4097]
BOUND = 2e-6


@pytest.fixture(scope="module")
def A(cuda):
    from ldm_amd import audio
    return audio


@pytest.fixture(scope="module")
def AP(cuda):
    from data.audio_processor import AudioPreprocessor
    return AudioPreprocessor()


@pytest.fixture(scope="module")
def noise():
    """[3, 4097] float32 noise, three different rows; never modified."""
    x = np.random.Generator(np.random.PCG64(21)).standard_normal((3, max(LENGTHS))).astype(np.float32)
    x.setflags(write=False)
    return x


def within(y, ref):
    err, top = float(np.abs(np.asarray(y, np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"max |y - ref| {err:.3e}, bound {BOUND * top:.3e}")
    return err <= BOUND * top


# ---- 1. resampler against the yardstick ---------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_resample_matches_yardstick(A, cuda, noise, sr_in, sr_out):
    up, down = RR.ratio(sr_in, sr_out)
    for L in LENGTHS:
        x = noise[:, :L].copy()
        ref = RR.resample(x, sr_in, sr_out)
        xd = torch.from_numpy(x).to(cuda)
        y = A.resample(xd, sr_in, sr_out)
        assert y.shape == (3, math.ceil(L * up / down)) == ref.shape and y.dtype == torch.float32
        assert within(y.cpu().numpy(), ref)
        assert torch.equal(y, A.resample(xd, sr_in, sr_out))                  # bitwise run to run
        for b in range(3):
            assert torch.equal(A.resample(xd[b], sr_in, sr_out), y[b])        # a row does not depend on the batch


def test_resample_same_rate_is_identity(A, cuda, noise):
    x = torch.from_numpy(noise[:, :100].copy()).to(cuda)
    assert A.resample(x, 22050, 22050) is x


# ---- 2. int16 form equals float form ------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
def test_pcm16_equals_float_form(A, cuda, ch):
    pcm = np.random.Generator(np.random.PCG64(22)).integers(-32768, 32768, (5000, ch)).astype(np.int16)
    mono = RR.pcm_to_mono(pcm)
    y16 = A.resample_pcm16(torch.from_numpy(pcm).to(cuda), 48000, 22050)
    yf = A.resample(torch.from_numpy(mono).to(cuda), 48000, 22050)
    assert y16.shape == yf.shape == (math.ceil(5000 * 147 / 320),)
    assert torch.equal(y16, yf)
    if ch == 1:
        assert torch.equal(A.resample_pcm16(torch.from_numpy(pcm[:, 0].copy()).to(cuda), 48000, 22050), yf)


# ---- 3. 64-bit indexing -------------------------------------------------------------------------------------------
def test_long_input_indexes_in_64_bits(A, cuda):
    L, up, down = 30_000_000, 147, 320
    i = np.arange(L, dtype=np.int64)
    pcm = ((i * 7919) % 65521 - 32760).astype(np.int16)
    del i
    y = A.resample_pcm16(torch.from_numpy(pcm).to(cuda), 48000, 22050)
    n_out = RR.n_out(L, up, down)
    assert y.shape == (n_out,)
    cross = (1 << 32) // down                               # n * down passes 2^32 between cross and cross + 1
    assert cross * down < (1 << 32) <= (cross + 1) * down and cross + 4 < n_out
    ns = set(range(n_out - 16, n_out)) | set(range(cross - 3, cross + 5)) | set(range(8))
    rng = np.random.Generator(np.random.PCG64(23))
    while len(ns) < 256:
        ns.add(int(rng.integers(0, n_out)))
    ns = sorted(ns)
    ref = RR.resample_at(_Scaled(pcm), 48000, 22050, ns)
    got = y[torch.tensor(ns, device=cuda)].cpu().numpy()
    assert within(got, ref)


class _Scaled:
    """int16 PCM read as s / 32768 slice by slice (the yardstick converts what it slices)."""

    def __init__(self, pcm):
        self.pcm = pcm

    def __len__(self):
        return len(self.pcm)

    def __getitem__(self, s):
        return self.pcm[s].astype(np.float64) / 32768.0


# ---- 4. trim ------------------------------------------------------------------------------------------------------
def test_trim_bounds_equal_yardstick(A, AP, cuda):
    sig = RR.trim_signal()
    cases = [sig, sig[:13000], np.zeros(5000)]
    want = [RR.trim(c) for c in cases]
    assert want == [RR.TRIM_BOUNDS, (3584, 13000), (0, 0)]
    for c, w in zip(cases, want):
        y = torch.from_numpy(c.astype(np.float32)).to(cuda)
        out, bounds = A.trim(y)
        assert bounds == w and out.is_cuda and torch.equal(out, y[w[0]:w[1]])
    # B = 2, different bounds per row: the signal, and the signal delayed by 1024 samples and cut to the same length
    two = np.stack([sig, np.concatenate([np.zeros(1024), sig])[:len(sig)]]).astype(np.float32)
    want2 = [RR.trim(r) for r in two]
    assert want2[0] != want2[1]
    b = A.trim(torch.from_numpy(two).to(cuda))
    assert b.is_cuda and b.dtype == torch.int64 and b.cpu().tolist() == [list(w) for w in want2]
    t = AP.trim_silence(torch.from_numpy(sig.astype(np.float32)).to(cuda))
    assert t.is_cuda and t.shape == (RR.TRIM_BOUNDS[1] - RR.TRIM_BOUNDS[0],)


# ---- 5. batched chunks equal per-chunk calls ----------------------------------------------------------------------
def test_chunk_images_equal_per_chunk_calls(A, AP, cuda):
    chunk = 66150
    t = np.arange(int(2.5 * chunk)) / 22050.0
    y = (0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.25 * np.sin(2 * np.pi * 3000.0 * t) * (t > 4.0)).astype(np.float32)
    yd = torch.from_numpy(y).to(cuda)
    imgs = A.chunk_mel_images(yd, 22050, chunk)
    assert imgs.shape == (3, 128, 130) and imgs.dtype == torch.uint8 and imgs.is_cuda
    for k in range(3):
        piece = yd[k * chunk:(k + 1) * chunk]
        piece = torch.nn.functional.pad(piece, (0, chunk - piece.numel()))      # the last chunk is zero-padded
        assert torch.equal(imgs[k], AP.quantize(AP.get_mel_spectogram(piece, 22050, n_mels=128)))
    assert len(torch.unique(imgs[2])) > 8 and not torch.equal(imgs[0], imgs[1])


# ---- 6, 7. end to end and surface ---------------------------------------------------------------------------------
def _write_stereo_wav(path, pcm, rate):
    body = np.ascontiguousarray(pcm, dtype="<i2").tobytes()
    ch = pcm.shape[1]
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, 1, ch, rate, rate * 2 * ch, 2 * ch, 16)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(body)) + body)


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """audio/piano/take1.wav (44100 Hz stereo PCM16) and audio/violin/solo.wav (22050 Hz mono PCM16)."""
    from data.audio_processor import save_wav
    root = tmp_path_factory.mktemp("rec")
    stereo, mono = RR.dataset_signals()
    (root / "audio" / "piano").mkdir(parents=True)
    (root / "audio" / "violin").mkdir(parents=True)
    _write_stereo_wav(root / "audio" / "piano" / "take1.wav", stereo, 44100)
    save_wav(root / "audio" / "violin" / "solo.wav", mono, 22050)
    return root, stereo, mono


def test_build_dataset_end_to_end(A, cuda, recordings):
    from PIL import Image
    from data.build_dataset import build_dataset_folder_structure
    root, stereo, mono = recordings
    out = root / "images"
    written = build_dataset_folder_structure(audio_dir=str(root / "audio"), output_root=str(out), verbose=False)
    assert sorted(p.name for p in out.iterdir()) == ["piano", "violin"]
    assert sorted(p.name for p in (out / "piano").iterdir()) == [f"take1_chunk{k}.png" for k in range(3)]
    assert sorted(p.name for p in (out / "violin").iterdir()) == [f"solo_chunk{k}.png" for k in range(3)]
    assert len(written) == 6
    for p in written:
        with Image.open(p) as im:
            assert im.mode == "L" and im.size == (130, 128)

    def first_image(folder, name):
        with Image.open(out / folder / name) as im:
            return np.array(im)

    def yardstick_image(y64):
        s, e = RR.trim(y64)
        y = torch.from_numpy(y64[s:e].astype(np.float32)).to(cuda)
        return A.chunk_mel_images(y, 22050, 66150)[0].cpu().numpy()

    # 22050 Hz: no resampling, the yardstick's audio is the file's audio: exact
    assert np.array_equal(first_image("violin", "solo_chunk0.png"), yardstick_image(RR.pcm_to_mono(mono).astype(np.float64)))
    # 44100 Hz: the fp32 resampler against the float64 one: at most one grey level on at most 0.1 % of the pixels
    want = yardstick_image(RR.resample(RR.pcm_to_mono(stereo), 44100, 22050))
    d = np.abs(first_image("piano", "take1_chunk0.png").astype(np.int32) - want.astype(np.int32))
    print(f"pixels that differ: {int((d > 0).sum())} of {d.size}, largest step {int(d.max())}")
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_load_audio_native_and_trim_silence_surface(AP, cuda, recordings):
    root, stereo, mono = recordings
    y, sr = AP.load_audio_native(str(root / "audio" / "piano" / "take1.wav"))
    assert sr == 22050 and y.is_cuda and y.dtype == torch.float32 and y.shape == (math.ceil(len(stereo) / 2),)
    y2, sr2 = AP.load_audio_native(str(root / "audio" / "violin" / "solo.wav"))
    assert sr2 == 22050 and np.array_equal(y2.cpu().numpy(), RR.pcm_to_mono(mono))
    t = AP.trim_silence(y)
    assert t.is_cuda and 0 < t.numel() < y.numel()
    from data.audio_processor import _have_librosa
    tn = AP.trim_silence(y.cpu().numpy())              # numpy in, numpy out
    assert isinstance(tn, np.ndarray)
    if not _have_librosa():                            # the native path
        assert np.array_equal(tn, t.cpu().numpy())
