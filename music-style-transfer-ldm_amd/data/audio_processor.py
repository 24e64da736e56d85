"""The reference's AudioPreprocessor (data/audio_processor.py): the 8-bit mel PNG format either side of
the path.

The quantisation (log-mel dB -> uint8 pixel, :55-73) and its inverse (:91-93) are kept bit-exact with
the reference's numpy float32 arithmetic; given a CUDA tensor they run as HIP kernels (dataio.hip),
given a numpy array they run the reference's numpy code.

The audio steps (mel spectrogram, STFT, Griffin-Lim) are librosa calls in the reference.  Here a CUDA tensor runs
the native kernels (ldm_amd/audio.py, csrc/audio.hip) and returns CUDA tensors; a numpy array goes to librosa
when it is importable, else through the native path when a HIP device is present (numpy out); with neither the
method raises ImportError naming librosa.  trim_silence follows the same rule (ldm_amd.audio.trim).  load_audio
falls back to a RIFF reader (PCM16 / float32) and refuses a file at another rate; load_audio_native reads the same
files at any rate and resamples them to target_sr on the GPU (ldm_amd.audio.resample / resample_pcm16).
"""
import os
import sys
from io import BytesIO

import struct
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _librosa():
    try:
        import librosa
    except ImportError as e:
        raise ImportError("AudioPreprocessor: this method needs librosa (audio decoding / mel filterbank / "
                          "Griffin-Lim), which is not installed") from e
    return librosa


def _is_cuda_tensor(x):
    try:
        import torch
    except ImportError:   # pragma: no cover
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


def _have_librosa():
    try:
        import librosa  # noqa: F401
    except ImportError:
        return False
    return True


def _native(x):
    """None: use librosa.  Else (audio module, CUDA tensor of x, whether x came as numpy)."""
    if _is_cuda_tensor(x):
        from ldm_amd import audio
        return audio, x, False
    if _have_librosa():
        return None
    import torch
    if not torch.cuda.is_available():
        _librosa()   # raises the ImportError
    from ldm_amd import audio
    return audio, torch.as_tensor(np.asarray(x)).to("cuda"), True


def _out(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


def read_wav_raw(filepath):
    """(samples [frames, channels] as stored: int16 PCM or float32, rate) of a PCM16 or float32 .wav file."""
    with open(filepath, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{filepath}: not a RIFF/WAVE file")
        fmt = data = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                break
            size = struct.unpack("<I", ck[4:])[0]
            body = f.read(size + (size & 1))[:size]
            if ck[:4] == b"fmt ":
                fmt = struct.unpack("<HHIIHH", body[:16])
            elif ck[:4] == b"data":
                data = body
    if fmt is None or data is None:
        raise ValueError(f"{filepath}: missing fmt or data chunk")
    tag, ch, rate, _, _, bits = fmt
    if tag == 1 and bits == 16:
        x = np.frombuffer(data[:len(data) // 2 * 2], dtype="<i2").astype(np.int16)
    elif tag == 3 and bits == 32:
        x = np.frombuffer(data[:len(data) // 4 * 4], dtype="<f4").astype(np.float32)
    else:
        raise ValueError(f"{filepath}: only PCM16 and float32 .wav are read (format tag {tag}, {bits} bits)")
    return x[:len(x) // ch * ch].reshape(-1, ch), rate


def read_wav(filepath):
    """(float32 samples [frames, channels] in [-1, 1), rate) of a PCM16 or float32 .wav file."""
    x, rate = read_wav_raw(filepath)
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    return x, rate


def save_wav(path, audio, sr):
    """Write mono audio in [-1, 1] as 16-bit PCM (clipped, scaled by 32767), the counterpart of load_audio."""
    if _is_cuda_tensor(audio):
        audio = audio.detach().cpu().numpy()
    a = np.asarray(audio)
    if a.dtype != np.int16:
        a = (np.clip(a.astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(a.reshape(-1).astype("<i2").tobytes())


class AudioPreprocessor:
    def __init__(self, target_sr=22050):
        self.target_sr = target_sr

    def load_audio(self, filepath):
        if _have_librosa():
            return _librosa().load(filepath, sr=self.target_sr, mono=True)
        x, rate = read_wav(filepath)
        if rate != self.target_sr:
            raise ValueError(f"{filepath}: sample rate {rate} differs from target_sr {self.target_sr} and "
                             "resampling is unsupported without librosa")
        return x.mean(axis=1, dtype=np.float32), rate

    def load_audio_native(self, filepath, device="cuda"):
        """(CUDA float32 mono [L'], target_sr) of a PCM16 or float32 .wav at any rate: PCM16 travels to the device as
        int16 and is decoded and mixed inside the resampler, float32 is mixed on the host and uploaded as float."""
        import torch
        from ldm_amd import audio
        x, rate = read_wav_raw(filepath)
        if x.shape[0] == 0:
            raise ValueError(f"{filepath}: no samples")
        if x.dtype == np.int16 and rate != self.target_sr:
            return audio.resample_pcm16(torch.from_numpy(x).to(device), rate, self.target_sr), self.target_sr
        if x.dtype == np.int16:
            x = x.astype(np.float32) / 32768.0
        y = torch.from_numpy(x.mean(axis=1, dtype=np.float32)).to(device)
        return audio.resample(y, rate, self.target_sr), self.target_sr

    save_wav = staticmethod(save_wav)

    def trim_silence(self, audio, top_db=20):
        nat = _native(audio)
        if nat is not None:
            A, y, as_np = nat
            return _out(A.trim(y, top_db=top_db)[0], as_np)
        trimmed, _ = _librosa().effects.trim(audio, top_db=top_db)
        return trimmed

    def normalize_audio(self, audio, target_lufs=-23.0, true_peak_db=-1.0):
        """The reference's TODO stub made real: mono audio at target_sr brought to target_lufs of integrated loudness
        (ITU-R BS.1770-4) under a look-ahead limiter that holds the true peak below true_peak_db
        (ldm_amd.audio.loudness_normalize, on the GPU like trim_silence).  numpy in -> numpy out, CUDA tensor in -> CUDA
        tensor out.  Silence is returned as it is.  The dataset builder does not call it: every chunk's log-mel is
        referred to its own maximum, so a gain changes no image."""
        from ldm_amd import audio as A
        A.check_loudness_args(target_lufs, true_peak_db, 5.0, "normalize_audio")
        if _is_cuda_tensor(audio):
            y, as_np = audio, False
        else:
            import torch
            y, as_np = torch.as_tensor(np.asarray(audio, dtype=np.float32)).to("cuda"), True
        return _out(A.loudness_normalize(y, float(target_lufs), true_peak_db, sr=self.target_sr)[0], as_np)

    def get_mel_spectogram(self, audio, sr, n_mels=256):
        nat = _native(audio)
        if nat is not None:
            A, y, as_np = nat
            return _out(A.power_to_db(A.melspectrogram(y, sr=sr, n_mels=n_mels)), as_np)
        lr = _librosa()
        return lr.power_to_db(lr.feature.melspectrogram(y=audio, sr=sr, n_mels=n_mels), ref=np.max)

    @staticmethod
    def quantize(spectogram, max_db=80):
        """uint8 pixels of a log-mel dB array: clip((db + max_db) * 255/max_db, 0, 255) + 0.5, truncated.
        numpy in -> numpy out (the reference's arithmetic); CUDA tensor in -> CUDA uint8 tensor (HIP)."""
        if _is_cuda_tensor(spectogram):
            from ldm_amd import ops
            return ops.mel_quantize(spectogram, max_db)
        spectogram = np.asarray(spectogram, dtype=np.float32)
        spectogram = spectogram + max_db
        spectogram = spectogram * (255.0 / max_db)
        spectogram = np.clip(spectogram, 0, 255)
        return (spectogram + 0.5).astype(np.uint8)

    @staticmethod
    def dequantize(pixels, max_db=80):
        """log-mel dB of uint8 pixels: u8 * max_db/255 - max_db (the first half of :81-100)."""
        if _is_cuda_tensor(pixels):
            from ldm_amd import ops
            return ops.mel_dequantize(pixels, max_db)
        return np.asarray(pixels, dtype=np.uint8).astype(np.float32) * (max_db / 255.0) - max_db

    def mel_spectogram_to_grayscale_image(self, spectogram, max_db=80):
        from PIL import Image
        px = self.quantize(spectogram, max_db)
        if _is_cuda_tensor(px):
            px = px.cpu().numpy()
        return Image.fromarray(px)

    def get_raw_image_bytes(self, image):
        with BytesIO() as output:
            image.save(output, format="PNG")
            return output.getvalue()

    @staticmethod
    def _pixels(image, im_height, im_width):
        if _is_cuda_tensor(image):
            return image.reshape(image.shape[:-2] + (im_height, im_width))
        return np.frombuffer(image.tobytes(), dtype=np.uint8).reshape(im_height, im_width)

    def grayscale_mel_spectogram_image_to_audio(self, image, sr, im_height, im_width, max_db=80):
        """image: a PIL image (as the reference), or a CUDA uint8 tensor [..., im_height, im_width] of its pixels."""
        px = self._pixels(image, im_height, im_width)
        nat = _native(px)
        if nat is not None:
            A, p, as_np = nat
            return _out(A.mel_to_audio(A.db_to_power(self.dequantize(p, max_db)), sr=sr), as_np)
        lr = _librosa()
        return lr.feature.inverse.mel_to_audio(lr.db_to_power(self.dequantize(px, max_db)), sr=sr)

    def grayscale_spectogram_image_to_audio(self, image, im_height, im_width, max_db=80, n_iter=32):
        """The inverse of get_spectogram's 8-bit image: amplitude dB pixels -> |STFT| -> Griffin-Lim."""
        px = self._pixels(image, im_height, im_width)
        nat = _native(px)
        if nat is not None:
            A, p, as_np = nat
            return _out(A.griffinlim(A.db_to_power(self.dequantize(p, max_db) * 0.5), n_iter=n_iter), as_np)
        lr = _librosa()
        return lr.griffinlim(lr.db_to_amplitude(self.dequantize(px, max_db)), n_iter=n_iter)

    def audio_to_model_input(self, audio, n_mels=128, frames=512, max_db=80):
        """Audio [B, L] or [L] (CUDA tensor, or numpy with a HIP device) -> the model's [B, 1, n_mels, frames] input
        in [0, 1]: the audio is cut or zero-padded to (frames - 1) * hop samples, then log-mel -> 8-bit -> / 255."""
        import torch
        from ldm_amd import audio as A, ops
        y = audio if _is_cuda_tensor(audio) else torch.as_tensor(np.asarray(audio, dtype=np.float32)).to("cuda")
        y = y.reshape(1, -1) if y.dim() == 1 else y
        want = (frames - 1) * (A.N_FFT // 4)
        y = y[:, :want] if y.shape[1] >= want else torch.nn.functional.pad(y, (0, want - y.shape[1]))
        db = A.power_to_db(A.melspectrogram(y, sr=self.target_sr, n_mels=n_mels))
        return ops.u8_to_unit(ops.mel_quantize(db, max_db)).unsqueeze(1)

    def model_output_to_audio(self, x, sr, max_db=80, seed=None):
        """The model's [B, 1, n_mels, T] output in [0, 1] -> waveform [B, (T - 1) * hop] (CUDA tensor)."""
        import torch
        from ldm_amd import audio as A, ops
        px = (x.reshape(x.shape[0], x.shape[-2], x.shape[-1]).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
        return A.mel_to_audio(A.db_to_power(ops.mel_dequantize(px, max_db)), sr=sr, seed=seed)

    def get_spectogram(self, audio):
        nat = _native(audio)
        if nat is not None:
            A, y, as_np = nat
            return _out(A.power_to_db(A.spectrogram(y, power=2)), as_np)   # amplitude_to_db(|S|) = power_to_db(|S|^2)
        lr = _librosa()
        return lr.amplitude_to_db(np.abs(lr.stft(audio)), ref=np.max)

    def spectogram_to_grayscale_image(self, spectogram, max_db=80):
        return self.mel_spectogram_to_grayscale_image(spectogram, max_db)
