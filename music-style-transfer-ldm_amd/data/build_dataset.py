"""The chunking half of the reference's data/build_dataset.py: a directory of recordings, one folder per instrument,
becomes the folders of 8-bit log-mel PNGs that ImageFolderNoSubdirs, SpectrogramDataset and SpectrogramPairDataset
read.  Each file is loaded and resampled (AudioPreprocessor.load_audio_native), trimmed (ldm_amd.audio.trim) and
turned into all of its chunk images by one ldm_amd.audio.chunk_mel_images call, on the GPU and without librosa.

.wav input only: .mp3 decoding needs librosa and is not attempted, and the reference's network ingestion and its
parquet variant are not built.
"""
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data.audio_processor import AudioPreprocessor   # noqa: E402


def chunks_within(n_samples, chunk_size, sr, max_duration):
    """How many chunks of chunk_size samples the reference's loop writes for n_samples: one per start i = k * chunk_size
    below n_samples, stopping at the first start with i / sr >= max_duration (None: no limit)."""
    n = -(-n_samples // chunk_size)
    if max_duration is not None:
        k = 0
        while k < n and (k * chunk_size) / sr < max_duration:
            k += 1
        n = k
    return n


def build_dataset_folder_structure(audio_dir="downloads", output_root="processed_images", chunk_size_sec=3,
                                   max_duration=1800, n_mels=128, pattern="*.wav", device="cuda", verbose=True):
    """Write {output_root}/{instrument}/{stem}_chunk{idx}.png for every file under audio_dir that matches pattern;
    the instrument is the file's parent folder name.  A chunk is int(chunk_size_sec * sr) samples, the last one
    zero-padded; chunks starting at or after max_duration seconds are not written.  Returns the paths written."""
    from PIL import Image
    from ldm_amd import audio

    ap = AudioPreprocessor()
    written = []
    for path in sorted(Path(audio_dir).rglob(pattern)):
        out_dir = Path(output_root) / path.parent.name
        out_dir.mkdir(parents=True, exist_ok=True)
        if verbose:
            print(f"Processing file: {path}")
        y, sr = ap.load_audio_native(str(path), device=device)
        y, _ = audio.trim(y)
        chunk_size = int(chunk_size_sec * sr)
        n = chunks_within(y.numel(), chunk_size, sr, max_duration)
        if n == 0:
            continue
        images = audio.chunk_mel_images(y[:n * chunk_size], sr, chunk_size, n_mels=n_mels).cpu().numpy()
        for idx, px in enumerate(images):
            target = out_dir / f"{path.stem}_chunk{idx}.png"
            Image.fromarray(px).save(target)   # mode L, as mel_spectogram_to_grayscale_image
            written.append(target)
        if verbose:
            print(f"Finished processing file: {path} ({len(images)} images)")
    return written


if __name__ == "__main__":
    build_dataset_folder_structure()
