"""Score a transfer that already exists as files: what it kept of the content and how far it moved towards the style
(ldm_amd.metrics.transfer_report).  No model is needed.

    python -m models.evaluate --content a.wav --output o.wav --style b.wav
    python -m models.evaluate --content a.wav --output o.wav --style b.wav c.wav --keep-time 0:10 --keep-band 0:200
    python -m models.evaluate --content a.wav --output o.wav --style b.wav --trim --report scores.json
    python -m models.evaluate --content a.wav --output o.wav --style b.wav --loudness

The files are read and resampled to 22050 Hz as python -m models.transfer reads them.  Content and output must have
one length: models.transfer trims the silence around its content before the transfer, so for an output it wrote pass
--trim, which trims the content (and the styles) the same way.
"""
import argparse
import math

import torch

from . import _pathfix  # noqa: F401
from ldm_amd import audio, longform, metrics
from .transfer import HOP, _span, write_report


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m models.evaluate", description=__doc__.split("\n\n")[0])
    p.add_argument("--content", required=True, help="the recording that was transferred (.wav)")
    p.add_argument("--output", required=True, help="the result of the transfer (.wav)")
    p.add_argument("--style", required=True, nargs="+", help="the style recording(s) (.wav); several are pooled")
    p.add_argument("--keep-time", action="append", default=[], dest="keep_time", metavar="T0:T1", type=_span,
                   help="the seconds T0 to T1 were kept (repeatable): adds kept_rms_db / changed_rms_db")
    p.add_argument("--keep-band", action="append", default=[], dest="keep_band", metavar="F0:F1", type=_span,
                   help="the mel bins whose centre frequency lies in F0 to F1 Hz were kept (repeatable)")
    p.add_argument("--keep-feather", type=int, default=0, dest="keep_feather", metavar="N",
                   help="the kept regions were ramped over their N outermost frames (bins)")
    p.add_argument("--trim", action="store_true",
                   help="trim the silence around the content and the styles as python -m models.transfer does")
    p.add_argument("--n-mfcc", type=int, default=20, dest="n_mfcc", help="MFCCs of the timbre distances (2..32)")
    p.add_argument("--loudness", action="store_true",
                   help="also print the content's, the output's and the style's integrated loudness (LUFS, ITU-R "
                        "BS.1770-4) and true peaks (dB relative to full scale)")
    p.add_argument("--report", default="-", metavar="PATH", help="write the JSON to PATH instead of printing it")
    args = p.parse_args(argv)
    if args.keep_feather < 0:
        p.error("--keep-feather must not be negative")
    if not 2 <= args.n_mfcc <= 32:
        p.error("--n-mfcc must lie in 2..32")
    return args


def evaluate_files(content, output, styles, keep_time=(), keep_band=(), keep_feather=0, trim=False, n_mfcc=20,
                   loudness=False):
    """The report dict of the .wav files content, output and styles (a list); with loudness also content_lufs,
    output_lufs, style_lufs and the three true peaks in dB."""
    from data.audio_processor import AudioPreprocessor
    ap = AudioPreprocessor()

    def load(path, trimmed):
        y, sr = ap.load_audio_native(path)
        return (ap.trim_silence(y) if trimmed else y), sr
    c, sr = load(content, trim)
    o, _ = load(output, False)
    s = [load(f, trim)[0] for f in styles]
    if c.numel() != o.numel():
        raise ValueError(f"evaluate: {content} has {c.numel()} samples and {output} {o.numel()} at {sr} Hz; the frame-"
                         "paired scores need one length" + ("" if trim else " (an output of models.transfer: --trim)"))
    keep = None
    if keep_time or keep_band:
        keep = longform.keep_mask(1 + c.numel() // HOP, 128, sr, times=list(keep_time), bands=list(keep_band),
                                  feather=keep_feather)
    if not loudness:
        return metrics.transfer_report(c, o, s, sr=sr, keep=keep, n_mfcc=n_mfcc)
    rep = metrics.transfer_report(c, o, s, sr=sr, keep=keep, n_mfcc=n_mfcc, loudness=True)
    peaks = torch.stack([audio.true_peak(c, sr)] + [audio.true_peak(y, sr) for y in s]).tolist()
    db = [20.0 * math.log10(v) if v > 0 else -math.inf for v in peaks]
    rep["content_true_peak_db"], rep["style_true_peak_db"] = db[0], max(db[1:])
    return rep


def main(argv=None):
    args = parse_args(argv)
    try:
        rep = evaluate_files(args.content, args.output, args.style, args.keep_time, args.keep_band, args.keep_feather,
                             args.trim, args.n_mfcc, args.loudness)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if args.loudness:
        for name in ("content", "output", "style"):
            print(f"{name}: {rep[name + '_lufs']:.2f} LUFS, true peak {rep[name + '_true_peak_db']:.2f} dB")
    write_report(rep, args.report)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
