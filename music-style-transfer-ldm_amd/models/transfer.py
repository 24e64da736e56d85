"""Style transfer of a whole recording: the content is cut into overlapping windows (ldm_amd.longform), every window
goes through LDM.content_style_transfer_wrapper paired with a window of the style recording, and the decoded windows
are crossfaded into one mel spectrogram that is vocoded once, so the phase is continuous across the seams.

    python -m models.transfer --content a.wav --style b.wav --out c.wav [--checkpoint ldm.pth]
    python -m models.transfer --content a.wav --style b.wav c.wav --style-weights 0.7 0.3 --style-refs 2 --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --guidance-scale 2.5 --out o.wav
    python -m models.transfer --content a.wav --style b.wav c.wav --solver dpmpp2m --style-morph --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --keep-time 0:10 --keep-band 0:200 --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --joint --batch 16 --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --keep-time 0:10 --vocoder content --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --keep-percussive --vocoder content --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --report scores.json --out o.wav
    python -m models.transfer --content a.wav --style b.wav --solver dpmpp2m --loudness content --true-peak -1 --out o.wav

The reference has no counterpart: its audio_reconstruction_test.py handles a single window.
"""
import argparse
import json
import math
from types import SimpleNamespace

import torch

from . import _pathfix  # noqa: F401
from ldm_amd import audio, longform, metrics

HOP = audio.N_FFT // 4


def style_window_indices(Ns, refs):
    """The `refs` style windows taken from a recording with Ns full windows: evenly spaced from the first to the last,
    index round(i (Ns - 1) / (refs - 1)), halves rounding up; a single window is index 0."""
    Ns, refs = int(Ns), int(refs)
    if Ns < 1 or refs < 1:
        raise ValueError(f"style_window_indices: need Ns >= 1 and refs >= 1, got {Ns}, {refs}")
    if refs == 1:
        return [0]
    return [int(math.floor(i * (Ns - 1) / (refs - 1) + 0.5)) for i in range(refs)]


def transfer_recording(model, content, style, sr=22050, frames=512, overlap=64, num_timesteps=100, eta=0.0,
                       batch_size=8, seed=0, n_iter=32, nnls_iters=32, max_db=80, solver=None, t_start=None,
                       style_weights=None, style_refs=1, guidance_scale=1.0, base_style=None, keep=None,
                       composite=True, style_map=None, joint=False, vocoder="griffinlim", max_gain_db=40.0,
                       anchor_db=6.0, residual=True, keep_component=None, hpss_kernel=31, hpss_margin=1.0,
                       report=False, loudness=None, true_peak_db=-1.0):
    """content, style: mono CUDA waveforms [L] at sr.  Returns an object with audio [L], mel_power [n_mels, T_total],
    windows_out [N, 1, n_mels, frames], ref_db [N] and N.

    Call model.eval() first: the decoder's train-mode BatchNorm takes its statistics over the batch, which couples
    the windows of a group and makes the result depend on batch_size.  This function leaves module modes alone.

    Content window n is paired with style window n mod Ns, Ns the style's full windows (overlap 0; its single padded
    window when it has no full one).  The q_sample noise of window n is row n of one CPU draw seeded with `seed`,
    whatever batch_size is.  ValueError for a recording shorter than n_fft / 2 + 1 samples, a bad window plan, or
    num_timesteps beyond the model's schedule.

    solver=None is the reference's sampler: num_timesteps is both the noise level (index num_timesteps - 1) and the
    step count.  With solver "dpmpp2m", "dpmpp1" or "ddim" every window goes through LDM.content_style_transfer
    instead: the content is noised at index t_start (default 99) and denoised in num_timesteps steps.

    Style mixing: `style` may be a list of waveforms, style_refs windows are taken from each (style_window_indices),
    and every content window attends over all of them at once (LDM.encode_styles) instead of being paired with one.
    style_weights: one weight per recording, or [N, recordings] per content window (a morph along the recording);
    default equal.  A recording's weight is shared equally among its windows.  At most LDM.MAX_STYLE_REFS windows
    in all.  One recording, style_refs = 1 and no weights is the cyclic pairing above, unchanged.

    Style guidance (needs a solver): guidance_scale s (a finite float) steers every step from a base style towards
    the target, e_b + s (e_t - e_b) (LDM.content_style_transfer): s > 1 exaggerates the style, 0 < s < 1 applies
    it partly.  base_style "content" (the default when s is not 1) takes each window's own content mel as the
    base; a waveform [L] is windowed and paired like `style`.  s = 1 without a base_style is the unguided call.

    Regional transfer (needs a solver): keep is a mask [n_mels, T_total] in [0, 1] (longform.keep_mask) of what stays
    as it is.  It is cut into windows like the content (longform.mask_windows) and every window's sampler holds the
    kept region on the content's own noising trajectory (LDM.content_style_transfer); with composite the kept region
    of every decoded window is the content window itself.  Composes with mixing and guidance.

    Keeping a component (needs a solver): keep_component "percussive" or "harmonic" keeps that part of the content,
    found by median-filter harmonic / percussive separation of its own STFT (audio.hpss_keep):
    hpss_kernel is the median window (a number or a (harmonic, percussive) pair of odd lengths up to 63 frames / bins),
    hpss_margin the separation margin (likewise, at least 1).  The mask is the share of each mel bin's energy the
    component holds; with keep= as well the two are united by their element-wise maximum.  From there on it is the
    regional transfer above, unchanged.  keep_component=None is the call it always was.

    Style map (needs a solver and style_refs = 1): style_map [recordings, n_mels, T_total] or [recordings, T_total]
    (non-negative, a positive sum over the recordings everywhere; longform.morph_map makes a morph from the first
    recording to the last) says which style applies where, per mel bin and frame.  It is cut into windows like the
    content (longform.style_map_windows) and every window's sampler weighs the references per position
    (LDM.content_style_transfer's style_map).  Composes with style_weights, guidance and keep.

    Joint sampling (joint=True; needs a solver and an overlap that is a multiple of 8): the windows of a model call are
    denoised as one latent canvas.  The q_sample noise comes from longform.noise_windows (one canvas draw seeded with
    `seed`, so neighbours share their overlap's noise) instead of the per-window rows, and every group of batch_size
    consecutive windows goes through LDM.content_style_transfer with seam_overlap=overlap: after every step the
    latent columns two neighbours share are replaced in both by one weighted average, and the crossfade then meets
    two decodings of the same latent instead of two independent samples.  The seam between two groups is not fused
    (its windows only share the canvas noise): batch_size >= N gives one coherent canvas.  Beyond 8 windows per call
    the sampler's bottleneck runs without its value fold (slower per window, the same results up to rounding).
    Composes with mixing, guidance, keep and the style map.  joint=False is the call it always was.

    Vocoder: "griffinlim" (the default, the call it always was) inverts the stitched mel (audio.mel_to_audio: NNLS,
    then Griffin-Lim from a random phase seeded with `seed`).  "content" reads the result as an edit of the content's
    own STFT (audio.mel_to_audio_content): the content's magnitudes scaled by the mel-domain gain
    between the stitched output and the content's mel after the same window / dB clip / crossfade round trip
    (clamped at max_gain_db), plus, with residual, the energy the style adds where the content has none; n_iter
    iterations of Griffin-Lim start from the content's phase and stay anchored to it where the gain is within
    anchor_db of unity (anchor_db <= 0: no anchor), so an untouched or composited region comes back as the content
    itself.  `seed` plays no part in it.  Works with every solver and with solver=None.

    Report: report=True adds .report to the result, the dict of ldm_amd.metrics.transfer_report(content, audio, style)
    (DESIGN.md §7m): onset_corr, chroma_sim, the three timbre distances and timbre_shift, and, when something was
    kept, kept_rms_db / changed_rms_db under the mask the transfer actually used (keep=, keep_component= or their
    union).  It is computed after the audio and changes none of it.  report=False is the call it always was.

    Loudness: loudness="content" brings the output to the content's integrated loudness (ITU-R
    BS.1770-4, audio.integrated_loudness), a float to that many LUFS, and a look-ahead limiter holds the true peak under
    true_peak_db (audio.loudness_normalize).  It is applied after the vocoder, whichever it is; the result gains
    .loudness, loudness_normalize's info plus content_lufs, and .report, when asked for, is computed on the normalised
    audio.  loudness=None is the call it always was: no launch more, bitwise the same audio."""
    n_mels = 128
    if loudness is not None:
        if isinstance(loudness, str):
            if loudness != "content":
                raise ValueError(f"transfer_recording: loudness must be \"content\", a LUFS target or None, got "
                                 f"{loudness!r}")
        elif isinstance(loudness, bool) or not isinstance(loudness, (int, float)):
            raise ValueError(f"transfer_recording: loudness must be \"content\", a LUFS target or None, got "
                             f"{loudness!r}")
        audio.check_loudness_args(None if isinstance(loudness, str) else loudness, true_peak_db, 5.0,
                                  "transfer_recording")
    if vocoder not in ("griffinlim", "content"):
        raise ValueError(f"transfer_recording: vocoder must be \"griffinlim\" or \"content\", got {vocoder!r}")
    audio.check_vocoder_args(max_gain_db, anchor_db, "transfer_recording")
    if joint:
        if solver is None:
            raise ValueError("transfer_recording: joint needs a solver (the reference's sampler has no seam fuse)")
        if int(overlap) % 8:
            raise ValueError(f"transfer_recording: joint needs an overlap that is a multiple of 8 mel frames (whole "
                             f"latent columns), got {overlap}")
    if style_map is not None:
        n_rec = len(style) if isinstance(style, (list, tuple)) else 1
        if solver is None:
            raise ValueError("transfer_recording: style_map needs a solver (the reference's sampler has no style map)")
        if int(style_refs) != 1:
            raise ValueError("transfer_recording: style_map needs style_refs = 1 (one map row per recording)")
        style_map = torch.as_tensor(style_map)
        T_map = 1 + content.numel() // HOP if content.dim() == 1 else -1
        if style_map.dim() not in (2, 3) or style_map.shape[0] != n_rec or style_map.shape[-1] != T_map or \
                (style_map.dim() == 3 and style_map.shape[1] != n_mels):
            raise ValueError(f"transfer_recording: style_map must be [{n_rec}, {n_mels}, {T_map}] or [{n_rec}, {T_map}] "
                             f"(one row per style recording), got {tuple(style_map.shape)}")
        sm = style_map.detach().to(torch.float64)
        if not bool(torch.isfinite(sm).all()) or bool((sm < 0).any()) or bool((sm.sum(0) <= 0).any()):
            raise ValueError("transfer_recording: style_map must be finite and non-negative, with a positive sum over "
                             "the recordings at every position")
    if keep_component is not None:
        if keep_component not in audio.HPSS_COMPONENTS:
            raise ValueError(f"transfer_recording: keep_component must be \"percussive\", \"harmonic\" or None, got "
                             f"{keep_component!r}")
        if solver is None:
            raise ValueError("transfer_recording: keep_component needs a solver (the reference's sampler has no "
                             "regional keep)")
        audio.check_hpss_args(hpss_kernel, 2.0, hpss_margin, "transfer_recording")
        if content.dim() != 1 or content.numel() < audio.N_FFT // 2 + 1:
            raise ValueError(f"transfer_recording: content must be a mono waveform [L] of at least "
                             f"{audio.N_FFT // 2 + 1} samples, got shape {tuple(content.shape)}")
        part = audio.hpss_keep(content, keep_component, kernel_size=hpss_kernel, margin=hpss_margin, sr=sr,
                               n_mels=n_mels).cpu()
        if keep is None:
            keep = part
        else:       # the union of the two, as longform.keep_mask unites its regions
            keep = torch.as_tensor(keep, dtype=torch.float32)
            if keep.shape != part.shape:
                raise ValueError(f"transfer_recording: keep must be a mask [n_mels, T_total] = {list(part.shape)}, "
                                 f"got {tuple(keep.shape)}")
            keep = torch.maximum(keep.cpu(), part)
    if keep is not None:
        if solver is None:
            raise ValueError("transfer_recording: keep needs a solver (the reference's sampler has no regional keep)")
        keep = torch.as_tensor(keep, dtype=torch.float32)
        T_keep = 1 + content.numel() // HOP if content.dim() == 1 else -1
        if tuple(keep.shape) != (n_mels, T_keep):
            raise ValueError(f"transfer_recording: keep must be a mask [n_mels, T_total] = [{n_mels}, {T_keep}], got "
                             f"{tuple(keep.shape)}")
        if not bool(torch.isfinite(keep).all()) or float(keep.min()) < 0 or float(keep.max()) > 1:
            raise ValueError("transfer_recording: keep must be finite and lie in [0, 1]")
    guided = base_style is not None or float(guidance_scale) != 1.0
    if guided:
        if not math.isfinite(float(guidance_scale)):
            raise ValueError(f"transfer_recording: guidance_scale must be finite, got {guidance_scale}")
        if solver is None:
            raise ValueError("transfer_recording: guidance_scale / base_style need a solver (the reference's sampler "
                             "has no guidance)")
        if base_style is None:
            base_style = "content"
        if not isinstance(base_style, str) and (base_style.dim() != 1 or base_style.numel() < audio.N_FFT // 2 + 1):
            raise ValueError(f"transfer_recording: base_style must be \"content\" or a mono waveform [L] of at least "
                             f"{audio.N_FFT // 2 + 1} samples")
        if isinstance(base_style, str) and base_style != "content":
            raise ValueError(f"transfer_recording: base_style must be \"content\" or a waveform, got {base_style!r}")
    styles = list(style) if isinstance(style, (list, tuple)) else [style]
    if not styles:
        raise ValueError("transfer_recording: no style recording")
    style_refs = int(style_refs)
    mixing = len(styles) > 1 or style_refs != 1 or style_weights is not None or style_map is not None
    if style_refs < 1 or len(styles) * style_refs > model.MAX_STYLE_REFS:
        raise ValueError(f"transfer_recording: {len(styles)} recordings x style_refs {style_refs} must give 1 to "
                         f"{model.MAX_STYLE_REFS} style windows")
    style = styles[0]
    for name, y in [("content", content)] + [("style", y) for y in styles]:
        if y.dim() != 1 or y.numel() < audio.N_FFT // 2 + 1:
            raise ValueError(f"transfer_recording: {name} must be a mono waveform [L] of at least "
                             f"{audio.N_FFT // 2 + 1} samples, got shape {tuple(y.shape)}")
    if solver is None and t_start is not None:
        raise ValueError("transfer_recording: t_start needs a solver (solver=None is the reference's sampler, whose "
                         "noise level is num_timesteps - 1)")
    if solver is not None:
        t_start = 99 if t_start is None else int(t_start)
        model.sample_times(t_start, num_timesteps)    # ValueError for a bad (t_start, steps) pair
    if not 1 <= num_timesteps <= model.num_timesteps:
        raise ValueError(f"transfer_recording: num_timesteps {num_timesteps} outside the model's schedule "
                         f"(1..{model.num_timesteps})")
    if batch_size < 1:
        raise ValueError(f"transfer_recording: batch_size must be positive, got {batch_size}")
    Ln = content.numel()
    T_total = 1 + Ln // HOP
    N, _ = longform.window_plan(T_total, frames, overlap)

    x, ref_db = longform.mel_windows(audio.melspectrogram(content, sr=sr, n_mels=n_mels), frames, overlap, max_db)
    Ps = audio.melspectrogram(style, sr=sr, n_mels=n_mels)
    xs, _ = longform.mel_windows(Ps, frames, 0, max_db)
    Ns = max(1, Ps.shape[-1] // frames)       # the full windows; a style shorter than one keeps its padded window
    xs = xs[:Ns]

    voc = None
    if vocoder == "content":
        voc = dict(content=content, x=x, max_gain_db=float(max_gain_db), anchor_db=float(anchor_db),
                   residual=bool(residual))

    latent = model.unet.enc1.weight.shape[1]
    if joint:
        noise = longform.noise_windows(N, latent, n_mels // 8, frames // 8, overlap // 8, seed)
    else:
        noise = torch.randn((N, latent, n_mels // 8, frames // 8), generator=torch.Generator().manual_seed(int(seed)))
    noise = noise.to(content.device)

    keep_w = None if keep is None else longform.mask_windows(keep, frames, overlap).to(content.device)
    map_w = None if style_map is None else longform.style_map_windows(style_map, frames, overlap, n_mels)

    def guide_kw(b0, b1):
        """content_style_transfer's guidance and keep arguments for windows [b0, b1): none when neither is asked for."""
        kw = {} if keep_w is None else {"keep": keep_w[b0:b1], "composite": bool(composite)}
        if joint and overlap:     # the group's windows as one canvas (a group of one has no seam to fuse)
            kw["seam_overlap"] = int(overlap)
        if map_w is not None:
            kw["style_map"] = map_w[b0:b1]
        if not guided:
            return kw
        if isinstance(base_style, str):
            return dict(kw, guidance_scale=float(guidance_scale), base_style=x[b0:b1])
        return dict(kw, guidance_scale=float(guidance_scale),
                    base_style=xb[torch.arange(b0, b1, device=xb.device) % Nb])

    def done(out):
        res = _finish(out, ref_db, overlap, T_total, max_db, sr, n_iter, nnls_iters, seed, Ln, N, voc)
        if loudness is not None:
            content_lufs = audio.integrated_loudness(content, sr)
            target = content_lufs.reshape(1) if isinstance(loudness, str) else float(loudness)
            res.audio, res.loudness = audio.loudness_normalize(res.audio, target, true_peak_db, sr=sr)
            res.loudness["content_lufs"] = float(content_lufs)
        if report:
            res.report = metrics.transfer_report(content, res.audio, styles, sr=sr, keep=keep)
        return res

    if guided and not isinstance(base_style, str):
        Pb = audio.melspectrogram(base_style, sr=sr, n_mels=n_mels)
        xb, _ = longform.mel_windows(Pb, frames, 0, max_db)
        Nb = max(1, Pb.shape[-1] // frames)
        xb = xb[:Nb]
    if mixing:
        refs = [xs[style_window_indices(Ns, style_refs)]]
        for y in styles[1:]:
            Pr = audio.melspectrogram(y, sr=sr, n_mels=n_mels)
            xr, _ = longform.mel_windows(Pr, frames, 0, max_db)
            refs.append(xr[style_window_indices(max(1, Pr.shape[-1] // frames), style_refs)])
        refs = torch.cat(refs)                                  # [R, 1, n_mels, frames], recording-major
        w = None
        if style_weights is not None:
            w = torch.as_tensor(style_weights, dtype=torch.float64).detach().cpu()
            if w.dim() not in (1, 2) or w.shape[-1] != len(styles) or (w.dim() == 2 and w.shape[0] != N):
                raise ValueError(f"transfer_recording: style_weights must be [{len(styles)}] (one per recording) or "
                                 f"[{N}, {len(styles)}] (per content window), got {tuple(w.shape)}")
            model.normalise_style_weights(w, len(styles))              # the checks; encode_styles normalises
            w = w.repeat_interleave(style_refs, dim=-1) / style_refs   # shared equally among a recording's windows
        out = []
        with torch.no_grad():
            for b0 in range(0, N, batch_size):
                b1 = min(b0 + batch_size, N)
                spec = refs.unsqueeze(0).expand((b1 - b0,) + tuple(refs.shape))
                wb = None if w is None else (w if w.dim() == 1 else w[b0:b1])
                if solver is None:
                    decoded, _ = model.content_style_transfer_wrapper(x[b0:b1], spec, num_timesteps=num_timesteps,
                                                                      eta=eta, noise=noise[b0:b1], style_weights=wb)
                else:
                    decoded, _ = model.content_style_transfer(x[b0:b1], spec, t_start=t_start, steps=num_timesteps,
                                                              solver=solver, eta=eta, noise=noise[b0:b1],
                                                              style_weights=wb, **guide_kw(b0, b1))
                out.append(decoded)
        return done(out)
    pair = torch.arange(N, device=content.device) % Ns
    out = []
    with torch.no_grad():
        for b0 in range(0, N, batch_size):
            b1 = min(b0 + batch_size, N)
            if solver is None:
                decoded, _ = model.content_style_transfer_wrapper(x[b0:b1], xs[pair[b0:b1]],
                                                                  num_timesteps=num_timesteps, eta=eta,
                                                                  noise=noise[b0:b1])
            else:
                decoded, _ = model.content_style_transfer(x[b0:b1], xs[pair[b0:b1]], t_start=t_start,
                                                          steps=num_timesteps, solver=solver, eta=eta,
                                                          noise=noise[b0:b1], **guide_kw(b0, b1))
            out.append(decoded)
    return done(out)


def _finish(out, ref_db, overlap, T_total, max_db, sr, n_iter, nnls_iters, seed, Ln, N, voc=None):
    windows_out = torch.cat(out)
    mel_power = longform.stitch_windows(windows_out, ref_db, overlap, T_total, max_db)
    if voc is None:
        y = audio.mel_to_audio(mel_power, sr=sr, n_iter=n_iter, nnls_iters=nnls_iters, seed=seed, length=Ln)
    else:
        # the content's mel through the windows, the dB clip and the crossfade the output went through: G = 1 wherever
        # a decoded window is the content window
        mel_content = longform.stitch_windows(voc["x"], ref_db, overlap, T_total, max_db)
        y = audio.mel_to_audio_content(mel_power, voc["content"], mel_content, sr=sr, n_iter=n_iter,
                                       max_gain_db=voc["max_gain_db"], anchor_db=voc["anchor_db"],
                                       residual=voc["residual"], nnls_iters=nnls_iters, max_db=max_db, length=Ln)
    return SimpleNamespace(audio=y, mel_power=mel_power, windows_out=windows_out, ref_db=ref_db, N=N)


def load_model(checkpoint=None, device="cuda"):
    """An eval-mode LDM on `device`; `checkpoint` is a full ldm.pth state dict, loaded by component prefix the way
    LDM.__init__ does (None: freshly initialised weights)."""
    from .config import config
    from .model import LDM
    model = LDM(config["latent_dim_encoder"], pretrained_path="")
    if checkpoint:
        sd = torch.load(checkpoint, map_location="cpu", weights_only=True)
        for prefix, mod in (("encoder.", model.encoder), ("decoder.", model.decoder), ("unet.", model.unet),
                            ("style_encoder.", model.style_encoder), ("noise_scheduler.", model.noise_scheduler)):
            mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    return model.to(device).eval()


def _span(text):
    """argparse type of --keep-time / --keep-band: "A:B" with A <= B as a pair of floats."""
    try:
        a, b = (float(v) for v in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected LOW:HIGH, got {text!r}") from None
    if not (math.isfinite(a) and math.isfinite(b) and a <= b):
        raise argparse.ArgumentTypeError(f"expected finite LOW <= HIGH, got {text!r}")
    return (a, b)


def _loudness(text):
    """argparse type of --loudness: "content" or a finite number of LUFS."""
    if text == "content":
        return text
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected \"content\" or a number of LUFS, got {text!r}") from None
    if not math.isfinite(v):
        raise argparse.ArgumentTypeError(f"expected a finite number of LUFS, got {text!r}")
    return v


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m models.transfer", description=__doc__.split("\n\n")[0])
    p.add_argument("--content", required=True, help="the recording to transfer (.wav, PCM16 or float32, any rate)")
    p.add_argument("--style", required=True, nargs="+",
                   help="the recording whose style is applied (.wav); several files are mixed")
    p.add_argument("--style-weights", type=float, nargs="+", default=None, dest="style_weights",
                   help="one non-negative weight per --style file (default equal)")
    p.add_argument("--style-morph", action="store_true", dest="style_morph",
                   help="morph from the first --style file to the last along the recording (needs --solver and at "
                        "least two --style files): a style map of triangular weights over time")
    p.add_argument("--style-refs", type=int, default=1, dest="style_refs",
                   help="windows taken from each style recording, evenly spaced; with more than one window in all, "
                        "every content window attends over all of them")
    p.add_argument("--out", required=True, help="the .wav to write (mono PCM16 at 22050 Hz)")
    p.add_argument("--checkpoint", default=None, help="a full ldm.pth state dict (default: untrained weights)")
    p.add_argument("--frames", type=int, default=512, help="mel frames per window")
    p.add_argument("--overlap", type=int, default=64, help="mel frames two neighbouring windows share")
    p.add_argument("--steps", type=int, default=100, help="diffusion steps per window")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--solver", choices=("dpmpp2m", "dpmpp1", "ddim"), default=None,
                   help="sample with this solver from --t-start in --steps steps (default: the reference's sampler, "
                        "where --steps is also the noise level)")
    p.add_argument("--t-start", type=int, default=None, dest="t_start",
                   help="schedule index the content is noised at (needs --solver; default 99)")
    p.add_argument("--guidance-scale", type=float, default=1.0, dest="guidance_scale",
                   help="style strength s (needs --solver): every step steers the noise prediction from the base style "
                        "towards the target, e_b + s (e_t - e_b); 1 = off, above 1 exaggerates the style, between 0 "
                        "and 1 applies it partly")
    p.add_argument("--base-style", default=None, dest="base_style", metavar="{content|PATH}",
                   help="what the guidance steers away from: \"content\" (each window's own content, the default "
                        "when --guidance-scale is not 1) or a .wav")
    p.add_argument("--keep-time", action="append", default=[], dest="keep_time", metavar="T0:T1", type=_span,
                   help="leave the seconds T0 to T1 of the content as they are (needs --solver; repeatable)")
    p.add_argument("--keep-band", action="append", default=[], dest="keep_band", metavar="F0:F1", type=_span,
                   help="leave the mel bins whose centre frequency lies in F0 to F1 Hz as they are (needs --solver; "
                        "repeatable)")
    p.add_argument("--keep-feather", type=int, default=0, dest="keep_feather", metavar="N",
                   help="ramp every kept region linearly over its N outermost frames (bins)")
    comp = p.add_mutually_exclusive_group()
    comp.add_argument("--keep-percussive", action="store_const", const="percussive", dest="keep_component",
                      default=None,
                      help="leave the percussive part of the content (its drums) as it is (needs --solver): "
                           "median-filter harmonic / percussive separation of the content's own STFT")
    comp.add_argument("--keep-harmonic", action="store_const", const="harmonic", dest="keep_component",
                      help="leave the harmonic part of the content as it is and restyle its percussion (needs --solver)")
    p.add_argument("--hpss-kernel", type=int, nargs="+", default=[31], dest="hpss_kernel", metavar="N",
                   help="the separation's median window, odd, at most 63: one length, or the harmonic filter's frames "
                        "and the percussive filter's bins")
    p.add_argument("--hpss-margin", type=float, nargs="+", default=[1.0], dest="hpss_margin", metavar="M",
                   help="the separation's margin, at least 1: one value, or harmonic and percussive")
    p.add_argument("--no-composite", action="store_false", dest="composite",
                   help="do not paste the content back over the kept region of the decoded windows")
    p.add_argument("--joint", action="store_true",
                   help="denoise the windows of a model call as one latent canvas (needs --solver and an --overlap "
                        "that is a multiple of 8): the columns neighbouring windows share are fused after every step; "
                        "--batch at least the window count gives one coherent canvas")
    p.add_argument("--vocoder", choices=("griffinlim", "content"), default="griffinlim",
                   help="how the stitched mel becomes audio: \"griffinlim\" inverts it from a random phase; "
                        "\"content\" edits the content's own STFT (its magnitudes times the mel-domain gain, its "
                        "phase kept where little changed), so untouched regions come back as they went in")
    p.add_argument("--max-gain-db", type=float, default=40.0, dest="max_gain_db",
                   help="--vocoder content: the most a bin's power may be raised, in dB")
    p.add_argument("--anchor-db", type=float, default=6.0, dest="anchor_db",
                   help="--vocoder content: bins whose power changes by less than this many dB keep (part of) the "
                        "content's phase; 0 or less anchors nothing")
    p.add_argument("--no-residual", action="store_false", dest="residual",
                   help="--vocoder content: do not add the energy the style puts where the content is silent")
    p.add_argument("--report", nargs="?", const="-", default=None, metavar="PATH",
                   help="score the transfer (ldm_amd.metrics.transfer_report: rhythm and harmony kept, timbre moved "
                        "towards the style) and print the scores as one JSON line, or write them to PATH")
    p.add_argument("--loudness", default=None, metavar="{content|LUFS}", type=_loudness,
                   help="bring the output to the content's integrated loudness (\"content\") or to this many LUFS "
                        "(ITU-R BS.1770-4), under a look-ahead true-peak limiter")
    p.add_argument("--true-peak", type=float, default=-1.0, dest="true_peak_db", metavar="DB",
                   help="--loudness: the limiter's true-peak ceiling in dB relative to full scale, at most 0")
    p.add_argument("--batch", type=int, default=8, help="windows per model call")
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if args.style_weights is not None and len(args.style_weights) != len(args.style):
        p.error(f"--style-weights: {len(args.style_weights)} weights for {len(args.style)} --style files")
    if args.style_refs < 1:
        p.error("--style-refs must be positive")
    if args.style_morph and (args.solver is None or len(args.style) < 2 or args.style_refs != 1):
        p.error("--style-morph needs --solver, at least two --style files and --style-refs 1")
    if not math.isfinite(args.guidance_scale):
        p.error("--guidance-scale must be finite")
    if (args.guidance_scale != 1.0 or args.base_style is not None) and args.solver is None:
        p.error("--guidance-scale / --base-style need --solver")
    if (args.keep_time or args.keep_band) and args.solver is None:
        p.error("--keep-time / --keep-band need --solver")
    if args.keep_component is not None and args.solver is None:
        p.error("--keep-percussive / --keep-harmonic need --solver")
    for flag, vals in (("--hpss-kernel", args.hpss_kernel), ("--hpss-margin", args.hpss_margin)):
        if len(vals) > 2:
            p.error(f"{flag} takes one or two values, got {len(vals)}")
    args.hpss_kernel = args.hpss_kernel[0] if len(args.hpss_kernel) == 1 else tuple(args.hpss_kernel)
    args.hpss_margin = args.hpss_margin[0] if len(args.hpss_margin) == 1 else tuple(args.hpss_margin)
    try:
        audio.check_hpss_args(args.hpss_kernel, 2.0, args.hpss_margin, "--hpss-kernel / --hpss-margin")
    except ValueError as e:
        p.error(str(e))
    if args.keep_feather < 0:
        p.error("--keep-feather must not be negative")
    if not math.isfinite(args.max_gain_db) or args.max_gain_db < 0:
        p.error("--max-gain-db must be finite and non-negative")
    if not math.isfinite(args.anchor_db):
        p.error("--anchor-db must be finite")
    if not math.isfinite(args.true_peak_db) or args.true_peak_db > 0:
        p.error("--true-peak must be finite and at most 0 dB")
    if args.joint and args.solver is None:
        p.error("--joint needs --solver")
    if args.joint and args.overlap % 8:
        p.error("--joint needs an --overlap that is a multiple of 8 (whole latent columns)")
    if len(args.style) == 1:
        args.style = args.style[0]      # a single file: the string it always was
    return args


def main(argv=None):
    args = parse_args(argv)
    from data.audio_processor import AudioPreprocessor
    ap = AudioPreprocessor()
    content, sr = ap.load_audio_native(args.content)
    files = [args.style] if isinstance(args.style, str) else list(args.style)
    styles = [ap.trim_silence(ap.load_audio_native(f)[0]) for f in files]
    content = ap.trim_silence(content)
    style = styles[0] if len(styles) == 1 else styles
    model = load_model(args.checkpoint)
    guide = {}
    if args.guidance_scale != 1.0 or args.base_style is not None:   # (without the flags: today's call)
        base = args.base_style
        if base is not None and base != "content":
            base = ap.trim_silence(ap.load_audio_native(base)[0])
        guide = {"guidance_scale": args.guidance_scale, "base_style": base}
    if args.keep_time or args.keep_band:
        guide["keep"] = longform.keep_mask(1 + content.numel() // HOP, 128, sr, times=args.keep_time,
                                           bands=args.keep_band, feather=args.keep_feather)
        guide["composite"] = args.composite
    if args.keep_component is not None:   # (without the flags: today's call)
        guide.update(keep_component=args.keep_component, hpss_kernel=args.hpss_kernel, hpss_margin=args.hpss_margin,
                     composite=args.composite)
    if args.style_morph:
        guide["style_map"] = longform.morph_map(len(styles), 1 + content.numel() // HOP)
    if args.joint:
        guide["joint"] = True
    if args.vocoder != "griffinlim":      # (without the flag: today's call)
        guide.update(vocoder=args.vocoder, max_gain_db=args.max_gain_db, anchor_db=args.anchor_db,
                     residual=args.residual)
    if args.report is not None:           # (without the flag: today's call)
        guide["report"] = True
    if args.loudness is not None:         # (without the flag: today's call)
        guide.update(loudness=args.loudness, true_peak_db=args.true_peak_db)
    res = transfer_recording(model, content, style, sr=sr, frames=args.frames, overlap=args.overlap,
                             num_timesteps=args.steps, eta=args.eta, batch_size=args.batch, seed=args.seed,
                             solver=args.solver, t_start=args.t_start, style_weights=args.style_weights,
                             style_refs=args.style_refs, **guide)
    ap.save_wav(args.out, res.audio, sr)
    print(f"{args.out}: {res.audio.numel() / sr:.1f} s, {res.N} windows of {args.frames} frames "
          f"({math.ceil(res.N / args.batch)} model calls)")
    if args.loudness is not None:
        info = res.loudness
        print(f"loudness: content {info['content_lufs']:.2f} LUFS, output {info['input_lufs']:.2f} -> "
              f"{info['output_lufs']:.2f} LUFS ({info['gain_db']:+.2f} dB), true peak {info['true_peak_db']:.2f} dB, "
              f"limiter up to {info['max_reduction_db']:.2f} dB")
    if args.report is not None:
        write_report(res.report, args.report)
    return 0


def write_report(report, path):
    """The report as JSON: one line on standard output for "-", else the file `path` (a score without a value is NaN,
    which json.loads reads back)."""
    text = json.dumps(report)
    if path == "-":
        print(text)
    else:
        with open(path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    raise SystemExit(main())
