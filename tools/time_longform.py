"""Times the whole-recording path at a 3-minute recording: T_total = 7752 mel frames, N = 18
windows at the defaults (frames 512, overlap 64, n_mels 128).

  * ldm_amd.longform.mel_windows against unfold + power_to_db + mel_quantize + u8_to_unit, and stitch_windows
    against torch dequantise-style arithmetic + db_to_power, each as a captured graph of INNER back-to-back calls
    replayed between stream events (device time without the host's launch cost), per call;
  * each kernel's time next to its byte floor at 8 TB/s, with the bytes counted;
  * one transfer_recording call split into front end, N windows of diffusion, stitch and vocoder (eager, events).

3 warm-up runs and the median of 15 throughout.  Needs a HIP device.   python tools/time_longform.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]
from ldm_amd import audio, longform, ops  # noqa: E402

N_MELS, FRAMES, OVERLAP, T_TOTAL = 128, 512, 64, 7752
INNER, WARMUP, RUNS = 20, 3, 15
HBM_BYTES_PER_S = 8e12


def median_ms(run):
    """Median over RUNS of run()'s stream time in ms (events), after WARMUP runs."""
    out = []
    for i in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def graphed_ms(fn):
    """Device time per call of fn(): INNER calls captured into one graph, replayed between events."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                     # caches and allocator pools made outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    return median_ms(g.replay) / INNER


def composed_windows(P, N, stride):
    pad = torch.nn.functional.pad(P, (0, (N - 1) * stride + FRAMES - P.shape[1]))
    W = pad.unfold(1, FRAMES, stride).permute(1, 0, 2).contiguous()
    return ops.u8_to_unit(ops.mel_quantize(ops.power_to_db(W, amin=1e-10, top_db=80.0), 80)).unsqueeze(1)


def composed_stitch(y, ref_db, N, stride):
    """The same crossfade from torch elementwise ops on whole windows, then db_to_power."""
    d = y[:, 0].clamp(0, 1) * 80.0 - 80.0 + ref_db[:, None, None]
    w1 = (torch.arange(OVERLAP, device=y.device, dtype=torch.float32) + 1) / (OVERLAP + 1)
    parts = [d[0, :, :stride]]
    for n in range(1, N):
        head = (1 - w1) * d[n - 1, :, stride:] + w1 * d[n, :, :OVERLAP]
        parts += [head, d[n, :, OVERLAP:stride if n < N - 1 else FRAMES]]
    return ops.db_to_power(torch.cat(parts, dim=1)[:, :T_TOTAL].contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    ap.add_argument("--steps", type=int, default=100, help="diffusion steps per window in the split")
    ap.add_argument("--no-split", action="store_true", help="kernels only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_longform: needs a HIP device")
    dev = torch.device("cuda:0")
    N, stride = longform.window_plan(T_TOTAL, FRAMES, OVERLAP)
    g = torch.Generator().manual_seed(1)
    P = (10.0 ** (8.0 * (torch.rand((N_MELS, T_TOTAL), generator=g) - 0.5))).to(dev)
    res = {"T_total": T_TOTAL, "N": N, "frames": FRAMES, "overlap": OVERLAP, "n_mels": N_MELS}

    x, ref_db = longform.mel_windows(P, FRAMES, OVERLAP)
    assert torch.equal(x, composed_windows(P, N, stride))
    y = torch.rand(x.shape, generator=g).to(dev)
    got = longform.stitch_windows(y, ref_db, OVERLAP, T_TOTAL)
    want = composed_stitch(y, ref_db, N, stride)
    assert float(((got - want).abs() / want).max()) < 1e-4

    # bytes the fused kernels must move: the maximum pass reads every window's frames, the elementwise pass reads
    # them again and writes x; the stitch reads every decoded element once and writes the power map
    win_elems, rec_elems = N * N_MELS * FRAMES, N_MELS * T_TOTAL
    bytes_windows = 4 * (2 * win_elems + win_elems)
    bytes_stitch = 4 * (win_elems + rec_elems)
    for name, fused, composed, nbytes in (
            ("mel_windows", lambda: longform.mel_windows(P, FRAMES, OVERLAP), lambda: composed_windows(P, N, stride),
             bytes_windows),
            ("stitch_windows", lambda: longform.stitch_windows(y, ref_db, OVERLAP, T_TOTAL),
             lambda: composed_stitch(y, ref_db, N, stride), bytes_stitch)):
        t_f, t_c = graphed_ms(fused) * 1e3, graphed_ms(composed) * 1e3
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        res[name] = {"fused_us": t_f, "composed_us": t_c, "bytes": nbytes, "floor_us_at_8TBps": floor}
        print(f"{name}: fused {t_f:.1f} us, composition of existing ops {t_c:.1f} us per call; {nbytes} bytes, "
              f"floor at 8 TB/s {floor:.2f} us", flush=True)

    if not args.no_split:
        import models.model as M
        torch.manual_seed(0)
        model = M.LDM(32, pretrained_path="").eval().to(dev)
        Ln = (T_TOTAL - 1) * 512
        t = torch.arange(Ln, device=dev, dtype=torch.float32) / 22050.0
        content = 0.5 * torch.sin(2 * torch.pi * 440.0 * t) + 0.05 * torch.randn(Ln, generator=g).to(dev)
        style = 0.5 * torch.sin(2 * torch.pi * 660.0 * t) + 0.05 * torch.randn(Ln, generator=g).to(dev)
        noise = torch.randn((N, 32, N_MELS // 8, FRAMES // 8), generator=g).to(dev)
        st = {}

        def front():
            st["x"], st["ref"] = longform.mel_windows(audio.melspectrogram(content), FRAMES, OVERLAP)
            st["xs"] = longform.mel_windows(audio.melspectrogram(style), FRAMES, 0)[0][:T_TOTAL // FRAMES]

        def diffusion():
            out = []
            with torch.no_grad():
                for b0 in range(0, N, 8):
                    idx = torch.arange(b0, min(b0 + 8, N), device=dev) % st["xs"].shape[0]
                    out.append(model.content_style_transfer_wrapper(st["x"][b0:b0 + 8], st["xs"][idx],
                                                                    num_timesteps=args.steps, noise=noise[b0:b0 + 8])[0])
            st["y"] = torch.cat(out)

        def stitch():
            st["mel"] = longform.stitch_windows(st["y"], st["ref"], OVERLAP, T_TOTAL)

        def vocoder():
            st["audio"] = audio.mel_to_audio(st["mel"], seed=0, length=Ln)

        split = {}
        for name, fn in (("front_end", front), ("diffusion", diffusion), ("stitch", stitch), ("vocoder", vocoder)):
            split[name + "_ms"] = median_ms(fn)
        res["split"] = dict(split, steps=args.steps, batch_size=8, seconds_of_audio=Ln / 22050.0)
        print("transfer_recording split (ms): " + ", ".join(f"{k[:-3]} {v:.2f}" for k, v in split.items())
              + f"; {Ln / 22050.0:.0f} s of audio, {N} windows x {args.steps} steps", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
