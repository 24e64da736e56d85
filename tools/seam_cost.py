"""Times what joint sampling costs the reverse loop: GraphedDDIM.replay of the captured 49-iteration
loop (linspace(99, 0, 50): the flagship's) at the config-2 shape, B = 8 on the 16 x 64 latent, fp32, DDIM update, with
seam_cols = 0 and seam_cols = 8 (50 extra launches of the seam-fuse kernel: one before step 0, one after every step).

Both graphs are built first and replayed alternately (plain, joint, plain, joint, ...), so that clock and thermal
drift fall on both alike: 5 warm-up rounds, then the median and the min..max of 30 rounds between stream events,
divided by the iteration count.  The loop's pre-loop work (time MLP, K/V projections, key fold, layout conversion) is
inside both.

Needs a HIP device.   python tools/seam_cost.py [--seam 8] [--batch 8] [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

H, W, ITERS = 16, 64, 49
WARMUP, RUNS = 5, 30


def build(dev, B, seam_cols):
    """A captured fp32 DDIM loop on q_sample(z0, 99, n0) with the given seam width."""
    import models.model as M
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    eng = UNetEngine(ldm.unet, dtype="fp32")
    g = torch.Generator().manual_seed(B)
    z0, n0 = torch.randn(B, 32, H, W, generator=g).to(dev), torch.randn(B, 32, H, W, generator=g).to(dev)
    s5, s6 = torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev), torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev)
    times = torch.linspace(99, 0, ITERS + 1).long()
    fd = ldm.noise_scheduler
    z, _ = fd(z0, torch.full((B,), 99, dtype=torch.long, device=dev), noise=n0)
    coef = fd.reverse_coefs(times).to(dev)
    t_table = times[:-1].view(ITERS, 1).expand(ITERS, B).contiguous().to(dev)
    with torch.no_grad():
        return GraphedDDIM(eng, z, s5, s6, t_table, coef, 0.0, logs=False, seam_cols=seam_cols)


def timed(gd):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    gd.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS


def stats(ts):
    return {"median_us_per_iteration": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seam", type=int, default=8, help="seam width in latent columns (1 .. 32)")
    ap.add_argument("--batch", type=int, default=8, help="windows per loop")
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_cost: needs a HIP device")
    dev = torch.device("cuda:0")
    plain, joint = build(dev, args.batch, 0), build(dev, args.batch, args.seam)
    tp, tj = [], []
    for i in range(WARMUP + RUNS):
        p, j = timed(plain), timed(joint)
        if i >= WARMUP:
            tp.append(p)
            tj.append(j)
    W_ = plain.x.shape[3]
    assert bool(torch.isfinite(plain.x).all()) and bool(torch.isfinite(joint.x).all())
    assert torch.equal(joint.x[0, :, :, W_ - args.seam:], joint.x[1, :, :, :args.seam])
    res = {"B": args.batch, "H": H, "W": W, "seam_cols": args.seam, "iterations": ITERS, "warmup": WARMUP, "runs": RUNS,
           "plain": stats(tp), "joint": stats(tj),
           "difference_us_per_iteration": statistics.median(tj) - statistics.median(tp),
           "paired_difference_median": statistics.median([j - p for p, j in zip(tp, tj)])}
    for key in ("plain", "joint"):
        r = res[key]
        print(f"{key}: {r['median_us_per_iteration']:.2f} us per iteration (min {r['min']:.2f}, max {r['max']:.2f}; {RUNS} "
              f"interleaved replays of the {ITERS}-iteration graph)")
    print(f"difference of the medians: {res['difference_us_per_iteration']:.2f} us per iteration "
          f"({100 * res['difference_us_per_iteration'] / res['plain']['median_us_per_iteration']:.1f} %); median of the "
          f"paired differences: {res['paired_difference_median']:.2f}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
