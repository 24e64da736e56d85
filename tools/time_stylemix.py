"""Times what several style references cost the reverse loop: the captured 49-iteration loop
(linspace(99, 0, 50): the flagship's) at B = 8 on the 16 x 64 latent, fp32 and fp16 operands, for R = 1, 2, 4
references.  R = 1 is the plain path (ldm_sample without a mix); R > 1 stacks random style maps with equal weights.

Per configuration: one GraphedDDIM, 3 warm-up replays, then the median and the min..max of 15 replays between stream
events, divided by the iteration count.  The loop's pre-loop work (time MLP, K/V projections, key fold) is inside.

  --once DTYPE R   runs one configuration's eager loop a single time and exits: the target of a kernel trace taken
                   in a run of its own, whose per-kernel statistics separate the two attention launches and the
                   bottleneck from the rest.

Needs a HIP device.   python tools/time_stylemix.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

B, H, W, ITERS = 8, 16, 64, 49
WARMUP, RUNS = 3, 15


def build(dev, dtype, R):
    import models.model as M
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    eng = UNetEngine(ldm.unet, dtype=dtype)
    g = torch.Generator().manual_seed(R)
    z = torch.randn(B, 32, H, W, generator=g).to(dev)
    s5 = torch.rand(B, 256, R * H // 4, W // 4, generator=g).to(dev)
    s6 = torch.rand(B, 512, R * H // 8, W // 8, generator=g).to(dev)
    times = torch.linspace(99, 0, ITERS + 1).long()
    coef = ldm.noise_scheduler.reverse_coefs(times).to(dev)
    t_table = times[:-1].view(ITERS, 1).expand(ITERS, B).contiguous().to(dev)
    return ldm, eng, z, s5, s6, t_table, coef, GraphedDDIM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    ap.add_argument("--once", nargs=2, metavar=("DTYPE", "R"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stylemix: needs a HIP device")
    dev = torch.device("cuda:0")
    if args.once:
        ldm, eng, z, s5, s6, t_table, coef, _ = build(dev, args.once[0], int(args.once[1]))
        with torch.no_grad():
            for _ in range(2):      # the first packs weights and allocates; the trace's per-call statistics take both
                eng.ddim_loop(z.clone(), s5, s6, t_table, coef, 0.0)
        torch.cuda.synchronize()
        return
    res = {"B": B, "H": H, "W": W, "iterations": ITERS, "warmup": WARMUP, "runs": RUNS, "loops": {}}
    for dtype in ("fp32", "fp16"):
        for R in (1, 2, 4):
            ldm, eng, z, s5, s6, t_table, coef, GraphedDDIM = build(dev, dtype, R)
            with torch.no_grad():
                gd = GraphedDDIM(eng, z, s5, s6, t_table, coef, 0.0, logs=False)
            ts = []
            for i in range(WARMUP + RUNS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gd.replay()
                b.record()
                b.synchronize()
                if i >= WARMUP:
                    ts.append(a.elapsed_time(b) * 1e3 / ITERS)
            assert bool(torch.isfinite(gd.x).all())
            r = {"median_us_per_iteration": statistics.median(ts), "min": min(ts), "max": max(ts)}
            res["loops"][f"{dtype}-R{R}"] = r
            print(f"{dtype} R {R}: {r['median_us_per_iteration']:.1f} us per iteration (min {r['min']:.1f}, max "
                  f"{r['max']:.1f}; {RUNS} replays of the {ITERS}-iteration graph)", flush=True)
            del gd
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
