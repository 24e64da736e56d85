"""Times what the regional keep costs the reverse loop: the captured 49-iteration loop (linspace(99, 0,
50): the flagship's) on the 16 x 64 latent, fp32 and fp16 operands, DDIM and 2M update, for
  * the plain loop at B = 8,
  * the keep loop at B = 8 (keep_blend fused into dec1's epilogue),
  * the unfused alternative, built here only: the plain loop plus one stand-alone ldm_keep_blend launch per iteration.
    The 49 blend launches are captured and timed as a graph of their own, back to back on the NCHW state, and their
    time per iteration is added to the plain loop's.  That is a lower bound of an in-loop launch: inside the
    step-kernel loop the state is NHWC between steps, and a launch between dec1 and the next enc1 waits for the one
    and holds up the other;
  * the guided loop at B = 4 (scale 2.5) with and without the keep.

Per configuration: one captured graph, 3 warm-up replays, then the median and the min..max of 15 replays between stream
events, divided by the iteration count.  The loop's pre-loop work (time MLP, K/V projections, key fold, and with the
keep the layout conversion of z0 / n0) is inside.

Needs a HIP device.   python tools/time_regional.py [--json out]
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
WARMUP, RUNS = 3, 15


def operands(dev, B):
    g = torch.Generator().manual_seed(B)
    z0, n0 = torch.randn(B, 32, H, W, generator=g).to(dev), torch.randn(B, 32, H, W, generator=g).to(dev)
    w = torch.zeros(B, H, W)
    w[:, :, 5:23] = 1.0          # a column band that is not aligned to a wave's 16 columns
    w[:, 3:6] = 0.25
    maps = [torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev), torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev),
            torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev), torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev)]
    return z0, n0, w.to(dev), maps


def build(dev, dtype, B, solver, guided, keep):
    """A captured loop: GraphedDDIM on q_sample(z0, 99, n0)."""
    import models.model as M
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    eng = UNetEngine(ldm.unet, dtype=dtype)
    z0, n0, w, maps = operands(dev, B)
    times = torch.linspace(99, 0, ITERS + 1).long()
    fd = ldm.noise_scheduler
    z, _ = fd(z0, torch.full((B,), 99, dtype=torch.long, device=dev), noise=n0)
    coef = (fd.multistep_coefs(times) if solver == "msolver" else fd.reverse_coefs(times)).to(dev)
    t_table = times[:-1].view(ITERS, 1).expand(ITERS, B).contiguous().to(dev)
    kw = dict(base=(maps[2], maps[3], None, None), guidance_scale=2.5) if guided else {}
    if keep:
        kw["keep"] = (z0, n0, w, fd.keep_coefs(times))
    with torch.no_grad():
        return GraphedDDIM(eng, z, maps[0], maps[1], t_table, coef, 0.0, logs=solver == "msolver", solver=solver, **kw)


class BlendChain:
    """ITERS stand-alone ldm_keep_blend launches on one state, captured as a graph."""

    def __init__(self, dev, B):
        import models.model as M
        from ldm_amd import ops
        from ldm_amd.graphs import capture
        z0, n0, w, _ = operands(dev, B)
        coefs = M.ForwardDiffusion().keep_coefs(torch.linspace(99, 0, ITERS + 1).long()).to(dev)
        rows = [coefs[i].contiguous() for i in range(ITERS)]
        self.x = z0.clone()
        ops.keep_blend_(self.x, z0, n0, w, rows[0])      # (loads the library outside the capture)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with capture(self.graph):
            for i in range(ITERS):
                ops.keep_blend_(self.x, z0, n0, w, rows[i])
        self._keep = (z0, n0, w, rows)

    def replay(self):
        self.graph.replay()
        return self.x


def measure(gd):
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
    return {"median_us_per_iteration": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_regional: needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"H": H, "W": W, "iterations": ITERS, "warmup": WARMUP, "runs": RUNS, "loops": {}}

    def report(key, r):
        res["loops"][key] = r
        print(f"{key}: {r['median_us_per_iteration']:.2f} us per iteration (min {r['min']:.2f}, max {r['max']:.2f}; {RUNS} "
              f"replays of the {ITERS}-iteration graph)", flush=True)

    chain = BlendChain(dev, 8)
    blend = measure(chain)
    report("blend-chain-B8 (stand-alone ldm_keep_blend, per launch)", blend)
    del chain
    for dtype in ("fp32", "fp16"):
        for solver in ("ddim", "msolver"):
            for name, B, guided, keep in (("plain-B8", 8, False, False), ("keep-B8", 8, False, True),
                                          ("guided-B4", 4, True, False), ("guided-keep-B4", 4, True, True)):
                gd = build(dev, dtype, B, solver, guided, keep)
                r = measure(gd)
                report(f"{dtype}-{solver}-{name}", r)
                if name == "plain-B8":      # the unfused alternative: its iteration plus one blend launch
                    report(f"{dtype}-{solver}-unfused-B8 (plain + blend chain)",
                           {k: r[k] + blend[k] for k in ("median_us_per_iteration", "min", "max")})
                del gd
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
