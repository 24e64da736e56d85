"""Times what gradient-norm clipping and the EMA of the weights cost the train step.

Two levels, both on the trainable parameters of LDM(32) (the set config 3 / 4 train):

  optimizer launches alone (random gradients, the capturable Adam under a GradScaler, ITER sequences captured
  into one hipGraph so that no host time is measured; per sequence, median and min..max of RUNS replays):
    base        unscale_check + adam                                   (the step without either option)
    clip_fused  unscale_check_norm + finalize + adam_ext(grad_mul)
    clip_split  unscale_check + clip_grad_norm_ in place (norm pass, finalize, scale pass) + adam
    ema_fused   unscale_check + adam_ext(ema)
    ema_split   unscale_check + adam + ema_update
    both_fused  unscale_check_norm + finalize + adam_ext(grad_mul, ema)

  the whole graphed train step at bench.py's config-3 shape (batch 32, 1x128x512, the default fp16 region),
  options off / clip / EMA / both: ms per step over STEPS replays, RUNS times.

Needs a HIP device.   python tools/time_clip_ema.py [--json out] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

ITER, WARMUP, RUNS, STEPS = 20, 3, 9, 20
MAX_NORM, DECAY = 1.0, 0.999


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def optimizer_level(dev):
    import models.model as M
    from ldm_amd import optim as hoptim
    from ldm_amd.graphs import capture
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").to(dev)
    shapes = [p.shape for p in ldm.parameters() if p.requires_grad]
    del ldm
    out = {"parameters": int(sum(s.numel() for s in shapes)), "tensors": len(shapes), "unit": "us per sequence"}
    for mode in ("base", "clip_fused", "clip_split", "ema_fused", "ema_split", "both_fused"):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 64.0
        opt = hoptim.Adam(ps, lr=1e-4, capturable=True)
        if mode in ("ema_fused", "both_fused"):
            opt.attach_ema(DECAY)
        emas = [p.detach().clone() for p in ps] if mode == "ema_split" else None
        sc = hoptim.GradScaler("cuda", init_scale=1.0)     # scale 1: the gradients stay what they are every replay

        def seq():
            if mode in ("clip_fused", "both_fused"):
                sc.unscale_(opt, max_norm=MAX_NORM)
            else:
                sc.unscale_(opt)
            if mode == "clip_split":
                hoptim.clip_grad_norm_(ps, MAX_NORM)
            sc.step(opt)
            if mode == "ema_split":
                hoptim.ema_update_(emas, [p.detach() for p in ps], DECAY, found_inf=sc._found_inf)
            sc._unscaled.clear()

        seq()                                # eager once: every table and buffer is built outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            for _ in range(ITER):
                seq()
        for _ in range(WARMUP):
            g.replay()
        ts = []
        for _ in range(RUNS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / ITER)
        out[mode] = stats(ts)
        print(mode, out[mode], flush=True)
        del g
    return out


def step_level(dev):
    import time

    import models.model as M
    from models.train import LDMTrainer
    out = {"unit": "ms per step", "batch": 32}
    g = torch.Generator().manual_seed(11)
    content = torch.rand(32, 1, 128, 512, generator=g).to(dev)
    style = torch.rand(32, 1, 128, 512, generator=g).to(dev)
    for mode, kw in (("off", {}), ("clip", dict(max_grad_norm=MAX_NORM)), ("ema", dict(ema_decay=DECAY)),
                     ("both", dict(max_grad_norm=MAX_NORM, ema_decay=DECAY))):
        torch.manual_seed(0)
        ldm = M.LDM(32, pretrained_path="").to(dev).train()
        tr = LDMTrainer(ldm, None, dev, lr=1e-4, **kw)
        tr.graph_step = True
        torch.manual_seed(7)
        for _ in range(4):
            tr.train_step(content, style)
        gin = tr.graph_inputs()
        gin[0].copy_(content)
        gin[1].copy_(style)
        ts = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                tr.train_step(gin[0], gin[1])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / STEPS * 1e3)
        out[mode] = stats(ts)
        if tr.last_grad_norm is not None:
            out[mode]["grad_norm"] = float(tr.last_grad_norm)
        print(mode, out[mode], flush=True)
        del tr, ldm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true", help="the optimizer launches only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "optimizer": optimizer_level(dev)}
    if not args.no_step:
        res["step"] = step_level(dev)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
