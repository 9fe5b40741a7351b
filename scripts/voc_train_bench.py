#!/usr/bin/env python3
"""Times the vocabulary training (flvis_hip_voc_train) on synthetic descriptors generated on the device: clusters of 256-bit
prototypes with a few flipped bits, ~1000 per image.

  voc_train_bench.py [--images 64] [--k 10] [--L 3] [--repeat 3] [--small-node-max 0] [--restatement]

Prints one JSON line: wall time of a training (best of --repeat, after one warm-up), the time per level -- trainings of depth 1 .. L
differ only in the levels they run, so level l costs t(L = l) - t(L = l - 1) (the weights' descent rides along) --, launches and
association passes.  --restatement also times tests/_voc_train.py on the same descriptors, for scale only, and compares the trees."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def make(n_img, cap=1024, n_proto=4000, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    protos = torch.randint(0, 256, (n_proto, 32), dtype=torch.uint8, device="cuda", generator=g)
    cnt = torch.randint(900, cap + 1, (n_img,), dtype=torch.int32, device="cuda", generator=g)
    which = torch.randint(0, n_proto, (n_img, cap), device="cuda", generator=g)
    d = protos[which]
    flip = torch.zeros_like(d)
    for b in range(8):                                                   # each bit flips with probability 1/40
        flip |= (torch.rand(d.shape, device="cuda", generator=g) < 0.025).to(torch.uint8) << b
    return (d ^ flip).contiguous(), cnt


def timed(ctx, desc, cnt, repeat, **kw):
    import torch
    best, voc = None, None
    for i in range(repeat + 1):
        if voc is not None:
            voc.close()
        torch.cuda.synchronize()
        t = time.perf_counter()
        voc = ctx.voc_train(desc, cnt, **kw)
        dt = time.perf_counter() - t
        if i > 0:
            best = dt if best is None else min(best, dt)
    return best, voc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--small-node-max", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    import flvis_amd
    ctx = flvis_amd.Context(0)
    desc, cnt = make(args.images)
    levels, prev, voc = [], 0.0, None
    for L in range(1, args.L + 1):
        if voc is not None:
            voc.close()
        t, voc = timed(ctx, desc, cnt, args.repeat, k=args.k, L=L, seed=1, small_node_max=args.small_node_max)
        levels.append(round((t - prev) * 1e3, 3))
        prev = t
    out = dict(voc.stats, images=args.images, k=args.k, L=args.L, small_node_max=args.small_node_max or 2048,
               wall_ms=round(prev * 1e3, 3), level_ms=levels)
    if args.restatement:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import numpy as np
        import _voc_train as T
        hd, hc = desc.cpu().numpy(), cnt.cpu().numpy()
        t = time.perf_counter()
        want = T.train([hd[i, :hc[i]] for i in range(args.images)], args.k, args.L, seed=1)
        out["restatement_s"] = round(time.perf_counter() - t, 2)
        out["same_tree"] = bool(np.array_equal(want["arrays"][2], voc.info["desc"]) and np.array_equal(want["arrays"][0], voc.info["child_ptr"]))
    voc.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
