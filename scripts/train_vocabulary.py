#!/usr/bin/env python3
"""Trains a DBoW3 vocabulary on the descriptors THIS library's ORB extractor produces, and saves it as a binary .dbow3 file that
`run_sequence.py --loop-closing --voc` (flvis_hip_bow_load_vocabulary) reads.

  train_vocabulary.py (--euroc DIR | --kitti DIR | --synth N) [--every E] [--k 10] [--L 5] [--seed 1] --out voc.dbow3

The extractor's default sampling pattern is OpenCV's makeRandomPattern, not cv::ORB's learned one, so a public ORB vocabulary does
not fit its descriptors; this tool is how a vocabulary for it is made.  ORB runs with the loop closer's parameters (1000 features,
1.2, 8 levels, FAST 20, capacity 1024) on every E-th left image; the training is flvis_hip_voc_train (DBoW3's Vocabulary::create on
the device).  Prints one JSON line with the statistics."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

CAP = 1024
BATCH = 16


def images(args):
    """yields uint8 [b,h,w] cuda tensors"""
    import torch
    from flvis_amd import synth, traj_io
    if args.synth:
        tr = [synth.Trajectory(s) for s in range(args.synth)]
        i0, _ = synth.Renderer("cuda").stereo_frame(tr, 0.5, 10)
        yield i0.contiguous()
        return
    seq = traj_io.KittiSequence(args.kitti) if args.kitti else traj_io.EurocSequence(args.euroc)
    batch = []
    for k in range(0, len(seq), max(1, args.every)):
        batch.append(traj_io.load_gray(seq.files[k][0]))
        if len(batch) == BATCH:
            yield torch.from_numpy(np.stack(batch)).cuda()
            batch = []
    if batch:
        yield torch.from_numpy(np.stack(batch)).cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--euroc", help="EuRoC ASL sequence folder (cam0 is used)")
    src.add_argument("--kitti", help="KITTI odometry sequence folder (image_0 is used)")
    src.add_argument("--synth", type=int, help="N rendered frames of the synthetic scene")
    ap.add_argument("--every", type=int, default=5, help="use every E-th frame of a sequence")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--weighting", type=int, default=0, choices=[0, 1], help="0 TF_IDF, 1 TF")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch
    import flvis_amd
    ctx = flvis_amd.Context(0)
    descs, counts = [], []
    t0 = time.time()
    for img in images(args):
        _, desc, cnt, _ = ctx.orb_detect_and_compute(img, cap=CAP)
        descs.append(desc)
        counts.append(cnt)
    if not descs:
        sys.exit("no image found")
    desc, cnt = torch.cat(descs), torch.cat(counts)
    torch.cuda.synchronize()
    t1 = time.time()
    voc = ctx.voc_train(desc, cnt, k=args.k, L=args.L, seed=args.seed, weighting=args.weighting)
    t2 = time.time()
    voc.save(args.out)
    # a word every training image holds has Ni = NDocs and the TF-IDF weight log(1) = 0: it scores nothing
    unweighted = int(np.sum(voc.info["weight"][voc.info["word_id"] >= 0] == 0))
    if unweighted == voc.stats["words"]:
        print("warning: every word occurs in every training image, so all weights are 0 and every score will be 0; "
              "use more images, a larger k or L, or --weighting 1", file=sys.stderr)
    out = dict(voc.stats, words_without_weight=unweighted, images=int(desc.shape[0]), k=args.k, L=args.L, seed=args.seed,
               weighting=args.weighting, out=args.out, bytes=os.path.getsize(args.out), orb_s=round(t1 - t0, 3),
               train_s=round(t2 - t1, 3))
    voc.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
