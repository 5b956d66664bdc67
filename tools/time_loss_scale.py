"""Cost of DeepCNN loss scaling: us/step of the fp16 training step with
loss_scale off and with the given loss_scale, in one process, the two
trainers alternating block by block (bench.py has no loss-scale flag).

    python tools/time_loss_scale.py --batch-size 256 --loss-scale dynamic

Prints one JSON line: per variant the median, min and max block in us/step,
and the scaler state at the end (no step may have been skipped, or the two
variants did different work).  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir))
from parallel_cnn_amd.config import TrainConfig  # noqa: E402
from parallel_cnn_amd.data.mnist import synthetic_images  # noqa: E402
from parallel_cnn_amd.engine.deep import DeepTrainer  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--loss-scale", default="dynamic")
    ap.add_argument("--optimizer", default="sgd")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_loss_scale.py needs a GPU")
    B = args.batch_size
    nb = 8
    x, y = synthetic_images(nb * B, 32, 32, 3, seed=1234, structured=False)
    variants = {}
    for name, ls in (("off", "off"), ("on", args.loss_scale)):
        t = DeepTrainer(TrainConfig(
            model="deepcnn", batch_size=B, act_dtype="fp16", device="cuda",
            backend="hip", log_interval=0, optimizer=args.optimizer,
            loss_scale=ls))
        xp, yp = t.stage_batch(x, y)
        variants[name] = (t, xp.contiguous(), yp.contiguous(), [])

    def block(t, xp, yp, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(n):
            i = (s % nb) * B
            t.step(xp[i:i + B], yp[i:i + B])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    for t, xp, yp, _ in variants.values():
        block(t, xp, yp, args.warmup)
    for _ in range(args.blocks):
        for t, xp, yp, out in variants.values():
            out.append(block(t, xp, yp, args.steps))
    res = {"batch_size": B, "steps_per_block": args.steps,
           "loss_scale": args.loss_scale, "optimizer": args.optimizer}
    for name, (t, _, _, out) in variants.items():
        out.sort()
        res[name] = {"median_us": out[len(out) // 2], "min_us": out[0],
                     "max_us": out[-1]}
    res["scaler"] = variants["on"][0].loss_scale_state()
    res["delta_us"] = res["on"]["median_us"] - res["off"]["median_us"]
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
