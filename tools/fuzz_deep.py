"""Randomized cross-validation of the DeepCNN hip path against the fp32
oracle: random channel sets (2-4 stages, multiples of 16), batch sizes,
activation dtypes, and engine modes (implicit / materialized), one full
training step each, the parameter move compared block by block with the
float64 chain-rule oracle (tools/deep_emul.py).

Run on a GPU box:  python tools/fuzz_deep.py [--n 12] [--seed 0]
Exit code != 0 on the first mismatch (prints the failing config).
"""
from __future__ import annotations

import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))   # deep_emul: the float64
                                                  # oracle with rounding hooks

import torch


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=12)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert torch.cuda.is_available(), "fuzz needs a GPU"
    from parallel_cnn_amd.config import TrainConfig
    from parallel_cnn_amd.engine.deep import DeepTrainer
    from parallel_cnn_amd.models.deepcnn import DeepCNN, DeepCNNSpec
    from parallel_cnn_amd.data.mnist import synthetic_images
    import deep_emul

    rng = random.Random(args.seed)
    fails = 0
    for trial in range(args.n):
        nstages = rng.choice([2, 3, 4])
        channels = tuple(16 * rng.randint(1, 4) for _ in range(nstages))
        B = rng.choice([2, 3, 8, 16, 32])
        dtype = rng.choice(["fp32", "fp32", "bf16"])
        implicit = rng.choice([True, False])
        desc = (f"trial {trial}: channels={channels} B={B} "
                f"dtype={dtype} implicit={implicit}")
        cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                          act_dtype=dtype, log_interval=0,
                          deep_channels=",".join(map(str, channels)),
                          deep_implicit=implicit, seed=trial)
        try:
            t = DeepTrainer(cfg)
            x, labels = synthetic_images(B, 32, 32, 3, seed=100 + trial,
                                         structured=False)
            t.step(*t.stage_batch(x, labels))
            torch.cuda.synchronize()
            spec = DeepCNNSpec(channels=channels)
            p0 = DeepCNN(seed=cfg.seed, spec=spec).params
            got = t.model.params.cpu()
            assert torch.isfinite(got).all(), "non-finite params"
            # per-block rule of the suite: relative L2 of the parameter move
            # against the float64 oracle, tolerance 4 x the
            # rounding-emulating oracle's own ratio (an uninformative block
            # raises, it never passes silently)
            g, _, emul = deep_emul.oracle_pair(x.view(B, 32, 32, 3), labels,
                                               p0, spec, dtype)
            dp_ref = cfg.dt * (1.0 / B) * g
            lines = []
            bad, _ = deep_emul.compare_blocks(
                f"trial{trial}", got.double() - p0.double(), dp_ref, emul,
                dtype, spec,
                floor=deep_emul.step_delta_floor(got, dp_ref, spec),
                log=lines.append)
            status = "OK " if not bad else "FAIL"
            print(f"{status} {desc}: worst emulated "
                  f"{max(emul.values()):.2e}" +
                  (f" failing {bad}" if bad else ""), flush=True)
            if bad:
                print("\n".join(lines), flush=True)
                fails += 1
        except Exception as e:
            print(f"FAIL {desc}: {type(e).__name__}: {e}", flush=True)
            fails += 1
    print(f"{args.n - fails}/{args.n} configs passed")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
