"""Checkpoint/resume: flat LE fp32 weights (the parity format)
plus a JSON sidecar with training state for EXACT resume (global step,
epoch cursor, host/device RNG states — so train(2N epochs) ==
train(N) -> save -> load -> train(N)).  A non-default optimizer (momentum
or weight decay) adds its velocity as flat LE fp32 at `path + '.vel'`; Adam
puts its first moment there, its second moment at `path + '.sq'` and its
update count in the sidecar.  A DeepCNN loss scaler adds its device state
(`loss_scale`: scale, good_steps, skipped, t) to the sidecar; a sidecar
without it resumes from the configured initial scale."""
from __future__ import annotations

import base64
import json
import os
from typing import Optional

import torch


def _rng_capture() -> dict:
    state = {"torch_cpu": base64.b64encode(
        torch.get_rng_state().numpy().tobytes()).decode()}
    if torch.cuda.is_available():
        state["torch_cuda"] = base64.b64encode(
            torch.cuda.get_rng_state().numpy().tobytes()).decode()
    return state


def _rng_restore(state: dict) -> None:
    import numpy as np
    cpu = state.get("torch_cpu")
    if cpu:
        torch.set_rng_state(torch.from_numpy(np.frombuffer(
            base64.b64decode(cpu), dtype=np.uint8).copy()))
    cuda = state.get("torch_cuda")
    if cuda and torch.cuda.is_available():
        torch.cuda.set_rng_state(torch.from_numpy(np.frombuffer(
            base64.b64decode(cuda), dtype=np.uint8).copy()))


def save_checkpoint(trainer, path: str) -> None:
    """Weights to `path`, training state to `path + '.meta.json'`."""
    trainer.model.save(path)
    meta = {
        "global_step": trainer.global_step,
        "epoch": getattr(trainer, "epoch", 0),
        "model": trainer.cfg.model,
        "dt": trainer.cfg.dt,
        "grad_reduction": trainer.cfg.grad_reduction,
        "pool": getattr(trainer.cfg, "pool", "trainable"),
        "loss": getattr(trainer.cfg, "loss", "residual"),
        "n_params": int(trainer.model.params.numel()),
        "rng": _rng_capture(),
    }
    vel = getattr(trainer, "vel", None)
    sq = getattr(trainer, "sq", None)
    if sq is not None:
        vel.detach().cpu().numpy().astype("<f4").tofile(path + ".vel")
        sq.detach().cpu().numpy().astype("<f4").tofile(path + ".sq")
        for key in ("optimizer", "beta1", "beta2", "adam_eps",
                    "weight_decay"):
            meta[key] = getattr(trainer.cfg, key)
        meta["opt_step"] = trainer.opt_step
    elif vel is not None:
        # non-default optimizer only: the default writes exactly the files
        # and keys it always wrote
        vel.detach().cpu().numpy().astype("<f4").tofile(path + ".vel")
        meta["momentum"] = trainer.cfg.momentum
        meta["weight_decay"] = trainer.cfg.weight_decay
        meta["nesterov"] = trainer.cfg.nesterov
    ls = getattr(trainer, "loss_scale_state", lambda: None)()
    if ls is not None:
        meta["loss_scale"] = ls
    with open(path + ".meta.json", "w") as f:
        json.dump(meta, f, indent=1)


def _load_bucket(buf: torch.Tensor, file_path: str, what: str) -> None:
    import numpy as np
    arr = np.fromfile(file_path, dtype="<f4")
    if arr.size != buf.numel():
        raise ValueError(
            f"{what} file {file_path!r} has {arr.size} floats, "
            f"expected {buf.numel()}")
    with torch.no_grad():
        buf.copy_(torch.from_numpy(arr.copy()).to(buf.device))


def _load_velocity(trainer, path: str) -> None:
    """Restore trainer.vel from `path + '.vel'`: a size mismatch raises; a
    missing file under momentum > 0 starts from zero with a warning."""
    vel = getattr(trainer, "vel", None)
    if vel is None:
        return
    vel_path = path + ".vel"
    if not os.path.exists(vel_path):
        if trainer.cfg.momentum > 0:
            print(f"warning: checkpoint {path!r} has no velocity file; "
                  f"momentum restarts from zero velocity")
        with torch.no_grad():
            vel.zero_()
        return
    _load_bucket(vel, vel_path, "velocity")


def _load_adam_state(trainer, path: str, meta: Optional[dict]) -> None:
    """Restore Adam's m (`.vel`), s (`.sq`) and update count (sidecar
    `opt_step`).  A size mismatch raises.  The three only mean something
    together: if any is missing, Adam restarts from zero moments and update
    0, with a warning."""
    missing = [ext for ext in (".vel", ".sq")
               if not os.path.exists(path + ext)]
    if meta is None or "opt_step" not in meta:
        missing.append("opt_step")
    if missing:
        print(f"warning: checkpoint {path!r} lacks adam state "
              f"({', '.join(missing)}); adam restarts from zero moments")
        with torch.no_grad():
            trainer.vel.zero_()
            trainer.sq.zero_()
        trainer.opt_step = 0
        return
    _load_bucket(trainer.vel, path + ".vel", "first-moment")
    _load_bucket(trainer.sq, path + ".sq", "second-moment")
    trainer.opt_step = int(meta["opt_step"])


def _load_loss_scaler(trainer, meta: Optional[dict]) -> None:
    """Restore the device loss scaler from the sidecar's `loss_scale`.  A
    sidecar without it (or none) leaves the scaler at the configured initial
    scale, with the update count the optimizer state above gave it."""
    if getattr(trainer, "ls_state", None) is None:
        return
    ls = (meta or {}).get("loss_scale")
    if ls is None:
        return
    trainer.set_loss_scale_state(float(ls["scale"]), int(ls["good_steps"]),
                                 int(ls["skipped"]), int(ls["t"]))


def load_checkpoint(trainer, path: str) -> Optional[dict]:
    """Loads weights; restores global_step/epoch/RNG from the sidecar if
    present.  Returns the metadata dict (or None)."""
    trainer.model.load(path)
    if hasattr(trainer, "invalidate_weight_cache"):
        trainer.invalidate_weight_cache()
    meta_path = path + ".meta.json"
    meta = None
    if os.path.exists(meta_path):
        with open(meta_path) as f:
            meta = json.load(f)
    if getattr(trainer, "sq", None) is not None:
        _load_adam_state(trainer, path, meta)
    else:
        _load_velocity(trainer, path)
    _load_loss_scaler(trainer, meta)
    if meta is None:
        return None
    if meta.get("n_params") not in (None, int(trainer.model.params.numel())):
        raise ValueError(
            f"checkpoint {path!r} is for a model with {meta['n_params']} "
            f"params, this model has {trainer.model.params.numel()}")
    # a matching parameter COUNT does not make a matching model: a
    # pool=max or loss=softmax_ce checkpoint would load silently into a
    # trainable/residual config and predict garbage
    for key, cur in (("model", trainer.cfg.model),
                     ("pool", getattr(trainer.cfg, "pool", "trainable")),
                     ("loss", getattr(trainer.cfg, "loss", "residual"))):
        want = meta.get(key)
        if want is not None and want != cur:
            raise ValueError(
                f"checkpoint {path!r} was trained with {key}={want!r}, "
                f"but the running config has {key}={cur!r}")
    trainer.global_step = int(meta.get("global_step", 0))
    if hasattr(trainer, "epoch"):
        trainer.epoch = int(meta.get("epoch", 0))
    if meta.get("rng"):
        _rng_restore(meta["rng"])
    return meta
