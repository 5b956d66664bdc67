"""Config/flag system (the reference hardcodes every constant — SURVEY.md §5.6).

All reference hyperparameters are exposed with their reference defaults;
everything is overridable from YAML or CLI flags.
"""
from __future__ import annotations

import argparse
import dataclasses
import math
from dataclasses import dataclass, field
from typing import Optional

from .ops.shapes import REF_DT, REF_THRESHOLD


LOSS_SCALE_MAX = 16777216.0      # 2^24, the scaler's upper clamp (1 below)


@dataclass
class TrainConfig:
    # model / numerics
    model: str = "lenet5"
    deep_channels: str = "32,64,64"  # DeepCNN stage widths (x16 each)
    act_dtype: str = "bf16"          # activation storage on GPU: bf16 | fp16 | fp32
    pool: str = "trainable"          # trainable (reference) | max
    loss: str = "residual"           # residual (reference) | softmax_ce
    seed: int = 0

    # optimizer (reference semantics: p += dt * grad)
    dt: float = REF_DT
    grad_reduction: str = "mean"     # mean | sum over the global batch
    grad_accum: int = 1              # micro-batches per optimizer step
    threshold: float = REF_THRESHOLD  # early-stop when mean err-norm < this
    # beyond the reference: u = scale*g - weight_decay*p; v = momentum*v + u;
    # p += dt*v (nesterov: p += dt*(u + momentum*v)).  All zero/False keeps
    # the plain update, with no velocity buffer
    momentum: float = 0.0
    weight_decay: float = 0.0
    nesterov: bool = False
    # optimizer: sgd (everything above) | adam.  Adam with decoupled weight
    # decay, for the 1-based update count t: u = scale*g;
    # m = beta1*m + (1-beta1)*u; s = beta2*s + (1-beta2)*u*u;
    # p += dt*(mhat/(sqrt(shat) + adam_eps) - weight_decay*p), mhat and shat
    # bias-corrected by 1/(1-beta^t).  momentum and nesterov must stay off.
    optimizer: str = "sgd"
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8

    # fp16 loss scaling, DeepCNN hip path only: off | dynamic | a fixed
    # power of two in [1, 2^24].  The backward pass starts from scale x the
    # residual, so the gradients stored in activation dtype (fp16's smallest
    # subnormal is 6e-8) stay representable; the update divides by scale
    # again and skips a step whose gradient bucket holds an inf or NaN.
    # dynamic starts at loss_scale_init, halves on a skipped step and
    # doubles after loss_scale_growth_interval applied updates in a row
    # (factors 2 and 0.5, clamp [1, 2^24]).  The scaler lives on the device;
    # the host never reads it during a step.
    loss_scale: str = "off"
    loss_scale_init: float = 65536.0
    loss_scale_growth_interval: int = 2000

    def __post_init__(self):
        # YAML reads `loss_scale: 8192` as a number; the field is a string
        self.loss_scale = str(self.loss_scale)

    def loss_scaling(self):
        """None when loss scaling is off, else (initial scale, dynamic);
        validates the three loss_scale fields (ValueError).  On the cpu and
        torchref backends the key is accepted and has no numeric effect:
        their storage is fp32 and nothing underflows.  LeNet refuses it: its
        in-block step never stores a gradient in activation dtype."""
        def pow2(v, what):
            try:
                f = float(v)
            except (TypeError, ValueError):
                f = 0.0
            m, _ = math.frexp(f)
            if not (1.0 <= f <= LOSS_SCALE_MAX and m == 0.5):
                raise ValueError(
                    f"{what} must be a power of two in [1, 2^24], got {v!r}")
            return f
        if int(self.loss_scale_growth_interval) < 1:
            raise ValueError(
                f"loss_scale_growth_interval must be >= 1, got "
                f"{self.loss_scale_growth_interval}")
        init = pow2(self.loss_scale_init, "loss_scale_init")
        mode = str(self.loss_scale).strip().lower()
        if mode == "off":
            return None
        if self.model == "lenet5":
            raise ValueError(
                "loss_scale is a DeepCNN option; model lenet5 never stores "
                "gradients in activation dtype")
        if mode == "dynamic":
            return init, True
        return pow2(mode, "loss_scale (off, dynamic or a number)"), False

    def uses_adam(self) -> bool:
        """True when the optimizer is Adam (first- and second-moment
        buffers, an update counter); validates the optimizer fields
        (ValueError)."""
        if self.optimizer not in ("sgd", "adam"):
            raise ValueError(
                f"optimizer must be sgd or adam, got {self.optimizer!r}")
        for name in ("beta1", "beta2"):
            if not 0.0 <= getattr(self, name) < 1.0:
                raise ValueError(
                    f"{name} must be in [0, 1), got {getattr(self, name)}")
        if not self.adam_eps > 0.0:
            raise ValueError(f"adam_eps must be > 0, got {self.adam_eps}")
        if self.weight_decay < 0.0:
            raise ValueError(
                f"weight_decay must be >= 0, got {self.weight_decay}")
        if self.optimizer != "adam":
            return False
        if self.momentum != 0.0 or self.nesterov:
            raise ValueError(
                "optimizer adam excludes momentum and nesterov (beta1 is "
                "its momentum)")
        return True

    def uses_momentum(self) -> bool:
        """True when the sgd optimizer needs the velocity buffer; validates
        the optimizer fields (ValueError).  False under adam, whose state
        uses_adam() reports."""
        if self.uses_adam():
            return False
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError(
                f"momentum must be in [0, 1), got {self.momentum}")
        if self.weight_decay < 0.0:
            raise ValueError(
                f"weight_decay must be >= 0, got {self.weight_decay}")
        if self.nesterov and not self.momentum > 0.0:
            raise ValueError("nesterov requires momentum > 0")
        return self.momentum != 0.0 or self.weight_decay != 0.0

    # schedule
    epochs: int = 1                  # reference trains exactly one epoch
    batch_size: int = 64             # per-rank batch

    # data
    data: str = "synthetic"          # synthetic | mnist
    data_dir: str = "data"
    train_count: int = 60000
    test_count: int = 10000

    # execution
    backend: str = "auto"            # auto | hip | cpu | torchref
    device: str = "auto"             # auto | cuda | cpu
    wgrad_chunk: int = 0             # conv1 wgrad slices/channel (0 = auto)
    overlap_comm: bool = False       # two-bucket DP: all-reduce the ready
                                     # bucket while the other wgrad runs
    fuse_wgrad: bool = False         # experimental: conv/pool wgrad inside
                                     # the fwdbwd kernel (measured slower)
    deep_implicit: bool = True       # DeepCNN: implicit-im2col GEMMs (no
                                     # materialized cols for Cin%8==0
                                     # stages, dgrad-as-conv w/ fused
                                     # sigmoid-bwd); False = round-1
                                     # materialized path

    # io / observability
    log_interval: int = 100          # steps between loss readouts
    ckpt_save: Optional[str] = None
    ckpt_load: Optional[str] = None

    def resolved_device(self) -> str:
        if self.device != "auto":
            return self.device
        import torch
        return "cuda" if torch.cuda.is_available() else "cpu"

    def resolved_backend(self) -> str:
        if self.backend != "auto":
            return self.backend
        return "hip" if self.resolved_device() == "cuda" else "cpu"

    @classmethod
    def from_yaml(cls, path: str) -> "TrainConfig":
        import yaml
        with open(path) as f:
            raw = yaml.safe_load(f) or {}
        known = {f.name for f in dataclasses.fields(cls)}
        unknown = set(raw) - known
        if unknown:
            raise ValueError(f"unknown config keys: {sorted(unknown)}")
        return cls(**raw)

    @classmethod
    def add_cli_args(cls, p: argparse.ArgumentParser) -> None:
        p.add_argument("--config", type=str, default=None,
                       help="YAML config file (CLI flags override it)")
        for f in dataclasses.fields(cls):
            name = "--" + f.name.replace("_", "-")
            if f.type == "bool":
                p.add_argument(name, type=lambda s: s.lower() in ("1", "true"),
                               default=None)
            else:
                p.add_argument(name, type=str, default=None)

    @classmethod
    def from_args(cls, args: argparse.Namespace) -> "TrainConfig":
        cfg = cls.from_yaml(args.config) if getattr(args, "config", None) \
            else cls()
        for f in dataclasses.fields(cls):
            v = getattr(args, f.name, None)
            if v is None:
                continue
            if isinstance(v, bool):
                # bool flags are already parsed by the CLI lambda; coercing
                # through str() would turn False into the truthy "False"
                setattr(cfg, f.name, v)
                continue
            typ = {int: int, float: float, str: str}.get(
                type(getattr(cfg, f.name)), str)
            setattr(cfg, f.name, typ(v))
        return cfg


@dataclass
class BenchConfig(TrainConfig):
    steps: int = 200
    warmup: int = 20
    data: str = "synthetic"
    field_note: str = field(default="", repr=False)
