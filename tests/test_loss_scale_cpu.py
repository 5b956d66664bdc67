"""Loss scaling without a GPU: config validation, the emulator facts the GPU
tests rely on, the advance-rule reference and the checkpoint sidecar."""
import argparse
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import deep_emul  # noqa: E402
from parallel_cnn_amd.config import TrainConfig  # noqa: E402
from parallel_cnn_amd.data.mnist import synthetic_images  # noqa: E402
from parallel_cnn_amd.engine.deep import DeepTrainer  # noqa: E402
from parallel_cnn_amd.engine.trainer import Trainer  # noqa: E402
from parallel_cnn_amd.models.deepcnn import DeepCNN, DeepCNNSpec  # noqa: E402
from parallel_cnn_amd.ops import loss_scale_ref as ref  # noqa: E402
from parallel_cnn_amd.utils.checkpoint import (load_checkpoint,  # noqa: E402
                                               save_checkpoint)

EXAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        os.pardir, "examples")


# ------------------------------------------------------------------- config
def deep_cfg(**kw):
    return TrainConfig(model="deepcnn", **kw)


def test_loss_scale_values():
    assert TrainConfig().loss_scale == "off"
    assert TrainConfig().loss_scaling() is None
    assert deep_cfg(loss_scale="off").loss_scaling() is None
    assert deep_cfg(loss_scale="dynamic").loss_scaling() == (65536.0, True)
    assert deep_cfg(loss_scale="dynamic",
                    loss_scale_init=1024.0).loss_scaling() == (1024.0, True)
    assert deep_cfg(loss_scale="8192").loss_scaling() == (8192.0, False)
    assert deep_cfg(loss_scale=8192).loss_scaling() == (8192.0, False)
    assert deep_cfg(loss_scale="1").loss_scaling() == (1.0, False)
    assert deep_cfg(loss_scale=str(2 ** 24)).loss_scaling() == \
        (2.0 ** 24, False)


@pytest.mark.parametrize("kw", [
    dict(loss_scale="3000"), dict(loss_scale="0.5"), dict(loss_scale="0"),
    dict(loss_scale="-8"), dict(loss_scale=str(2 ** 25)),
    dict(loss_scale="on"), dict(loss_scale="nan"), dict(loss_scale="inf"),
    dict(loss_scale="dynamic", loss_scale_init=3000.0),
    dict(loss_scale="dynamic", loss_scale_growth_interval=0),
])
def test_loss_scale_rejected(kw):
    with pytest.raises(ValueError):
        deep_cfg(**kw).loss_scaling()


def test_loss_scale_refused_for_lenet():
    for v in ("dynamic", "8192"):
        with pytest.raises(ValueError, match="lenet5"):
            TrainConfig(model="lenet5", loss_scale=v).loss_scaling()
        with pytest.raises(ValueError, match="lenet5"):
            Trainer(TrainConfig(model="lenet5", loss_scale=v, device="cpu",
                                backend="torchref"))


def test_loss_scale_yaml_and_cli(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text("model: deepcnn\nact_dtype: fp16\nloss_scale: 8192\n"
                 "loss_scale_growth_interval: 7\n")
    cfg = TrainConfig.from_yaml(str(p))
    assert cfg.loss_scaling() == (8192.0, False)
    assert cfg.loss_scale_growth_interval == 7
    ap = argparse.ArgumentParser()
    TrainConfig.add_cli_args(ap)
    args = ap.parse_args(["--config", str(p), "--loss-scale", "dynamic",
                          "--loss-scale-init", "4096",
                          "--loss-scale-growth-interval", "11"])
    cfg = TrainConfig.from_args(args)
    assert cfg.loss_scaling() == (4096.0, True)
    assert cfg.loss_scale_growth_interval == 11
    args = ap.parse_args(["--model", "deepcnn", "--loss-scale", "3000"])
    with pytest.raises(ValueError):
        TrainConfig.from_args(args).loss_scaling()
    ex = TrainConfig.from_yaml(os.path.join(EXAMPLES, "deepcnn_fp16.yaml"))
    assert ex.act_dtype == "fp16" and ex.model == "deepcnn"
    assert ex.loss_scaling() == (65536.0, True)


def test_torchref_accepts_the_key_without_effect():
    """Storage is fp32 there: same step, no scaler state."""
    B = 2
    x, labels = synthetic_images(B, 32, 32, 3, seed=3, structured=False)
    out = []
    for ls in ("off", "8192"):
        t = DeepTrainer(TrainConfig(
            model="deepcnn", deep_channels="16,16", batch_size=B,
            device="cpu", backend="torchref", log_interval=0, loss_scale=ls))
        assert t.ls_state is None and t.loss_scale_state() is None
        t.step(*t.stage_batch(x, labels))
        assert t.opt_step == 1
        out.append(t.model.params.clone())
    assert torch.equal(out[0], out[1])


# ----------------------------------------------------------- emulator facts
def emul_ratios(channels, seed, scale):
    B = 8
    spec = DeepCNNSpec(channels=tuple(int(c) for c in channels.split(",")))
    p = DeepCNN(seed=0, spec=spec).params
    x, labels = synthetic_images(B, 32, 32, 3, seed=seed, structured=False)
    _, _, emul = deep_emul.oracle_pair(x.view(B, 32, 32, 3), labels, p, spec,
                                       "fp16", loss_scale=scale)
    return emul


def test_emulated_fp16_unscaled_loses_conv0():
    emul = emul_ratios("32,64,64", 7, 1.0)
    print({k: f"{v:.3g}" for k, v in emul.items()})
    assert emul["conv0_w"] >= deep_emul.FP16_BLOCK_LIMIT
    _, excluded = deep_emul.block_tolerances(emul, "fp16")
    assert "conv0_w" in excluded


@pytest.mark.parametrize("channels,seed", [("32,64,64", 7),
                                           ("16,32,32,64", 29)])
def test_emulated_fp16_scaled_keeps_every_block(channels, seed):
    emul = emul_ratios(channels, seed, 8192.0)
    print({k: f"{v:.3g}" for k, v in emul.items()})
    _, excluded = deep_emul.block_tolerances(emul, "fp16")   # raises nothing
    assert excluded == set()
    assert max(emul.values()) < deep_emul.FP16_BLOCK_LIMIT


def test_grads64_scale_is_exact_without_rounding():
    """Scaling by a power of two and back is the identity in float64: the
    default argument leaves every current caller where it was."""
    B = 2
    spec = DeepCNNSpec(channels=(16, 16))
    p = DeepCNN(seed=0, spec=spec).params
    x, labels = synthetic_images(B, 32, 32, 3, seed=5, structured=False)
    xh = x.view(B, 32, 32, 3)
    g1, l1 = deep_emul.grads64(xh, labels, p, spec)
    g2, l2 = deep_emul.grads64(xh, labels, p, spec, loss_scale=8192.0)
    assert torch.equal(g1, g2) and l1 == l2


# ------------------------------------------------------------- advance rule
# (found_inf per step, growth_interval = 3) -- shared with the GPU test
SCRIPT = [0, 0, 0,          # growth at the interval, counter reset
          0, 1,             # backoff, counter reset mid-run
          0, 0, 1, 1,       # two skips in a row
          0, 0, 0, 0]       # growth again, then one more


def run_script(state, script, interval, dynamic=True, b1=0.9, b2=0.999):
    out = [state]
    for f in script:
        out.append(ref.advance_reference(out[-1], bool(f), interval, dynamic,
                                         b1, b2))
    return out


def test_advance_reference_script():
    tr = run_script(ref.scaler_state(1024.0, 0.9, 0.999), SCRIPT, 3)
    assert [s["scale"] for s in tr] == [
        1024, 1024, 1024, 2048, 2048, 1024, 1024, 1024, 512, 256, 256, 256,
        512, 512]
    assert [s["good_steps"] for s in tr] == [
        0, 1, 2, 0, 1, 0, 1, 2, 0, 0, 1, 2, 0, 1]
    assert [s["skipped"] for s in tr] == [
        0, 0, 0, 0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 3]
    # t: 1-based count of the next update; a skip does not move it
    assert [s["t"] for s in tr] == [
        1, 2, 3, 4, 5, 5, 6, 7, 7, 7, 8, 9, 10, 11]
    for s in tr:
        assert s["found_inf"] == 0
        assert s["inv_scale"] * s["scale"] == 1.0
        t = s["t"]
        assert s["c1"] == float(np.float32(1.0 / (1.0 - 0.9 ** t)))
        assert s["c2"] == float(np.float32(
            1.0 / math.sqrt(1.0 - 0.999 ** t)))


def test_advance_reference_clamps():
    lo = run_script(ref.scaler_state(2.0), [1, 1, 1], 3)
    assert [s["scale"] for s in lo] == [2, 1, 1, 1]
    assert lo[-1]["skipped"] == 3 and lo[-1]["t"] == 1
    hi = run_script(ref.scaler_state(2.0 ** 23), [0, 0], 1)
    assert [s["scale"] for s in hi] == [2.0 ** 23, 2.0 ** 24, 2.0 ** 24]
    assert hi[-1]["t"] == 3


def test_advance_reference_fixed_scale():
    tr = run_script(ref.scaler_state(8192.0), [0, 1, 0, 0, 0], 2,
                    dynamic=False)
    assert all(s["scale"] == 8192.0 and s["good_steps"] == 0 for s in tr)
    assert tr[-1]["skipped"] == 1 and tr[-1]["t"] == 5


# --------------------------------------------------------------- checkpoint
class HostScaled(DeepTrainer):
    """A torchref DeepTrainer whose scaler state lives in a dict, so the
    sidecar can be exercised without a device."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.ls_state = object()
        self._ls = dict(scale=cfg.loss_scaling()[0], good_steps=0, skipped=0,
                        t=1)

    def loss_scale_state(self):
        return dict(self._ls)

    def set_loss_scale_state(self, scale, good_steps=0, skipped=0, t=1):
        self._ls = dict(scale=scale, good_steps=good_steps, skipped=skipped,
                        t=t)


def host_cfg(**kw):
    return TrainConfig(model="deepcnn", deep_channels="16,16", batch_size=2,
                       device="cpu", backend="torchref", log_interval=0,
                       loss_scale="dynamic", **kw)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_sidecar_round_trip(opt, tmp_path):
    a = HostScaled(host_cfg(optimizer=opt))
    a.set_loss_scale_state(4096.0, good_steps=17, skipped=3, t=42)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(a, path)
    meta = json.load(open(path + ".meta.json"))
    assert meta["loss_scale"] == dict(scale=4096.0, good_steps=17, skipped=3,
                                      t=42)
    if opt == "adam":
        assert meta["opt_step"] == 41     # read back from the scaler's t
    b = HostScaled(host_cfg(optimizer=opt))
    load_checkpoint(b, path)
    assert b.loss_scale_state() == a.loss_scale_state()
    assert b.opt_step == 41


def test_old_sidecar_loads_with_initial_values(tmp_path):
    plain = DeepTrainer(TrainConfig(
        model="deepcnn", deep_channels="16,16", batch_size=2, device="cpu",
        backend="torchref", log_interval=0, optimizer="adam"))
    plain.opt_step = 5
    path = str(tmp_path / "old.bin")
    save_checkpoint(plain, path)
    assert "loss_scale" not in json.load(open(path + ".meta.json"))
    b = HostScaled(host_cfg(optimizer="adam", loss_scale_init=1024.0))
    load_checkpoint(b, path)
    assert b.loss_scale_state() == dict(scale=1024.0, good_steps=0,
                                        skipped=0, t=6)
