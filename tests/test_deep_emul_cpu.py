"""CPU checks of the float64 oracle the GPU gradient tests lean on."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import deep_emul  # noqa: E402  (tools/: shared with tools/fuzz_deep.py)
from parallel_cnn_amd.data.mnist import synthetic_images
from parallel_cnn_amd.models.deepcnn import DeepCNN, DeepCNNSpec
from parallel_cnn_amd.ops import deep_ref


def batch(channels, seed, B=8):
    spec = DeepCNNSpec(channels=channels)
    m = DeepCNN(seed=0, spec=spec)
    x, labels = synthetic_images(B, 32, 32, 3, seed=seed, structured=False)
    return spec, m, x.view(B, 32, 32, 3), labels


@pytest.mark.parametrize("channels", [(32, 64, 64), (16, 32, 32, 64)])
def test_exact_oracle_is_deep_ref_in_float64(channels):
    """With identity hooks the copy is deep_ref.forward/backward: every
    block agrees with the fp32 oracle to fp32 accuracy."""
    spec, m, xh, labels = batch(channels, 7)
    g64, loss64 = deep_emul.grads64(xh, labels, m.params, spec)
    acts, pouts, y = deep_ref.forward(xh, m)
    g32, loss32 = deep_ref.backward(xh, m, acts, pouts, y, labels)
    ratios = deep_emul.block_ratios(g32, g64, spec)
    assert max(ratios.values()) < 1e-4, ratios
    assert abs(loss32 - loss64) < 1e-4 * loss64


def test_emulated_ratios_are_informative_at_fp32_and_bf16():
    for act in ("fp32", "bf16"):
        for channels, seed in (((32, 64, 64), 7), ((16, 32, 48), 23),
                               ((16, 32, 32, 64), 29)):
            spec, m, xh, labels = batch(channels, seed)
            _, _, emul = deep_emul.oracle_pair(xh, labels, m.params, spec,
                                               act)
            tol, excluded = deep_emul.block_tolerances(emul, act)
            assert not excluded
            assert 0 < min(emul.values()) and max(tol.values()) < 0.12, emul


def test_fp16_loses_exactly_the_stage0_conv_blocks():
    spec, m, xh, labels = batch((32, 64, 64), 7)
    _, _, emul = deep_emul.oracle_pair(xh, labels, m.params, spec, "fp16")
    _, excluded = deep_emul.block_tolerances(emul, "fp16")
    assert excluded == {"conv0_w", "conv0_b"}, emul


def test_uninformative_block_is_an_error_not_a_pass():
    spec, m, xh, labels = batch((16, 32, 32, 64), 29)
    _, _, emul = deep_emul.oracle_pair(xh, labels, m.params, spec, "fp16")
    with pytest.raises(AssertionError):
        # at fp16 the four-stage config loses pool0/conv1 as well; treated
        # as bf16 (no exclusions allowed) such a table must raise
        deep_emul.block_tolerances(emul, "bf16")


def test_compare_blocks_sees_a_zeroed_and_a_negated_block():
    spec, m, xh, labels = batch((32, 64, 64), 7)
    g, _, emul = deep_emul.oracle_pair(xh, labels, m.params, spec, "bf16")
    quiet = lambda *_: None
    ok, _ = deep_emul.compare_blocks("id", g, g, emul, "bf16", spec,
                                     log=quiet)
    assert not ok
    for name, factor in (("conv1_w", 0.0), ("pool0_w", -1.0)):
        bad = g.clone()
        off, n = spec.offsets[name]
        bad[off:off + n] *= factor
        fails, _ = deep_emul.compare_blocks("mut", bad, g, emul, "bf16",
                                            spec, log=quiet)
        assert len(fails) == 1 and fails[0].startswith(name), fails
