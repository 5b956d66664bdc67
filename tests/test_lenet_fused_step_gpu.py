"""GPU tests for the reduced-launch LeNet training step (PCNN_LENET_STEP).

Every shipped variant is selected through the environment knob, exactly as
a user would, and driven through Trainer.step so the new binding runs:
  * one step against the fp32 torch_ref oracle (params, y, loss, and the
    all-zero gradient bucket / ticket afterwards);
  * a 5-step trajectory against the cpu backend and the 3-launch path;
  * the masked-role modes (max pooling, softmax cross-entropy);
  * bf16 activation storage;
  * uneven block arrival (a busy device) against the same run done quiet.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import lenet_emul  # noqa: E402  (tools/: the per-block rule)

from parallel_cnn_amd.config import TrainConfig
from parallel_cnn_amd.data.mnist import synthetic_mnist
from parallel_cnn_amd.engine.trainer import Trainer
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

# launches per step of every shipped reduced-launch variant
VARIANTS = ["2"]


def make_case(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, S.IN_PIX, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).float()
    return x, labels, params


def make_trainer(monkeypatch, variant, B, **kw):
    monkeypatch.setenv("PCNN_LENET_STEP", variant)
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      log_interval=0, **kw)
    t = Trainer(cfg)
    assert t._step_mode == int(variant)
    return t


def assert_clean_state(t):
    """After a step the flat bucket reads all-zero and the ticket 0."""
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert int(t.ws.ticket.item()) == 0


def one_step_vs_oracle(monkeypatch, variant, B, act_dtype, gtol, pool,
                       loss):
    """One step from known params; the update is checked against
    params + step * ref_grads with the grads tolerance times the step.
    grad_reduction="sum" makes step == dt, so the bound sits far above the
    fp32 rounding of the parameter add itself."""
    x, labels, params = make_case(B, seed=100 + B)
    t = make_trainer(monkeypatch, variant, B, act_dtype=act_dtype,
                     pool=pool, loss=loss, grad_reduction="sum")
    assert t._fused_step_mode() == int(variant)
    with torch.no_grad():
        t.model.params.copy_(params.to(t.device))
    t.step(*t.stage_batch(x, labels))
    torch.cuda.synchronize()
    a1, a2, y = torch_ref.forward(x, params, pool, loss)
    _, _, _, g, ref_loss = torch_ref.backward(x, params, a1, a2, y, labels,
                                              pool, loss)
    step = t.cfg.dt
    want = params.double() + step * g.double()
    got = t.model.params.cpu().double()
    gmax = g.abs().max().item()
    diff = (got - want).abs().max().item()
    tol = gtol * max(1.0, gmax) * step
    print(f"variant {variant} B {B} {act_dtype} {pool}/{loss}: "
          f"param diff {diff:.3e} tol {tol:.3e} |g|max {gmax:.3e}")
    assert diff < tol, f"params: max abs diff {diff} (tol {tol})"
    fails = lenet_emul.check_step(
        f"variant {variant} B{B} {act_dtype} {pool}/{loss}", params,
        t.model.params.cpu(), t.cfg.dt, x, labels, pool, loss, "inblock",
        act_dtype)
    assert not fails, fails
    # the step must have moved the parameters by the oracle's amount
    assert (got - params.double()).abs().max().item() > 0.5 * step * gmax
    return t, y, ref_loss


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B", [1, 3, 16, 65])
def test_one_step_fp32_matches_oracle(variant, B, device, monkeypatch):
    t, y, ref_loss = one_step_vs_oracle(monkeypatch, variant, B, "fp32",
                                        2e-4, "trainable", "residual")
    ydiff = (t.ws.y[:B].cpu() - y).abs().max().item()
    assert ydiff < 2e-4, f"y: max abs diff {ydiff}"
    assert_clean_state(t)
    loss, n = t.consume_loss()
    assert n == B
    assert abs(loss - ref_loss) < 1e-2 * max(1.0, abs(ref_loss))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("pool,loss", [("max", "residual"),
                                       ("trainable", "softmax_ce")])
def test_one_step_masked_modes_match_oracle(variant, pool, loss, device,
                                            monkeypatch):
    """Under max pooling the pool-role blocks return before doing any work;
    they must still arrive or the update never happens."""
    B = 3
    t, y, ref_loss = one_step_vs_oracle(monkeypatch, variant, B, "fp32",
                                        2e-4, pool, loss)
    ydiff = (t.ws.y[:B].cpu() - y).abs().max().item()
    assert ydiff < 2e-4, f"y: max abs diff {ydiff}"
    assert_clean_state(t)
    got_loss, _ = t.consume_loss()
    assert abs(got_loss - ref_loss) < 1e-2 * max(1.0, abs(ref_loss))


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_step_bf16_close_to_oracle(variant, device, monkeypatch):
    t, _, _ = one_step_vs_oracle(monkeypatch, variant, 16, "bf16", 2e-2,
                                 "trainable", "residual")
    assert_clean_state(t)


@pytest.mark.parametrize("variant", VARIANTS)
def test_five_steps_match_cpu_and_three_launch(variant, device, monkeypatch):
    """One workspace, no host sync between steps: the ticket must be back at
    0 and the bucket re-zeroed for every following launch."""
    B = 16
    x, y = synthetic_mnist(5 * B, seed=3)
    tn = make_trainer(monkeypatch, variant, B, act_dtype="fp32")
    tp = make_trainer(monkeypatch, variant, B, act_dtype="fp32")
    t3 = make_trainer(monkeypatch, "3", B, act_dtype="fp32")
    assert t3._fused_step_mode() == 3
    tc = Trainer(TrainConfig(batch_size=B, device="cpu", backend="cpu",
                             log_interval=0))
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        tn.step(*tn.stage_batch(xb, yb))
        t3.step(*t3.stage_batch(xb, yb))
        tc.step(*tc.stage_batch(xb, yb))
    xp, yp = tp.stage_batch(x, y)
    tp.run_steps_pooled(xp.contiguous(), yp.contiguous(), 5)  # C++ loop
    torch.cuda.synchronize()
    d_cpu = (tn.model.params.cpu() - tc.model.params).abs().max().item()
    d_3 = (tn.model.params - t3.model.params).abs().max().item()
    d_loop = (tn.model.params - tp.model.params).abs().max().item()
    print(f"variant {variant}: vs cpu {d_cpu:.3e}, vs 3-launch {d_3:.3e}, "
          f"vs C++ loop {d_loop:.3e}")
    assert d_cpu < 5e-4, d_cpu
    assert d_3 < 1e-5, d_3
    assert d_loop < 1e-5, d_loop
    assert_clean_state(tn)
    assert_clean_state(tp)
    ln, nn = tn.consume_loss()
    lc, nc = tc.consume_loss()
    assert nn == nc == 5 * B
    assert abs(ln - lc) < 1e-2 * max(1.0, lc)


@pytest.mark.parametrize("variant", VARIANTS)
def test_uneven_arrival_matches_quiet_run(variant, device, monkeypatch):
    """20 steps at B=65 while an unrelated large elementwise kernel keeps
    the device busy on a second stream, so the blocks of one launch start
    and arrive unevenly; every parameter word is compared with the same run
    on an idle device."""
    B, steps = 65, 20
    x, y = synthetic_mnist(steps * B, seed=23)

    def run(busy):
        t = make_trainer(monkeypatch, variant, B, act_dtype="fp32")
        xs, ys = t.stage_batch(x, y)
        side = torch.cuda.Stream()
        noise = torch.ones(1 << 24, device=t.device)
        side.wait_stream(torch.cuda.current_stream())
        for s in range(steps):
            if busy:
                with torch.cuda.stream(side):
                    noise.mul_(1.0001).add_(1e-3)
            t.step(xs[s * B:(s + 1) * B], ys[s * B:(s + 1) * B])
        torch.cuda.synchronize()
        assert_clean_state(t)
        return t.model.params.clone()

    quiet = run(False)
    loaded = run(True)
    diff = (quiet - loaded).abs().max().item()
    print(f"variant {variant}: busy vs quiet max abs diff {diff:.3e}")
    assert diff < 1e-5, diff
