"""GPU tests for the in-block weight-grad LeNet step (PCNN_LENET_WGRAD).

The step is k_fwdbwd with the conv/pool weight gradients formed in the
per-image block and stored as one slab row per image, then k_reduce_update
(slab reduce + fc weight grads + SGD apply, one owner per parameter).

  * the slab rows of kernel 1 against the per-image torch_ref gradients;
  * one step against the fp32 torch_ref oracle, for `inblock` and for
    `grid` (the k_wgrad_update path, which no other test selects once the
    default is `inblock`);
  * a 5-step trajectory against `grid`, the 3-launch path and the cpu
    backend, and Trainer.step / the C++ loop / the captured graph against
    one another;
  * bit-identical reruns, on a quiet and on a busy device;
  * the knob's values and the launcher's large-batch fallback.

The slab kernel is called through its binding and never reads the knob, so
its cases are not parametrised over it.
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
from parallel_cnn_amd.ops import native
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

KNOBS = ["inblock", "grid"]


def make_case(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, S.IN_PIX, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).float()
    return x, labels, params


def make_trainer(monkeypatch, knob, B, step="2", **kw):
    monkeypatch.setenv("PCNN_LENET_STEP", step)
    monkeypatch.setenv("PCNN_LENET_WGRAD", knob)
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      log_interval=0, **kw)
    t = Trainer(cfg)
    assert t._use_inblock() == (knob == "inblock" and step == "2")
    return t


def assert_clean_state(t):
    """After a step the flat bucket reads all-zero and the ticket 0."""
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert int(t.ws.ticket.item()) == 0


# ------------------------------------------------------------------ slab
@pytest.mark.parametrize("pool,loss", [("trainable", "residual"),
                                       ("max", "residual"),
                                       ("trainable", "softmax_ce")])
def test_slab_rows_match_per_image_oracle(pool, loss, device):
    """Row b of the slab carries image b's conv/pool gradient with the
    reference scale factors already applied (1/576 conv, 1/216 pool bias),
    i.e. exactly torch_ref.backward's first 173 entries for that image."""
    C = native.require()
    B = 3
    x, labels, params = make_case(B, seed=7)
    xd = x.to(device)
    ld = labels.to(device, dtype=torch.int32)
    pd = params.to(device)
    a2 = torch.empty(B, S.S1_OUT, device=device)
    y = torch.empty(B, S.FC_OUT, device=device)
    dz = torch.empty(B, S.FC_OUT, device=device)
    loss_accum = torch.zeros(1, device=device)
    slab = torch.full((B, S.GSLAB_LD), float("nan"), device=device)
    C.hip_fwdbwd_inblock(xd, pd, a2, y, dz, ld, loss_accum, slab, B,
                         native.current_stream_handle(),
                         1 if pool == "max" else 0,
                         1 if loss == "softmax_ce" else 0)
    torch.cuda.synchronize()
    got = slab[:, :S.OFF_FW].cpu()
    assert torch.isfinite(got).all(), "a slab column was not written"
    for b in range(B):
        xb, lb = x[b:b + 1], labels[b:b + 1]
        a1r, a2r, yr = torch_ref.forward(xb, params, pool, loss)
        dzr, _, _, g, _ = torch_ref.backward(xb, params, a1r, a2r, yr, lb,
                                             pool, loss)
        want = g[:S.OFF_FW]
        gmax = g.abs().max().item()
        diff = (got[b] - want).abs().max().item()
        tol = 2e-4 * max(1.0, gmax)
        print(f"{pool}/{loss} image {b}: slab diff {diff:.3e} tol {tol:.3e}")
        assert diff < tol, f"image {b}: max abs diff {diff} (tol {tol})"
        assert got[b][:S.OFF_S1W].abs().max().item() > 0
        # the stores kernel 2 depends on are still made
        assert (dz[b].cpu() - dzr[0]).abs().max().item() < 2e-4
        assert (a2[b].cpu() - a2r.reshape(-1)).abs().max().item() < 2e-4
    if pool == "max":
        assert torch.count_nonzero(got[:, S.OFF_S1W:]).item() == 0
    fails = lenet_emul.check_slab_rows(f"{pool}/{loss}", got, x, labels,
                                       params, pool, loss, "fp32")
    assert not fails, fails


# -------------------------------------------------------------- one step
def one_step_vs_oracle(monkeypatch, knob, B, act_dtype, gtol, pool, loss):
    """One step from known params against params + step * ref_grads, with
    the grads tolerance times the step (grad_reduction="sum": step == dt)."""
    x, labels, params = make_case(B, seed=100 + B)
    t = make_trainer(monkeypatch, knob, B, act_dtype=act_dtype, pool=pool,
                     loss=loss, grad_reduction="sum")
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
    print(f"{knob} B {B} {act_dtype} {pool}/{loss}: param diff {diff:.3e} "
          f"tol {tol:.3e} |g|max {gmax:.3e}")
    assert diff < tol, f"params: max abs diff {diff} (tol {tol})"
    fails = lenet_emul.check_step(
        f"{knob} B{B} {act_dtype} {pool}/{loss}", params,
        t.model.params.cpu(), t.cfg.dt, x, labels, pool, loss, knob,
        act_dtype)
    assert not fails, fails
    assert (got - params.double()).abs().max().item() > 0.5 * step * gmax
    if pool == "max":  # the pool parameters come out unchanged
        assert torch.equal(t.model.params[S.OFF_S1W:S.OFF_FW].cpu(),
                           params[S.OFF_S1W:S.OFF_FW])
    assert_clean_state(t)
    return t, y, ref_loss


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("B", [1, 3, 16, 65])
def test_one_step_fp32_matches_oracle(knob, B, device, monkeypatch):
    t, y, ref_loss = one_step_vs_oracle(monkeypatch, knob, B, "fp32", 2e-4,
                                        "trainable", "residual")
    ydiff = (t.ws.y[:B].cpu() - y).abs().max().item()
    assert ydiff < 2e-4, f"y: max abs diff {ydiff}"
    loss, n = t.consume_loss()
    assert n == B
    assert abs(loss - ref_loss) < 1e-2 * max(1.0, abs(ref_loss))


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("act_dtype", ["bf16", "fp16"])
def test_one_step_half_acts_close_to_oracle(knob, act_dtype, device,
                                            monkeypatch):
    one_step_vs_oracle(monkeypatch, knob, 16, act_dtype, 2e-2, "trainable",
                       "residual")


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("pool,loss", [("max", "residual"),
                                       ("trainable", "softmax_ce")])
def test_one_step_masked_modes_match_oracle(knob, pool, loss, device,
                                            monkeypatch):
    B = 3
    t, y, ref_loss = one_step_vs_oracle(monkeypatch, knob, B, "fp32", 2e-4,
                                        pool, loss)
    ydiff = (t.ws.y[:B].cpu() - y).abs().max().item()
    assert ydiff < 2e-4, f"y: max abs diff {ydiff}"
    got_loss, _ = t.consume_loss()
    assert abs(got_loss - ref_loss) < 1e-2 * max(1.0, abs(ref_loss))


# ------------------------------------------------------------ trajectory
def test_five_steps_match_other_paths(device, monkeypatch):
    """inblock against grid, the 3-launch path and the cpu backend; and the
    three ways of driving it (Trainer.step, the C++ loop, the captured
    graph) against one another.  No host sync between steps."""
    B = 16
    x, y = synthetic_mnist(5 * B, seed=3)
    ti = make_trainer(monkeypatch, "inblock", B, act_dtype="fp32")
    tp = make_trainer(monkeypatch, "inblock", B, act_dtype="fp32")
    tgr = make_trainer(monkeypatch, "inblock", B, act_dtype="fp32")
    tg = make_trainer(monkeypatch, "grid", B, act_dtype="fp32")
    t3 = make_trainer(monkeypatch, "inblock", B, step="3", act_dtype="fp32")
    assert t3._fused_step_mode() == 3
    tc = Trainer(TrainConfig(batch_size=B, device="cpu", backend="cpu",
                             log_interval=0))
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        for t in (ti, tg, t3, tc):
            t.step(*t.stage_batch(xb, yb))
    xp, yp = tp.stage_batch(x, y)
    tp.run_steps_pooled(xp.contiguous(), yp.contiguous(), 5)   # C++ loop
    tgr.enable_graph()
    tgr.run_steps_pooled(xp.contiguous(), yp.contiguous(), 5)  # graph
    torch.cuda.synchronize()
    pi = ti.model.params
    d_grid = (pi - tg.model.params).abs().max().item()
    d_3 = (pi - t3.model.params).abs().max().item()
    d_cpu = (pi.cpu() - tc.model.params).abs().max().item()
    d_loop = (pi - tp.model.params).abs().max().item()
    d_graph = (pi - tgr.model.params).abs().max().item()
    d_lg = (tp.model.params - tgr.model.params).abs().max().item()
    print(f"inblock vs grid {d_grid:.3e}, vs 3-launch {d_3:.3e}, vs cpu "
          f"{d_cpu:.3e}; step vs C++ loop {d_loop:.3e}, vs graph "
          f"{d_graph:.3e}, loop vs graph {d_lg:.3e}")
    assert d_grid < 1e-5, d_grid
    assert d_3 < 1e-5, d_3
    assert d_cpu < 5e-4, d_cpu
    assert d_loop < 1e-5, d_loop
    assert d_graph < 1e-5, d_graph
    assert d_lg < 1e-5, d_lg
    for t in (ti, tp, tgr):
        assert_clean_state(t)
    li, ni = ti.consume_loss()
    lc, nc = tc.consume_loss()
    assert ni == nc == 5 * B
    assert abs(li - lc) < 1e-2 * max(1.0, lc)


# ----------------------------------------------------------- determinism
@pytest.mark.parametrize("busy", [False, True])
def test_reruns_are_bit_identical(busy, device, monkeypatch):
    """20 steps at B=65 twice from the same state: every owner adds in a
    fixed order, so params and y must be equal bit for bit — also while an
    unrelated kernel on a second stream keeps the device busy during the
    second run."""
    B, steps = 65, 20
    x, y = synthetic_mnist(steps * B, seed=23)

    def run(noisy):
        t = make_trainer(monkeypatch, "inblock", B, act_dtype="fp32")
        xs, ys = t.stage_batch(x, y)
        side = torch.cuda.Stream()
        noise = torch.ones(1 << 24, device=t.device)
        side.wait_stream(torch.cuda.current_stream())
        for s in range(steps):
            if noisy:
                with torch.cuda.stream(side):
                    noise.mul_(1.0001).add_(1e-3)
            t.step(xs[s * B:(s + 1) * B], ys[s * B:(s + 1) * B])
        torch.cuda.synchronize()
        assert_clean_state(t)
        return t.model.params.clone(), t.ws.y.clone()

    p0, y0 = run(False)
    p1, y1 = run(busy)
    assert torch.equal(p0, p1), (p0 - p1).abs().max().item()
    assert torch.equal(y0, y1), (y0 - y1).abs().max().item()


# ------------------------------------------------------ knob and fallback
def test_bad_knob_raises(device, monkeypatch):
    monkeypatch.setenv("PCNN_LENET_WGRAD", "fused")
    with pytest.raises(ValueError):
        Trainer(TrainConfig(batch_size=4, device="cuda", backend="hip",
                            log_interval=0))
    monkeypatch.setenv("PCNN_LENET_WGRAD", "inblock")
    monkeypatch.setenv("PCNN_LENET_STEP", "1")
    with pytest.raises(ValueError):
        Trainer(TrainConfig(batch_size=4, device="cuda", backend="hip",
                            log_interval=0))


def test_step_launcher_above_threshold_matches_three_launch(device,
                                                            monkeypatch):
    """One call of the step launcher at the smallest batch it hands to the
    k_wgrad_update path, against the 3-launch step."""
    C = native.require()
    B = C.INBLOCK_MAX_BATCH + 1
    x, y = synthetic_mnist(B, seed=5)
    t = make_trainer(monkeypatch, "inblock", B, act_dtype="fp32")
    t3 = make_trainer(monkeypatch, "grid", B, step="3", act_dtype="fp32")
    xb, yb = t.stage_batch(x, y)
    m, w = t.model, t.ws
    C.hip_step_inblock(xb, m.params, w.a1, w.a2, w.y, w.dz, w.dz2, w.dz1, yb,
                       w.loss_accum, m.grads, w.ticket, w.gslab,
                       t.cfg.dt * t._update_scale(B), B, t.cfg.wgrad_chunk,
                       native.current_stream_handle(), 0, 0)
    t3.step(xb, yb)
    torch.cuda.synchronize()
    diff = (m.params - t3.model.params).abs().max().item()
    moved = (t3.model.params - Trainer(t3.cfg).model.params).abs().max()
    print(f"B {B}: launcher vs 3-launch {diff:.3e}, step moved {moved:.3e}")
    assert diff < 1e-5, diff
    assert moved.item() > 0
    assert_clean_state(t)
