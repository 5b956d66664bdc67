"""GPU tests for k_fwdbwd_pair, the two-lanes-per-cell kernel 1 of the
in-block weight-grad LeNet step (PCNN_LENET_FWDBWD=pair).

The pair kernel keeps the cell kernel's term order in every conv output, in
the pool pre-activation (lane 0's running sum is handed to lane 1, which
continues it), in the fc dot products and in the residual, and both kernels
now fuse every forward multiply-add explicitly.  When this file was written
the cell kernel's `acc += w * x` was compiled to a compiler-chosen mix of
fused FMAs and unfused packed multiplies + adds, and a2 differed by one ulp
(5.96e-08); a2, y and dz are therefore still held to the 1e-6 bound that
applies when the forward is not bit-identical.  The slab rows differ in
summation order as well: two 200-term partials per cell added pairwise, and
owner sums over 18 + 18 (conv) or 8 x 27 (pool) rows instead of 36 or 4 x 54.

  * the slab rows, a2 and dz against the per-image torch_ref oracle;
  * pair against cell through the direct launcher;
  * one step against the fp32 oracle in all three activation dtypes;
  * a 5-step trajectory against cell, `grid`, the C++ loop and the graph;
  * bit-identical reruns and one momentum step;
  * the knob's values, and where it must have no effect.

Every test runs with the knob set to `pair` (direct launcher calls pass
variant=1, which is what the knob selects).
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

CELL, PAIR = 0, 1


def make_case(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, S.IN_PIX, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).float()
    return x, labels, params


def make_trainer(monkeypatch, fwdbwd, B, step="2", wgrad="inblock", **kw):
    monkeypatch.setenv("PCNN_LENET_STEP", step)
    monkeypatch.setenv("PCNN_LENET_WGRAD", wgrad)
    monkeypatch.setenv("PCNN_LENET_FWDBWD", fwdbwd)
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      log_interval=0, **kw)
    t = Trainer(cfg)
    assert t._inblock_variant == {"cell": CELL, "pair": PAIR}[fwdbwd]
    assert t._use_inblock() == (wgrad == "inblock" and step == "2")
    return t


def assert_clean_state(t):
    """After a step the flat bucket reads all-zero and the ticket 0."""
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert int(t.ws.ticket.item()) == 0


def run_kernel1(variant, x, labels, params, device, pool=0, loss=0):
    """One launch of kernel 1 through its binding on a NaN-filled slab."""
    C = native.require()
    B = x.shape[0]
    xd = x.to(device)
    ld = labels.to(device, dtype=torch.int32)
    pd = params.to(device)
    a2 = torch.empty(B, S.S1_OUT, device=device)
    y = torch.empty(B, S.FC_OUT, device=device)
    dz = torch.empty(B, S.FC_OUT, device=device)
    loss_accum = torch.zeros(1, device=device)
    slab = torch.full((B, S.GSLAB_LD), float("nan"), device=device)
    C.hip_fwdbwd_inblock(xd, pd, a2, y, dz, ld, loss_accum, slab, B,
                         native.current_stream_handle(), pool, loss,
                         variant=variant)
    torch.cuda.synchronize()
    return (slab[:, :S.OFF_FW].cpu(), a2.cpu(), y.cpu(), dz.cpu(),
            loss_accum.item())


# ------------------------------------------------------------------ slab
@pytest.mark.parametrize("pool,loss", [("trainable", "residual"),
                                       ("max", "residual"),
                                       ("trainable", "softmax_ce")])
def test_slab_rows_match_per_image_oracle(pool, loss, device, monkeypatch):
    monkeypatch.setenv("PCNN_LENET_FWDBWD", "pair")
    B = 3
    x, labels, params = make_case(B, seed=7)
    got, a2, _, dz, _ = run_kernel1(PAIR, x, labels, params, device,
                                    1 if pool == "max" else 0,
                                    1 if loss == "softmax_ce" else 0)
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
        assert (dz[b] - dzr[0]).abs().max().item() < 2e-4
        assert (a2[b] - a2r.reshape(-1)).abs().max().item() < 2e-4
    if pool == "max":
        assert torch.count_nonzero(got[:, S.OFF_S1W:]).item() == 0
    fails = lenet_emul.check_slab_rows(f"pair {pool}/{loss}", got, x, labels,
                                       params, pool, loss, "fp32")
    assert not fails, fails


# ---------------------------------------------------------- pair vs cell
@pytest.mark.parametrize("B", [1, 3, 65])
def test_pair_matches_cell_direct_launcher(B, device, monkeypatch):
    """fp32, direct launcher.  The forward term order was kept but its
    rounding is not the cell kernel's (every multiply-add fused here, a
    compiler-chosen mix there; see the module docstring), so a2, y and dz
    are held to 1e-6, not to torch.equal; slab rows are within the oracle
    tolerance of one another."""
    monkeypatch.setenv("PCNN_LENET_FWDBWD", "pair")
    x, labels, params = make_case(B, seed=40 + B)
    sc, a2c, yc, dzc, _ = run_kernel1(CELL, x, labels, params, device)
    sp, a2p, yp, dzp, _ = run_kernel1(PAIR, x, labels, params, device)
    assert torch.isfinite(sp).all()
    gmax = sc.abs().max().item()
    diff = (sp - sc).abs().max().item()
    tol = 2e-4 * max(1.0, gmax)
    print(f"B {B}: slab pair vs cell {diff:.3e} tol {tol:.3e} "
          f"|g|max {gmax:.3e}")
    assert diff < tol, diff
    assert gmax > 0
    d_a2 = (a2p - a2c).abs().max().item()
    d_y = (yp - yc).abs().max().item()
    d_dz = (dzp - dzc).abs().max().item()
    print(f"B {B}: a2 {d_a2:.3e} y {d_y:.3e} dz {d_dz:.3e}")
    assert d_a2 < 1e-6, d_a2
    assert d_y < 1e-6, d_y
    assert d_dz < 1e-6, d_dz


# -------------------------------------------------------------- one step
@pytest.mark.parametrize("act_dtype,gtol", [("bf16", 2e-2), ("fp16", 2e-2),
                                            ("fp32", 2e-4)])
def test_one_step_matches_oracle(act_dtype, gtol, device, monkeypatch):
    """One step from known params against params + step * ref_grads, with
    the grads tolerance times the step (grad_reduction="sum": step == dt)."""
    B = 16
    x, labels, params = make_case(B, seed=100 + B)
    t = make_trainer(monkeypatch, "pair", B, act_dtype=act_dtype,
                     grad_reduction="sum")
    with torch.no_grad():
        t.model.params.copy_(params.to(t.device))
    t.step(*t.stage_batch(x, labels))
    torch.cuda.synchronize()
    a1, a2, y = torch_ref.forward(x, params, "trainable", "residual")
    _, _, _, g, ref_loss = torch_ref.backward(x, params, a1, a2, y, labels,
                                              "trainable", "residual")
    step = t.cfg.dt
    want = params.double() + step * g.double()
    got = t.model.params.cpu().double()
    gmax = g.abs().max().item()
    diff = (got - want).abs().max().item()
    tol = gtol * max(1.0, gmax) * step
    print(f"pair B {B} {act_dtype}: param diff {diff:.3e} tol {tol:.3e} "
          f"|g|max {gmax:.3e}")
    assert diff < tol, f"params: max abs diff {diff} (tol {tol})"
    fails = lenet_emul.check_step(
        f"pair B{B} {act_dtype}", params, t.model.params.cpu(), t.cfg.dt, x,
        labels, "trainable", "residual", "inblock", act_dtype)
    assert not fails, fails
    assert (got - params.double()).abs().max().item() > 0.5 * step * gmax
    assert_clean_state(t)
    loss, n = t.consume_loss()
    assert n == B
    assert abs(loss - ref_loss) < 1e-2 * max(1.0, abs(ref_loss))


# ------------------------------------------------------------ trajectory
def test_five_steps_match_other_paths(device, monkeypatch):
    """pair against cell and against grid; Trainer.step against the C++
    loop and the captured graph of pair."""
    B = 16
    x, y = synthetic_mnist(5 * B, seed=3)
    tp = make_trainer(monkeypatch, "pair", B, act_dtype="fp32")
    tl = make_trainer(monkeypatch, "pair", B, act_dtype="fp32")
    tgr = make_trainer(monkeypatch, "pair", B, act_dtype="fp32")
    tc = make_trainer(monkeypatch, "cell", B, act_dtype="fp32")
    tg = make_trainer(monkeypatch, "pair", B, wgrad="grid",
                      act_dtype="fp32")
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        for t in (tp, tc, tg):
            t.step(*t.stage_batch(xb, yb))
    xp, yp = tl.stage_batch(x, y)
    tl.run_steps_pooled(xp.contiguous(), yp.contiguous(), 5)    # C++ loop
    tgr.enable_graph()
    tgr.run_steps_pooled(xp.contiguous(), yp.contiguous(), 5)   # graph
    torch.cuda.synchronize()
    pp = tp.model.params
    d_cell = (pp - tc.model.params).abs().max().item()
    d_grid = (pp - tg.model.params).abs().max().item()
    d_loop = (pp - tl.model.params).abs().max().item()
    d_graph = (pp - tgr.model.params).abs().max().item()
    print(f"pair vs cell {d_cell:.3e}, vs grid {d_grid:.3e}, vs C++ loop "
          f"{d_loop:.3e}, vs graph {d_graph:.3e}")
    assert d_cell < 1e-5, d_cell
    assert d_grid < 1e-5, d_grid
    assert d_loop < 1e-5, d_loop
    assert d_graph < 1e-5, d_graph
    moved = (pp - Trainer(tp.cfg).model.params).abs().max().item()
    assert moved > 1e-4, moved
    for t in (tp, tc, tg, tl, tgr):
        assert_clean_state(t)


# ------------------------------------------- reproducibility and momentum
def test_reruns_are_bit_identical(device, monkeypatch):
    B, steps = 65, 20
    x, y = synthetic_mnist(steps * B, seed=23)

    def run():
        t = make_trainer(monkeypatch, "pair", B, act_dtype="fp32")
        xs, ys = t.stage_batch(x, y)
        for s in range(steps):
            t.step(xs[s * B:(s + 1) * B], ys[s * B:(s + 1) * B])
        torch.cuda.synchronize()
        assert_clean_state(t)
        return t.model.params.clone(), t.ws.y.clone()

    p0, y0 = run()
    p1, y1 = run()
    assert torch.equal(p0, p1), (p0 - p1).abs().max().item()
    assert torch.equal(y0, y1), (y0 - y1).abs().max().item()


def test_momentum_step_matches_cell(device, monkeypatch):
    B = 3
    x, labels, params = make_case(B, seed=11)
    res = []
    for knob in ("pair", "cell"):
        t = make_trainer(monkeypatch, knob, B, act_dtype="fp32",
                         momentum=0.9, weight_decay=1e-4)
        assert t.vel is not None
        with torch.no_grad():
            t.model.params.copy_(params.to(t.device))
        t.step(*t.stage_batch(x, labels))
        torch.cuda.synchronize()
        assert_clean_state(t)
        res.append((t.model.params.clone(), t.vel.clone()))
    dp = (res[0][0] - res[1][0]).abs().max().item()
    dv = (res[0][1] - res[1][1]).abs().max().item()
    moved = (res[0][0].cpu() - params).abs().max().item()
    print(f"momentum step pair vs cell: params {dp:.3e} vel {dv:.3e}, "
          f"moved {moved:.3e}")
    assert dp < 1e-5, dp
    assert moved > 0


# ----------------------------------------------------------------- knob
def test_bad_knob_raises(device, monkeypatch):
    monkeypatch.setenv("PCNN_LENET_FWDBWD", "quad")
    with pytest.raises(ValueError):
        Trainer(TrainConfig(batch_size=4, device="cuda", backend="hip",
                            log_interval=0))
    C = native.require()
    x, labels, params = make_case(1)
    with pytest.raises(RuntimeError):
        run_kernel1(2, x, labels, params, device)
    assert C.INBLOCK_DEFAULT_VARIANT in (CELL, PAIR)


@pytest.mark.parametrize("step,wgrad", [("3", "inblock"), ("2", "grid")])
def test_knob_has_no_effect_outside_inblock_step(step, wgrad, device,
                                                 monkeypatch):
    """Under the 3-launch step and under the grid weight-grad kernel
    kernel 1 of the in-block step does not run whatever the knob says: the
    slab, filled with NaN beforehand, is left alone, and the step agrees
    with the same path under `cell`."""
    B = 16
    x, y = synthetic_mnist(B, seed=9)
    res = []
    for knob in ("pair", "cell"):
        t = make_trainer(monkeypatch, knob, B, step=step, wgrad=wgrad,
                         act_dtype="fp32")
        t.ws.gslab.fill_(float("nan"))
        t.step(*t.stage_batch(x, y))
        torch.cuda.synchronize()
        assert torch.isnan(t.ws.gslab).all()
        assert torch.isfinite(t.model.params).all()
        assert_clean_state(t)
        res.append(t.model.params.clone())
    diff = (res[0] - res[1]).abs().max().item()
    assert diff < 1e-5, diff


def test_knob_has_no_effect_above_max_batch(device, monkeypatch):
    """B = INBLOCK_MAX_BATCH + 1: the step launcher hands over to
    k_wgrad_update for either variant and leaves the slab alone."""
    C = native.require()
    B = C.INBLOCK_MAX_BATCH + 1
    x, y = synthetic_mnist(B, seed=5)
    res = []
    for variant, knob in ((PAIR, "pair"), (CELL, "cell")):
        t = make_trainer(monkeypatch, knob, B, act_dtype="fp32")
        xb, yb = t.stage_batch(x, y)
        m, w = t.model, t.ws
        w.gslab.fill_(float("nan"))
        C.hip_step_inblock(xb, m.params, w.a1, w.a2, w.y, w.dz, w.dz2, w.dz1,
                           yb, w.loss_accum, m.grads, w.ticket, w.gslab,
                           t.cfg.dt * t._update_scale(B), B,
                           t.cfg.wgrad_chunk,
                           native.current_stream_handle(), 0, 0,
                           variant=variant)
        torch.cuda.synchronize()
        assert torch.isnan(w.gslab).all()
        assert_clean_state(t)
        res.append(m.params.clone())
    diff = (res[0] - res[1]).abs().max().item()
    moved = (res[0] - Trainer(t.cfg).model.params).abs().max().item()
    print(f"B {B}: pair vs cell {diff:.3e}, step moved {moved:.3e}")
    assert diff < 1e-5, diff
    assert moved > 0
