"""GPU tests for SGD momentum / Nesterov / weight decay in the fused update
kernels.

  * every update site on known params / grads / velocity against
    torch_ref.update_momentum (k_update_mom, the tail of k_wgrad_update_mom,
    the owner lanes of k_reduce_update_mom, k_update_n_mom,
    k_update_cast_all_mom);
  * LeNet steps and 5-step trajectories against the fp32 torch_ref oracle on
    the in-block, grid and 3-launch paths, across the batch sizes at which
    the launchers change kernels;
  * Trainer.step / the C++ loop / the captured graph against one another,
    with the capture warm-up leaving params and velocity as they were;
  * DeepCNN trajectory, zero pad rows, graph replay;
  * exact resume, and the default optimizer holding no velocity at all.

Ascent convention: u = scale*g - wd*p; v = mu*v + u; p += dt*v (nesterov:
p += dt*(u + mu*v)).
"""
import os

import pytest
import torch

from parallel_cnn_amd.config import TrainConfig
from parallel_cnn_amd.data.mnist import synthetic_images, synthetic_mnist
from parallel_cnn_amd.engine.deep import DeepTrainer
from parallel_cnn_amd.engine.trainer import Trainer
from parallel_cnn_amd.ops import native
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref
from parallel_cnn_amd.utils.checkpoint import load_checkpoint, save_checkpoint

pytestmark = pytest.mark.gpu

EPS = torch.finfo(torch.float32).eps
OPTS = [(0.9, 0.0, False), (0.9, 5e-4, False), (0.9, 5e-4, True),
        (0.0, 1e-3, False)]
DT, SCALE = 0.1, 0.25
PATHS = [("inblock", "2"), ("grid", "2"), ("grid", "3")]
# deep_channels: the smallest widths the MFMA path accepts (multiples of
# 16); the parameter count, 35396, is not a multiple of the 256-thread block
DEEP_CH = "16,32"


def rand_pm(n, gen):
    """Uniform in (-0.5, 0.5], the model's own init range."""
    return 0.5 - torch.rand(n, generator=gen)


def check_site(p, v, g, p_ref, v_ref):
    """p, v within 4 eps of their own largest magnitude (three multiply-adds
    per element whose contraction may differ), g all zero."""
    pd = (p.cpu() - p_ref).abs().max().item()
    vd = (v.cpu() - v_ref).abs().max().item()
    ptol = 4 * EPS * p_ref.abs().max().item()
    vtol = 4 * EPS * v_ref.abs().max().item()
    print(f"p diff {pd:.3e} tol {ptol:.3e}; v diff {vd:.3e} tol {vtol:.3e}")
    assert pd <= ptol, (pd, ptol)
    assert vd <= vtol, (vd, vtol)
    assert torch.count_nonzero(g).item() == 0


def site_case(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return rand_pm(n, gen), rand_pm(n, gen), rand_pm(n, gen)


# ------------------------------------------------------- 7 kernel-level sites
@pytest.mark.parametrize("mu,wd,nesterov", OPTS)
def test_hip_update_momentum_site(mu, wd, nesterov, device):
    C = native.require()
    p, g, v = site_case(S.N_PARAMS, 1)
    pr, gr, vr = p.clone(), g.clone(), v.clone()
    torch_ref.update_momentum(pr, gr, vr, DT, SCALE, mu, wd, nesterov)
    pd, gd, vd = p.to(device), g.to(device), v.to(device)
    C.hip_update_momentum(pd, gd, vd, DT, SCALE, mu, wd, nesterov,
                          native.current_stream_handle())
    torch.cuda.synchronize()
    check_site(pd, vd, gd, pr, vr)
    # N_PARAMS = 4*585 + 3: the scalar tail moved too
    assert S.N_PARAMS % 4 == 3
    assert ((pd.cpu() - p)[-3:].abs() > 1e-4).all()
    assert ((pd.cpu() - p)[:8].abs() > 0).any()


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mu,wd,nesterov", OPTS[1:3])
def test_hip_wgrad_update_momentum_tail_site(mu, wd, nesterov, act, device):
    """All-zero dz / dz1 / dz2 add nothing to the bucket, so the last
    arriver's tail applies exactly the grads that were put there."""
    C = native.require()
    B = 3
    p, g, v = site_case(S.N_PARAMS, 2)
    pr, gr, vr = p.clone(), g.clone(), v.clone()
    torch_ref.update_momentum(pr, gr, vr, DT, SCALE, mu, wd, nesterov)
    pd, gd, vd = p.to(device), g.to(device), v.to(device)
    x = torch.rand(B, S.IN_PIX, device=device).to(act)
    a1 = torch.rand(B, S.C1_OUT, device=device).to(act)
    a2 = torch.rand(B, S.S1_OUT, device=device).to(act)
    dz = torch.zeros(B, S.FC_OUT, device=device)
    dz2 = torch.zeros(B, S.S1_OUT, device=device)
    dz1 = torch.zeros(B, S.C1_OUT, device=device, dtype=act)
    ticket = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_wgrad_update_momentum(x, a1, a2, dz, dz2, dz1, gd, pd, vd, DT,
                                SCALE, mu, wd, nesterov, ticket, B, 0, 7,
                                native.current_stream_handle())
    torch.cuda.synchronize()
    check_site(pd, vd, gd, pr, vr)
    assert int(ticket.item()) == 0
    assert ((pd.cpu() - p)[-3:].abs() > 1e-4).all()


@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("mu,wd,nesterov", OPTS[1:3])
def test_hip_reduce_update_momentum_site(mu, wd, nesterov, B, device):
    """Slab, dz and a2 hold small multiples of 1/16, so every batch sum is
    exact in fp32 whatever the order and the gradient the owner lane sees is
    known to the bit; B=33 crosses the 32-image stride."""
    C = native.require()
    gen = torch.Generator().manual_seed(3)
    q = lambda *shape: torch.randint(-8, 9, shape, generator=gen) / 16.0
    slab = q(B, S.GSLAB_LD)
    a2 = q(B, S.S1_OUT)
    dz = q(B, S.FC_OUT)
    g = torch.empty(S.N_PARAMS)
    g[:S.OFF_FW] = slab[:, :S.OFF_FW].sum(0)
    g[S.OFF_FW:S.OFF_FB] = (dz.T @ a2).reshape(-1)
    g[S.OFF_FB:] = dz.sum(0)
    assert torch.equal(g.double(), torch.cat([
        slab[:, :S.OFF_FW].double().sum(0),
        (dz.double().T @ a2.double()).reshape(-1), dz.double().sum(0)]))
    p, _, v = site_case(S.N_PARAMS, 4)
    pr, vr = p.clone(), v.clone()
    torch_ref.update_momentum(pr, g.clone(), vr, DT, SCALE, mu, wd, nesterov)
    pd, vd = p.to(device), v.to(device)
    C.hip_reduce_update_momentum(slab.to(device), a2.to(device),
                                 dz.to(device), pd, vd, DT, SCALE, mu, wd,
                                 nesterov, B, native.current_stream_handle())
    torch.cuda.synchronize()
    check_site(pd, vd, torch.zeros(1), pr, vr)
    assert (pd.cpu() - p).abs().max().item() > 1e-3


def deep_trainer(device, B=4, **kw):
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      model="deepcnn", deep_channels=DEEP_CH,
                      log_interval=0, **kw)
    return DeepTrainer(cfg)


def pad_row_mask(spec):
    """True on the conv-weight pad rows (kc >= Kc) of the flat vector."""
    mask = torch.zeros(spec.n_params, dtype=torch.bool)
    for i, st in enumerate(spec.stages):
        off, n = spec.offsets[f"conv{i}_w"]
        m = torch.zeros(st.kcp, st.cout, dtype=torch.bool)
        m[st.kc:] = True
        mask[off:off + n] = m.reshape(-1)
    assert mask.any()
    return mask


@pytest.mark.parametrize("mu,wd,nesterov", OPTS[1:])
def test_deep_update_cast_momentum_site(mu, wd, nesterov, device):
    C = native.require()
    t = deep_trainer(device, momentum=0.9)
    spec = t.model.spec
    n = spec.n_params
    assert n % 256 != 0
    pad = pad_row_mask(spec)
    p = t.model.params.cpu().clone()
    assert torch.count_nonzero(p[pad]).item() == 0
    _, g, v = site_case(n, 5)
    g[pad] = 0.0
    v[pad] = 0.0
    pr, gr, vr = p.clone(), g.clone(), v.clone()
    torch_ref.update_momentum(pr, gr, vr, DT, SCALE, mu, wd, nesterov)
    pd, gd, vd = p.to(device), g.to(device), v.to(device)
    d = t.ws.cast_desc
    desc = (d["R"], d["C"], d["K"], d["Cin"], d["w_off"], d["bf_off"],
            d["bfT_off"], d["rot_off"], d["p8_off"])
    wbuf = torch.zeros_like(t.ws.wbuf)
    sh = native.current_stream_handle()
    C.deep_update_cast_momentum(pd, gd, vd, DT, SCALE, mu, wd, nesterov,
                                wbuf, *desc, sh)
    torch.cuda.synchronize()
    check_site(pd, vd, gd, pr, vr)
    assert (pd.cpu() - p)[-1].abs().item() > 1e-4     # last, partial block
    assert torch.count_nonzero(pd.cpu()[pad]).item() == 0
    assert torch.count_nonzero(vd.cpu()[pad]).item() == 0
    # the bf16 images are those of the post-momentum params
    want = torch.zeros_like(wbuf)
    C.deep_cast_all(pd, want, *desc, sh)
    torch.cuda.synchronize()
    assert torch.count_nonzero(want).item() > 0
    assert torch.equal(wbuf.view(torch.int16), want.view(torch.int16))
    # the generic kernel on the same inputs
    p2, g2, v2 = p.to(device), g.to(device), v.to(device)
    C.deep_update_momentum(p2, g2, v2, DT, SCALE, mu, wd, nesterov, sh)
    torch.cuda.synchronize()
    check_site(p2, v2, g2, pr, vr)


def test_velocity_argument_is_checked(device):
    C = native.require()
    p, g, v = (t.to(device) for t in site_case(S.N_PARAMS, 6))
    sh = native.current_stream_handle()
    for bad in (v[:-1], v.cpu(), v.double(), torch.cat([v, v])[::2]):
        with pytest.raises(RuntimeError, match="vel must be"):
            C.hip_update_momentum(p, g, bad, DT, SCALE, 0.9, 0.0, False, sh)


# --------------------------------------------- 8 LeNet steps vs fp32 oracle
def make_trainer(monkeypatch, knob, step, B, **kw):
    monkeypatch.setenv("PCNN_LENET_STEP", step)
    monkeypatch.setenv("PCNN_LENET_WGRAD", knob)
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      log_interval=0, **kw)
    t = Trainer(cfg)
    assert t._use_inblock() == (knob == "inblock" and step == "2")
    assert t._fused_step_mode() == int(step)
    return t


def lenet_trajectory_vs_oracle(monkeypatch, knob, step, B, act_dtype, gtol,
                               nesterov):
    """Params after step 1 and after step 5 against the fp32 oracle.
    Bound: the per-gradient tolerance gtol * max(1, |g|max) of the plain
    step tests, on the scaled gradient the update sees, times
    dt * n_steps / (1 - mu): momentum amplifies a gradient error by at most
    the geometric sum."""
    mu, wd, n_steps = 0.9, 5e-4, 5
    x, y = synthetic_mnist(n_steps * B, seed=40 + B)
    t = make_trainer(monkeypatch, knob, step, B, act_dtype=act_dtype,
                     momentum=mu, weight_decay=wd, nesterov=nesterov)
    assert t.vel is not None and t.vel.is_cuda
    p = t.model.params.cpu().clone()
    v = torch.zeros_like(p)
    scale = 1.0 / B
    gmax = 0.0
    for s in range(n_steps):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        t.step(*t.stage_batch(xb, yb))
        a1, a2, yy = torch_ref.forward(xb, p)
        _, _, _, g, _ = torch_ref.backward(xb, p, a1, a2, yy, yb)
        gmax = max(gmax, (scale * g).abs().max().item())
        torch_ref.update_momentum(p, g, v, t.cfg.dt, scale, mu, wd, nesterov)
        if s in (0, n_steps - 1):
            torch.cuda.synchronize()
            tol = gtol * max(1.0, gmax) * t.cfg.dt * (s + 1) / (1.0 - mu)
            pdiff = (t.model.params.cpu() - p).abs().max().item()
            vdiff = (t.vel.cpu() - v).abs().max().item()
            print(f"{knob}/{step} B {B} {act_dtype} step {s + 1}: p diff "
                  f"{pdiff:.3e} v diff {vdiff:.3e} tol {tol:.3e} "
                  f"|scale*g|max {gmax:.3e}")
            assert pdiff < tol, (s + 1, pdiff, tol)
            assert vdiff < tol / t.cfg.dt, (s + 1, vdiff, tol / t.cfg.dt)
    assert v.abs().max().item() > 1e-3
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert int(t.ws.ticket.item()) == 0


@pytest.mark.parametrize("knob,step", PATHS)
@pytest.mark.parametrize("B", [3, 33, 257])
def test_lenet_momentum_fp32_matches_oracle(knob, step, B, device,
                                            monkeypatch):
    """B=3: odd, under one reduce stride; 33: crosses the 32-image stride of
    k_reduce_update; 257: the in-block launcher's hand-off to
    k_wgrad_update."""
    assert native.require().INBLOCK_MAX_BATCH == 256
    lenet_trajectory_vs_oracle(monkeypatch, knob, step, B, "fp32", 2e-4,
                               nesterov=(B == 33))


def test_lenet_momentum_bf16_close_to_oracle(device, monkeypatch):
    lenet_trajectory_vs_oracle(monkeypatch, "inblock", "2", 33, "bf16", 2e-2,
                               nesterov=False)


# ------------------------------------------------------------ 9 path agreement
@pytest.mark.parametrize("knob,step", PATHS)
def test_step_loop_and_graph_agree(knob, step, device, monkeypatch):
    """6 steps at B=33, momentum 0.9 + nesterov: Trainer.step, the C++ loop
    and graph replay.  The in-block step has one owner per parameter, so
    there the three are equal bit for bit; the grid paths sum with atomics
    and get the 1e-5 of the plain path-agreement test times 1/(1 - mu)."""
    B, n = 33, 6
    x, y = synthetic_mnist(n * B, seed=9)
    kw = dict(act_dtype="fp32", momentum=0.9, weight_decay=5e-4,
              nesterov=True)
    ts = make_trainer(monkeypatch, knob, step, B, **kw)
    tl = make_trainer(monkeypatch, knob, step, B, **kw)
    tg = make_trainer(monkeypatch, knob, step, B, **kw)
    xs, ys = ts.stage_batch(x, y)
    xs, ys = xs.contiguous(), ys.contiguous()
    for s in range(n):
        ts.step(xs[s * B:(s + 1) * B], ys[s * B:(s + 1) * B])
    tl.run_steps_pooled(xs, ys, n)                      # C++ loop
    # one eager step first, so the capture warm-up meets a non-zero velocity
    tg.step(xs[:B], ys[:B])
    torch.cuda.synchronize()
    p_pre, v_pre = tg.model.params.clone(), tg.vel.clone()
    assert v_pre.abs().max().item() > 0
    tg.enable_graph()
    assert torch.equal(tg.model.params, p_pre)
    assert torch.equal(tg.vel, v_pre)
    tg.run_steps_pooled(xs[B:], ys[B:], n - 1)          # graph replay
    torch.cuda.synchronize()
    for name, other in (("loop", tl), ("graph", tg)):
        dp = (ts.model.params - other.model.params).abs().max().item()
        dv = (ts.vel - other.vel).abs().max().item()
        print(f"{knob}/{step} step vs {name}: p {dp:.3e} v {dv:.3e}")
        if knob == "inblock":
            assert torch.equal(ts.model.params, other.model.params), dp
            assert torch.equal(ts.vel, other.vel), dv
        else:
            assert dp < 1e-5 / (1 - 0.9), dp
            assert dv < 1e-5 / (1 - 0.9) / ts.cfg.dt, dv
    assert ts.global_step == tl.global_step == tg.global_step == n


# ------------------------------------------------------------------ 10 DeepCNN
def test_deep_momentum_trajectory_pad_rows_and_graph(device):
    """3 steps, B=4, fp32 activations, against the torchref backend: the
    plain one-step bound of the DeepCNN tests (5e-3) times 1/(1 - mu)."""
    B, n, mu = 4, 3, 0.9
    kw = dict(momentum=mu, weight_decay=5e-4)
    x, y = synthetic_images(n * B, 32, 32, 3, seed=7, structured=False)
    th = deep_trainer(device, B, act_dtype="fp32", **kw)
    tg = deep_trainer(device, B, act_dtype="fp32", **kw)
    tr = DeepTrainer(TrainConfig(batch_size=B, device="cpu",
                                 backend="torchref", model="deepcnn",
                                 deep_channels=DEEP_CH, log_interval=0,
                                 **kw))
    p0 = tr.model.params.clone()
    tg.enable_graph()
    assert torch.equal(tg.model.params.cpu(), p0)
    assert torch.count_nonzero(tg.vel).item() == 0
    for s in range(n):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        th.step(*th.stage_batch(xb, yb))
        tr.step(*tr.stage_batch(xb, yb))
        tg.step_graph(*tg.stage_batch(xb, yb))
    torch.cuda.synchronize()
    diff = (th.model.params.cpu() - tr.model.params).abs().max().item()
    moved = (tr.model.params - p0).abs().max().item()
    delta = ((th.model.params.cpu() - p0) - (tr.model.params - p0)
             ).abs().max().item() / moved
    print(f"deep momentum: p diff {diff:.3e} (moved {moved:.3e}, relative "
          f"to the move {delta:.3e})")
    assert diff < 5e-3 / (1 - mu), diff
    assert moved > 1e-3
    pad = pad_row_mask(th.model.spec)
    for t in (th, tg):
        assert torch.count_nonzero(t.model.params.cpu()[pad]).item() == 0
        assert torch.count_nonzero(t.vel.cpu()[pad]).item() == 0
    assert th.vel.abs().max().item() > 0
    # graph replay == eager (the plain graph test's 1e-5, times 1/(1 - mu))
    gd = (th.model.params - tg.model.params).abs().max().item()
    gv = (th.vel - tg.vel).abs().max().item()
    print(f"deep graph vs eager: p {gd:.3e} v {gv:.3e}")
    assert gd < 1e-5 / (1 - mu), gd
    assert gv < 1e-5 / (1 - mu) / th.cfg.dt, gv


# ------------------------------------------------------------- 11 exact resume
def test_exact_resume_with_velocity_hip(tmp_path, device, monkeypatch):
    B = 33
    x, y = synthetic_mnist(4 * B, seed=12)
    kw = dict(act_dtype="fp32", momentum=0.9, weight_decay=5e-4)

    def run(t, lo, hi):
        for s in range(lo, hi):
            t.step(*t.stage_batch(x[s * B:(s + 1) * B],
                                  y[s * B:(s + 1) * B]))
        torch.cuda.synchronize()

    full = make_trainer(monkeypatch, "inblock", "2", B, **kw)
    run(full, 0, 4)
    half = make_trainer(monkeypatch, "inblock", "2", B, **kw)
    run(half, 0, 2)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(half, path)
    resumed = make_trainer(monkeypatch, "inblock", "2", B, **kw)
    load_checkpoint(resumed, path)
    assert torch.equal(resumed.vel, half.vel)
    run(resumed, 2, 4)
    assert torch.equal(resumed.model.params, full.model.params)
    assert torch.equal(resumed.vel, full.vel)
    # teeth: without the velocity file the two diverge
    os.remove(path + ".vel")
    cold = make_trainer(monkeypatch, "inblock", "2", B, **kw)
    load_checkpoint(cold, path)
    run(cold, 2, 4)
    assert not torch.equal(cold.model.params, full.model.params)


# ---------------------------------------------------------- 12 default untouched
def test_default_optimizer_holds_no_velocity(device, monkeypatch):
    B = 33
    x, y = synthetic_mnist(5 * B, seed=13)
    ta = make_trainer(monkeypatch, "inblock", "2", B, act_dtype="fp32")
    tb = make_trainer(monkeypatch, "inblock", "2", B, act_dtype="fp32",
                      momentum=0.0, weight_decay=0.0, nesterov=False)
    assert ta.vel is None and tb.vel is None
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        ta.step(*ta.stage_batch(xb, yb))
        tb.step(*tb.stage_batch(xb, yb))
    torch.cuda.synchronize()
    assert torch.equal(ta.model.params, tb.model.params)
    td = deep_trainer(device)
    assert td.vel is None
