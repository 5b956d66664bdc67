"""GPU tests for the Adam / AdamW optimizer in the fused update kernels.

  * every update site on known p, g, m, s against torch_ref.update_adam
    evaluated in float64 (k_update_adam, the tail of k_wgrad_update_adam, the
    owner lanes of k_reduce_update_adam, k_update_n_adam,
    k_update_cast_all_adam), and the first update against dt*sign(g);
  * LeNet 5-step trajectories against the fp32 torch_ref oracle on the
    in-block, grid and 3-launch paths, across the batch sizes at which the
    launchers change kernels;
  * Trainer.step against the C++ loop;
  * graph capture refused, exact resume, the sgd configs untouched;
  * DeepCNN: three engine updates on a known bucket, and whole steps against
    the torchref backend.

Ascent convention, t the 1-based update count:
  u = scale*g;  m = beta1*m + (1-beta1)*u;  s = beta2*s + (1-beta2)*u*u
  p += dt*((c1*m)/(c2*sqrt(s) + eps) - wd*p)
  c1 = 1/(1-beta1^t),  c2 = 1/sqrt(1-beta2^t)
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
DT, SCALE, B1, B2, AEPS = 0.1, 0.25, 0.9, 0.999, 1e-8
T = 7                      # c1 = 1.92, c2 = 11.97: far from 1
WDS = [0.0, 1e-2]
PATHS = [("inblock", "2"), ("grid", "2"), ("grid", "3")]
# deep_channels: the smallest widths the MFMA path accepts (multiples of
# 16); the parameter count, 35396, is not a multiple of the 256-thread block
DEEP_CH = "16,32"


def rand_pm(n, gen):
    """Uniform in (-0.5, 0.5], the model's own init range."""
    return 0.5 - torch.rand(n, generator=gen)


def site_case(n, seed):
    """p, g, m as the momentum site tests draw them, and s = (0.1 +
    0.4*rand)^2 so that the quotient m/sqrt(s) stays bounded."""
    gen = torch.Generator().manual_seed(seed)
    p, g, m = rand_pm(n, gen), rand_pm(n, gen), rand_pm(n, gen)
    s = (0.1 + 0.4 * torch.rand(n, generator=gen)) ** 2
    return p, g, m, s


def oracle(p, g, m, s, wd, dtype, t=T, n_updates=1, dt=DT, scale=SCALE):
    """n_updates of torch_ref.update_adam from update count t on copies of
    the inputs in `dtype`, the same bucket g each time."""
    p, m, s = p.to(dtype).clone(), m.to(dtype).clone(), s.to(dtype).clone()
    for k in range(n_updates):
        torch_ref.update_adam(p, g.to(dtype).clone(), m, s, dt, scale, B1,
                              B2, AEPS, wd, t + k)
    return p, m, s


def check_site(what, dev, inputs, wd, gd=None, **kw):
    """dev = (p, m, s) from the device against the oracle in float64.
    Tolerance per tensor: 4 x the largest difference between the fp32 oracle
    and the float64 oracle on the same inputs (device contraction into FMAs,
    and the device's divide and square root, may each round differently from
    the host's; 4 is the margin the momentum site check gives three
    multiply-adds), floor 1 fp32 eps of the tensor's largest magnitude."""
    o64 = oracle(*inputs, wd, torch.float64, **kw)
    o32 = oracle(*inputs, wd, torch.float32, **kw)
    for name, d, r32, r64 in zip("pms", dev, o32, o64):
        odiff = (r32.double() - r64).abs().max().item()
        ddiff = (d.cpu().double() - r64).abs().max().item()
        tol = max(4 * odiff, EPS * r64.abs().max().item())
        print(f"{what} wd {wd} {name}: fp32-oracle diff {odiff:.3e} device "
              f"diff {ddiff:.3e} tol {tol:.3e}")
        assert ddiff <= tol, (what, name, ddiff, tol)
    if gd is not None:
        assert torch.count_nonzero(gd).item() == 0
    return o64


# -------------------------------------------------------- kernel-level sites
@pytest.mark.parametrize("wd", WDS)
def test_hip_update_adam_site(wd, device):
    C = native.require()
    inputs = site_case(S.N_PARAMS, 1)
    p = inputs[0]
    pd, gd, md, sd = (t.to(device) for t in inputs)
    C.hip_update_adam(pd, gd, md, sd, DT, SCALE, B1, B2, AEPS, wd, T,
                      native.current_stream_handle())
    torch.cuda.synchronize()
    check_site("k_update_adam", (pd, md, sd), inputs, wd, gd)
    # N_PARAMS = 4*585 + 3: the scalar tail moved too
    assert S.N_PARAMS % 4 == 3
    assert ((pd.cpu() - p)[-3:].abs() > 1e-4).all()
    assert ((pd.cpu() - p)[:8].abs() > 0).any()


def test_first_update_moves_by_dt_sign_g(device):
    """m = s = 0, t = 1, wd = 0: mhat = u and shat = u*u, so the rule moves
    every parameter with |u| > 1e-4 by dt*sign(g), to within 2*eps/|u|
    relative (the eps in the denominator) plus 4 fp32 eps.  Without the bias
    correction the move is dt*(1-beta1)/sqrt(1-beta2), 3.2 times too
    large."""
    C = native.require()
    p, g, _, _ = site_case(S.N_PARAMS, 2)
    pd, gd = p.to(device), g.to(device)
    md, sd = torch.zeros_like(pd), torch.zeros_like(pd)
    C.hip_update_adam(pd, gd, md, sd, DT, SCALE, B1, B2, AEPS, 0.0, 1,
                      native.current_stream_handle())
    torch.cuda.synchronize()
    u = (SCALE * g).double()
    live = u.abs() > 1e-4
    assert live.sum().item() > S.N_PARAMS // 2
    move = (pd.cpu().double() - p.double())[live]
    err = (move - DT * torch.sign(u[live])).abs() / DT
    bound = 2 * AEPS / u[live].abs() + 4 * EPS
    print(f"first update: worst err/bound {(err / bound).max().item():.3f}, "
          f"worst err {err.max().item():.3e}")
    assert (err <= bound).all()
    assert torch.count_nonzero(gd).item() == 0


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wd", WDS)
def test_hip_wgrad_update_adam_tail_site(wd, act, device):
    """All-zero dz / dz1 / dz2 add nothing to the bucket, so the last
    arriver's tail applies exactly the grads that were put there."""
    C = native.require()
    B = 3
    inputs = site_case(S.N_PARAMS, 3)
    p = inputs[0]
    pd, gd, md, sd = (t.to(device) for t in inputs)
    x = torch.rand(B, S.IN_PIX, device=device).to(act)
    a1 = torch.rand(B, S.C1_OUT, device=device).to(act)
    a2 = torch.rand(B, S.S1_OUT, device=device).to(act)
    dz = torch.zeros(B, S.FC_OUT, device=device)
    dz2 = torch.zeros(B, S.S1_OUT, device=device)
    dz1 = torch.zeros(B, S.C1_OUT, device=device, dtype=act)
    ticket = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_wgrad_update_adam(x, a1, a2, dz, dz2, dz1, gd, pd, md, sd, DT,
                            SCALE, B1, B2, AEPS, wd, T, ticket, B, 0, 7,
                            native.current_stream_handle())
    torch.cuda.synchronize()
    check_site("k_wgrad_update_adam tail", (pd, md, sd), inputs, wd, gd)
    assert int(ticket.item()) == 0
    assert ((pd.cpu() - p)[-3:].abs() > 1e-4).all()


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("wd", WDS)
def test_hip_reduce_update_adam_site(wd, B, act, device):
    """Slab, dz and a2 hold small multiples of 1/16 (exact in bf16 too), so
    every batch sum is exact in fp32 whatever the order and the gradient the
    owner lane sees is known to the bit; B=33 crosses the 32-image
    stride."""
    C = native.require()
    gen = torch.Generator().manual_seed(4)
    q = lambda *shape: torch.randint(-8, 9, shape, generator=gen) / 16.0
    slab = q(B, S.GSLAB_LD)
    a2 = q(B, S.S1_OUT)
    dz = q(B, S.FC_OUT)
    assert torch.equal(a2.to(act).float(), a2)
    g = torch.empty(S.N_PARAMS)
    g[:S.OFF_FW] = slab[:, :S.OFF_FW].sum(0)
    g[S.OFF_FW:S.OFF_FB] = (dz.T @ a2).reshape(-1)
    g[S.OFF_FB:] = dz.sum(0)
    assert torch.equal(g.double(), torch.cat([
        slab[:, :S.OFF_FW].double().sum(0),
        (dz.double().T @ a2.double()).reshape(-1), dz.double().sum(0)]))
    p, _, m, s = site_case(S.N_PARAMS, 5)
    pd, md, sd = p.to(device), m.to(device), s.to(device)
    C.hip_reduce_update_adam(slab.to(device), a2.to(device).to(act),
                             dz.to(device), pd, md, sd, DT, SCALE, B1, B2,
                             AEPS, wd, T, B, native.current_stream_handle())
    torch.cuda.synchronize()
    check_site(f"k_reduce_update_adam B {B}", (pd, md, sd), (p, g, m, s), wd)
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


def deep_site_case(t, seed):
    """site_case on the DeepCNN bucket: p the model's own, and g = m = s = 0
    on the pad rows, as the engine keeps them."""
    spec = t.model.spec
    pad = pad_row_mask(spec)
    p = t.model.params.cpu().clone()
    assert torch.count_nonzero(p[pad]).item() == 0
    _, g, m, s = site_case(spec.n_params, seed)
    for b in (g, m, s):
        b[pad] = 0.0
    return (p, g, m, s), pad


@pytest.mark.parametrize("wd", WDS)
def test_deep_update_cast_adam_site(wd, device):
    C = native.require()
    t = deep_trainer(device, optimizer="adam")
    assert t.model.spec.n_params % 256 != 0
    inputs, pad = deep_site_case(t, 6)
    p = inputs[0]
    pd, gd, md, sd = (b.to(device) for b in inputs)
    d = t.ws.cast_desc
    desc = (d["R"], d["C"], d["K"], d["Cin"], d["w_off"], d["bf_off"],
            d["bfT_off"], d["rot_off"], d["p8_off"])
    wbuf = torch.zeros_like(t.ws.wbuf)
    sh = native.current_stream_handle()
    C.deep_update_cast_adam(pd, gd, md, sd, DT, SCALE, B1, B2, AEPS, wd, T,
                            wbuf, *desc, sh)
    torch.cuda.synchronize()
    check_site("k_update_cast_all_adam", (pd, md, sd), inputs, wd, gd)
    assert (pd.cpu() - p)[-1].abs().item() > 1e-4     # last, partial block
    for b in (pd, md, sd):
        assert torch.count_nonzero(b.cpu()[pad]).item() == 0
    # the bf16 images are those of the post-Adam params
    want = torch.zeros_like(wbuf)
    C.deep_cast_all(pd, want, *desc, sh)
    torch.cuda.synchronize()
    assert torch.count_nonzero(want).item() > 0
    assert torch.equal(wbuf.view(torch.int16), want.view(torch.int16))
    # the generic kernel on the same inputs
    p2, g2, m2, s2 = (b.to(device) for b in inputs)
    C.deep_update_adam(p2, g2, m2, s2, DT, SCALE, B1, B2, AEPS, wd, T, sh)
    torch.cuda.synchronize()
    check_site("k_update_n_adam", (p2, m2, s2), inputs, wd, g2)
    for b in (p2, m2, s2):
        assert torch.count_nonzero(b.cpu()[pad]).item() == 0


def test_second_moment_argument_is_checked(device):
    C = native.require()
    p, g, m, s = (t.to(device) for t in site_case(S.N_PARAMS, 7))
    sh = native.current_stream_handle()
    for bad in (s[:-1], s.cpu(), s.double(), torch.cat([s, s])[::2]):
        with pytest.raises(RuntimeError, match="sq must be"):
            C.hip_update_adam(p, g, m, bad, DT, SCALE, B1, B2, AEPS, 0.0, T,
                              sh)
    with pytest.raises(RuntimeError, match="vel must be"):
        C.hip_update_adam(p, g, m[:-1], s, DT, SCALE, B1, B2, AEPS, 0.0, T,
                          sh)
    with pytest.raises(RuntimeError, match="1-based"):
        C.hip_update_adam(p, g, m, s, DT, SCALE, B1, B2, AEPS, 0.0, 0, sh)


# ------------------------------------------------ LeNet steps vs fp32 oracle
def make_trainer(monkeypatch, knob, step, B, **kw):
    monkeypatch.setenv("PCNN_LENET_STEP", step)
    monkeypatch.setenv("PCNN_LENET_WGRAD", knob)
    cfg = TrainConfig(batch_size=B, device="cuda", backend="hip",
                      log_interval=0, **kw)
    t = Trainer(cfg)
    assert t._use_inblock() == (knob == "inblock" and step == "2")
    assert t._fused_step_mode() == int(step)
    return t


@pytest.mark.parametrize("knob,step", PATHS)
@pytest.mark.parametrize("B", [3, 33, 257])
def test_lenet_adam_fp32_matches_oracle(knob, step, B, device, monkeypatch):
    """B=3: odd, under one reduce stride; 33: crosses the 32-image stride of
    k_reduce_update; 257: the in-block launcher's hand-off to
    k_wgrad_update.

    Adam divides by the gradient's own scale, so a gradient error du moves
    the update by at most (1+R)*du/adam_eps: the shift in c1*m is at most
    du, and so is the shift in c2*sqrt(s) (a weighted 2-norm); R is the
    largest |update|/dt the oracle saw.  With the project's fp32
    per-gradient tolerance du = scale * 2e-4 * max(1, |g|max), the bound on
    p after step k is dt * k * (1+R) * du / adam_eps."""
    assert native.require().INBLOCK_MAX_BATCH == 256
    n_steps, dt, aeps, wd = 5, 0.01, 1e-2, 1e-2
    x, y = synthetic_mnist(n_steps * B, seed=50 + B)
    t = make_trainer(monkeypatch, knob, step, B, act_dtype="fp32",
                     optimizer="adam", dt=dt, adam_eps=aeps, weight_decay=wd)
    assert t.vel is not None and t.sq is not None and t.sq.is_cuda
    p = t.model.params.cpu().clone()
    p0 = p.clone()
    m, s = torch.zeros_like(p), torch.zeros_like(p)
    scale = 1.0 / B
    gmax, R = 0.0, 0.0
    for k in range(1, n_steps + 1):
        xb, yb = x[(k - 1) * B:k * B], y[(k - 1) * B:k * B]
        t.step(*t.stage_batch(xb, yb))
        a1, a2, yy = torch_ref.forward(xb, p)
        _, _, _, g, _ = torch_ref.backward(xb, p, a1, a2, yy, yb)
        gmax = max(gmax, g.abs().max().item())
        before = p.clone()
        torch_ref.update_adam(p, g, m, s, dt, scale, B1, B2, aeps, wd, k)
        R = max(R, (p - before).abs().max().item() / dt)
        if k in (1, n_steps):
            torch.cuda.synchronize()
            du = scale * 2e-4 * max(1.0, gmax)
            tol = dt * k * (1.0 + R) * du / aeps
            pdiff = (t.model.params.cpu() - p).abs().max().item()
            print(f"{knob}/{step} B {B} step {k}: p diff {pdiff:.3e} tol "
                  f"{tol:.3e} R {R:.3f} |g|max {gmax:.3e}")
            assert pdiff < tol, (k, pdiff, tol)
            assert t.opt_step == k
    assert (p - p0).abs().max().item() > dt
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert int(t.ws.ticket.item()) == 0


# ------------------------------------------------------------ path agreement
@pytest.mark.parametrize("knob,step", PATHS)
def test_step_and_loop_agree(knob, step, device, monkeypatch):
    """6 steps at B=33: Trainer.step against the C++ loop, which forms the
    bias corrections itself from t0.  The in-block step has one owner per
    parameter, so there params, m, s and opt_step are equal bit for bit, at
    the default adam_eps.  The grid paths sum with atomics and get the 1e-5
    of the plain path-agreement test times (1+R)/adam_eps as in the
    trajectory test, at adam_eps = 1e-2; R is the largest |move|/dt of the
    Trainer.step run."""
    B, n, dt = 33, 6, 0.01
    aeps = 1e-8 if knob == "inblock" else 1e-2
    x, y = synthetic_mnist(n * B, seed=9)
    kw = dict(act_dtype="fp32", optimizer="adam", dt=dt, adam_eps=aeps,
              weight_decay=1e-2)
    ts = make_trainer(monkeypatch, knob, step, B, **kw)
    tl = make_trainer(monkeypatch, knob, step, B, **kw)
    xs, ys = ts.stage_batch(x, y)
    xs, ys = xs.contiguous(), ys.contiguous()
    R = 0.0
    for k in range(n):
        before = ts.model.params.clone()
        ts.step(xs[k * B:(k + 1) * B], ys[k * B:(k + 1) * B])
        R = max(R, (ts.model.params - before).abs().max().item() / dt)
    tl.run_steps_pooled(xs[:2 * B], ys[:2 * B], 2)      # C++ loop, t0 = 0
    assert tl.opt_step == 2
    tl.run_steps_pooled(xs[2 * B:], ys[2 * B:], n - 2)  # and t0 = 2
    torch.cuda.synchronize()
    assert ts.opt_step == tl.opt_step == n
    assert ts.global_step == tl.global_step == n
    tol = 1e-5 * (1.0 + R) / aeps
    for name, a, b in (("p", ts.model.params, tl.model.params),
                       ("m", ts.vel, tl.vel), ("s", ts.sq, tl.sq)):
        d = (a - b).abs().max().item()
        print(f"{knob}/{step} step vs loop {name}: {d:.3e} (R {R:.3f})")
        if knob == "inblock":
            assert torch.equal(a, b), (name, d)
        else:
            assert d < tol, (name, d, tol)
    assert R > 0


# -------------------------------------------------------- engine and DeepCNN
def test_enable_graph_raises_under_adam(device, monkeypatch):
    t = make_trainer(monkeypatch, "inblock", "2", 8, optimizer="adam")
    with pytest.raises(RuntimeError, match="adam"):
        t.enable_graph()
    td = deep_trainer(device, optimizer="adam")
    with pytest.raises(RuntimeError, match="adam"):
        td.enable_graph()


def test_exact_resume_with_adam_state_hip(tmp_path, device, monkeypatch):
    B = 33
    x, y = synthetic_mnist(4 * B, seed=12)
    kw = dict(act_dtype="fp32", optimizer="adam", dt=0.01, weight_decay=1e-2)

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
    assert torch.equal(resumed.sq, half.sq)
    assert resumed.opt_step == 2
    run(resumed, 2, 4)
    assert torch.equal(resumed.model.params, full.model.params)
    assert torch.equal(resumed.vel, full.vel)
    assert torch.equal(resumed.sq, full.sq)
    assert resumed.opt_step == full.opt_step == 4
    # teeth: without the second-moment file the two diverge
    os.remove(path + ".sq")
    cold = make_trainer(monkeypatch, "inblock", "2", B, **kw)
    load_checkpoint(cold, path)
    run(cold, 2, 4)
    assert not torch.equal(cold.model.params, full.model.params)


@pytest.mark.parametrize("kw", [dict(), dict(momentum=0.9,
                                             weight_decay=5e-4)])
def test_sgd_configs_hold_no_second_moment(kw, device, monkeypatch):
    """The default and the momentum optimizer with the Adam fields spelled
    out at their defaults are the runs they were."""
    B = 33
    x, y = synthetic_mnist(5 * B, seed=13)
    ta = make_trainer(monkeypatch, "inblock", "2", B, act_dtype="fp32", **kw)
    tb = make_trainer(monkeypatch, "inblock", "2", B, act_dtype="fp32",
                      optimizer="sgd", beta1=0.9, beta2=0.999, adam_eps=1e-8,
                      **kw)
    assert ta.sq is None and tb.sq is None
    assert (ta.vel is None) == (not kw)
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        ta.step(*ta.stage_batch(xb, yb))
        tb.step(*tb.stage_batch(xb, yb))
    torch.cuda.synchronize()
    assert torch.equal(ta.model.params, tb.model.params)
    if kw:
        assert torch.equal(ta.vel, tb.vel)
    td = deep_trainer(device, **kw)
    assert td.sq is None and (td.vel is None) == (not kw)


@pytest.mark.parametrize("wd", WDS)
def test_deep_trainer_three_updates_on_known_bucket(wd, device):
    """The engine's own update call, three times on the same known bucket
    from zero moments: opt_step, the bias corrections for t = 1, 2, 3 and
    the fused cast, at the site tolerance."""
    t = deep_trainer(device, optimizer="adam", dt=DT, weight_decay=wd)
    (p, g, _, _), pad = deep_site_case(t, 8)
    z = torch.zeros_like(p)
    gd = g.to(device)
    for k in range(3):
        with torch.no_grad():
            t.model.grads.copy_(gd)
        t._hip_update(SCALE)
        assert t.opt_step == k + 1
    torch.cuda.synchronize()
    check_site("DeepTrainer x3", (t.model.params, t.vel, t.sq),
               (p, g, z, z), wd, t.model.grads, t=1, n_updates=3)
    for b in (t.model.params, t.vel, t.sq):
        assert torch.count_nonzero(b.cpu()[pad]).item() == 0
    assert (t.model.params.cpu() - p).abs().max().item() > 2 * DT
    # the weight images the next forward reads are those of the new params
    d = t.ws.cast_desc
    want = torch.zeros_like(t.ws.wbuf)
    native.require().deep_cast_all(
        t.model.params, want, d["R"], d["C"], d["K"], d["Cin"], d["w_off"],
        d["bf_off"], d["bfT_off"], d["rot_off"], d["p8_off"],
        native.current_stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(t.ws.wbuf.view(torch.int16), want.view(torch.int16))


def test_deep_adam_steps_against_torchref(device):
    """3 whole steps, B=4, fp32 activations, against the torchref backend.
    Adam moves every live parameter by about dt per step, so a lost or
    sign-flipped update costs at least a full move: the largest parameter
    difference must stay below half the largest move.

    adam_eps = 1e-2, for the reason the LeNet trajectories give.  The MFMA
    path rounds its GEMM operands to bf16 by design; rounding the conv
    weights alone shifts the oracle's scaled gradient on this very batch by
    up to 5.4e-5 and flips the sign of one (while whole layers have
    |u| < 2e-4), and at the default 1e-8 a parameter whose gradient changes
    sign rightly moves the other way by a full dt.  At 1e-2 the shift moves
    an update by at most (1+R)*du/adam_eps, about 0.01 of dt; the default
    adam_eps runs through the engine in the known-bucket test above."""
    B, n = 4, 3
    kw = dict(optimizer="adam", dt=0.01, weight_decay=1e-2, adam_eps=1e-2)
    x, y = synthetic_images(n * B, 32, 32, 3, seed=7, structured=False)
    th = deep_trainer(device, B, act_dtype="fp32", **kw)
    tr = DeepTrainer(TrainConfig(batch_size=B, device="cpu",
                                 backend="torchref", model="deepcnn",
                                 deep_channels=DEEP_CH, log_interval=0,
                                 **kw))
    p0 = tr.model.params.clone()
    assert torch.equal(th.model.params.cpu(), p0)
    for s in range(n):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        th.step(*th.stage_batch(xb, yb))
        tr.step(*tr.stage_batch(xb, yb))
    torch.cuda.synchronize()
    assert th.opt_step == tr.opt_step == n
    diff = (th.model.params.cpu() - tr.model.params).abs().max().item()
    moved = (tr.model.params - p0).abs().max().item()
    print(f"deep adam: p diff {diff:.3e}, largest move {moved:.3e}")
    assert moved > 0.01
    assert diff < 0.5 * moved, (diff, moved)
    pad = pad_row_mask(th.model.spec)
    for b in (th.model.params, th.vel, th.sq):
        assert torch.count_nonzero(b.cpu()[pad]).item() == 0
    assert th.sq.abs().max().item() > 0
