"""CPU tests for the Adam / AdamW optimizer: the config plumbing, the two CPU
oracles against torch.optim.AdamW in float64, the LeNet trainer on the cpu
backend (descent, exact resume with both moment files and the update count)
and 2-rank data parallelism.

Ascent convention: the bucket entry g is the direction the plain update
adds, so torch.optim.AdamW(lr=dt, betas=(beta1, beta2), eps=eps,
weight_decay=wd) fed grad = -scale*g is the independent oracle.
"""
import argparse
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

from parallel_cnn_amd import _C
from parallel_cnn_amd.config import TrainConfig
from parallel_cnn_amd.data.mnist import synthetic_mnist
from parallel_cnn_amd.engine.deep import DeepTrainer
from parallel_cnn_amd.engine.trainer import Trainer
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref
from parallel_cnn_amd.parallel import dist as pdist
from parallel_cnn_amd.utils.checkpoint import load_checkpoint, save_checkpoint

# the 2-rank test below follows test_dist_cpu's spawn pattern at its sizes
from test_dist_cpu import GLOBAL_BATCH, STEPS

EPS32 = torch.finfo(torch.float32).eps
EPS64 = torch.finfo(torch.float64).eps
DT, SCALE, B1, B2, AEPS = 0.1, 0.25, 0.9, 0.999, 1e-8


# ------------------------------------------------------------------ 1 config
def test_adam_fields_yaml_and_cli_roundtrip(tmp_path):
    d = TrainConfig()
    assert (d.optimizer, d.beta1, d.beta2, d.adam_eps) == (
        "sgd", 0.9, 0.999, 1e-8)
    assert d.uses_adam() is False and d.uses_momentum() is False
    p = tmp_path / "cfg.yaml"
    p.write_text("optimizer: adam\nbeta1: 0.8\nbeta2: 0.99\n"
                 "adam_eps: 1.0e-6\nweight_decay: 0.01\n")
    cfg = TrainConfig.from_yaml(str(p))
    assert (cfg.optimizer, cfg.beta1, cfg.beta2, cfg.adam_eps,
            cfg.weight_decay) == ("adam", 0.8, 0.99, 1e-6, 0.01)
    assert cfg.uses_adam() is True
    # weight decay under adam is the decoupled one: no velocity semantics
    assert cfg.uses_momentum() is False
    ap = argparse.ArgumentParser()
    TrainConfig.add_cli_args(ap)
    args = ap.parse_args(["--optimizer", "adam", "--beta1", "0.85",
                          "--beta2", "0.98", "--adam-eps", "1e-7"])
    cfg = TrainConfig.from_args(args)
    assert (cfg.optimizer, cfg.beta1, cfg.beta2, cfg.adam_eps) == (
        "adam", 0.85, 0.98, 1e-7)
    args = ap.parse_args(["--config", str(p), "--optimizer", "sgd"])
    cfg = TrainConfig.from_args(args)
    assert cfg.optimizer == "sgd" and cfg.beta1 == 0.8
    assert cfg.uses_adam() is False and cfg.uses_momentum() is True
    here = os.path.dirname(os.path.abspath(__file__))
    ex = TrainConfig.from_yaml(
        os.path.join(here, "..", "examples", "lenet_adam.yaml"))
    assert ex.optimizer == "adam" and ex.uses_adam()
    assert isinstance(ex.adam_eps, float) and ex.adam_eps > 0


@pytest.mark.parametrize("kw", [
    dict(optimizer="adamw"), dict(optimizer="adam", beta1=1.0),
    dict(optimizer="adam", beta1=-0.1), dict(optimizer="adam", beta2=1.0),
    dict(optimizer="adam", beta2=-1e-3), dict(optimizer="adam", adam_eps=0.0),
    dict(optimizer="adam", adam_eps=-1e-8),
    dict(optimizer="adam", momentum=0.9),
    dict(optimizer="adam", momentum=0.9, nesterov=True),
    dict(optimizer="adam", weight_decay=-1e-4), dict(beta2=1.5)])
@pytest.mark.parametrize("cls,model", [(Trainer, "lenet5"),
                                       (DeepTrainer, "deepcnn")])
def test_bad_adam_config_raises(cls, model, kw):
    backend = "cpu" if cls is Trainer else "torchref"
    cfg = TrainConfig(backend=backend, device="cpu", model=model,
                      deep_channels="16,32", batch_size=2, log_interval=0,
                      **kw)
    with pytest.raises(ValueError):
        cls(cfg)


def test_default_config_reports_no_adam_state():
    for kw in (dict(), dict(momentum=0.9, weight_decay=5e-4)):
        t = Trainer(TrainConfig(backend="cpu", device="cpu", batch_size=2,
                                log_interval=0, **kw))
        assert t.sq is None and t.opt_step == 0
        assert (t.vel is None) == (not kw)
    t = Trainer(TrainConfig(backend="cpu", device="cpu", batch_size=2,
                            log_interval=0, optimizer="adam"))
    assert t.vel is not None and t.sq is not None
    assert t.vel.shape == t.sq.shape == t.model.params.shape
    assert torch.count_nonzero(t.vel).item() == 0
    assert torch.count_nonzero(t.sq).item() == 0


# ----------------------------------------------------------------- 2 oracles
def adamw_oracle(p0, wd):
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([p], lr=DT, betas=(B1, B2), eps=AEPS,
                            weight_decay=wd)
    return p, opt


def draw(n, gen):
    """Uniform in (-0.5, 0.5], the model's own init range."""
    return 0.5 - torch.rand(n, generator=gen)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_torch_ref_update_adam_is_adamw_in_float64(wd):
    """The formula in float64 against torch.optim.AdamW in float64, 5
    updates: 4 float64 eps of the largest magnitude per update taken (the
    two differ in how they group the bias correction)."""
    gen = torch.Generator().manual_seed(21)
    p = draw(S.N_PARAMS, gen).double()
    p0 = p.clone()
    m, sq = torch.zeros_like(p), torch.zeros_like(p)
    ref, opt = adamw_oracle(p, wd)
    for t in range(1, 6):
        g = draw(S.N_PARAMS, gen).double()
        ref.grad = -SCALE * g
        opt.step()
        gb = g.clone()
        torch_ref.update_adam(p, gb, m, sq, DT, SCALE, B1, B2, AEPS, wd, t)
        assert torch.count_nonzero(gb).item() == 0
        st = opt.state[ref]
        for name, got, want in (("p", p, ref.data),
                                ("m", m, -st["exp_avg"]),
                                ("s", sq, st["exp_avg_sq"])):
            diff = (got - want).abs().max().item()
            tol = 4 * EPS64 * want.abs().max().item() * t
            print(f"f64 wd {wd} t {t} {name}: diff {diff:.3e} tol {tol:.3e}")
            assert diff <= tol, (name, t, diff, tol)
    assert (p - p0).abs().max().item() > 4 * DT


@pytest.mark.parametrize("impl", ["torch_ref", "cpu"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fp32_update_adam_tracks_adamw_float64(impl, wd):
    """The fp32 implementations against AdamW in float64 over 5 updates from
    zero moments.  Tolerance per tensor and update: 4 x the distance between
    the plain-tensor-op fp32 oracle and the float64 one at that update
    (contraction into FMAs, the divide and the square root may each round
    differently), floor 1 fp32 eps of the tensor's largest magnitude."""
    gen = torch.Generator().manual_seed(22)
    p = draw(S.N_PARAMS, gen)
    p0 = p.clone()
    m, sq = torch.zeros_like(p), torch.zeros_like(p)
    po, mo, so = p.clone(), m.clone(), sq.clone()        # fp32 oracle
    ref, opt = adamw_oracle(p, wd)
    for t in range(1, 6):
        g = draw(S.N_PARAMS, gen)
        ref.grad = -SCALE * g.double()
        opt.step()
        torch_ref.update_adam(po, g.clone(), mo, so, DT, SCALE, B1, B2, AEPS,
                              wd, t)
        gb = g.clone()
        if impl == "cpu":
            _C.cpu_update_adam(p, gb, m, sq, DT, SCALE, B1, B2, AEPS, wd, t)
        else:
            torch_ref.update_adam(p, gb, m, sq, DT, SCALE, B1, B2, AEPS, wd,
                                  t)
        assert torch.count_nonzero(gb).item() == 0
        st = opt.state[ref]
        for name, got, orc, want in (("p", p, po, ref.data),
                                     ("m", m, mo, -st["exp_avg"]),
                                     ("s", sq, so, st["exp_avg_sq"])):
            odiff = (orc.double() - want).abs().max().item()
            diff = (got.double() - want).abs().max().item()
            tol = max(4 * odiff, EPS32 * want.abs().max().item())
            print(f"{impl} wd {wd} t {t} {name}: oracle diff {odiff:.3e} "
                  f"impl diff {diff:.3e} tol {tol:.3e}")
            assert diff <= tol, (name, t, diff, tol)
    assert (p - p0).abs().max().item() > 4 * DT


def test_cpu_update_adam_first_update_moves_by_dt():
    """m = s = 0, t = 1, wd = 0: mhat = u and shat = u*u, so every parameter
    with |u| > 1e-4 moves by dt*sign(g) to within 2*eps/|u| relative plus
    4 fp32 eps.  Without bias correction the move would be dt*0.1/sqrt(1e-3),
    3.2 times too large."""
    gen = torch.Generator().manual_seed(23)
    p, g = draw(S.N_PARAMS, gen), draw(S.N_PARAMS, gen)
    p0 = p.clone()
    m, sq = torch.zeros_like(p), torch.zeros_like(p)
    _C.cpu_update_adam(p, g.clone(), m, sq, DT, SCALE, B1, B2, AEPS, 0.0, 1)
    u = (SCALE * g).double()
    live = u.abs() > 1e-4
    assert live.sum().item() > S.N_PARAMS // 2
    move = (p.double() - p0.double())[live]
    err = (move - DT * torch.sign(u[live])).abs() / DT
    bound = 2 * AEPS / u[live].abs() + 4 * EPS32
    print(f"first update: worst err/bound {(err / bound).max().item():.3f}, "
          f"worst err {err.max().item():.3e}")
    assert (err <= bound).all()


# ----------------------------------------------------------- 3 LeNet trainer
def adam_cfg(B, **kw):
    kw.setdefault("dt", 0.01)
    return TrainConfig(backend="cpu", device="cpu", batch_size=B,
                       log_interval=0, optimizer="adam", weight_decay=1e-2,
                       **kw)


def _run(t, x, y, lo, hi, B):
    for s in range(lo, hi):
        t.step(*t.stage_batch(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]))


def test_lenet_cpu_adam_descends():
    B, n = 16, 30
    x, y = synthetic_mnist(n * B, seed=31)
    t = Trainer(adam_cfg(B))
    losses = []
    for s in range(n):
        _run(t, x, y, s, s + 1, B)
        loss, cnt = t.consume_loss()
        assert cnt == B
        losses.append(loss / cnt)
    print(f"adam loss/sample: first {losses[0]:.4f} last {losses[-1]:.4f}")
    assert losses[-1] < losses[0]
    assert t.opt_step == n
    assert t.vel.abs().max().item() > 0 and t.sq.abs().max().item() > 0


def test_opt_step_counts_updates_not_micro_batches():
    B = 4
    x, y = synthetic_mnist(6 * B, seed=32)
    t = Trainer(adam_cfg(B, grad_accum=3))
    p0 = t.model.params.clone()
    _run(t, x, y, 0, 2, B)
    assert t.opt_step == 0 and torch.equal(t.model.params, p0)
    _run(t, x, y, 2, 6, B)
    assert t.opt_step == 2 and t.global_step == 6
    assert not torch.equal(t.model.params, p0)


def test_exact_resume_with_adam_state_cpu(tmp_path, capsys):
    B = 4
    x, y = synthetic_mnist(4 * B, seed=33)
    cfg = adam_cfg(B)
    full = Trainer(cfg)
    _run(full, x, y, 0, 4, B)
    half = Trainer(cfg)
    _run(half, x, y, 0, 2, B)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(half, path)
    assert os.path.getsize(path + ".vel") == 4 * S.N_PARAMS
    assert os.path.getsize(path + ".sq") == 4 * S.N_PARAMS
    meta = json.load(open(path + ".meta.json"))
    assert (meta["optimizer"], meta["beta1"], meta["beta2"], meta["adam_eps"],
            meta["weight_decay"], meta["opt_step"]) == (
        "adam", 0.9, 0.999, 1e-8, 1e-2, 2)
    resumed = Trainer(cfg)
    load_checkpoint(resumed, path)
    assert torch.equal(resumed.vel, half.vel)
    assert torch.equal(resumed.sq, half.sq)
    assert resumed.opt_step == 2
    _run(resumed, x, y, 2, 4, B)
    assert torch.equal(resumed.model.params, full.model.params)
    assert torch.equal(resumed.vel, full.vel)
    assert torch.equal(resumed.sq, full.sq)
    assert resumed.opt_step == full.opt_step == 4
    # teeth: without the second-moment file the two diverge
    os.remove(path + ".sq")
    cold = Trainer(cfg)
    capsys.readouterr()
    load_checkpoint(cold, path)
    assert ".sq" in capsys.readouterr().out
    _run(cold, x, y, 2, 4, B)
    assert not torch.equal(cold.model.params, full.model.params)


@pytest.mark.parametrize("ext", [".vel", ".sq"])
def test_adam_state_file_size_mismatch_raises(tmp_path, ext):
    cfg = adam_cfg(4)
    t = Trainer(cfg)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(t, path)
    with open(path + ext, "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match="moment"):
        load_checkpoint(Trainer(cfg), path)


def test_default_optimizer_checkpoint_has_no_adam_keys(tmp_path):
    t = Trainer(TrainConfig(backend="cpu", device="cpu", batch_size=4,
                            log_interval=0))
    path = str(tmp_path / "ck.bin")
    save_checkpoint(t, path)
    assert sorted(os.listdir(tmp_path)) == ["ck.bin", "ck.bin.meta.json"]
    meta = json.load(open(path + ".meta.json"))
    assert not {"optimizer", "beta1", "beta2", "adam_eps", "opt_step"} & \
        set(meta)


# ---------------------------------------------------------------- 4 gloo DP
def _adam_worker(rank, world, port, result_q):
    os.environ.update({
        "RANK": str(rank),
        "LOCAL_RANK": str(rank),
        "WORLD_SIZE": str(world),
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    ctx = pdist.init_from_env(device="cpu")
    cfg = adam_cfg(GLOBAL_BATCH // world)
    t = Trainer(cfg, ctx=ctx)
    x, y = synthetic_mnist(GLOBAL_BATCH * STEPS, seed=0)
    Bl = cfg.batch_size
    for s in range(STEPS):
        lo = s * GLOBAL_BATCH + rank * Bl
        t.step(*t.stage_batch(x[lo:lo + Bl], y[lo:lo + Bl]))
    result_q.put((rank, t.model.params.clone(), t.vel.clone(), t.sq.clone(),
                  t.opt_step))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_adam_matches_single_rank():
    """Adam divides by the gradient's own scale, so the 1e-5 of the plain DP
    test does not carry over to params; the bucket differs between 1 and 2
    ranks only in summation order, a few fp32 eps of its magnitude, which
    the quotient passes on as a few eps of dt per update.  The bound on
    params is 1e-3 of dt per update: a thousand times that, and a thousand
    times below a lost or doubled update.  m (1e-5, as there) and s (1e-5
    times the largest |u|, at most 1 here) take the gradient's bound
    directly."""
    ref = Trainer(adam_cfg(GLOBAL_BATCH))
    x, y = synthetic_mnist(GLOBAL_BATCH * STEPS, seed=0)
    _run(ref, x, y, 0, STEPS, GLOBAL_BATCH)

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_adam_worker, args=(r, 2, 29551, q))
             for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, rest) for r, *rest in (q.get(), q.get()))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in (0, 1):
        params, vel, sq, opt_step = got[r]
        assert opt_step == ref.opt_step == STEPS
        pd = (params - ref.model.params).abs().max().item()
        print(f"rank {r}: p diff {pd:.3e} (dt {ref.cfg.dt})")
        assert pd < 1e-3 * ref.cfg.dt * STEPS, pd
        assert torch.allclose(vel, ref.vel, atol=1e-5)
        assert torch.allclose(sq, ref.sq, atol=1e-5)
    # the update is deterministic and identical on every rank
    for k in range(3):
        assert torch.equal(got[0][k], got[1][k])
    assert (ref.model.params - Trainer(adam_cfg(GLOBAL_BATCH)).model.params
            ).abs().max().item() > ref.cfg.dt
