"""CPU tests for SGD momentum / Nesterov / weight decay: the two CPU oracles
against torch.optim.SGD, the trainers on the cpu and torchref backends,
exact resume with the velocity file, 2-rank data parallelism and the config
plumbing.

Ascent convention: the bucket entry g is the direction the plain update
adds, so torch.optim.SGD(lr=dt, momentum=mu, weight_decay=wd, nesterov=...)
fed grad = -scale*g is the independent oracle.
"""
import argparse
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

from parallel_cnn_amd import _C
from parallel_cnn_amd.config import TrainConfig
from parallel_cnn_amd.data.mnist import synthetic_images, synthetic_mnist
from parallel_cnn_amd.engine.deep import DeepTrainer
from parallel_cnn_amd.engine.trainer import Trainer
from parallel_cnn_amd.models.deepcnn import DeepCNN, DeepCNNSpec
from parallel_cnn_amd.models.lenet import LeNet5
from parallel_cnn_amd.ops import deep_ref, torch_ref
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.parallel import dist as pdist
from parallel_cnn_amd.utils.checkpoint import load_checkpoint, save_checkpoint

# the 2-rank test below follows test_dist_cpu's spawn pattern at its sizes
from test_dist_cpu import GLOBAL_BATCH, STEPS

EPS = torch.finfo(torch.float32).eps
OPTS = [(0.9, 0.0, False), (0.9, 5e-4, False), (0.9, 5e-4, True),
        (0.0, 1e-3, False)]


def sgd_oracle(p0, mu, wd, nesterov, dt):
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=dt, momentum=mu, weight_decay=wd,
                          nesterov=nesterov)
    return p, opt


# ---------------------------------------------------------------- 1 oracles
@pytest.mark.parametrize("impl", ["torch_ref", "cpu"])
@pytest.mark.parametrize("mu,wd,nesterov", OPTS)
def test_update_momentum_tracks_torch_sgd(impl, mu, wd, nesterov):
    """5 steps on random p, g (both uniform in (-0.5, 0.5], the model's own
    init range) of size N_PARAMS.  Bound per step taken: 4*eps*max|p| — the
    formulas are three fused multiply-adds per element whose contraction
    may differ."""
    dt, scale = 0.1, 0.25
    g = torch.Generator().manual_seed(11)
    p = 0.5 - torch.rand(S.N_PARAMS, generator=g)
    p0 = p.clone()
    vel = torch.zeros(S.N_PARAMS)
    ref, opt = sgd_oracle(p, mu, wd, nesterov, dt)
    for k in range(1, 6):
        grads = 0.5 - torch.rand(S.N_PARAMS, generator=g)
        ref.grad = -scale * grads
        opt.step()
        gb = grads.clone()
        if impl == "cpu":
            _C.cpu_update_momentum(p, gb, vel, dt, scale, mu, wd, nesterov)
        else:
            torch_ref.update_momentum(p, gb, vel, dt, scale, mu, wd,
                                      nesterov)
        assert torch.count_nonzero(gb).item() == 0
        diff = (p - ref.data).abs().max().item()
        tol = 4 * EPS * ref.data.abs().max().item() * k
        print(f"{impl} mu {mu} wd {wd} nes {nesterov} step {k}: "
              f"diff {diff:.3e} tol {tol:.3e}")
        assert diff <= tol, (k, diff, tol)
    if mu > 0:
        buf = opt.state[ref]["momentum_buffer"]
        vdiff = (vel + buf).abs().max().item()   # buffer == -v
        assert vdiff <= 4 * EPS * buf.abs().max().item() * 5, vdiff
    assert (p - p0).abs().max().item() > 1e-3


# ------------------------------------------------ 2 momentum-off equivalence
@pytest.mark.parametrize("backend", ["cpu", "torchref"])
def test_momentum_off_is_todays_update_bitwise(backend):
    B = 4
    x, y = synthetic_mnist(3 * B, seed=2)
    t = Trainer(TrainConfig(backend=backend, device="cpu", batch_size=B,
                            log_interval=0, momentum=0.0, weight_decay=0.0))
    assert t.vel is None
    m = LeNet5(seed=0)
    for s in range(3):
        xb = x[s * B:(s + 1) * B]
        yb = y[s * B:(s + 1) * B]
        t.step(*t.stage_batch(xb, yb))
        if backend == "cpu":
            a1 = torch.empty(B, S.C1_OUT)
            a2 = torch.empty(B, S.S1_OUT)
            yy = torch.empty(B, S.FC_OUT)
            _C.cpu_forward(xb, m.params, a1, a2, yy, 0, 0)
            _C.cpu_backward(xb, m.params, a1, a2, yy, yb.to(torch.int64),
                            torch.empty(B, S.FC_OUT),
                            torch.empty(B, S.S1_OUT),
                            torch.empty(B, S.C1_OUT), m.grads, 0, 0)
            _C.cpu_update(m.params, m.grads, t.cfg.dt, 1.0 / B)
        else:
            a1, a2, yy = torch_ref.forward(xb, m.params)
            _, _, _, g, _ = torch_ref.backward(xb, m.params, a1, a2, yy, yb)
            m.grads += g
            torch_ref.update(m.params, m.grads, t.cfg.dt, 1.0 / B)
    assert torch.equal(t.model.params, m.params)


# ------------------------------------------------------------ 3 trajectories
def test_cpu_and_torchref_momentum_trajectories_match():
    B = 4
    x, y = synthetic_mnist(5 * B, seed=3)
    kw = dict(device="cpu", batch_size=B, log_interval=0, momentum=0.9,
              weight_decay=5e-4)
    t1 = Trainer(TrainConfig(backend="cpu", **kw))
    t2 = Trainer(TrainConfig(backend="torchref", **kw))
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        t1.step(*t1.stage_batch(xb, yb))
        t2.step(*t2.stage_batch(xb, yb))
    assert torch.allclose(t1.model.params, t2.model.params, atol=1e-5)
    assert torch.allclose(t1.vel, t2.vel, atol=1e-5)
    assert t1.vel.abs().max().item() > 0
    # and momentum is not a no-op: the plain trajectory differs
    t0 = Trainer(TrainConfig(backend="cpu", device="cpu", batch_size=B,
                             log_interval=0))
    for s in range(5):
        t0.step(*t0.stage_batch(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]))
    assert (t0.model.params - t1.model.params).abs().max().item() > 1e-4


def test_deep_torchref_momentum_matches_torch_sgd_loop():
    B, mu, wd = 4, 0.9, 5e-4
    cfg = TrainConfig(backend="torchref", device="cpu", model="deepcnn",
                      deep_channels="16,32", batch_size=B, log_interval=0,
                      momentum=mu, weight_decay=wd)
    t = DeepTrainer(cfg)
    x, y = synthetic_images(5 * B, 32, 32, 3, seed=4, structured=False)
    ref = DeepCNN(seed=cfg.seed, spec=DeepCNNSpec(channels=(16, 32)))
    p, opt = sgd_oracle(ref.params, mu, wd, False, cfg.dt)
    ref.params = p.data
    for s in range(5):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        t.step(*t.stage_batch(xb, yb))
        xh = xb.view(B, 32, 32, 3)
        acts, pouts, yy = deep_ref.forward(xh, ref)
        grads, _ = deep_ref.backward(xh, ref, acts, pouts, yy, yb)
        p.grad = -(1.0 / B) * grads
        opt.step()
    assert torch.allclose(t.model.params, p.data, atol=1e-5), \
        (t.model.params - p.data).abs().max()
    assert (t.model.params - DeepCNN(
        seed=cfg.seed, spec=DeepCNNSpec(channels=(16, 32))).params
            ).abs().max().item() > 1e-4


# ------------------------------------------------------------ 4 exact resume
def _run(t, x, y, lo, hi, B):
    for s in range(lo, hi):
        t.step(*t.stage_batch(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]))


def test_exact_resume_with_velocity_cpu(tmp_path):
    B = 4
    x, y = synthetic_mnist(4 * B, seed=5)
    cfg = TrainConfig(backend="cpu", device="cpu", batch_size=B,
                      log_interval=0, momentum=0.9, weight_decay=5e-4,
                      nesterov=True)
    full = Trainer(cfg)
    _run(full, x, y, 0, 4, B)
    half = Trainer(cfg)
    _run(half, x, y, 0, 2, B)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(half, path)
    assert os.path.getsize(path + ".vel") == 4 * S.N_PARAMS
    meta = json.load(open(path + ".meta.json"))
    assert meta["momentum"] == 0.9 and meta["weight_decay"] == 5e-4
    assert meta["nesterov"] is True
    resumed = Trainer(cfg)
    load_checkpoint(resumed, path)
    assert torch.equal(resumed.vel, half.vel)
    _run(resumed, x, y, 2, 4, B)
    assert torch.equal(resumed.model.params, full.model.params)
    assert torch.equal(resumed.vel, full.vel)


def test_resume_without_velocity_file_diverges(tmp_path, capsys):
    B = 4
    x, y = synthetic_mnist(4 * B, seed=5)
    cfg = TrainConfig(backend="cpu", device="cpu", batch_size=B,
                      log_interval=0, momentum=0.9, weight_decay=5e-4)
    full = Trainer(cfg)
    _run(full, x, y, 0, 4, B)
    half = Trainer(cfg)
    _run(half, x, y, 0, 2, B)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(half, path)
    os.remove(path + ".vel")
    resumed = Trainer(cfg)
    load_checkpoint(resumed, path)
    assert "zero velocity" in capsys.readouterr().out
    assert torch.count_nonzero(resumed.vel).item() == 0
    _run(resumed, x, y, 2, 4, B)
    assert not torch.equal(resumed.model.params, full.model.params)


def test_velocity_file_size_mismatch_raises(tmp_path):
    cfg = TrainConfig(backend="cpu", device="cpu", batch_size=4,
                      log_interval=0, momentum=0.9)
    t = Trainer(cfg)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(t, path)
    with open(path + ".vel", "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match="velocity"):
        load_checkpoint(Trainer(cfg), path)


def test_default_optimizer_checkpoint_is_unchanged(tmp_path):
    t = Trainer(TrainConfig(backend="cpu", device="cpu", batch_size=4,
                            log_interval=0))
    path = str(tmp_path / "ck.bin")
    save_checkpoint(t, path)
    assert sorted(os.listdir(tmp_path)) == ["ck.bin", "ck.bin.meta.json"]
    meta = json.load(open(path + ".meta.json"))
    assert sorted(meta) == sorted(
        ["global_step", "epoch", "model", "dt", "grad_reduction", "pool",
         "loss", "n_params", "rng"])


# ---------------------------------------------------------------- 5 gloo DP
MOM_KW = dict(momentum=0.9, weight_decay=5e-4, nesterov=True)


def _mom_worker(rank, world, port, result_q):
    os.environ.update({
        "RANK": str(rank),
        "LOCAL_RANK": str(rank),
        "WORLD_SIZE": str(world),
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    ctx = pdist.init_from_env(device="cpu")
    cfg = TrainConfig(backend="cpu", device="cpu",
                      batch_size=GLOBAL_BATCH // world, log_interval=0,
                      **MOM_KW)
    t = Trainer(cfg, ctx=ctx)
    x, y = synthetic_mnist(GLOBAL_BATCH * STEPS, seed=0)
    Bl = cfg.batch_size
    for s in range(STEPS):
        lo = s * GLOBAL_BATCH + rank * Bl
        t.step(*t.stage_batch(x[lo:lo + Bl], y[lo:lo + Bl]))
    result_q.put((rank, t.model.params.clone(), t.vel.clone()))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_momentum_matches_single_rank():
    cfg = TrainConfig(backend="cpu", device="cpu", batch_size=GLOBAL_BATCH,
                      log_interval=0, **MOM_KW)
    ref = Trainer(cfg)
    x, y = synthetic_mnist(GLOBAL_BATCH * STEPS, seed=0)
    _run(ref, x, y, 0, STEPS, GLOBAL_BATCH)

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_mom_worker, args=(r, 2, 29541, q))
             for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (pp, vv)) for r, pp, vv in (q.get(), q.get()))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in (0, 1):
        params, vel = got[r]
        assert torch.allclose(params, ref.model.params, atol=1e-5), \
            (params - ref.model.params).abs().max()
        assert torch.allclose(vel, ref.vel, atol=1e-5)
    # the update is deterministic and identical on every rank
    assert torch.equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])


# ------------------------------------------------------------------ 6 config
def test_optimizer_fields_yaml_and_cli_roundtrip(tmp_path):
    assert TrainConfig().momentum == 0.0
    assert TrainConfig().weight_decay == 0.0
    assert TrainConfig().nesterov is False
    p = tmp_path / "cfg.yaml"
    p.write_text("momentum: 0.9\nweight_decay: 0.0005\nnesterov: true\n")
    cfg = TrainConfig.from_yaml(str(p))
    assert (cfg.momentum, cfg.weight_decay, cfg.nesterov) == (0.9, 5e-4, True)
    ap = argparse.ArgumentParser()
    TrainConfig.add_cli_args(ap)
    args = ap.parse_args(["--momentum", "0.8", "--weight-decay", "1e-3",
                          "--nesterov", "true"])
    cfg = TrainConfig.from_args(args)
    assert (cfg.momentum, cfg.weight_decay, cfg.nesterov) == (0.8, 1e-3, True)
    args = ap.parse_args(["--config", str(p), "--nesterov", "false"])
    cfg = TrainConfig.from_args(args)
    assert (cfg.momentum, cfg.weight_decay, cfg.nesterov) == (0.9, 5e-4,
                                                              False)
    here = os.path.dirname(os.path.abspath(__file__))
    ex = TrainConfig.from_yaml(
        os.path.join(here, "..", "examples", "lenet_momentum.yaml"))
    assert (ex.pool, ex.loss, ex.momentum, ex.weight_decay) == (
        "max", "softmax_ce", 0.9, 5e-4)


@pytest.mark.parametrize("kw", [dict(momentum=1.0), dict(momentum=-0.1),
                                dict(weight_decay=-1e-4),
                                dict(nesterov=True)])
@pytest.mark.parametrize("cls,model", [(Trainer, "lenet5"),
                                       (DeepTrainer, "deepcnn")])
def test_bad_optimizer_config_raises(cls, model, kw):
    backend = "cpu" if cls is Trainer else "torchref"
    cfg = TrainConfig(backend=backend, device="cpu", model=model,
                      deep_channels="16,32", batch_size=2, log_interval=0,
                      **kw)
    with pytest.raises(ValueError):
        cls(cfg)
