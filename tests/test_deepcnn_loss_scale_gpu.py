"""DeepCNN fp16 loss scaling on the GPU: k_fc_fwd with a scaler state,
k_ls_check, k_ls_advance against the Python reference, the skip semantics of
every update kernel, and the whole step (gradients per block with nothing
excluded, overflow recovery, graph replay, resume, and the off path)."""
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import deep_emul  # noqa: E402
from parallel_cnn_amd import _C  # noqa: E402
from parallel_cnn_amd.config import TrainConfig  # noqa: E402
from parallel_cnn_amd.data.mnist import synthetic_images  # noqa: E402
from parallel_cnn_amd.engine.deep import DeepTrainer  # noqa: E402
from parallel_cnn_amd.models.deepcnn import DeepCNN  # noqa: E402
from parallel_cnn_amd.ops import loss_scale_ref as ref  # noqa: E402
from parallel_cnn_amd.utils.checkpoint import (load_checkpoint,  # noqa: E402
                                               save_checkpoint)
from test_deepcnn_kernels_gpu import (DT, U32, check, check_bits,  # noqa: E402
                                      f64, fc_data, gen, sh, store_bound)
from test_loss_scale_cpu import SCRIPT  # noqa: E402

pytestmark = pytest.mark.gpu

S = 8192.0


def new_state(device, scale, good=0, skipped=0, t=1, b1=0.0, b2=0.0):
    st = torch.zeros(_C.LS_WORDS, dtype=torch.float32, device=device)
    c1, c2 = ref.adam_corrections(b1, b2, t)
    _C.deep_ls_init(st, scale, good, skipped, t, c1, c2)
    return st


def words(st):
    """The state's eight 32-bit words as Python ints."""
    return [int(v) for v in st.detach().cpu().view(torch.int32).tolist()]


def ref_words(s):
    f = lambda v: struct.unpack("i", struct.pack("f", v))[0]  # noqa: E731
    return [f(s["scale"]), f(s["inv_scale"]), s["found_inf"],
            s["good_steps"], s["skipped"], s["t"], f(s["c1"]), f(s["c2"])]


def set_found(st, v):
    st.view(torch.int32)[2] = v


def deep_cfg(B, **kw):
    kw.setdefault("act_dtype", "fp16")
    return TrainConfig(model="deepcnn", batch_size=B, device="cuda",
                       backend="hip", log_interval=0, **kw)


# ----------------------------------------------------------------- k_fc_fwd
@pytest.mark.parametrize("act", ["fp32", "fp16"])
@pytest.mark.parametrize("FCIN", [128, 48])
def test_fc_fwd_scaled(act, FCIN, device):
    """FCIN = 128 takes the 8-wide vector branch, 48 the scalar one.  dz is
    multiplied by a power of two: bit-equal to S x the unscaled launch; y
    and the loss never see the scale."""
    B = 3
    flat, fw, fb, labels, x, y, by, dz = fc_data(gen(B + FCIN), act, B, FCIN)
    fd, fwd, fbd = flat.to(device), fw.to(device), fb.to(device)
    lab = labels.to(device)
    st = new_state(device, S)
    out = {}
    for tag, ls in (("u", None), ("s", st)):
        yd = torch.zeros(B, 10, device=device)
        dzd = torch.zeros(B, 10, device=device)
        loss = torch.full((1,), 2.5, device=device)
        corr = torch.full((1,), 7, dtype=torch.int32, device=device)
        dflat = torch.zeros(B, FCIN, dtype=DT[act], device=device)
        _C.deep_fc_fwd(fd, fwd, fbd, lab, yd, dzd, loss, corr, B, FCIN, 10,
                       0, sh(), dflat=dflat, ls_state=ls)
        torch.cuda.synchronize()
        assert int(corr.item()) == 7
        out[tag] = (yd, dzd, loss, dflat)
    tag = f"[{act},FCIN{FCIN}]"
    check_bits("ls_fc_y" + tag, out["s"][0], out["u"][0])
    check_bits("ls_fc_dz" + tag, out["s"][1], out["u"][1] * S)
    # loss: each launch adds the same B addends to 2.5 in an order the
    # atomics choose; the accumulation term of test_fc_fwd_train, twice
    bdz = by + U32 * dz.abs()
    wl = dz.norm(dim=1).sum()
    acc_l = (B + 12) * U32 * (2.5 + wl)
    check("ls_fc_loss_vs_unscaled" + tag, out["s"][2], f64(out["u"][2]),
          (2 * acc_l).reshape(1))
    check("ls_fc_loss" + tag, f64(out["s"][2]) - 2.5, wl.reshape(1),
          (bdz.norm(dim=1).sum() + acc_l).reshape(1))
    # dflat from the scaled dz, the bound of test_fc_fwd_train at S x dz
    f = x * (1 - x)
    fw64 = f64(fw)
    dzs, bdzs = S * dz, S * bdz
    want = (dzs @ fw64) * f
    acc = 18 * U32 * (dzs.abs() @ fw64.abs()) * f
    bfl = (bdzs @ fw64.abs()) * f + acc + 4 * U32 * want.abs() + \
        store_bound(want, act)
    check("ls_fc_dflat" + tag, out["s"][3], want, bfl)
    # the state is read, never written
    assert words(st) == ref_words(ref.scaler_state(S))


# --------------------------------------------------------------- k_ls_check
NONFINITE = [float("inf"), float("-inf"), float("nan")]


def check_flag(bucket, device, before):
    st = new_state(device, 1024.0)
    set_found(st, before)
    w0 = words(st)
    _C.deep_ls_check(bucket.to(device), st, sh())
    torch.cuda.synchronize()
    w1 = words(st)
    assert w1[:2] + w1[3:] == w0[:2] + w0[3:], "only found_inf may change"
    return w1[2]


@pytest.mark.parametrize("n", [1, 5, 4099])
def test_ls_check(n, device):
    g = gen(n)
    base = (torch.rand(n, generator=g) - 0.5) * 2e3
    n4 = n // 4
    spots = {0}                              # the first element
    if n4:
        spots.add(4 * (n4 - 1) + 2)          # inside the last float4
    if n % 4:
        spots.add(n - 1)                     # the last tail element
        spots.add(4 * n4)                    # and the first
    for pos in sorted(spots):
        for v in NONFINITE:
            b = base.clone()
            b[pos] = v
            assert check_flag(b, device, 0) == 1, (n, pos, v)
    # finite, however large or small: the flag keeps whatever it held
    b = base.clone()
    b[0] = 3e38
    b[n - 1] = -3e38 if n > 1 else 3e38
    assert check_flag(b, device, 0) == 0
    assert check_flag(b, device, 1) == 1
    sub = torch.full((n,), 1e-45)
    sub[n // 2] = -1e-40
    assert sub.abs().max() < 1.2e-38 and sub.abs().min() > 0
    assert check_flag(sub, device, 0) == 0
    assert check_flag(base, device, 0) == 0
    assert check_flag(base, device, 1) == 1


# ------------------------------------------------------------- k_ls_advance
def run_advance(device, state, script, interval, dynamic, b1, b2):
    st = new_state(device, state["scale"], state["good_steps"],
                   state["skipped"], state["t"], b1, b2)
    assert words(st) == ref_words(state)
    for i, f in enumerate(script):
        set_found(st, int(f))
        _C.deep_ls_advance(st, interval, dynamic, b1, b2, sh())
        torch.cuda.synchronize()
        state = ref.advance_reference(state, bool(f), interval, dynamic, b1,
                                      b2)
        assert words(st) == ref_words(state), (i, f, words(st), state)
    return state


def test_ls_advance_matches_reference(device):
    """Every state word after every step of the scripted sequence, bit for
    bit: growth at the interval, backoff, the counter reset, t at rest on a
    skip, c1 and c2 from the double formula."""
    b1, b2 = 0.9, 0.999
    end = run_advance(device, ref.scaler_state(1024.0, b1, b2), SCRIPT, 3,
                      True, b1, b2)
    assert end["scale"] == 512.0 and end["skipped"] == 3 and end["t"] == 11
    # both clamps
    end = run_advance(device, ref.scaler_state(2.0, b1, b2), [1, 1, 1], 3,
                      True, b1, b2)
    assert end["scale"] == 1.0 and end["t"] == 1
    end = run_advance(device, ref.scaler_state(2.0 ** 23, b1, b2), [0, 0], 1,
                      True, b1, b2)
    assert end["scale"] == 2.0 ** 24
    # a fixed scale: counted skips, nothing else moves
    end = run_advance(device, ref.scaler_state(S), [0, 1, 0], 2, False, 0.0,
                      0.0)
    assert end["scale"] == S and end["skipped"] == 1 and end["c1"] == 1.0


# ----------------------------------------------------------- skip semantics
OPTS = {"plain": dict(), "momentum": dict(momentum=0.9, weight_decay=5e-4),
        "adam": dict(optimizer="adam", weight_decay=1e-2)}


def call_update(t, cast, ls):
    """The trainer's update launch alone: fused with the cast (the engine's
    own call) or the plain deep_update* binding."""
    c, p, g = t.cfg, t.model.params, t.model.grads
    scale = 0.5
    if cast:
        saved, t.ls_state = t.ls_state, ls
        try:
            t._hip_update(scale)
        finally:
            t.ls_state = saved
    elif t.sq is not None:
        _C.deep_update_adam(p, g, t.vel, t.sq, c.dt, scale, c.beta1, c.beta2,
                            c.adam_eps, c.weight_decay, 1, sh(), ls)
    elif t.vel is not None:
        _C.deep_update_momentum(p, g, t.vel, c.dt, scale, c.momentum,
                                c.weight_decay, c.nesterov, sh(), ls)
    else:
        _C.deep_update(p, g, c.dt * scale, sh(), ls)


@pytest.mark.parametrize("cast", [True, False])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_skip_and_apply(opt, cast, device):
    """An inf in the bucket: params, vel, sq and the bf16 images keep their
    bits, the bucket is zeroed, the scale halves, the skip is counted and t
    stays.  Then a finite bucket of S x g moves everything as the unscaled
    kernel moves it on g.  The scale is a power of two and t = 1, so the two
    are the same arithmetic up to where the compiler fuses multiply-adds,
    which differs between two kernels: each of the at most 6 roundings of an
    update is worth 2^-24 of its operands, on either side."""
    t = DeepTrainer(deep_cfg(2, deep_channels="16,16", loss_scale="dynamic",
                             loss_scale_init=2 * S, **OPTS[opt]))
    n = t.model.spec.n_params
    g = gen(11 + cast)
    t._hip_cast_weights(force=True)
    with torch.no_grad():
        for buf in (t.vel, t.sq):
            if buf is not None:
                buf.copy_((0.1 + torch.rand(n, generator=g)).to(device))
    grad = (torch.rand(n, generator=g) - 0.5)
    state0 = dict(t.loss_scale_state())
    assert state0 == dict(scale=2 * S, good_steps=0, skipped=0, t=1)

    def snap():
        return [b.clone() for b in (t.model.params, t.vel, t.sq, t.ws.wbuf)
                if b is not None]

    before = snap()
    bad = grad.clone() * (2 * S)
    bad[n // 3] = float("inf")
    with torch.no_grad():
        t.model.grads.copy_(bad.to(device))
    b1, b2 = t._ls_betas()
    _C.deep_ls_check(t.model.grads, t.ls_state, sh())
    call_update(t, cast, t.ls_state)
    _C.deep_ls_advance(t.ls_state, 2000, True, b1, b2, sh())
    torch.cuda.synchronize()
    for a, b in zip(before, snap()):
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2
                                  else torch.int32),
                           b.view(torch.int16 if b.element_size() == 2
                                  else torch.int32))
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert t.loss_scale_state() == dict(scale=S, good_steps=0, skipped=1,
                                        t=1)
    assert t.opt_step == 0
    # applied: S x g with the state == g without one
    with torch.no_grad():
        t.model.grads.copy_((grad * S).to(device))
    _C.deep_ls_check(t.model.grads, t.ls_state, sh())
    call_update(t, cast, t.ls_state)
    _C.deep_ls_advance(t.ls_state, 2000, True, b1, b2, sh())
    torch.cuda.synchronize()
    after = snap()
    u = DeepTrainer(deep_cfg(2, deep_channels="16,16", **OPTS[opt]))
    u._hip_cast_weights(force=True)
    with torch.no_grad():
        for dst, src in zip([b for b in (u.model.params, u.vel, u.sq)
                             if b is not None], before):
            dst.copy_(src)
        u.model.grads.copy_(grad.to(device))
    u._opt_step = 0
    call_update(u, cast, None)
    torch.cuda.synchronize()
    want = [b for b in (u.model.params, u.vel, u.sq) if b is not None]
    p0, c = f64(before[0]), t.cfg
    for k, (a, b, b0) in enumerate(zip(after, want, before)):
        a, b, b0 = f64(a), f64(b), f64(b0)
        if k == 0:      # params: the move, the decay term, the final store
            bound = U32 * (12 * ((b - b0).abs() + 2 * c.dt * c.weight_decay
                                 * p0.abs()) + 2 * b.abs())
        else:           # m / v / s: a sum of terms no larger than these
            bound = U32 * 12 * (b.abs() + b0.abs() + p0.abs())
        check(f"ls_apply[{opt},cast={cast}] buffer {k}", a, b,
              bound + 1e-45)
    if cast:
        # the bf16 images are the cast of the parameters just written
        img = t.ws.wbuf.clone()
        t._hip_cast_weights(force=True)
        torch.cuda.synchronize()
        assert torch.equal(img.view(torch.int16),
                           t.ws.wbuf.view(torch.int16))
    assert not torch.equal(after[0], before[0])
    assert torch.count_nonzero(t.model.grads).item() == 0
    assert t.loss_scale_state() == dict(scale=S, good_steps=1, skipped=1,
                                        t=2)
    assert t.opt_step == 1


# ------------------------------------------------------- whole-step, fp16
def scaled_grads(cfg, x, labels):
    t = DeepTrainer(cfg)
    B = x.shape[0]
    xb, lb = t.stage_batch(x, labels)
    t._hip_forward(xb, lb, B, 0)
    t._hip_backward(xb, B)
    torch.cuda.synchronize()
    return t, t.model.grads.cpu().clone()


@pytest.mark.parametrize("channels,implicit,seed", [
    ("32,64,64", True, 7), ("32,64,64", False, 7), ("16,32,32,64", True, 29)])
def test_hip_grads_per_block_fp16_scaled(channels, implicit, seed, device):
    """fp16 storage with loss_scale 8192: every block of the bucket / 8192
    within 4 x the emulated ratio at the same scale, conv0 included -- the
    blocks test_hip_grads_per_block_fp16 has to exclude, and the four-stage
    widths it cannot run at all.  Measured ratios: PARITY.md."""
    B = 8
    cfg = deep_cfg(B, deep_channels=channels, deep_implicit=implicit,
                   loss_scale="8192")
    x, labels = synthetic_images(B, 32, 32, 3, seed=seed, structured=False)
    t, g_hip = scaled_grads(cfg, x, labels)
    assert torch.isfinite(g_hip).all()
    spec = t.model.spec
    g, _, emul = deep_emul.oracle_pair(x.view(B, 32, 32, 3), labels,
                                       t.model.params, spec, "fp16",
                                       loss_scale=S)
    what = f"grads[fp16,ls8192,{channels},implicit={implicit}]"
    fails, excluded = deep_emul.compare_blocks(what, g_hip.double() / S, g,
                                               emul, "fp16", spec)
    assert excluded == set()
    assert not fails, (what, fails)


def test_hip_step_fp16_scaled(device):
    """One fp16 step with loss_scale 8192 under the per-block parameter-move
    rule of assert_step_blocks (tests/test_deepcnn_gpu.py), the emulation at
    the same scale; nothing is excluded."""
    B = 8
    t = DeepTrainer(deep_cfg(B, loss_scale="8192"))
    x, labels = synthetic_images(B, 32, 32, 3, seed=13, structured=False)
    t.step(*t.stage_batch(x, labels))
    torch.cuda.synchronize()
    spec = t.model.spec
    p0 = DeepCNN(seed=t.cfg.seed, spec=spec).params
    g, loss, emul = deep_emul.oracle_pair(x.view(B, 32, 32, 3), labels, p0,
                                          spec, "fp16", loss_scale=S)
    dp_ref = t.cfg.dt * (1.0 / B) * g
    p1 = t.model.params.cpu()
    fails, excluded = deep_emul.compare_blocks(
        "step[fp16,ls8192]", p1.double() - p0.double(), dp_ref, emul, "fp16",
        spec, floor=deep_emul.step_delta_floor(p1, dp_ref, spec))
    assert excluded == set()
    assert not fails, fails
    assert t.loss_scale_state() == dict(scale=S, good_steps=0, skipped=0,
                                        t=2)
    lg, n = t.consume_loss()
    assert n == B and abs(lg - loss) < 1e-2 * max(1.0, loss)  # unscaled


def test_overflow_recovery(device):
    """Dynamic scaling from 2^24: the first step overflows fp16 and is
    skipped bit for bit; the scale backs off until an update applies.  The
    emulation overflows at 2^22 and above and is finite at 2^20, so about 4
    skips are expected; 6 are allowed."""
    B = 8
    t = DeepTrainer(deep_cfg(B, loss_scale="dynamic",
                             loss_scale_init=2.0 ** 24))
    x, labels = synthetic_images(B, 32, 32, 3, seed=7, structured=False)
    xb, lb = t.stage_batch(x, labels)
    p0 = t.model.params.clone()
    t.step(xb, lb)
    torch.cuda.synchronize()
    assert torch.equal(t.model.params.view(torch.int32), p0.view(torch.int32))
    assert torch.count_nonzero(t.model.grads).item() == 0
    st = t.loss_scale_state()
    assert st == dict(scale=2.0 ** 23, good_steps=0, skipped=1, t=1)
    for _ in range(7):
        t.step(xb, lb)
    torch.cuda.synchronize()
    st = t.loss_scale_state()
    print("overflow recovery:", st)
    assert st["skipped"] <= 6
    assert st["t"] - 1 == 8 - st["skipped"] >= 1 and t.opt_step == st["t"] - 1
    assert st["scale"] == 2.0 ** (24 - st["skipped"])
    assert torch.isfinite(t.model.params).all()
    assert not torch.equal(t.model.params, p0)


def test_deep_graph_matches_eager_scaled(device):
    """test_deep_graph_matches_eager with fp16 storage and loss_scale 8192
    (sgd): the scaler is device state, so the captured step carries it."""
    B = 16
    cfg = deep_cfg(B, loss_scale="8192")
    x, labels = synthetic_images(B * 3, 32, 32, 3, seed=21, structured=False)
    te = DeepTrainer(cfg)
    tg = DeepTrainer(cfg)
    tg.enable_graph()
    assert torch.allclose(te.model.params, tg.model.params)
    assert tg.loss_scale_state() == te.loss_scale_state()
    for s in range(3):
        xb, lb = te.stage_batch(x[s * B:(s + 1) * B],
                                labels[s * B:(s + 1) * B])
        te.step(xb, lb)
        xg, lg = tg.stage_batch(x[s * B:(s + 1) * B],
                                labels[s * B:(s + 1) * B])
        tg.step_graph(xg, lg)
    torch.cuda.synchronize()
    diff = (te.model.params - tg.model.params).abs().max().item()
    assert diff < 1e-5, diff
    le, ne = te.consume_loss()
    lg_, ng = tg.consume_loss()
    assert ne == ng == 3 * B
    assert abs(le - lg_) < 1e-3 * max(1.0, abs(le))
    assert tg.loss_scale_state() == te.loss_scale_state() == \
        dict(scale=S, good_steps=0, skipped=0, t=4)
    assert tg.opt_step == te.opt_step == 3


def test_graph_still_refused_under_adam(device):
    t = DeepTrainer(deep_cfg(4, deep_channels="16,16", optimizer="adam",
                             loss_scale="dynamic"))
    with pytest.raises(RuntimeError, match="adam"):
        t.enable_graph()


def test_resume_adam_dynamic(tmp_path, device):
    """Adam + dynamic scaler: 3 steps, save, load, 2 more, against 5 straight
    steps.  What the checkpoint carries is compared bit for bit, as in
    test_exact_resume_with_adam_state_hip: params, m, s, the scaler state
    and t after the load, and the scaler state and t at the end.  The
    DeepCNN weight gradients are summed with float atomics, so two runs of
    the same steps differ in the last bits and Adam's quotient magnifies
    that: the continued parameters get the bound tests/test_adam_gpu.py
    gives its atomically summed paths, 1e-5 * (1 + R) / adam_eps at
    adam_eps = 1e-2, R the largest |move| / dt."""
    B, dt, aeps = 4, 0.01, 1e-2
    x, labels = synthetic_images(5 * B, 32, 32, 3, seed=31, structured=False)
    cfg = deep_cfg(B, deep_channels="16,32", optimizer="adam", dt=dt,
                   adam_eps=aeps, weight_decay=1e-2, loss_scale="dynamic",
                   loss_scale_growth_interval=2)
    R = [0.0]

    def run(t, lo, hi):
        for s in range(lo, hi):
            before = t.model.params.clone()
            t.step(*t.stage_batch(x[s * B:(s + 1) * B],
                                  labels[s * B:(s + 1) * B]))
            R[0] = max(R[0], (t.model.params - before).abs().max().item()
                       / dt)
        torch.cuda.synchronize()

    full = DeepTrainer(cfg)
    run(full, 0, 5)
    half = DeepTrainer(cfg)
    run(half, 0, 3)
    path = str(tmp_path / "ck.bin")
    save_checkpoint(half, path)
    resumed = DeepTrainer(cfg)
    load_checkpoint(resumed, path)
    assert torch.equal(resumed.model.params, half.model.params)
    assert torch.equal(resumed.vel, half.vel)
    assert torch.equal(resumed.sq, half.sq)
    assert words(resumed.ls_state) == words(half.ls_state)
    assert resumed.loss_scale_state() == dict(
        scale=2 * 65536.0, good_steps=1, skipped=0, t=4)
    assert resumed.opt_step == 3
    run(resumed, 3, 5)
    assert words(resumed.ls_state) == words(full.ls_state)
    assert resumed.loss_scale_state() == dict(
        scale=4 * 65536.0, good_steps=1, skipped=0, t=6)
    assert resumed.opt_step == full.opt_step == 5
    tol = 1e-5 * (1.0 + R[0]) / aeps
    for name, a, b in (("p", resumed.model.params, full.model.params),
                       ("m", resumed.vel, full.vel),
                       ("s", resumed.sq, full.sq)):
        d = (a - b).abs().max().item()
        print(f"resume {name}: {d:.3e} (tol {tol:.3e}, R {R[0]:.3f})")
        assert d < tol, (name, d, tol)
    assert R[0] > 0
    # teeth: a sidecar without the scaler restarts it at the initial scale
    cold = DeepTrainer(cfg)
    import json
    meta = json.load(open(path + ".meta.json"))
    del meta["loss_scale"]
    json.dump(meta, open(path + ".meta.json", "w"))
    load_checkpoint(cold, path)
    assert cold.loss_scale_state() == dict(scale=65536.0, good_steps=0,
                                           skipped=0, t=4)


# ------------------------------------------------------------------ off path
class Recorder:
    """Stands in for the extension module and notes every launcher call."""

    def __init__(self, mod):
        self._mod, self.calls = mod, []

    def __getattr__(self, name):
        attr = getattr(self._mod, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.calls.append(name)
            return attr(*a, **k)
        return call


def recorded_step(cfg, device):
    t = DeepTrainer(cfg)
    x, labels = synthetic_images(cfg.batch_size, 32, 32, 3, seed=5,
                                 structured=False)
    xb, lb = t.stage_batch(x, labels)
    t._C = Recorder(t._C)
    t.step(xb, lb)
    torch.cuda.synchronize()
    return t, t._C.calls


def test_loss_scale_off_adds_nothing(device):
    off, calls_off = recorded_step(deep_cfg(4, loss_scale="off"), device)
    assert off.ls_state is None and off.loss_scale_state() is None
    assert off.update_launches == ["deep_update_cast"]
    assert not [c for c in calls_off if c.startswith("deep_ls_")]
    assert calls_off[-1] == "deep_update_cast"
    on, calls_on = recorded_step(deep_cfg(4, loss_scale="8192"), device)
    assert on.update_launches == ["deep_ls_check", "deep_update_cast",
                                  "deep_ls_advance"]
    assert calls_on[-3:] == on.update_launches
    assert calls_on[:-3] == calls_off[:-1]      # two launches more, no other


def test_grad_accum_checks_once_per_update(device):
    cfg = deep_cfg(4, deep_channels="16,16", loss_scale="8192", grad_accum=2)
    t = DeepTrainer(cfg)
    x, labels = synthetic_images(4, 32, 32, 3, seed=5, structured=False)
    xb, lb = t.stage_batch(x, labels)
    t._C = Recorder(t._C)
    t.step(xb, lb)
    assert not [c for c in t._C.calls if c.startswith("deep_ls_")]
    t.step(xb, lb)
    torch.cuda.synchronize()
    assert t._C.calls.count("deep_ls_check") == 1
    assert t._C.calls.count("deep_ls_advance") == 1
    assert t.loss_scale_state()["t"] == 2
