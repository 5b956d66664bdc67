"""Every LeNet launcher alone against the float64 oracle (tools/lenet_emul.py),
at the smallest shapes, with bounds derived from the code.

The flat tolerance of the older LeNet tests, 2e-4 max(1, |g|max) (2e-2 in
bf16/fp16), is set by the pool-weight and fc blocks, whose entries are 1.7 to
77; the conv1 blocks are three to five orders of magnitude smaller and were
invisible to it.  Here every block is held to its own bound.

fp32, elementwise:  |got - want64| <= C 2^-24 M + 2^-24 |want64|, M from
lenet_emul.magnitude64 (the backward over absolute values).  C is the number
of fp32 roundings on the longest path into an element, counted from
csrc/hip/lenet_kernels.hip (lenet_emul.fp32_counts), term by term:

  conv forward    26   25 products added to the bias (acc += w * x)
  sigmoid 1       ceil(|z1|max) + 4   1/(1 + __expf(-v)): the exponent
                       product is rounded once, which moves the power by a
                       relative |v| 2^-24; exp2 is good to an ulp (2); the
                       add (1); the divide (1)
  pool forward    17   16 products added to the bias (0 under max pooling)
  sigmoid 2       ceil(|z2|max) + 4
  fc forward      217  216 products (14 per lane, 4 shuffle adds) + bias
  sigmoid 3       ceil(|z3|max) + 4; softmax_ce instead: 2 (subtract, the
                       exponent product over the logit range, exp2) + the
                       10-term sum + the divide
  residual        1    onehot - y
                  ---- F, about 290 at the inputs used here
  fc_b            F + B                    sum of dz over the batch
  fc_w            F + 1 + B                dz * a2
  dz2             F + 10 + 3               da = sum_k fw dz; da a2 (1 - a2)
  pool_b          F + 13 + 216 + 1 + B     216 cells, 1/216
  pool_w          F + 13 + 1 + 216 + B     d2 * a1
  dz1             F + 13 + 4               d2 s1w a1 (1 - a1)
  conv1_b         F + 17 + 576 + 1 + B     576 positions, 1/576
  conv1_w         F + 17 + 1 + 576 + 1 + B dz1 * x

B is 0 for kernel 1 alone (a slab row is one image's gradient) and the batch
size wherever a batch is summed, in any order: the slab reduce, the atomics
of k_wgrad.  The pre-activation ranges are taken from the float64 oracle of
the very inputs.  The kernels sum in trees and in several accumulators, so
their longest path is shorter than the term counts above; the count is an
upper bound of it.  The fp32 torch_ref gradient needs C <= 12 under this
rule (tests/test_lenet_emul_cpu.py asserts it stays under the derived C).

bf16 / fp16, per block, relative L2 against the exact oracle: the larger of
4 x the ratio of the oracle that rounds where the path rounds (a1, a2 and dz1
as weight-gradient operands, see the table in tools/lenet_emul.py) and the
block's fp32 bound as relative L2; more than 2e-2 is an error.  x is rounded
to the activation dtype on the host, so input rounding is no error source.

Intermediates (a1, a2, y, dz, dz2, dz1, the loss) are held elementwise to
lenet_emul.forward_bounds64, a first-order running error bound of the fp32
chain, plus u_out |want| where the tensor is stored in activation dtype.

The weight-gradient kernel alone gets operands that are already rounded and
is compared with their float64 sums: (K + 8) 2^-24 (|A| . |B|), K the
reduction length, as in tests/test_deepcnn_kernels_gpu.py.

Every test prints the C it needed per block; PARITY.md records them.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import lenet_emul as E  # noqa: E402  (tools/: test support)
from parallel_cnn_amd.config import TrainConfig
from parallel_cnn_amd.engine.trainer import Trainer
from parallel_cnn_amd.ops import native
from parallel_cnn_amd.ops import shapes as S

pytestmark = pytest.mark.gpu

MODES = [("trainable", "residual"), ("max", "residual"),
         ("trainable", "softmax_ce")]
# seeds at which the CPU tests found the emulated ratios under the cap, no
# undecided max-pool window and no undecided prediction
SEED = {1: 1, 2: 2, 3: 7, 17: 17, 33: 35, 257: 257}
CELL, PAIR = 0, 1
NAN = float("nan")


def make_case(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, S.IN_PIX, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).float()
    return x, labels, params


@functools.lru_cache(maxsize=None)
def case(B, pool, loss, act):
    """Inputs (x rounded to act on the host) and the exact oracle, computed
    once and shared; nothing in it is modified."""
    x, labels, params = make_case(B, SEED[B])
    x = E.round_input(x, act)
    o = E.grads64(x, labels, params, pool, loss)
    return x, labels, params, o, E.forward_bounds64(o, params)


def dev_inputs(x, labels, params, act, device):
    return (x.to(device, dtype=E.STORE_DTYPE[act]),
            labels.to(device, dtype=torch.int32), params.to(device))


def within(name, got, want, bound):
    d = (got.detach().cpu().to(torch.float64).reshape(want.shape)
         - want).abs()
    assert torch.isfinite(d).all(), f"{name}: an entry was not written"
    worst = (d / bound.clamp_min(1e-300)).max().item()
    print(f"BOUND {name}: max error / bound {worst:.3f}")
    assert (d <= bound).all(), f"{name}: {worst:.3f} x its bound"


def run_fwdbwd(x, labels, params, act, device, mode, pool, loss, corr=None):
    C = native.require()
    B = x.shape[0]
    ad = E.STORE_DTYPE[act]
    xd, ld, pd = dev_inputs(x, labels, params, act, device)
    full = lambda n, dt: torch.full((B, n), NAN, dtype=dt, device=device)  # noqa: E731
    t = {"a1": full(S.C1_OUT, ad), "a2": full(S.S1_OUT, ad),
         "y": full(S.FC_OUT, torch.float32),
         "dz": full(S.FC_OUT, torch.float32),
         "dz2": full(S.S1_OUT, torch.float32), "dz1": full(S.C1_OUT, ad)}
    lacc = torch.zeros(1, device=device)
    if corr is None:
        corr = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_fwdbwd(xd, pd, t["a1"], t["a2"], t["y"], t["dz"], t["dz2"],
                 t["dz1"], ld, lacc, corr, B, mode,
                 native.current_stream_handle(), 1 if pool == "max" else 0,
                 1 if loss == "softmax_ce" else 0)
    torch.cuda.synchronize()
    t["loss"] = lacc.item()
    return t


# ------------------------------------------------- hip_fwdbwd, train mode
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pool,loss", MODES)
@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
def test_fwdbwd_train_intermediates(act, pool, loss, B, device):
    x, labels, params, o, eb = case(B, pool, loss, act)
    t = run_fwdbwd(x, labels, params, act, device, 0, pool, loss)
    for name in ("a1", "a2", "y", "dz", "dz2", "dz1"):
        want = o[name].reshape(B, -1)
        stored = act if name in ("a1", "a2", "dz1") else "fp32"
        within(f"{act} {pool}/{loss} B{B} {name}", t[name], want,
               E.store_bound(eb[name], want, stored))
    lb = eb["loss"] + E.U32 * abs(o["loss"])
    print(f"BOUND loss: error {abs(t['loss'] - o['loss']):.3e} bound "
          f"{lb:.3e}")
    assert abs(t["loss"] - o["loss"]) <= lb


# ----------------------------------------- hip_wgrad / hip_wgrad_roles alone
def wgrad_operands(B, act):
    """Oracle intermediates rounded to the dtype k_wgrad reads, the float64
    sums of those rounded values, and (K + 8) 2^-24 (|A| . |B|)."""
    x, labels, params, o, _ = case(B, "trainable", "residual", act)
    ra = E.rounder(E.STORE_DTYPE[act])
    r32 = E.rounder(torch.float32)
    ops = {"x": x.double(), "a1": ra(o["a1"]), "a2": ra(o["a2"]),
           "dz": r32(o["dz"]), "dz2": r32(o["dz2"]), "dz1": ra(o["dz1"])}
    patches = torch.nn.functional.unfold(
        ops["x"].view(B, 1, S.IN_H, S.IN_W), S.C1_K)
    want = E._weight_grads(ops["dz"], ops["a2"], ops["dz2"], ops["a1"],
                           ops["dz1"], patches, "trainable").sum(0)
    mag = E._weight_grads(ops["dz"].abs(), ops["a2"].abs(), ops["dz2"].abs(),
                          ops["a1"].abs(), ops["dz1"].abs(), patches.abs(),
                          "trainable").sum(0)
    K = {"conv1_w": S.C1_PIX * B, "conv1_b": S.C1_PIX * B,
         "pool_w": S.S1_OUT * B, "pool_b": S.S1_OUT * B, "fc_w": B, "fc_b": B}
    bound = torch.zeros_like(mag)
    for name, (off, n) in E.BLOCKS.items():
        bound[off:off + n] = (K[name] + 8) * E.U32 * mag[off:off + n]
    return ops, want, bound


def run_wgrad(ops, B, act, device, chunk, roles=None):
    C = native.require()
    ad = E.STORE_DTYPE[act]
    d = {k: v.to(device, dtype=ad if k in ("x", "a1", "a2", "dz1")
                 else torch.float32).contiguous() for k, v in ops.items()}
    grads = torch.zeros(S.N_PARAMS, device=device)   # the kernel adds into it
    st = native.current_stream_handle()
    if roles is None:
        C.hip_wgrad(d["x"], d["a1"], d["a2"], d["dz"], d["dz2"], d["dz1"],
                    grads, B, chunk, st)
    else:
        C.hip_wgrad_roles(d["x"], d["a1"], d["a2"], d["dz"], d["dz2"],
                          d["dz1"], grads, B, chunk, roles, st)
    torch.cuda.synchronize()
    return grads.cpu()


@pytest.mark.parametrize("chunk", [2, 8])
@pytest.mark.parametrize("B", [1, 2, 3, 17])
@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_wgrad_alone_sums_its_operands(act, B, chunk, device):
    """Odd and tiny item counts: the conv role keeps two items in flight per
    loop trip over 144 B items, on 6 x chunk blocks of 256 threads."""
    ops, want, bound = wgrad_operands(B, act)
    got = run_wgrad(ops, B, act, device, chunk)
    within(f"wgrad {act} B{B} chunk{chunk}", got, want, bound)
    assert got[:S.OFF_C1B].abs().max().item() > 0


@pytest.mark.parametrize("roles", [1, 2, 4])
def test_wgrad_roles_write_their_own_blocks_only(roles, device):
    B = 3
    ops, want, bound = wgrad_operands(B, "fp32")
    got = run_wgrad(ops, B, "fp32", device, 2, roles)
    own = {1: ("conv1_w", "conv1_b"), 2: ("pool_w", "pool_b"),
           4: ("fc_w", "fc_b")}[roles]
    for name, (off, n) in E.BLOCKS.items():
        sl = slice(off, off + n)
        if name in own:
            within(f"roles {roles} {name}", got[sl], want[sl], bound[sl])
            assert got[sl].abs().max().item() > 0
        else:
            assert torch.equal(got[sl].view(torch.int32),
                               torch.zeros(n, dtype=torch.int32)), name


# -------------------------------------- hip_fwdbwd_inblock, cell and pair
def image_oracles(B, pool, loss, act):
    """Per image: (oracle, M, C, tolerance) of that image's own gradient."""
    x, labels, params, _, _ = case(B, pool, loss, act)
    return [E.oracle(x[b:b + 1], labels[b:b + 1], params, pool, loss,
                     "inblock", act, n_batch=0) for b in range(B)]


@pytest.mark.parametrize("variant", [CELL, PAIR])
@pytest.mark.parametrize("pool,loss", MODES)
@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_inblock_slab_rows(act, pool, loss, variant, device):
    """Row b of the slab is image b's conv and pool gradient, per block and
    per element; columns [OFF_FW, GSLAB_LD) are padding that nothing reads
    (csrc/lenet_dims.h) and are not looked at."""
    C = native.require()
    B = 3
    x, labels, params, o, eb = case(B, pool, loss, act)
    xd, ld, pd = dev_inputs(x, labels, params, act, device)
    ad = E.STORE_DTYPE[act]
    a2 = torch.full((B, S.S1_OUT), NAN, dtype=ad, device=device)
    y = torch.full((B, S.FC_OUT), NAN, device=device)
    dz = torch.full((B, S.FC_OUT), NAN, device=device)
    lacc = torch.zeros(1, device=device)
    slab = torch.full((B, S.GSLAB_LD), NAN, device=device)
    C.hip_fwdbwd_inblock(xd, pd, a2, y, dz, ld, lacc, slab, B,
                         native.current_stream_handle(),
                         1 if pool == "max" else 0,
                         1 if loss == "softmax_ce" else 0, variant=variant)
    torch.cuda.synchronize()
    got = slab[:, :S.OFF_FW].cpu().double()
    assert torch.isfinite(got).all(), "a slab column was not written"
    what = f"{'pair' if variant else 'cell'} {act} {pool}/{loss}"
    fails = []
    for b, (ob, M, _, Cb, tol) in enumerate(image_oracles(B, pool, loss,
                                                          act)):
        row = ob["g"].clone()
        row[:S.OFF_FW] = got[b]
        fails += E.check_gradient(f"{what} row {b}", row, ob["g"], M, Cb, tol,
                                  blocks=E.SLAB_BLOCKS)
        assert got[b, :S.OFF_S1W].abs().max().item() > 0
    assert not fails, fails
    if pool == "max":
        assert torch.count_nonzero(got[:, S.OFF_S1W:]).item() == 0
    within(f"{what} a2", a2, o["a2"], E.store_bound(eb["a2"], o["a2"], act))
    within(f"{what} y", y, o["y"], E.store_bound(eb["y"], o["y"], "fp32"))
    within(f"{what} dz", dz, o["dz"], E.store_bound(eb["dz"], o["dz"],
                                                    "fp32"))
    assert abs(lacc.item() - o["loss"]) <= eb["loss"] + E.U32 * abs(o["loss"])


# ------------------------------------- the whole step, every Trainer path
def make_trainer(monkeypatch, path, B, act):
    step, wgrad, fwdbwd = {"pair": ("2", "inblock", "pair"),
                           "cell": ("2", "inblock", "cell"),
                           "grid": ("2", "grid", "pair"),
                           "three_launch": ("3", "inblock", "pair"),
                           "handoff": ("2", "inblock", "pair")}[path]
    monkeypatch.setenv("PCNN_LENET_STEP", step)
    monkeypatch.setenv("PCNN_LENET_WGRAD", wgrad)
    monkeypatch.setenv("PCNN_LENET_FWDBWD", fwdbwd)
    t = Trainer(TrainConfig(batch_size=B, device="cuda", backend="hip",
                            log_interval=0, act_dtype=act,
                            grad_reduction="sum"))
    assert t._use_inblock() == (path in ("pair", "cell", "handoff"))
    assert t._fused_step_mode() == int(step)
    return t


STEP_CASES = [("pair", "fp32", 3), ("pair", "bf16", 3), ("pair", "fp16", 3),
              ("cell", "fp32", 3), ("cell", "bf16", 3), ("grid", "fp32", 3),
              ("grid", "bf16", 3), ("three_launch", "fp32", 3),
              ("three_launch", "bf16", 3), ("handoff", "fp32", 257)]


@pytest.mark.parametrize("path,act,B", STEP_CASES)
def test_whole_step_gradient_per_block(path, act, B, device, monkeypatch):
    """(params_after - params_before) / step, block by block.  The update is
    p = fl(p + step * g): the store adds 2^-24 |p| per entry and, where the
    multiply-add is not fused, 2^-24 |step g| more; both are allowed on top.
    The gradient the GPU formed (to within that store) is then mutated four
    ways on the host, and every mutant has to fail: the check bites."""
    x, labels, params, o, _ = case(B, "trainable", "residual", act)
    if path == "handoff":
        assert B > native.require().INBLOCK_MAX_BATCH
    epath = {"pair": "inblock", "cell": "inblock", "handoff": "grid"}.get(
        path, path)
    _, M, _, C, tol = E.oracle(x, labels, params, "trainable", "residual",
                               epath, act)
    t = make_trainer(monkeypatch, path, B, act)
    with torch.no_grad():
        t.model.params.copy_(params.to(t.device))
    t.step(*t.stage_batch(x, labels))
    torch.cuda.synchronize()
    after = t.model.params.cpu()
    step = float(torch.tensor(t.cfg.dt, dtype=torch.float32).item())
    got = (after.double() - params.double()) / step
    extra = E.param_store_floor(after, step) + E.U32 * o["g"].abs()
    what = f"step {path} {act} B{B}"
    print(f"NEEDED {what}: " + ", ".join(
        f"{k} {v:.1f}" for k, v in E.needed_c(got, o["g"], M, extra).items()))
    print(f"RATIO {what}: " + ", ".join(
        f"{k} {v:.2e}" for k, v in E.block_ratios(got, o["g"]).items()))
    fails = E.check_gradient(what, got, o["g"], M, C, tol, extra)
    assert not fails, fails
    quiet = lambda *_: None  # noqa: E731
    for name, bad in E.mutants(got, o).items():
        if act != "fp32" and name not in ("conv1_w zeroed",
                                          "pool_w entries swapped"):
            continue
        assert E.check_gradient(name, bad, o["g"], M, C, tol, extra,
                                log=quiet), f"{name} went unnoticed"


# --------------------------------------------- eval and infer (modes 1, 2)
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("pool,loss", MODES)
@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
def test_eval_and_infer_modes(act, pool, loss, B, device):
    """The correct count is the float64 oracle's (no image at these seeds
    has its two largest outputs closer than the forward bound: CPU test);
    correct_accum adds across calls; y in infer mode is train mode's y bit
    for bit and within the forward bound."""
    x, labels, params, o, eb = case(B, pool, loss, act)
    assert E.undecided_images(o, eb["y"]) == 0
    want = int((o["y"].argmax(1) == o["labels"]).sum().item())
    corr = torch.zeros(1, dtype=torch.int32, device=device)
    ev = run_fwdbwd(x, labels, params, act, device, 1, pool, loss, corr)
    assert int(corr.item()) == want
    run_fwdbwd(x, labels, params, act, device, 1, pool, loss, corr)
    assert int(corr.item()) == 2 * want
    inf = run_fwdbwd(x, labels, params, act, device, 2, pool, loss, corr)
    assert int(corr.item()) == 2 * want
    tr = run_fwdbwd(x, labels, params, act, device, 0, pool, loss)
    within(f"infer {act} {pool}/{loss} B{B} y", inf["y"], o["y"],
           E.store_bound(eb["y"], o["y"], "fp32"))
    assert torch.equal(inf["y"], tr["y"])
    assert torch.equal(ev["y"], tr["y"])
    # neither mode runs the backward: its outputs stay as they were
    for name in ("dz", "dz2", "dz1"):
        assert torch.isnan(inf[name].float()).all(), name
