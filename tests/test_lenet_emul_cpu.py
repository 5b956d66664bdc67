"""CPU checks of the float64 LeNet oracle and of the comparison rule the
LeNet GPU tests lean on (tools/lenet_emul.py).

The rule is checked here against something that is not a kernel: the fp32
torch_ref gradient has to satisfy the fp32 bound, the rounding-emulating
oracle has to stay under the cap at every (B, seed) the GPU tests use, and
four seeded faults have to fail the new rule while the old flat tolerance
passes them.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                os.pardir, "tools"))
import lenet_emul as E  # noqa: E402  (tools/: test support)
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref

# (B, seed, pool, loss): every case a LeNet GPU test compares with the oracle
CASES = [(1, 1, "trainable", "residual"), (3, 7, "trainable", "residual"),
         (5, 11, "trainable", "residual"), (16, 116, "trainable", "residual"),
         (3, 7, "max", "residual"), (3, 7, "trainable", "softmax_ce"),
         (1, 1, "max", "residual"), (1, 1, "trainable", "softmax_ce"),
         (2, 2, "trainable", "residual"), (17, 17, "trainable", "residual"),
         (33, 35, "trainable", "residual"), (33, 35, "max", "residual"),
         (33, 35, "trainable", "softmax_ce"), (1, 64, "trainable", "residual"),
         (64, 64, "trainable", "residual"), (65, 165, "trainable", "residual"),
         (100, 100, "trainable", "residual"), (64, 5, "trainable", "residual"),
         (64, 15, "trainable", "residual"), (1, 101, "trainable", "residual"),
         (3, 103, "trainable", "residual"), (3, 103, "max", "residual"),
         (3, 103, "trainable", "softmax_ce"), (257, 257, "trainable", "residual")]
# the cases compared in bf16 / fp16
HALF_CASES = [c for c in CASES if c[0] <= 33] + [
    (64, 5, "trainable", "residual"), (64, 15, "trainable", "residual")]
# where a decision enters the comparison: max pooling routes the gradient to
# an argmax, eval mode counts argmax(y) == label (B in {1, 33})
DECISION_CASES = [c for c in CASES if c[2] == "max" or c[0] in (1, 33)]


def make_case(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, S.IN_PIX, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).float()
    return x, labels, params


def ref32(x, labels, params, pool, loss):
    a1, a2, y = torch_ref.forward(x, params, pool, loss)
    dz, dz2, dz1, g, lv = torch_ref.backward(x, params, a1, a2, y, labels,
                                             pool, loss)
    return {"a1": a1.reshape(x.shape[0], -1), "a2": a2.reshape(x.shape[0], -1),
            "y": y, "dz": dz, "dz2": dz2, "dz1": dz1, "g": g, "loss": lv}


def test_block_slices_cover_the_parameters_once():
    hit = torch.zeros(S.N_PARAMS, dtype=torch.int64)
    for off, n in E.BLOCKS.values():
        hit[off:off + n] += 1
    assert torch.equal(hit, torch.ones_like(hit))
    assert list(E.BLOCKS) == ["conv1_w", "conv1_b", "pool_w", "pool_b",
                              "fc_w", "fc_b"]


@pytest.mark.parametrize("B,seed,pool,loss", CASES)
def test_exact_oracle_is_torch_ref_in_float64(B, seed, pool, loss):
    """Identity rounding: every block within 1e-5 relative L2 of the fp32
    torch_ref, |g64| <= M everywhere, and the fp32 torch_ref gradient within
    the fp32 bound the kernels are held to (and every intermediate within
    its forward bound)."""
    x, labels, params = make_case(B, seed)
    o = E.grads64(x, labels, params, pool, loss)
    M, M_img = E.magnitude64(o, params)
    r = ref32(x, labels, params, pool, loss)
    ratios = E.block_ratios(r["g"], o["g"])
    if pool == "max":
        assert o["g"][S.OFF_S1W:S.OFF_FW].abs().max().item() == 0
        ratios.pop("pool_w"), ratios.pop("pool_b")
    assert max(ratios.values()) < 1e-5, ratios
    assert (o["g"].abs() <= M).all()
    assert (o["g_img"].abs() <= M_img).all()
    assert torch.allclose(o["g_img"].sum(0), o["g"], rtol=1e-12, atol=0)
    C, _ = E.fp32_counts(o, B)
    fails = E.compare_fp32(f"torch_ref B{B}", r["g"], o["g"], M, C,
                           log=lambda *_: None)
    assert not fails, fails
    eb = E.forward_bounds64(o, params)
    for name in ("a1", "a2", "y", "dz", "dz2", "dz1"):
        d = (r[name].double() - o[name].reshape(B, -1)).abs()
        assert (d <= eb[name] + E.U32 * o[name].reshape(B, -1).abs()).all(), \
            (name, (d / eb[name].clamp_min(1e-300)).max().item())
    assert abs(r["loss"] - o["loss"]) <= eb["loss"] + E.U32 * abs(o["loss"])


@pytest.mark.parametrize("B,seed,pool,loss", DECISION_CASES)
def test_decisions_are_decided_at_the_chosen_seeds(B, seed, pool, loss):
    """Zero max-pool windows whose argmax the fp32 forward error could move,
    zero images whose prediction it could move -- in fp32 and with x rounded
    to bf16 / fp16, which is what the kernels then read."""
    x, labels, params = make_case(B, seed)
    for act in ("fp32", "bf16", "fp16"):
        o = E.grads64(E.round_input(x, act), labels, params, pool, loss)
        eb = E.forward_bounds64(o, params)
        if pool == "max":
            assert E.max_pool_ties(o, eb["a1"]) == 0
        assert E.undecided_images(o, eb["y"]) == 0


@pytest.mark.parametrize("B,seed,pool,loss", HALF_CASES)
@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_emulated_ratios_stay_under_the_cap(act, B, seed, pool, loss):
    x, labels, params = make_case(B, seed)
    xr = E.round_input(x, act)
    for path in ("inblock", "three_launch"):
        o, M, _, C, tol = E.oracle(xr, labels, params, pool, loss, path, act)
        e = E.grads64(xr, labels, params, pool, loss,
                      E.round_points(path, act))
        emul = E.block_ratios(e["g"], o["g"])
        for name, v in emul.items():
            # fc_b and pool_b are sums of dz and dz2, which stay fp32; the
            # pool blocks are identically zero under max pooling
            if name in ("fc_b", "pool_b") or (pool == "max"
                                              and name == "pool_w"):
                assert v == 0, (name, v)
            else:
                assert 0 < E.MARGIN * v <= E.CAP, (name, v)
        assert max(tol.values()) <= E.CAP


def test_seed_3_is_refused():
    """B=3, seed 3: the conv1_b sum cancels (M/|g| about 2000) and the
    rounding-emulating oracle alone leaves the cap; such a seed must raise,
    not widen."""
    x, labels, params = make_case(3, 3)
    with pytest.raises(AssertionError):
        E.oracle(E.round_input(x, "bf16"), labels, params, "trainable",
                 "residual", "inblock", "bf16")


def old_flat_rule(got, want, act):
    gmax = want.abs().max().item()
    tol = (2e-4 if act == "fp32" else 2e-2) * max(1.0, gmax)
    return (got - want).abs().max().item() < tol


def mutants(g, o):
    """E.mutants plus a conv1_w block that is 40 % off."""
    m = E.mutants(g, o)
    m["conv1_w * 0.6"] = g.clone()
    m["conv1_w * 0.6"][S.OFF_C1W:S.OFF_C1B] *= 0.6
    return m


@pytest.mark.parametrize("B,seed", [(1, 1), (3, 7), (16, 116)])
def test_new_rule_bites_where_the_flat_one_is_blind(B, seed):
    """conv1_w zeroed, conv1_b scaled by 575/576, one of a channel's 36 cell
    rows dropped from the slab sum, two pool weights swapped: each fails the
    fp32 rule; the first and the last also fail the bf16 rule (and the
    unmutated gradient passes both).

    What the old flat rule does with them, asserted below: in fp32 it passes
    the 575/576 scale, the dropped row and a conv1_w block that is 40 % off
    at every case; it sees a zeroed conv1_w only where 2e-4 |g|max is below
    the block's largest entry (it is above it at B=3, seed 3, the third
    case of the blind test below), and it does see the pool-weight swap,
    the pool weights being the largest entries (the swapped pair is the
    block's largest and smallest entry).  In bf16 it passes the zeroed block
    everywhere and sees the swap."""
    x, labels, params = make_case(B, seed)
    quiet = lambda *_: None  # noqa: E731
    o, M, _, C, _ = E.oracle(x, labels, params, "trainable", "residual",
                             "inblock", "fp32")
    g = o["g"]
    muts = mutants(g, o)
    assert not E.compare_fp32("id", g, g, M, C, log=quiet)
    for what, bad in muts.items():
        assert E.compare_fp32(what, bad, g, M, C, log=quiet), what
        if what not in ("conv1_w zeroed", "pool_w entries swapped"):
            assert old_flat_rule(bad, g, "fp32"), what
    xr = E.round_input(x, "bf16")
    o, M, _, C, tol = E.oracle(xr, labels, params, "trainable", "residual",
                               "inblock", "bf16")
    g = o["g"]
    e = E.grads64(xr, labels, params, "trainable", "residual",
                  E.round_points("inblock", "bf16"))
    assert not E.compare_blocks("emul", e["g"], g, tol, log=quiet)
    muts = mutants(g, o)
    for what in ("conv1_w zeroed", "pool_w entries swapped"):
        assert E.compare_blocks(what, muts[what], g, tol, log=quiet), what
        if what == "conv1_w zeroed":
            assert old_flat_rule(muts[what], g, "bf16"), what


def test_flat_rule_passes_a_zeroed_conv1_block_in_fp32():
    """B=3, seed 3: 2e-4 |g|max is 3.2 times the largest conv1_w entry, so
    the flat fp32 rule passes an all-zero conv1_w; the new rule does not
    (seed 3 is refused for bf16, not for fp32)."""
    x, labels, params = make_case(3, 3)
    o, M, _, C, _ = E.oracle(x, labels, params, "trainable", "residual",
                             "inblock", "fp32")
    bad = mutants(o["g"], o)["conv1_w zeroed"]
    assert old_flat_rule(bad, o["g"], "fp32")
    assert E.compare_fp32("zeroed", bad, o["g"], M, C, log=lambda *_: None)


def test_forward_bounds_see_a_wrong_activation():
    """A 1e-3 relative fault is outside the bound of every intermediate."""
    x, labels, params = make_case(3, 7)
    o = E.grads64(x, labels, params)
    eb = E.forward_bounds64(o, params)
    for name in ("a1", "a2", "y", "dz", "dz2", "dz1"):
        w = o[name].reshape(3, -1)
        assert ((w * 1e-3).abs() > eb[name] + E.U32 * w.abs()).any(), name
        assert (eb[name] >= 0).all()
