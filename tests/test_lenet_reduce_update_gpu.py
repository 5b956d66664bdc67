"""GPU tests for k_reduce_update[_mom|_adam] on their own, through
_C.hip_reduce_update[_momentum|_adam].

  * exact arithmetic: slab, dz, a2 and params are integer multiples of 2^-6
    in [-1, 1] and step = 2^-3, so every product (multiple of 2^-12, at most
    1) and every partial sum (at most 256, 20 bits) is exact in fp32, and so
    is params + step*g (21 bits).  The expected params is then one number
    whatever the order of the sum or the contraction into FMAs: the float64
    result, which rounds to fp32 unchanged.  Rows >= B of all three buffers
    hold NaN, so any read past the batch shows;
  * order: on random fp32 data the columns that only add (slab columns and
    the fc biases) must match, to the bit, four lane sums in ascending image
    order combined as (s0 + s1) + (s2 + s3);
  * momentum and Adam on the exact inputs against torch_ref, at the
    tolerances of the site tests in test_momentum_gpu / test_adam_gpu, with
    the first parameter and the last three (the tail group of the last block)
    moved exactly once;
  * two calls from the same inputs agree to the bit in params, vel and sq.
"""
import pytest
import torch

from parallel_cnn_amd.ops import native
from parallel_cnn_amd.ops import shapes as S
from parallel_cnn_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

EPS = torch.finfo(torch.float32).eps
ROWS = 256                 # every buffer is sized for this many images
STEP = 2.0 ** -3
# both sides of every trip boundary: 4 lanes x 8 or 16 images, one or more
# trips, and the pipeline's first and second trip
EXACT_B = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256]
ACTS = [torch.float32, torch.bfloat16, torch.float16]
DT, SCALE, MU, B1, B2, AEPS, T = 0.1, 0.25, 0.9, 0.9, 0.999, 1e-8, 7


def q64(gen, *shape):
    """Integer multiples of 2^-6 in [-1, 1]."""
    return torch.randint(-64, 65, shape, generator=gen) / 64.0


def exact_case(B, seed):
    """slab, a2, dz ([ROWS, .] fp32, NaN from row B on), params, and the
    gradient in float64."""
    gen = torch.Generator().manual_seed(seed)
    slab = q64(gen, ROWS, S.GSLAB_LD)
    a2 = q64(gen, ROWS, S.S1_OUT)
    dz = q64(gen, ROWS, S.FC_OUT)
    params = q64(gen, S.N_PARAMS)
    s, a, d = slab[:B].double(), a2[:B].double(), dz[:B].double()
    g = torch.cat([s[:, :S.OFF_FW].sum(0), (d.T @ a).reshape(-1), d.sum(0)])
    assert g.numel() == S.N_PARAMS
    for t in (slab, a2, dz):
        t[B:] = float("nan")
    return slab, a2, dz, params, g


def to_dev(device, act, slab, a2, dz):
    a2d = a2.to(act)
    assert torch.equal(a2d[~a2.isnan()].float(), a2[~a2.isnan()])
    return slab.to(device), a2d.to(device), dz.to(device)


@pytest.mark.parametrize("act", ACTS, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B", EXACT_B)
def test_reduce_update_exact(B, act, device):
    C = native.require()
    slab, a2, dz, params, g = exact_case(B, 100 + B)
    want64 = params.double() + STEP * g
    want = want64.float()
    assert torch.equal(want.double(), want64)      # exact in fp32
    sd, ad, dd = to_dev(device, act, slab, a2, dz)
    pd = params.to(device)
    C.hip_reduce_update(sd, ad, dd, pd, STEP, B,
                        native.current_stream_handle())
    torch.cuda.synchronize()
    got = pd.cpu()
    bad = (got != want).nonzero().flatten()
    print(f"B {B} {act}: {bad.numel()} of {S.N_PARAMS} differ"
          f"{', first at ' + str(bad[0].item()) if bad.numel() else ''}")
    assert torch.equal(got, want)
    assert (got != params).sum().item() > S.N_PARAMS // 2


def lane_order_sum(v, B):
    """v [B, n] fp32 -> what the owner group computes: lane sub adds images
    sub, sub + 4, ... in ascending order from 0, then (s0 + s1) + (s2 + s3)."""
    lanes = []
    for sub in range(4):
        s = torch.zeros(v.shape[1])
        for b in range(sub, B, 4):
            s = s + v[b]
        lanes.append(s)
    return (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])


@pytest.mark.parametrize("B", [5, 33, 64, 65, 129])
def test_reduce_update_add_order(B, device):
    C = native.require()
    gen = torch.Generator().manual_seed(200 + B)
    slab = torch.randn(ROWS, S.GSLAB_LD, generator=gen)
    dz = torch.randn(ROWS, S.FC_OUT, generator=gen)
    a2 = torch.rand(ROWS, S.S1_OUT, generator=gen)
    params = 0.5 - torch.rand(S.N_PARAMS, generator=gen)
    for t in (slab, a2, dz):
        t[B:] = float("nan")
    pd = params.to(device)
    C.hip_reduce_update(slab.to(device), a2.to(device), dz.to(device), pd,
                        STEP, B, native.current_stream_handle())
    torch.cuda.synchronize()
    got = pd.cpu()
    # step is a power of two, so step*g is exact and p + step*g rounds once,
    # fused or not
    want_slab = params[:S.OFF_FW] + STEP * lane_order_sum(
        slab[:B, :S.OFF_FW], B)
    want_fb = params[S.OFF_FB:] + STEP * lane_order_sum(dz[:B], B)
    ds = (got[:S.OFF_FW] != want_slab).sum().item()
    db = (got[S.OFF_FB:] != want_fb).sum().item()
    print(f"B {B}: slab columns differing {ds}, fc biases differing {db}")
    assert torch.equal(got[:S.OFF_FW], want_slab)
    assert torch.equal(got[S.OFF_FB:], want_fb)
    assert torch.isfinite(got).all()


def state_case(seed):
    gen = torch.Generator().manual_seed(seed)
    v = 0.5 - torch.rand(S.N_PARAMS, generator=gen)
    s = (0.1 + 0.4 * torch.rand(S.N_PARAMS, generator=gen)) ** 2
    return v, s


def moved_once(got, before, want, tol):
    """The first parameter and the last three (the tail group of the last
    block) were updated exactly once: each holds the reference's value to
    the tensor's tolerance `tol`, and the reference moved it by far more than
    that, so neither no update nor a second one could pass."""
    idx = torch.tensor([0, S.N_PARAMS - 3, S.N_PARAMS - 2, S.N_PARAMS - 1])
    mv, ref = (got - before)[idx], (want - before)[idx]
    print(f"moves {mv.tolist()} reference {ref.tolist()}")
    assert (ref.abs() > 1e-4).all() and 1e-4 > 100 * tol
    assert ((got - want)[idx].abs() <= tol).all()


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("wd,nesterov", [(5e-4, False), (5e-4, True)])
@pytest.mark.parametrize("B", [3, 33, 65])
def test_reduce_update_momentum(B, wd, nesterov, act, device):
    """Tolerance of test_momentum_gpu.check_site: 4 eps of the tensor's
    largest magnitude (three multiply-adds per element whose contraction may
    differ)."""
    C = native.require()
    slab, a2, dz, params, g = exact_case(B, 300 + B)
    v, _ = state_case(301)
    pr, vr = params.clone(), v.clone()
    torch_ref.update_momentum(pr, g.float(), vr, DT, SCALE, MU, wd, nesterov)
    sd, ad, dd = to_dev(device, act, slab, a2, dz)
    pd, vd = params.to(device), v.to(device)
    C.hip_reduce_update_momentum(sd, ad, dd, pd, vd, DT, SCALE, MU, wd,
                                 nesterov, B, native.current_stream_handle())
    torch.cuda.synchronize()
    for name, got, ref in (("p", pd.cpu(), pr), ("v", vd.cpu(), vr)):
        diff = (got - ref).abs().max().item()
        tol = 4 * EPS * ref.abs().max().item()
        print(f"B {B} {name}: diff {diff:.3e} tol {tol:.3e}")
        assert diff <= tol, (name, diff, tol)
    moved_once(pd.cpu(), params, pr, 4 * EPS * pr.abs().max().item())


@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("B", [3, 33, 65])
def test_reduce_update_adam(B, wd, act, device):
    """Tolerance of test_adam_gpu.check_site: per tensor, 4 x the largest
    difference between the fp32 and the float64 oracle on the same inputs,
    floor 1 fp32 eps of the tensor's largest magnitude."""
    C = native.require()
    slab, a2, dz, params, g = exact_case(B, 400 + B)
    m, s = state_case(401)

    def oracle(dtype):
        p_, m_, s_ = (t.to(dtype).clone() for t in (params, m, s))
        torch_ref.update_adam(p_, g.to(dtype).clone(), m_, s_, DT, SCALE, B1,
                              B2, AEPS, wd, T)
        return p_, m_, s_

    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    sd, ad, dd = to_dev(device, act, slab, a2, dz)
    pd, md, s_d = params.to(device), m.to(device), s.to(device)
    C.hip_reduce_update_adam(sd, ad, dd, pd, md, s_d, DT, SCALE, B1, B2,
                             AEPS, wd, T, B, native.current_stream_handle())
    torch.cuda.synchronize()
    for name, got, r32, r64 in zip("pms", (pd, md, s_d), o32, o64):
        odiff = (r32.double() - r64).abs().max().item()
        ddiff = (got.cpu().double() - r64).abs().max().item()
        tol = max(4 * odiff, EPS * r64.abs().max().item())
        print(f"B {B} wd {wd} {name}: fp32-oracle diff {odiff:.3e} device "
              f"diff {ddiff:.3e} tol {tol:.3e}")
        assert ddiff <= tol, (name, ddiff, tol)
        if name == "p":
            ptol = tol
    # the float64 reference rounded to fp32: half an ulp more
    moved_once(pd.cpu(), params, o64[0].float(),
               ptol + EPS * o64[0].abs().max().item())


@pytest.mark.parametrize("opt", ["plain", "momentum", "adam"])
def test_reduce_update_rerun_bit_identical(opt, device):
    C = native.require()
    B = 65
    gen = torch.Generator().manual_seed(500)
    slab = torch.randn(B, S.GSLAB_LD, generator=gen).to(device)
    dz = torch.randn(B, S.FC_OUT, generator=gen).to(device)
    a2 = torch.rand(B, S.S1_OUT, generator=gen).to(device, torch.bfloat16)
    params = 0.5 - torch.rand(S.N_PARAMS, generator=gen)
    v, s = state_case(501)
    stream = native.current_stream_handle()
    outs = []
    for _ in range(2):
        pd, vd, sd = params.to(device), v.to(device), s.to(device)
        if opt == "plain":
            C.hip_reduce_update(slab, a2, dz, pd, STEP, B, stream)
        elif opt == "momentum":
            C.hip_reduce_update_momentum(slab, a2, dz, pd, vd, DT, SCALE, MU,
                                         5e-4, True, B, stream)
        else:
            C.hip_reduce_update_adam(slab, a2, dz, pd, vd, sd, DT, SCALE, B1,
                                     B2, AEPS, 1e-2, T, B, stream)
        torch.cuda.synchronize()
        outs.append((pd.cpu(), vd.cpu(), sd.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0], params)
