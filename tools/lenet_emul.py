"""float64 oracle of one LeNet forward + backward, with rounding points, a
magnitude chain and the per-block comparison rule of the LeNet GPU tests.

grads64 is torch_ref.forward / torch_ref.backward in float64 (unfold and
einsum on float64 tensors, nothing else).  With round_at=None it is the exact
chain rule.  round_at names the tensors a GPU path reads back in activation
dtype and gives the rounder for each.

Where the HIP paths round (csrc/hip/lenet_kernels.hip; every sum, product and
sigmoid is fp32 in registers or LDS):

  path                     a1              a2             dz1
  3-launch, grid           store l.337     store l.343    store l.460
   (k_fwdbwd + k_wgrad)    read l.1124/37  read l.1188    read l.1043/53
  in-block, cell           cast l.498      store l.343    cast l.482
   (k_fwdbwd<INBLOCK>)                     read l.1448/58
  in-block, pair           cast l.902      store l.771    cast l.878
   (k_fwdbwd_pair)                         read l.1448/58
  wgrad_fuse               -- (l.531)      store l.343    -- (l.513)
                                           read l.1188

In every path the rounded value is only an operand of a weight-gradient
product: a1 of the pool weights, a2 of the fc weights, dz1 of the conv
weights and bias.  The chain itself never sees a rounded value: kernel 1's
pool forward and backward use the a1 registers (a1v, l.326 / l.452; pair av,
l.746 / l.862), its fc forward uses the unrounded a2 in LDS (L.a2s, l.342 /
l.360; pair a2s, l.770 / l.789), its fc backward the a2 register (l.433 /
l.842), and dz1 is formed from the unrounded d2 (l.457 / l.864).  x is read in
activation dtype by every kernel; the tests round it on the host first, so
the kernel and the oracle see the same input.  dz, dz2, y, the parameters and
the slab are fp32 everywhere.  ROUNDED lists the set per path.

magnitude64 runs the same backward with every sum taken over absolute
values; it returns an elementwise M with |g| <= M.  The fp32 rule is

    |got - want64| <= C * 2^-24 * M + 2^-24 * |want64|

with C the number of fp32 roundings on the longest path into an element
(fp32_counts; the count is written out term by term in
tests/test_lenet_kernels_gpu.py).  The bf16/fp16 rule is per block, relative
L2 against the exact oracle: the larger of MARGIN times the ratio of the
rounding-emulating oracle and the block's fp32 bound as relative L2; a block
whose allowance exceeds CAP is an error, never an exclusion.

forward_bounds64 is a first-order running error analysis of the fp32
forward and backward-data chain; it bounds a1, a2, y, dz, dz2, dz1 and the
loss elementwise.

Test support, kept out of the package, next to tools/deep_emul.py.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from parallel_cnn_amd.ops import shapes as S

U32 = 2.0 ** -24            # fp32 unit roundoff
# unit roundoff: 24, 8 and 11 significand bits
U_OUT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
# smallest spacing of the format (subnormals), halved: absolute store error
# of a value below the normal range
TINY_OUT = {"fp32": 2.0 ** -150, "bf16": 2.0 ** -134, "fp16": 2.0 ** -25}
MARGIN = 4.0
CAP = 2e-2

STORE_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16,
               "fp16": torch.float16}

BLOCKS = {
    "conv1_w": (S.OFF_C1W, S.C1_WSZ),
    "conv1_b": (S.OFF_C1B, S.C1_CH),
    "pool_w": (S.OFF_S1W, S.S1_WSZ),
    "pool_b": (S.OFF_S1B, 1),
    "fc_w": (S.OFF_FW, S.FC_WSZ),
    "fc_b": (S.OFF_FB, S.FC_OUT),
}

# tensors a path reads in activation dtype as weight-gradient operands
ROUNDED = {
    "three_launch": ("a1", "a2", "dz1"),
    "grid": ("a1", "a2", "dz1"),
    "inblock": ("a1", "a2", "dz1"),
    "wgrad_fuse": ("a2",),
}


def rounder(dtype):
    def r(t: torch.Tensor) -> torch.Tensor:
        return t.to(dtype).to(torch.float64)
    return r


def round_points(path: str, act_dtype: str):
    """round_at for grads64: {tensor name: rounder} of one path."""
    r = rounder(STORE_DTYPE[act_dtype])
    return {name: r for name in ROUNDED[path]}


def round_input(x: torch.Tensor, act_dtype: str) -> torch.Tensor:
    """x as every kernel reads it: rounded to the activation dtype (fp32)."""
    return x.to(STORE_DTYPE[act_dtype]).to(torch.float32)


def _split(p):
    c1w = p[S.OFF_C1W:S.OFF_C1B].view(S.C1_CH, 1, S.C1_K, S.C1_K)
    c1b = p[S.OFF_C1B:S.OFF_S1W]
    s1w = p[S.OFF_S1W:S.OFF_S1B].view(S.S1_K, S.S1_K)
    s1b = p[S.OFF_S1B:S.OFF_FW]
    fw = p[S.OFF_FW:S.OFF_FB].view(S.FC_OUT, S.FC_IN)
    fb = p[S.OFF_FB:]
    return c1w, c1b, s1w, s1b, fw, fb


def _windows(a1):
    """[B,6,24,24] -> [B,6,6,6,16]: the 4x4 window of every pool cell."""
    B = a1.shape[0]
    w = a1.view(B, S.C1_CH, S.S1_H, S.S1_K, S.S1_W, S.S1_K)
    return w.permute(0, 1, 2, 4, 3, 5).reshape(B, S.C1_CH, S.S1_H, S.S1_W,
                                               S.S1_WSZ)


def _unwindows(w):
    B = w.shape[0]
    return w.view(B, S.C1_CH, S.S1_H, S.S1_W, S.S1_K, S.S1_K).permute(
        0, 1, 2, 4, 3, 5).reshape(B, S.C1_CH, S.C1_H, S.C1_W)


def _weight_grads(dz, a2w, dz2, a1w, dz1w, patches, pool):
    """Per-image flat gradient [B, N_PARAMS] from the backward tensors."""
    B = dz.shape[0]
    g = torch.zeros(B, S.N_PARAMS, dtype=torch.float64)
    g[:, S.OFF_FW:S.OFF_FB] = torch.einsum("bk,bm->bkm", dz, a2w).reshape(
        B, -1)
    g[:, S.OFF_FB:] = dz
    if pool != "max":
        g[:, S.OFF_S1B] = dz2.sum(1) / S.FC_IN
        g[:, S.OFF_S1W:S.OFF_S1B] = torch.einsum(
            "bopq,bopqw->bw", dz2.view(B, S.C1_CH, S.S1_H, S.S1_W),
            _windows(a1w))
    dz1f = dz1w.reshape(B, S.C1_CH, S.C1_PIX)
    g[:, S.OFF_C1W:S.OFF_C1B] = (
        torch.einsum("bot,bwt->bow", dz1f, patches) / S.C1_PIX).reshape(B, -1)
    g[:, S.OFF_C1B:S.OFF_S1W] = dz1f.sum(2) / S.C1_PIX
    return g


def grads64(x, labels, params, pool="trainable", loss="residual",
            round_at=None):
    """One forward + backward in float64.  x [B,784] (already in the values
    the kernel reads), params the fp32 master parameters.  Returns a dict:
    g (flat batch-sum gradient), g_img ([B, N_PARAMS], per image), loss,
    loss_img, the unrounded a1 [B,6,24,24], a2 [B,216], y, dz, dz2 [B,216],
    dz1 [B,3456], and the pre-activations z1, z2, z3."""
    ra = round_at or {}
    ident = lambda t: t  # noqa: E731
    r_a1, r_a2, r_dz1 = (ra.get(k, ident) for k in ("a1", "a2", "dz1"))
    p = params.detach().cpu().to(torch.float64)
    x = x.detach().cpu().to(torch.float64)
    labels = labels.detach().cpu().to(torch.int64)
    B = x.shape[0]
    c1w, c1b, s1w, s1b, fw, fb = _split(p)
    xi = x.view(B, 1, S.IN_H, S.IN_W)
    z1 = F.conv2d(xi, c1w, c1b)
    a1 = torch.sigmoid(z1)
    if pool == "max":
        z2 = F.max_pool2d(a1, S.S1_K)
    else:
        z2 = F.conv2d(a1, s1w.expand(S.C1_CH, 1, S.S1_K, S.S1_K),
                      s1b.expand(S.C1_CH), stride=S.S1_K, groups=S.C1_CH)
    a2 = torch.sigmoid(z2).reshape(B, S.FC_IN)
    z3 = F.linear(a2, fw, fb)
    y = torch.softmax(z3, 1) if loss == "softmax_ce" else torch.sigmoid(z3)

    dz = F.one_hot(labels, S.FC_OUT).to(torch.float64) - y
    if loss == "softmax_ce":
        loss_img = -torch.log(y.gather(1, labels.view(-1, 1)).clamp_min(
            1e-30)).view(-1)
    else:
        loss_img = dz.norm(dim=1)
    dz2 = (dz @ fw) * a2 * (1 - a2)
    d2 = dz2.view(B, S.C1_CH, S.S1_H, S.S1_W)
    if pool == "max":
        win = _windows(a1)
        da1w = torch.zeros_like(win)
        da1w.scatter_(-1, win.argmax(-1, keepdim=True), d2.unsqueeze(-1))
        da1 = _unwindows(da1w)
    else:
        up = d2.repeat_interleave(S.S1_K, 2).repeat_interleave(S.S1_K, 3)
        da1 = up * s1w.repeat(S.S1_H, S.S1_W)
    dz1 = da1 * a1 * (1 - a1)
    patches = F.unfold(xi, S.C1_K)
    g_img = _weight_grads(dz, r_a2(a2), dz2, r_a1(a1), r_dz1(dz1), patches,
                          pool)
    return {"g": g_img.sum(0), "g_img": g_img, "loss": loss_img.sum().item(),
            "loss_img": loss_img, "a1": a1, "a2": a2, "y": y, "dz": dz,
            "dz2": dz2, "dz1": dz1.reshape(B, -1), "z1": z1,
            "z2": z2.reshape(B, -1), "z3": z3, "x": x, "labels": labels,
            "pool": pool, "loss_mode": loss}


def magnitude64(o, params):
    """The backward of grads64 over absolute values (|onehot| + |y|,
    |dz| @ |fw|, |s1w|, |patches|): per-image M_img [B, N_PARAMS] and the
    batch sum M, with |g_img| <= M_img and |g| <= M elementwise.  o is the
    dict grads64 returned."""
    p = params.detach().cpu().to(torch.float64)
    _c1w, _c1b, s1w, _s1b, fw, _fb = _split(p)
    B = o["y"].shape[0]
    a1, a2 = o["a1"], o["a2"]
    mdz = F.one_hot(o["labels"], S.FC_OUT).to(torch.float64) + o["y"].abs()
    mdz2 = (mdz @ fw.abs()) * a2 * (1 - a2)
    d2 = mdz2.view(B, S.C1_CH, S.S1_H, S.S1_W)
    if o["pool"] == "max":
        win = _windows(a1)
        mw = torch.zeros_like(win)
        mw.scatter_(-1, win.argmax(-1, keepdim=True), d2.unsqueeze(-1))
        mda1 = _unwindows(mw)
    else:
        up = d2.repeat_interleave(S.S1_K, 2).repeat_interleave(S.S1_K, 3)
        mda1 = up * s1w.abs().repeat(S.S1_H, S.S1_W)
    mdz1 = mda1 * a1 * (1 - a1)
    patches = F.unfold(o["x"].view(B, 1, S.IN_H, S.IN_W), S.C1_K).abs()
    m_img = _weight_grads(mdz, a2, mdz2, a1, mdz1, patches, o["pool"])
    return m_img.sum(0), m_img


# ----------------------------------------------------------- fp32 count
def sigmoid_allowance(vmax: float) -> int:
    """fp32 roundings of sigmoidf_dev = 1/(1 + __expf(-v)), relative to the
    result, for |v| <= vmax.  __expf(-v) is exp2(-v * log2(e)): the product
    is rounded once, a relative u of an exponent of size |v| log2(e), i.e. a
    relative |v| u of the power (ceil(vmax) roundings); the hardware exp2 is
    good to one ulp (2); the add (1); the correctly rounded divide (1)."""
    return int(math.ceil(vmax)) + 4


def fp32_counts(o, n_batch: int):
    """{block: C} and the named terms, for the gradient of n_batch summed
    images (0: one image's own gradient, i.e. a slab row; B: any path that
    sums the batch).  Pre-activation ranges come from the oracle dict o."""
    t = {}
    t["conv_fwd"] = S.C1_K * S.C1_K + 1                      # 25 + bias
    t["sig1"] = sigmoid_allowance(o["z1"].abs().max().item())
    # max pooling selects, it does not round
    t["pool_fwd"] = 0 if o["pool"] == "max" else S.S1_WSZ + 1
    t["sig2"] = sigmoid_allowance(o["z2"].abs().max().item())
    t["fc_fwd"] = S.FC_IN + 1
    z3 = o["z3"]
    if o["loss_mode"] == "softmax_ce":
        # e_k = __expf(z_k - max): subtract (1), the exponent product
        # (ceil(range)), exp2 (2); numerator and denominator each carry it;
        # the 10-term sum (10) and the divide (1)
        rng = (z3.max(1).values - z3.min(1).values).max().item()
        t["out"] = 2 * (1 + int(math.ceil(rng)) + 2) + S.FC_OUT + 1
    else:
        t["out"] = sigmoid_allowance(z3.abs().max().item())
    t["residual"] = 1                                        # onehot - y
    fwd = sum(t.values())
    t["fc_bwd"] = S.FC_OUT          # da = sum_k fw[k,m] dz[k]
    t["dz2"] = 3                    # da * a2 * (1 - a2)
    t["dz1"] = 4                    # d2 * s1w * a1 * (1 - a1)
    t["product"] = 1                # the weight-gradient product
    t["scale"] = 1                  # 1/576, 1/216
    t["pool_sum"] = S.S1_OUT        # 216 cells per image
    t["conv_sum"] = S.C1_PIX        # 576 positions per image and channel
    t["batch"] = n_batch
    to_dz2 = fwd + t["fc_bwd"] + t["dz2"]
    to_dz1 = to_dz2 + t["dz1"]
    C = {
        "fc_b": fwd + n_batch,
        "fc_w": fwd + t["product"] + n_batch,
        "pool_b": to_dz2 + t["pool_sum"] + t["scale"] + n_batch,
        "pool_w": to_dz2 + t["product"] + t["pool_sum"] + n_batch,
        "conv1_b": to_dz1 + t["conv_sum"] + t["scale"] + n_batch,
        "conv1_w": to_dz1 + t["product"] + t["conv_sum"] + t["scale"]
        + n_batch,
    }
    return C, t


def fp32_bound(want, M, C):
    """Elementwise C * 2^-24 * M + 2^-24 * |want| over the flat layout (the
    last dimension is N_PARAMS)."""
    cvec = torch.zeros(S.N_PARAMS, dtype=torch.float64)
    for name, (off, n) in BLOCKS.items():
        cvec[off:off + n] = float(C[name])
    return cvec * U32 * M + U32 * want.abs()


def block_ratios(got, want):
    """{block: ||got - want|| / ||want||} (float64, flat layout)."""
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    out = {}
    for name, (off, n) in BLOCKS.items():
        w = want[..., off:off + n]
        out[name] = ((got[..., off:off + n] - w).norm()
                     / w.norm().clamp_min(1e-300)).item()
    return out


def needed_c(got, want, M, extra=None):
    """{block: max |got - want| / (2^-24 M)}: the C a block would need with
    nothing else allowed (the figure the tests print and PARITY.md records).
    extra, if given, is an absolute allowance taken off first."""
    d = (got.detach().cpu().to(torch.float64) - want).abs()
    if extra is not None:
        d = (d - extra).clamp_min(0.0)
    out = {}
    for name, (off, n) in BLOCKS.items():
        dd, mm = d[..., off:off + n], M[..., off:off + n]
        r = torch.where(dd > 0, dd / (U32 * mm).clamp_min(1e-300),
                        torch.zeros_like(dd))
        out[name] = r.max().item()
    return out


def compare_fp32(what, got, want, M, C, extra=None, blocks=None, log=print):
    """Elementwise fp32 rule; extra is an additional absolute allowance per
    element (e.g. the fp32 parameter store).  Prints the needed C next to
    the derived C of every block and returns the list of failures."""
    got = got.detach().cpu().to(torch.float64)
    bound = fp32_bound(want, M, C)
    if extra is not None:
        bound = bound + extra
    d = (got - want).abs()
    need = needed_c(got, want, M, extra)
    fails = []
    for name, (off, n) in BLOCKS.items():
        if blocks is not None and name not in blocks:
            continue
        bad = ~(d[..., off:off + n] <= bound[..., off:off + n])
        log(f"FP32 {what} {name}: needed C {need[name]:.1f} derived "
            f"{C[name]}")
        if bad.any():
            fails.append(f"{name}: {int(bad.sum())} entries past the bound, "
                         f"needed C {need[name]:.1f} > {C[name]}")
    return fails


def fp32_block_rel(want, M, C):
    """The fp32 elementwise bound of every block as a relative L2."""
    b = fp32_bound(want, M, C)
    return {name: (b[..., off:off + n].norm()
                   / want[..., off:off + n].norm().clamp_min(1e-300)).item()
            for name, (off, n) in BLOCKS.items()}


def block_tolerances(emul: dict, fp32_rel: dict, pool="trainable"):
    """Per-block relative-L2 tolerance of the bf16/fp16 rule: the larger of
    MARGIN * emulated ratio and the block's fp32 bound.  An allowance above
    CAP raises.  Under max pooling the pool blocks are identically zero and
    carry no tolerance (the kernel must give exact zeros)."""
    tol = {}
    for name in BLOCKS:
        if pool == "max" and name in ("pool_w", "pool_b"):
            tol[name] = 0.0
            continue
        tol[name] = max(MARGIN * emul[name], fp32_rel[name])
        if tol[name] > CAP:
            raise AssertionError(
                f"block {name}: allowance {tol[name]:.3g} > {CAP} "
                f"(emulated {emul[name]:.3g}, fp32 {fp32_rel[name]:.3g})")
    return tol


def compare_blocks(what, got, want, tol, extra=None, blocks=None, log=print):
    """Per-block ||got - want|| <= tol * ||want|| (+ ||extra|| of the block,
    an absolute allowance per element).  Returns the failures."""
    got = got.detach().cpu().to(torch.float64)
    fails = []
    for name, (off, n) in BLOCKS.items():
        if blocks is not None and name not in blocks:
            continue
        w = want[..., off:off + n]
        err = (got[..., off:off + n] - w).norm().item()
        ref = w.norm().item()
        fl = extra[..., off:off + n].norm().item() if extra is not None \
            else 0.0
        meas = err / max(ref, 1e-300)
        log(f"BLOCK {what} {name}: measured {meas:.2e} tol {tol[name]:.2e}")
        if not err <= tol[name] * ref + fl:
            fails.append(f"{name}: {meas:.3e} > {tol[name]:.3e}")
    return fails


def oracle(x, labels, params, pool, loss, path, act_dtype, n_batch=None):
    """Everything a gradient comparison needs, for x already rounded to
    act_dtype: the exact oracle dict o, M, M_img, the derived C, and for
    bf16/fp16 the per-block tolerance (None for fp32)."""
    o = grads64(x, labels, params, pool, loss)
    M, M_img = magnitude64(o, params)
    nb = x.shape[0] if n_batch is None else n_batch
    C, _ = fp32_counts(o, nb)
    tol = None
    if act_dtype != "fp32":
        e = grads64(x, labels, params, pool, loss,
                    round_points(path, act_dtype))
        tol = block_tolerances(block_ratios(e["g"], o["g"]),
                               fp32_block_rel(o["g"], M, C), pool)
    return o, M, M_img, C, tol


def check_gradient(what, got, want, M, C, tol, extra=None, blocks=None,
                   log=print):
    """The rule of the LeNet GPU tests: elementwise for fp32 (tol None), per
    block otherwise.  Returns the failures."""
    if tol is None:
        return compare_fp32(what, got, want, M, C, extra, blocks, log=log)
    return compare_blocks(what, got, want, tol, extra, blocks, log=log)


SLAB_BLOCKS = ("conv1_w", "conv1_b", "pool_w", "pool_b")


def without_cell(o, channel, pr, pc):
    """The batch gradient with one pool cell of one channel (one of the 36
    per-cell rows the in-block kernels sum) left out of the conv sums."""
    B = o["y"].shape[0]
    dz1 = o["dz1"].view(B, S.C1_CH, S.C1_H, S.C1_W).clone()
    dz1[:, channel, pr * S.S1_K:(pr + 1) * S.S1_K,
        pc * S.S1_K:(pc + 1) * S.S1_K] = 0
    patches = F.unfold(o["x"].view(B, 1, S.IN_H, S.IN_W), S.C1_K)
    d = dz1.reshape(B, S.C1_CH, S.C1_PIX)
    g = o["g"].clone()
    g[S.OFF_C1W:S.OFF_C1B] = (torch.einsum("bot,bwt->ow", d, patches)
                              / S.C1_PIX).reshape(-1)
    g[S.OFF_C1B:S.OFF_S1W] = d.sum(dim=(0, 2)) / S.C1_PIX
    return g


def mutants(got, o):
    """Four seeded faults of a gradient `got` whose exact value is o["g"]:
    conv1_w zeroed, conv1_b scaled by 575/576, one per-cell row of channel 2
    dropped, the largest and the smallest pool weight gradient swapped."""
    got = got.detach().cpu().to(torch.float64)
    zero_w = got.clone()
    zero_w[S.OFF_C1W:S.OFF_C1B] = 0
    scale_b = got.clone()
    scale_b[S.OFF_C1B:S.OFF_S1W] *= 575.0 / 576.0
    drop = got - (o["g"] - without_cell(o, 2, 1, 3))
    swap = got.clone()
    pw = got[S.OFF_S1W:S.OFF_S1B]
    i, j = S.OFF_S1W + int(pw.argmax()), S.OFF_S1W + int(pw.argmin())
    swap[i], swap[j] = got[j], got[i]
    return {"conv1_w zeroed": zero_w, "conv1_b * 575/576": scale_b,
            "one cell row of channel 2 dropped": drop,
            "pool_w entries swapped": swap}


def check_batch_gradient(what, got, x, labels, params, pool, loss, path,
                         act_dtype, log=print):
    """The per-block rule on a batch-sum gradient the GPU formed from x (x
    is rounded to act_dtype here, as the kernels read it).  Returns the
    failures."""
    xr = round_input(x, act_dtype)
    o, M, _, C, tol = oracle(xr, labels, params, pool, loss, path, act_dtype)
    return check_gradient(what, got, o["g"], M, C, tol, log=log)


def check_step(what, p_before, p_after, dt, x, labels, pool, loss, path,
               act_dtype, log=print):
    """The per-block rule on (p_after - p_before) / step of one plain SGD
    step with grad_reduction="sum" (step == dt as fp32), with the fp32
    parameter store allowed on top.  Returns the failures."""
    step = float(torch.tensor(dt, dtype=torch.float32).item())
    xr = round_input(x, act_dtype)
    o, M, _, C, tol = oracle(xr, labels, p_before, pool, loss, path,
                             act_dtype)
    after = p_after.detach().cpu()
    got = (after.double() - p_before.detach().cpu().double()) / step
    extra = param_store_floor(after, step) + U32 * o["g"].abs()
    return check_gradient(what, got, o["g"], M, C, tol, extra, log=log)


def check_slab_rows(what, rows, x, labels, params, pool, loss, act_dtype,
                    log=print):
    """The per-block rule on every slab row ([B, >= OFF_FW]) against that
    image's own gradient.  Returns the failures."""
    xr = round_input(x, act_dtype)
    rows = rows.detach().cpu().to(torch.float64)
    fails = []
    for b in range(xr.shape[0]):
        o, M, _, C, tol = oracle(xr[b:b + 1], labels[b:b + 1], params, pool,
                                 loss, "inblock", act_dtype, n_batch=0)
        row = o["g"].clone()
        row[:S.OFF_FW] = rows[b, :S.OFF_FW]
        fails += check_gradient(f"{what} row {b}", row, o["g"], M, C, tol,
                                blocks=SLAB_BLOCKS, log=log)
    return fails


def param_store_floor(p_after, step):
    """The fp32 parameter store p = fl(p0 + step * g) carries 2^-24 |p| per
    entry; as a gradient that is 2^-24 |p| / step."""
    return U32 * p_after.detach().cpu().to(torch.float64).abs() / step


# ------------------------------------------- forward / backward-data bounds
def forward_bounds64(o, params):
    """First-order running error bounds (absolute, elementwise, float64) of
    the fp32 chain of kernel 1 for a1, a2, y, dz, dz2, dz1 and the loss:
    an n-term fp32 sum carries n u sum|terms|, a sigmoid its allowance times
    its value, and every input error is passed through the derivative of the
    operation that reads it."""
    u = U32
    p = params.detach().cpu().to(torch.float64)
    c1w, c1b, s1w, s1b, fw, fb = _split(p)
    B = o["y"].shape[0]
    xi = o["x"].view(B, 1, S.IN_H, S.IN_W)
    a1, a2, y, dz = o["a1"], o["a2"], o["y"], o["dz"]
    s1 = sigmoid_allowance(o["z1"].abs().max().item())
    s2 = sigmoid_allowance(o["z2"].abs().max().item())
    mz1 = F.conv2d(xi.abs(), c1w.abs(), c1b.abs())
    e_a1 = u * ((S.C1_K ** 2 + 1) * mz1 * a1 * (1 - a1) + s1 * a1)
    if o["pool"] == "max":
        e_z2 = F.max_pool2d(e_a1, S.S1_K)       # >= the argmax's own error
    else:
        pw = s1w.abs().expand(S.C1_CH, 1, S.S1_K, S.S1_K)
        mz2 = F.conv2d(a1, pw, s1b.abs().expand(S.C1_CH), stride=S.S1_K,
                       groups=S.C1_CH)
        e_z2 = u * (S.S1_WSZ + 1) * mz2 + F.conv2d(
            e_a1, pw, None, stride=S.S1_K, groups=S.C1_CH)
    e_z2 = e_z2.reshape(B, S.FC_IN)
    e_a2 = a2 * (1 - a2) * e_z2 + u * s2 * a2
    mz3 = F.linear(a2, fw.abs(), fb.abs())
    e_z3 = u * (S.FC_IN + 1) * mz3 + e_a2 @ fw.abs().T
    z3 = o["z3"]
    if o["loss_mode"] == "softmax_ce":
        rng = z3.max(1, keepdim=True).values - z3
        # relative error of e_k = __expf(z_k - max)
        r = e_z3 + e_z3.max(1, keepdim=True).values + u * (2 * rng + 3)
        rs = (r * y).sum(1, keepdim=True) + u * S.FC_OUT   # of the sum
        e_y = y * (r + rs + u)
        lab = o["labels"].view(-1, 1)
        # -__logf(y): relative error of y, and the fast log itself, 2^-21.41
        # absolute on [0.5, 2] and 3 ulp of the result elsewhere (the public
        # figures of the intrinsic)
        e_loss_img = (e_y.gather(1, lab) / y.gather(1, lab)).view(-1) \
            + 2.0 ** -21 + 6 * u * o["loss_img"]
    else:
        s3 = sigmoid_allowance(z3.abs().max().item())
        e_y = y * (1 - y) * e_z3 + u * s3 * y
    e_dz = e_y + u * dz.abs()
    if o["loss_mode"] != "softmax_ce":
        nrm = o["loss_img"].clamp_min(1e-300)
        # sqrt(sum d^2): 10 squares, 10 adds, the root
        e_loss_img = (dz.abs() * e_dz).sum(1) / nrm + u * (S.FC_OUT + 3) * nrm
    da = dz @ fw
    e_da = u * S.FC_OUT * (dz.abs() @ fw.abs()) + e_dz @ fw.abs()
    dz2 = o["dz2"]
    e_dz2 = (e_da * a2 * (1 - a2) + da.abs() * e_a2 * (1 - 2 * a2).abs()
             + 3 * u * dz2.abs())
    d2 = dz2.view(B, S.C1_CH, S.S1_H, S.S1_W)
    e_d2 = e_dz2.view(B, S.C1_CH, S.S1_H, S.S1_W)
    if o["pool"] == "max":
        win = _windows(a1)
        idx = win.argmax(-1, keepdim=True)
        da1 = _unwindows(torch.zeros_like(win).scatter_(
            -1, idx, d2.unsqueeze(-1)))
        e_da1 = _unwindows(torch.zeros_like(win).scatter_(
            -1, idx, e_d2.unsqueeze(-1)))
    else:
        tile = s1w.abs().repeat(S.S1_H, S.S1_W)
        up = lambda t: t.repeat_interleave(S.S1_K, 2).repeat_interleave(  # noqa: E731
            S.S1_K, 3)
        da1 = up(d2) * s1w.repeat(S.S1_H, S.S1_W)
        e_da1 = up(e_d2) * tile
    dz1 = o["dz1"].view(B, S.C1_CH, S.C1_H, S.C1_W)
    e_dz1 = (e_da1 * a1 * (1 - a1) + da1.abs() * e_a1 * (1 - 2 * a1).abs()
             + 4 * u * dz1.abs())
    # the B-way atomic sum of the per-image losses
    e_loss = e_loss_img.sum().item() + u * B * abs(o["loss"])
    return {"a1": e_a1.reshape(B, -1), "a2": e_a2, "y": e_y, "dz": e_dz,
            "dz2": e_dz2, "dz1": e_dz1.reshape(B, -1), "loss": e_loss,
            "loss_img": e_loss_img}


def store_bound(e, want, act_dtype):
    """e plus the store into act_dtype: u_out |want| and the format's
    subnormal quantum."""
    return e + U_OUT[act_dtype] * want.abs() + TINY_OUT[act_dtype]


def max_pool_ties(o, e_a1):
    """Number of pool windows whose two largest a1 are closer than the sum
    of their fp32 forward bounds (the argmax is then not decided)."""
    win = _windows(o["a1"])
    ew = _windows(e_a1.view_as(o["a1"]))
    top, idx = win.topk(2, dim=-1)
    gap = top[..., 0] - top[..., 1]
    room = ew.gather(-1, idx).sum(-1)
    return int((gap <= room).sum().item())


def undecided_images(o, e_y):
    """Number of images whose two largest outputs are closer than the sum of
    their forward bounds (the prediction is then not decided)."""
    top, idx = o["y"].topk(2, dim=1)
    room = e_y.gather(1, idx).sum(1)
    return int(((top[:, 0] - top[:, 1]) <= room).sum().item())
