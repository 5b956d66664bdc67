"""float64 oracle of one DeepCNN forward + backward with two rounding hooks.

A float64 copy of deep_ref.forward / deep_ref.backward.  With both hooks the
identity it is the exact chain rule; with `round_operand` = bf16 and
`round_store` = the activation storage dtype it rounds where the gfx950 path
rounds:

  * round_operand: every MFMA operand -- the conv input and weights of the
    forward GEMM, dapre and the weights of the dgrad GEMM, the im2col view and
    dapre of the wgrad GEMM.  (The fc and pool kernels are plain fp32 FMAs and
    read their operands unrounded.)
  * round_store: every tensor the step keeps in activation storage -- the
    staged input, acts, pouts, dapre, dppre and dflat.

The ratio ||g_emul - g_exact|| / ||g_exact|| per parameter block is the error
the number formats alone cause; the GPU tests allow MARGIN times it (the
kernels round accumulate-then-store in their fused epilogues, at slightly
different points than this emulation).  A block whose allowance exceeds
INFORMATIVE cannot tell a right gradient from a zero one.

Test support, kept out of the package.  It lives in tools/ because
tools/fuzz_deep.py applies the same per-block rule and has to run without
the tests/ directory; the tests import it from here.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

MARGIN = 4.0
INFORMATIVE = 0.5
FP16_BLOCK_LIMIT = 0.1      # fp16: blocks whose emulated ratio is above this
                            # are excluded (and the excluded set is asserted)

STORE_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16,
               "fp16": torch.float16}


def identity(t: torch.Tensor) -> torch.Tensor:
    return t


def rounder(dtype):
    def r(t: torch.Tensor) -> torch.Tensor:
        return t.to(dtype).to(torch.float64)
    return r


def hooks_for(act_dtype: str, loss_scale: float = 1.0):
    """(round_operand, round_store) emulating the hip path at act_dtype.
    Loss scaling changes what is stored, not how it is rounded: grads64 takes
    the scale itself, and the hooks are the same at every loss_scale."""
    if not loss_scale >= 1.0:
        raise ValueError(f"loss_scale must be >= 1, got {loss_scale}")
    return rounder(torch.bfloat16), rounder(STORE_DTYPE[act_dtype])


def _view(params, spec, name):
    off, n = spec.offsets[name]
    return params[off:off + n]


def _conv_w_nchw(params, spec, i):
    st = spec.stages[i]
    w = _view(params, spec, f"conv{i}_w").view(st.kcp, st.cout)[:st.kc]
    w = w.view(st.k * st.k, st.cin, st.cout)
    return w.permute(2, 1, 0).reshape(st.cout, st.cin, st.k, st.k)


def _im2col(x_nchw, st):
    B = x_nchw.shape[0]
    u = F.unfold(x_nchw, st.k, padding=st.pad)
    u = u.view(B, st.cin, st.k * st.k, -1)
    u = u.permute(0, 3, 2, 1).reshape(B * st.h * st.w, st.kc)
    cols = torch.zeros(u.shape[0], st.kcp, dtype=u.dtype)
    cols[:, :st.kc] = u
    return cols


def grads64(x_nhwc: torch.Tensor, labels: torch.Tensor, params: torch.Tensor,
            spec, round_operand=identity, round_store=identity,
            loss_scale: float = 1.0):
    """Batch-SUM gradient of the flat parameter vector, float64, plus the
    summed loss.  x_nhwc [B,H,W,Cin], params: the fp32 master parameters.
    loss_scale: dz is multiplied by it ahead of dflat (where k_fc_fwd does),
    every stored backward tensor is rounded at the scaled magnitude, and the
    gradient is divided by it before it is returned; the loss is unscaled."""
    ro, rs = round_operand, round_store
    p = params.detach().cpu().to(torch.float64)
    B = x_nhwc.shape[0]
    stages = spec.stages
    xc = rs(x_nhwc.to(torch.float64)).permute(0, 3, 1, 2).contiguous()
    x0 = xc
    acts, pouts = [], []
    for i, st in enumerate(stages):
        a = rs(torch.sigmoid(
            F.conv2d(ro(xc), ro(_conv_w_nchw(p, spec, i)),
                     _view(p, spec, f"conv{i}_b"), padding=st.pad)))
        K = st.pool_k
        pw = _view(p, spec, f"pool{i}_w").view(1, 1, K, K).expand(
            st.cout, 1, K, K)
        po = rs(torch.sigmoid(
            F.conv2d(a, pw, _view(p, spec, f"pool{i}_b").expand(st.cout),
                     stride=K, groups=st.cout)))
        acts.append(a)
        pouts.append(po)
        xc = po
    flat = pouts[-1].permute(0, 2, 3, 1).reshape(B, spec.fc_in)
    fw = _view(p, spec, "fc_w").view(spec.n_classes, spec.fc_in)
    y = torch.sigmoid(F.linear(flat, fw, _view(p, spec, "fc_b")))

    g = torch.zeros(spec.n_params, dtype=torch.float64)

    def gv(name):
        return _view(g, spec, name)

    dz = F.one_hot(labels.to(torch.int64), spec.n_classes).to(
        torch.float64) - y
    loss = dz.norm(dim=1).sum().item()
    dz = dz * loss_scale
    gv("fc_w").add_(torch.einsum("bk,bm->km", dz, flat).reshape(-1))
    gv("fc_b").add_(dz.sum(0))
    dflat = rs((dz @ fw) * flat * (1 - flat))
    last = stages[-1]
    dppre = dflat.view(B, last.oh, last.ow, last.cout).permute(
        0, 3, 1, 2).contiguous()
    for i in range(len(stages) - 1, -1, -1):
        st = stages[i]
        a = acts[i]
        K = st.pool_k
        pw = _view(p, spec, f"pool{i}_w").view(K, K)
        aw = a.view(B, st.cout, st.oh, K, st.ow, K)
        gv(f"pool{i}_w").add_(
            torch.einsum("bcpq,bcpiqj->ij", dppre, aw).reshape(-1))
        gv(f"pool{i}_b").add_(dppre.sum().reshape(1))
        up = dppre.repeat_interleave(K, dim=2).repeat_interleave(K, dim=3)
        dapre = rs(up * pw.repeat(st.h // K, st.w // K) * a * (1 - a))
        x_in = x0 if i == 0 else pouts[i - 1]
        cols = _im2col(ro(x_in), st)
        dapre_f = dapre.permute(0, 2, 3, 1).reshape(-1, st.cout)
        gv(f"conv{i}_w").add_((cols.T @ ro(dapre_f)).reshape(-1))
        gv(f"conv{i}_b").add_(dapre_f.sum(0))
        if i > 0:
            w = _view(p, spec, f"conv{i}_w").view(st.kcp, st.cout)
            dcols = ro(dapre_f) @ ro(w).T
            dcols_u = dcols[:, :st.kc].view(
                B, st.h * st.w, st.k * st.k, st.cin).permute(0, 3, 2, 1)
            dx = F.fold(dcols_u.reshape(B, st.cin * st.k * st.k, -1),
                        (st.h, st.w), st.k, padding=st.pad)
            pprev = pouts[i - 1]
            dppre = rs(dx * pprev * (1 - pprev))
    if loss_scale != 1.0:
        g /= loss_scale
    return g, loss


def block_ratios(got: torch.Tensor, want: torch.Tensor, spec):
    """{block: ||got - want|| / ||want||} over spec.offsets (float64)."""
    out = {}
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    for name, (off, n) in spec.offsets.items():
        w = want[off:off + n]
        out[name] = ((got[off:off + n] - w).norm() /
                     w.norm().clamp_min(1e-300)).item()
    return out


def oracle_pair(x_nhwc, labels, params, spec, act_dtype: str,
                loss_scale: float = 1.0):
    """(g_exact, loss_exact, emulated ratio per block) for one batch; the
    emulation runs at loss_scale, the exact chain rule needs none."""
    g_exact, loss = grads64(x_nhwc, labels, params, spec)
    ro, rs = hooks_for(act_dtype, loss_scale)
    g_emul, _ = grads64(x_nhwc, labels, params, spec, ro, rs,
                        loss_scale=loss_scale)
    return g_exact, loss, block_ratios(g_emul, g_exact, spec)


def block_tolerances(emul: dict, act_dtype: str):
    """Per-block tolerance MARGIN * emulated ratio, and the blocks excluded
    from the check.  Only fp16 storage may exclude blocks (its stage-0
    pool-preact gradients underflow); elsewhere an uninformative block is an
    error, never a silent pass."""
    tol = {k: MARGIN * v for k, v in emul.items()}
    if act_dtype == "fp16":
        excluded = {k for k, v in emul.items() if v >= FP16_BLOCK_LIMIT}
    else:
        excluded = set()
    for k, t in tol.items():
        if k not in excluded and t > INFORMATIVE:
            raise AssertionError(
                f"block {k}: allowance {t:.3g} > {INFORMATIVE} is "
                f"uninformative at act_dtype={act_dtype}")
    return tol, excluded


def compare_blocks(what, got, want, emul, act_dtype, spec, floor=None,
                   log=print):
    """Per-block ||got - want|| <= tol_block * ||want|| (+ floor[block]).
    Prints the emulated and the measured ratio of every block and returns
    (failures, excluded)."""
    tol, excluded = block_tolerances(emul, act_dtype)
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    fails = []
    for name, (off, n) in spec.offsets.items():
        w = want[off:off + n]
        err = (got[off:off + n] - w).norm().item()
        ref = w.norm().item()
        fl = floor[name] if floor is not None else 0.0
        meas = err / max(ref, 1e-300)
        skip = name in excluded
        log(f"BLOCK {what} {name}: emulated {emul[name]:.2e} measured "
            f"{meas:.2e} tol {tol[name]:.2e}"
            + (f" floor/ref {fl / max(ref, 1e-300):.2e}" if fl else "")
            + (" (excluded)" if skip else ""))
        if not skip and not err <= tol[name] * ref + fl:
            fails.append(f"{name}: {meas:.3e} > {tol[name]:.3e}")
    return fails, excluded


def step_delta_floor(p_after: torch.Tensor, dp_ref: torch.Tensor, spec):
    """The parameters are fp32: p_after = fl(p0 + dp) carries up to half an
    ulp of the PARAMETER per element (2^-24 |p|), which for the early conv
    blocks is as large as the whole one-step move.  That quantum -- a
    property of the number format, not of any kernel -- is allowed on top of
    the per-block tolerance when deltas (not gradients) are compared."""
    u = 2.0 ** -24
    e = u * (p_after.detach().cpu().to(torch.float64).abs() + dp_ref.abs())
    return {name: e[off:off + n].norm().item()
            for name, (off, n) in spec.offsets.items()}
