"""Every DeepCNN launcher on its own against float64.

Pattern of each case: draw asymmetric random inputs on the host, round them
to the dtype the kernel reads from memory, upload, call the `_C.deep_*`
binding once, and compare with the same operation in float64 computed from
the rounded values.  The MFMA kernels cast every operand to bf16 while
staging, so the reference applies the same cast (`mf`) to the stored values;
what is left between kernel and reference is accumulation order and the
rounding of the output, and the bounds below are derived from that alone:

  dot product of length K, fp32 accumulation:
      |got - want| <= (K + 8) * 2^-24 * (|A| @ |B|) + u_out * |want|
  sigmoid epilogue: the pre-activation bound shrinks by sigmoid' <= 1/4, plus
      4 x the largest float32-vs-float64 torch.sigmoid difference at the same
      pre-activations after output rounding
  layout kernels: bit-equal.

Each check prints `RATIO <name> <worst error / bound>`.
"""
import pytest
import torch
import torch.nn.functional as F

from parallel_cnn_amd import _C
from parallel_cnn_amd.engine.deep import DeepWorkspace
from parallel_cnn_amd.ops import deep_ref, native

pytestmark = pytest.mark.gpu

ACTS = ["fp32", "bf16", "fp16"]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# unit roundoff of a round-to-nearest store, 2^-p for p significand bits
# (24 / 8 / 11).  The issue that asked for these tests wrote 2^-9 and 2^-12
# for bf16 and fp16; those are half the unit roundoff, and a correctly
# rounding kernel misses them by up to 2x (measured 1.98 on the first bf16
# store checked): 1 + 2^-8 lies midway between the bf16 neighbours 1 and
# 1 + 2^-7.
U_OUT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
# half of the smallest subnormal: the absolute rounding floor of a store
TINY = {"fp32": 2.0 ** -150, "bf16": 2.0 ** -134, "fp16": 2.0 ** -25}
U32 = 2.0 ** -24
BF = torch.bfloat16


def sh():
    return native.current_stream_handle()


def f64(t):
    return t.detach().cpu().to(torch.float64)


def mf(t):
    """The value an MFMA sees: the stored value cast to bf16."""
    return t.detach().cpu().to(BF).to(torch.float64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def draw(g, *shape, lo=-1.0, hi=1.0):
    """Asymmetric uniform draw (mean != 0, so a sign or transposition
    mistake cannot cancel)."""
    return torch.rand(*shape, generator=g) * (hi - lo) + lo + 0.25 * (hi - lo)


def store_bound(want, act):
    return U_OUT[act] * want.abs() + TINY[act]


def sig_term(z, act):
    """4 x the largest float32-vs-float64 torch.sigmoid difference at the
    pre-activations z, pushed through the output rounding."""
    s32 = torch.sigmoid(z.float()).to(DT[act]).to(torch.float64)
    s64 = torch.sigmoid(z).to(DT[act]).to(torch.float64)
    return 4.0 * (s32 - s64).abs().max().item()


def sig_bound(z, pre_bound, act):
    return 0.25 * pre_bound + store_bound(torch.sigmoid(z), act) + \
        sig_term(z, act)


def check(name, got, want, bound):
    got, want, bound = f64(got), f64(want), f64(bound)
    assert got.shape == want.shape == bound.shape, \
        (name, got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    assert (bound > 0).all(), f"{name}: bound must be positive"
    ratio = ((got - want).abs() / bound).max().item()
    print(f"RATIO {name} {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error / bound = {ratio:.3f}"
    return ratio


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_bits(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = int((bits(got) != bits(want)).sum())
    print(f"RATIO {name} bit-equal ({bad} mismatches)")
    assert bad == 0, f"{name}: {bad} elements differ bitwise"


EMPTY = torch.empty(0)


def gemm(device, A, Bsrc, bias, C, M, K, N, ldA, ldC, b_kxn, epilogue, **kw):
    _C.deep_gemm(A, Bsrc, bias if bias is not None else EMPTY, C, M, K, N,
                 ldA, ldC, b_kxn, epilogue, sh(), **kw)
    torch.cuda.synchronize()


def dot_bound(Aabs, Babs, K):
    return (K + 8) * U32 * (Aabs @ Babs)


# ---------------------------------------------------------------- deep_gemm
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,K,N,ldC,b_kxn,bpre,epilogue", [
    (200, 32, 16, 24, 1, False, 0),
    (200, 32, 16, 24, 0, True, 0),
    (200, 96, 48, 56, 0, False, 1),
    (200, 96, 48, 56, 1, True, 1),
    (128, 160, 64, 72, 1, False, 1),
    (128, 160, 48, 48, 0, True, 2),
])
def test_gemm_main(act, M, K, N, ldC, b_kxn, bpre, epilogue, device):
    """k_gemm: M tail, N tails with ldC > N, K that is no multiple of 64,
    both Bsrc layouts and the pre-cast image, epilogues 0/1/2."""
    g = gen(M + K + N + b_kxn)
    A = draw(g, M, K).to(DT[act])
    Bkn = draw(g, K, N, lo=-0.5, hi=0.5)            # logical [K][N]
    bias = draw(g, N)
    E = torch.sigmoid(draw(g, M, ldC)).to(DT[act])
    Bsrc = (Bkn if b_kxn else Bkn.T.contiguous())
    Bpre = Bkn.T.contiguous().to(BF).to(device) if bpre else EMPTY
    C = torch.full((M, ldC), -7.0, dtype=DT[act], device=device)
    gemm(device, A.to(device), Bsrc.to(device), bias.to(device), C, M, K, N,
         K, ldC, b_kxn, epilogue, Bpre=Bpre,
         epi=E.to(device) if epilogue == 2 else EMPTY)
    z = mf(A) @ mf(Bkn)
    pre = dot_bound(mf(A).abs(), mf(Bkn).abs(), K)
    if epilogue == 1:
        z = z + f64(bias)
        want, bound = torch.sigmoid(z), sig_bound(z, pre + U32 * z.abs(), act)
    elif epilogue == 2:
        e = f64(E)[:, :N]
        f = e * (1 - e)
        want = z * f
        bound = pre * f + 4 * U32 * want.abs() + store_bound(want, act)
    else:
        want, bound = z, pre + store_bound(z, act)
    check(f"gemm_main[{act},{M}x{K}x{N},kxn{b_kxn},bpre{int(bpre)},"
          f"e{epilogue}]", C[:, :N], want, bound)
    # columns past N belong to the caller
    assert (f64(C[:, N:]) == -7.0).all()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("epilogue", [0, 1])
def test_gemm_smallk(act, epilogue, device):
    """k_gemm_smallk at every K/N/M it accepts, against float64 and against
    the main kernel on the same data (Bsrc route: same bf16 values)."""
    worst = 0.0
    for K in (32, 96, 128):
        for N in (16, 64):
            for M in (64, 192):
                g = gen(K * 7 + N * 3 + M)
                A = draw(g, M, K).to(DT[act])
                Bnk = draw(g, N, K, lo=-0.5, hi=0.5).to(BF)
                bias = draw(g, N)
                Cs = torch.zeros(M, N, dtype=DT[act], device=device)
                Cm = torch.zeros(M, N, dtype=DT[act], device=device)
                Bf = Bnk.float().to(device)
                gemm(device, A.to(device), Bf, bias.to(device), Cs, M, K, N,
                     K, N, 0, epilogue, Bpre=Bnk.to(device))
                gemm(device, A.to(device), Bf, bias.to(device), Cm, M, K, N,
                     K, N, 0, epilogue)
                z = mf(A) @ f64(Bnk).T
                pre = dot_bound(mf(A).abs(), f64(Bnk).T.abs(), K)
                if epilogue == 1:
                    z = z + f64(bias)
                    want = torch.sigmoid(z)
                    bound = sig_bound(z, pre + U32 * z.abs(), act)
                else:
                    want, bound = z, pre + store_bound(z, act)
                tag = f"[{act},{M}x{K}x{N},e{epilogue}]"
                worst = max(worst,
                            check("gemm_smallk" + tag, Cs, want, bound),
                            check("gemm_smallk_vs_main" + tag, Cs, Cm,
                                  2 * bound))
    print(f"RATIO gemm_smallk_worst[{act},e{epilogue}] {worst:.3f}")


def pool_ref64(C_nhwc, pw, K):
    """deep_ref.pool_fwd_ref in float64 on an NHWC tensor -> (preact, out),
    both NHWC."""
    a = C_nhwc.permute(0, 3, 1, 2).contiguous()
    ch = a.shape[1]
    want = deep_ref.pool_fwd_ref(a, pw[:K * K], pw[K * K:], K)
    w = pw[:K * K].view(1, 1, K, K).expand(ch, 1, K, K)
    z = F.conv2d(a, w, pw[K * K:].expand(ch), stride=K, groups=ch)
    return z.permute(0, 2, 3, 1).contiguous(), \
        want.permute(0, 2, 3, 1).contiguous()


def pool_abs(Cabs_nhwc, pw, K):
    a = Cabs_nhwc.permute(0, 3, 1, 2).contiguous()
    ch = a.shape[1]
    w = pw[:K * K].abs().view(1, 1, K, K).expand(ch, 1, K, K)
    return F.conv2d(a, w, None, stride=K, groups=ch).permute(0, 2, 3, 1)


def fused_pool_case(device, act, XW, N, M, K, smallk, c32=None, tag=""):
    PK = 2
    XH = {8: 8, 16: 4, 32: 2}[XW]
    B = M // (XH * XW)
    g = gen(XW + N + M + K)
    A = draw(g, M, K).to(DT[act])
    Bnk = draw(g, N, K, lo=-0.3, hi=0.3).to(BF)
    bias = draw(g, N)
    pw = draw(g, PK * PK + 1)
    C = torch.zeros(M, N, dtype=DT[act], device=device)
    pout = torch.zeros(M // 4, N, dtype=DT[act], device=device)
    pout2 = torch.zeros_like(pout)
    kw = dict(pw=pw.to(device), pout=pout, PK=PK, XH=XH, XW=XW)
    if smallk:
        kw["Bpre"] = Bnk.to(device)
    if c32 is not None:
        kw["c32"] = c32
    gemm(device, A.to(device), Bnk.float().to(device), bias.to(device), C, M,
         K, N, K, N, 0, 3, **kw)
    _C.deep_pool_fwd(C, pw.to(device), pout2, B, XH, XW, N, PK, sh())
    torch.cuda.synchronize()
    z = mf(A) @ f64(Bnk).T + f64(bias)
    pre = dot_bound(mf(A).abs(), f64(Bnk).T.abs(), K) + U32 * z.abs()
    name = f"[{act},XW{XW},N{N},M{M}{tag}]"
    r = check("epi3_C" + name, C, torch.sigmoid(z), sig_bound(z, pre, act))
    # pool of the ROUNDED tile.  The fused epilogue pools the fp32 values
    # it holds before they are rounded to storage, so its pre-activation
    # may differ from the reference's by sum |pw| * u_out * |C|.
    Cst = f64(C).view(B, XH, XW, N)
    pw64 = f64(pw)
    pz, pwant = pool_ref64(Cst, pw64, PK)
    mag = pool_abs(Cst.abs(), pw64, PK) + pw64[PK * PK].abs()
    acc = (PK * PK + 8) * U32 * mag
    fused = acc + U_OUT[act] * pool_abs(Cst.abs(), pw64, PK)
    pwant = pwant.reshape(M // 4, N)
    r = max(r, check("epi3_pout" + name, pout, pwant,
                     sig_bound(pz, fused, act).reshape(M // 4, N)))
    r = max(r, check("pool_fwd" + name, pout2, pwant,
                     sig_bound(pz, acc, act).reshape(M // 4, N)))
    return r


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("smallk", [False, True])
def test_gemm_fused_pool(act, smallk, device):
    """Epilogue 3 in k_gemm (K = 160) and in k_gemm_smallk (K = 96): the
    sigmoid tile, the fused pool output and the standalone pool kernel."""
    worst = 0.0
    for XW in (8, 16, 32):
        for N in (16, 64):
            for M in (64, 192):
                worst = max(worst, fused_pool_case(
                    device, act, XW, N, M, 96 if smallk else 160, smallk,
                    tag=",smallk" if smallk else ""))
    print(f"RATIO gemm_fused_pool_worst[{act},smallk{int(smallk)}] "
          f"{worst:.3f}")


@pytest.mark.parametrize("act", ACTS)
def test_gemm_fused_pool_n48_runs_unsplit(act, device):
    """N = 48 fails the combine kernel's window alignment: with scratch on
    offer the launcher must run the fused epilogue unsplit."""
    c32 = torch.full((8 * 192 * 48,), float("nan"), device=device)
    fused_pool_case(device, act, 16, 48, 192, 160, False, c32=c32,
                    tag=",c32")
    assert torch.isnan(c32).all(), "split scratch was written"


@pytest.mark.parametrize("XW,M,N", [(24, 192, 16), (8, 96, 16),
                                    (8, 64, 128)])
def test_gemm_fused_pool_refusals(XW, M, N, device):
    """Shapes the fused pool cannot tile are refused, not launched."""
    K = 160
    A = torch.zeros(M, K, dtype=BF, device=device)
    W = torch.zeros(N, K, device=device)
    C = torch.full((M, N), 3.0, dtype=BF, device=device)
    pout = torch.full((M // 4, N), 3.0, dtype=BF, device=device)
    with pytest.raises(RuntimeError):
        _C.deep_gemm(A, W, torch.zeros(N, device=device), C, M, K, N, K, N,
                     0, 3, sh(), pw=torch.zeros(5, device=device), pout=pout,
                     PK=2, XH=8, XW=XW)
    torch.cuda.synchronize()
    assert (C.float() == 3.0).all() and (pout.float() == 3.0).all()


# ------------------------------------------------------------------ split-K
def launcher_split(M, N, K):
    """(ks_eff, slab elements) of pcnn_deep_gemm's split policy."""
    need = DeepWorkspace.split_need(M, N, K)
    return need // (M * N), need


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K,epilogue", [(128, 64, 800, 1),
                                            (8192, 128, 224, 2)])
def test_gemm_split_k(act, M, N, K, epilogue, device):
    """Split-K + k_split_epi with the scratch sized as the workspace sizes
    it; the second shape has ks_eff < ks after the tiles-per-chunk rounding
    (ks = 5, 7 K-tiles -> 4 chunks).  One element less and the launcher must
    take the plain path.  The split result is bitwise reproducible."""
    ks_eff, need = launcher_split(M, N, K)
    mn = ((M + 63) // 64) * ((N + 63) // 64)
    ktiles = (K + 31) // 32
    assert ks_eff > 1
    if M == 8192:
        assert ks_eff < min(ktiles, 1024 // mn + 1)
    g = gen(M + N + K)
    A = draw(g, M, K).to(DT[act])
    Bnk = draw(g, N, K, lo=-0.3, hi=0.3).to(BF)
    bias = draw(g, N)
    E = torch.sigmoid(draw(g, M, N)).to(DT[act])
    z = mf(A) @ f64(Bnk).T
    pre = dot_bound(mf(A).abs(), f64(Bnk).T.abs(), K)
    if epilogue == 1:
        z = z + f64(bias)
        want, bound = torch.sigmoid(z), sig_bound(z, pre + U32 * z.abs(), act)
    else:
        f = f64(E) * (1 - f64(E))
        want = z * f
        bound = pre * f + 4 * U32 * want.abs() + store_bound(want, act)

    def run(cap):
        c32 = torch.full((cap,), float("nan"), device=device)
        C = torch.zeros(M, N, dtype=DT[act], device=device)
        gemm(device, A.to(device), Bnk.float().to(device), bias.to(device),
             C, M, K, N, K, N, 0, epilogue, Bpre=Bnk.to(device),
             epi=E.to(device) if epilogue == 2 else EMPTY, c32=c32)
        return C, c32

    tag = f"[{act},{M}x{K}x{N},e{epilogue}]"
    C1, s1 = run(need + 64)
    assert torch.isfinite(s1[:need]).all(), "the split path did not run"
    assert torch.isnan(s1[need:]).all(), "wrote past ks_eff slabs"
    check("gemm_split" + tag, C1, want, bound)
    C2, _ = run(need + 64)
    check_bits("gemm_split_rerun" + tag, C2, C1)
    C3, s3 = run(need - 1)
    assert torch.isnan(s3).all(), "split ran on a scratch that is too small"
    check("gemm_split_fallback" + tag, C3, want, bound)


# ------------------------------------------------------- weight image casts
def make_conv_w(g, K, Cin, Cout):
    """fp32 master [KcP][Cout] (pad rows zero) and its NCHW form as
    deep_ref.conv_weight_nchw lays it out: w[co][ci][i][j] =
    W[(i*K+j)*Cin+ci][co]."""
    kc = K * K * Cin
    kcp = (kc + 31) // 32 * 32
    w_nchw = draw(g, Cout, Cin, K, K, lo=-0.2, hi=0.2)
    W = torch.zeros(kcp, Cout)
    W[:kc] = w_nchw.permute(2, 3, 1, 0).reshape(kc, Cout)
    return W, w_nchw, kc, kcp


def cast_all(device, stages, g):
    """stages: [(K, Cin, Cout, want_p8)].  Returns per stage a dict with the
    master W, w_nchw and the four device images."""
    out, params, d = [], [], {k: [] for k in (
        "R", "C", "K", "Cin", "w_off", "bf_off", "bfT_off", "rot_off",
        "p8_off")}
    poff = off = 0
    for K, Cin, Cout, p8 in stages:
        W, w_nchw, kc, kcp = make_conv_w(g, K, Cin, Cout)
        d["R"].append(kcp); d["C"].append(Cout); d["K"].append(K)
        d["Cin"].append(Cin); d["w_off"].append(poff)
        poff += kcp * Cout + 5            # a gap, as biases sit between
        params += [W.reshape(-1), draw(g, 5)]
        sizes = [kcp * Cout, Cout * kcp, Cin * K * K * Cout,
                 Cout * K * K * 8 if p8 else 0]
        offs = []
        for n in sizes:
            offs.append(off)
            off += n
        d["bf_off"].append(offs[0]); d["bfT_off"].append(offs[1])
        d["rot_off"].append(offs[2]); d["p8_off"].append(offs[3] if p8 else -1)
        out.append(dict(W=W, w=w_nchw, kc=kc, kcp=kcp, K=K, Cin=Cin,
                        Cout=Cout, offs=offs, sizes=sizes))
    params = torch.cat(params).to(device)
    wbuf = torch.zeros(off, dtype=BF, device=device)
    _C.deep_cast_all(params, wbuf, d["R"], d["C"], d["K"], d["Cin"],
                     d["w_off"], d["bf_off"], d["bfT_off"], d["rot_off"],
                     d["p8_off"], sh())
    torch.cuda.synchronize()
    for s in out:
        for name, o, n in zip(("wbf", "wbfT", "wrot", "wp8"), s["offs"],
                              s["sizes"]):
            s[name] = wbuf[o:o + n] if n else None
    return out


def test_cast_all_images(device):
    """wbf / wbfT / wrot / wp8 bit-equal to bf16 casts of index formulas
    written from the NCHW weight layout; pad rows of wbf exactly zero."""
    sts = cast_all(device, [(5, 3, 16, True), (3, 16, 32, False)], gen(5))
    for i, s in enumerate(sts):
        K, Cin, Cout, kc, kcp, w = (s["K"], s["Cin"], s["Cout"], s["kc"],
                                    s["kcp"], s["w"])
        wT = torch.zeros(Cout, kcp)
        wT[:, :kc] = w.permute(0, 2, 3, 1).reshape(Cout, kc)  # (i,j,ci)
        check_bits(f"cast_wbfT[{i}]", s["wbfT"].view(Cout, kcp), wT.to(BF))
        check_bits(f"cast_wbf[{i}]", s["wbf"].view(kcp, Cout),
                   wT.T.contiguous().to(BF))
        assert (s["wbf"].view(kcp, Cout)[kc:].float() == 0).all()
        # wrot[ci][(i'*K+j')*Cout+co] = w[co][ci][K-1-i'][K-1-j']
        rot = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, K * K * Cout)
        check_bits(f"cast_wrot[{i}]", s["wrot"].view(Cin, -1), rot.to(BF))
        if s["wp8"] is not None:
            p8 = torch.zeros(Cout, K, K, 8)
            p8[..., :Cin] = w.permute(0, 2, 3, 1)
            check_bits(f"cast_wp8[{i}]", s["wp8"].view(Cout, K * K * 8),
                       p8.reshape(Cout, -1).to(BF))


def test_cast_wt(device):
    R, C = 96, 48
    W = draw(gen(9), R, C)
    out = torch.zeros(R, C, dtype=BF, device=device)
    outT = torch.zeros(C, R, dtype=BF, device=device)
    _C.deep_cast_wt(W.to(device), out, outT, R, C, sh())
    torch.cuda.synchronize()
    check_bits("cast_wt", out, W.to(BF))
    check_bits("cast_wt_T", outT, W.T.contiguous().to(BF))


# ----------------------------------------------------------- layout kernels
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin,H,W", [(3, 8, 8), (3, 4, 16), (8, 4, 16)])
def test_im2col_bit_equal(act, Cin, H, W, device):
    B, K, P = 3, 5, 2
    kc = K * K * Cin
    kcp = (kc + 31) // 32 * 32
    x = draw(gen(Cin + H), B, H, W, Cin).to(DT[act])
    cols = torch.full((B * H * W, kcp), 9.0, dtype=DT[act], device=device)
    _C.deep_im2col(x.to(device), cols, B, H, W, Cin, K, P, kcp, sh())
    torch.cuda.synchronize()
    u = F.unfold(x.double().permute(0, 3, 1, 2), K, padding=P)
    u = u.view(B, Cin, K * K, -1).permute(0, 3, 2, 1).reshape(-1, kc)
    want = torch.zeros(B * H * W, kcp, dtype=torch.float64)
    want[:, :kc] = u
    check_bits(f"im2col[{act},Cin{Cin},{H}x{W}]", cols, want.to(DT[act]))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin", [1, 3, 8])
def test_pad_channels_bit_equal(act, Cin, device):
    npix = 300
    x = draw(gen(Cin), npix, Cin).to(DT[act])
    x8 = torch.full((npix, 8), 9.0, dtype=DT[act], device=device)
    _C.deep_pad_channels(x.to(device), x8, npix, Cin, sh())
    torch.cuda.synchronize()
    want = torch.zeros(npix, 8, dtype=DT[act])
    want[:, :Cin] = x
    check_bits(f"pad_channels[{act},Cin{Cin}]", x8, want)


def test_remap_dw8_exact_inverse(device):
    """dW[(p*Cin+ci)][c] += dW8[(p*8+ci)][c]; the consumed entries are
    zeroed, the pad rows (ci >= Cin) are left alone."""
    KK, Cin, Cout = 25, 3, 16
    g = gen(3)
    dW8 = draw(g, KK, 8, Cout)
    dW0 = draw(g, KK, Cin, Cout)
    d8 = dW8.clone().to(device)
    dW = dW0.clone().to(device)
    _C.deep_remap_dw8(d8, dW, KK, Cin, Cout, sh())
    torch.cuda.synchronize()
    check_bits("remap_dw8", dW, dW0 + dW8[:, :Cin])
    left = dW8.clone()
    left[:, :Cin] = 0
    check_bits("remap_dw8_src", d8, left)


# ------------------------------------------------- implicit-im2col forward
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("H,W", [(8, 8), (4, 16)])
@pytest.mark.parametrize("B", [1, 3])
def test_gemm_implicit_forward(act, Cin, H, W, B, device):
    """The implicit gather (clamp + select) against float64 F.conv2d; the
    outermost two rings are asserted on their own."""
    K, P, Cout = 5, 2, 32
    g = gen(Cin + H + B)
    s = cast_all(device, [(K, Cin, Cout, False)], g)[0]
    x = draw(g, B, H, W, Cin).to(DT[act])
    bias = draw(g, Cout)
    M = B * H * W
    C = torch.zeros(M, Cout, dtype=DT[act], device=device)
    xd = x.to(device)
    gemm(device, xd, s["W"].to(device), bias.to(device), C, M, s["kcp"],
         Cout, s["kcp"], Cout, 1, 1, Bpre=s["wbfT"], imx=xd, XH=H, XW=W,
         XC=Cin, XK=K, XP=P)
    xn = mf(x).permute(0, 3, 1, 2)
    wq = mf(s["w"])
    z = F.conv2d(xn, wq, f64(bias), padding=P)
    mag = F.conv2d(xn.abs(), wq.abs(), None, padding=P)
    pre = (s["kc"] + 8) * U32 * mag + U32 * z.abs()
    want = torch.sigmoid(z).permute(0, 2, 3, 1)
    bound = sig_bound(z, pre, act).permute(0, 2, 3, 1)
    got = f64(C).view(B, H, W, Cout)
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[2:H - 2, 2:W - 2] = False
    tag = f"[{act},Cin{Cin},{H}x{W},B{B}]"
    check("implicit_fwd_border" + tag, got[:, ring], want[:, ring],
          bound[:, ring])
    if (~ring).any():
        check("implicit_fwd_inner" + tag, got[:, ~ring], want[:, ~ring],
              bound[:, ~ring])


# ------------------------------------------------------------ dgrad-as-conv
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin", [16, 32])
def test_gemm_dgrad_as_conv(act, Cin, device):
    """Epilogue 2 over the rotated weight image against float64 F.fold of
    dapre @ W^T times p(1-p); the materialized pair (GEMM over wbf +
    col2im_sigbwd) on the same data agrees within the two bounds."""
    K, P, Cout, H, W, B = 5, 2, 16, 8, 8, 2
    g = gen(Cin)
    s = cast_all(device, [(K, Cin, Cout, False)], g)[0]
    M, kd, kcp, kc = B * H * W, K * K * Cout, s["kcp"], s["kc"]
    dapre = draw(g, M, Cout, lo=-0.1, hi=0.1).to(DT[act])
    pprev = torch.sigmoid(draw(g, M, Cin)).to(DT[act])
    Wd = s["W"].to(device)
    dd, pd = dapre.to(device), pprev.to(device)
    out = torch.zeros(M, Cin, dtype=DT[act], device=device)
    gemm(device, dd, Wd, None, out, M, kd, Cin, kd, Cin, 0, 2, Bpre=s["wrot"],
         imx=dd, XH=H, XW=W, XC=Cout, XK=K, XP=P, epi=pd)

    def fold(dcols):
        u = dcols[:, :kc].view(B, H * W, K * K, Cin).permute(0, 3, 2, 1)
        dx = F.fold(u.reshape(B, Cin * K * K, -1), (H, W), K, padding=P)
        return dx.permute(0, 2, 3, 1).reshape(M, Cin)

    Wq = mf(s["W"])
    dcols = mf(dapre) @ Wq.T
    mag = mf(dapre).abs() @ Wq.T.abs()
    f = f64(pprev) * (1 - f64(pprev))
    want = fold(dcols) * f
    b1 = (kd + 8) * U32 * fold(mag) * f + 4 * U32 * want.abs() + \
        store_bound(want, act)
    tag = f"[{act},Cin{Cin}]"
    check("dgrad_as_conv" + tag, out, want, b1)

    cols = torch.zeros(M, kcp, dtype=DT[act], device=device)
    out2 = torch.zeros(M, Cin, dtype=DT[act], device=device)
    gemm(device, dd, Wd, None, cols, M, Cout, kcp, Cout, kcp, 0, 0,
         Bpre=s["wbf"])
    _C.deep_col2im_sigbwd(cols, pd, out2, B, H, W, Cin, K, P, kcp, sh())
    torch.cuda.synchronize()
    # route 2 rounds dcols to storage before the fold
    bcols = (Cout + 8) * U32 * mag + store_bound(dcols, act)
    check("dgrad_cols" + tag, cols, dcols, bcols)
    b2 = (fold(bcols) + (K * K + 8) * U32 * fold(dcols.abs())) * f + \
        4 * U32 * want.abs() + store_bound(want, act)
    check("dgrad_col2im" + tag, out2, want, b2)
    check("dgrad_routes_agree" + tag, out, out2, b1 + b2)


# --------------------------------------------------------------- conv wgrad
def wgrad_inputs(g, act, src, Cin, H, W, B, M, N):
    """(device A tensor, float64 cols as the MFMA sees them, kc, kcp, geom)"""
    K, P = 5, 2
    kc = K * K * Cin
    kcp = (kc + 31) // 32 * 32
    if src == "imp":
        x = draw(g, B, H, W, Cin).to(DT[act])
        u = F.unfold(mf(x).permute(0, 3, 1, 2), K, padding=P)
        u = u.view(B, Cin, K * K, -1).permute(0, 3, 2, 1).reshape(M, kc)
        cols = torch.zeros(M, kcp, dtype=torch.float64)
        cols[:, :kc] = u
        return x, cols, kc, kcp, dict(XH=H, XW=W, XC=Cin, XK=K, XP=P)
    c = draw(g, M, kcp).to(DT[act])
    c[:, kc:] = 0
    return c, mf(c), kc, kcp, {}


WG_CASES = [
    # src, Cin, (H, W, B), N, MS, slab, db
    ("mat", 3, (8, 8, 2), 16, 1, False, True),
    ("mat", 3, (10, 10, 2), 48, 3, True, False),
    ("mat", 3, (10, 10, 2), 64, 3, False, False),
    ("imp", 16, (10, 10, 2), 64, 3, False, True),
    ("imp", 16, (8, 8, 2), 48, 1, True, True),
    ("imp", 16, (10, 10, 2), 16, 3, True, False),
]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("src,Cin,geom,N,MS,slab,with_db", WG_CASES)
def test_wgrad_gemm(act, src, Cin, geom, N, MS, slab, with_db, device):
    """k_wgrad_gemm (+ k_wsum): KcP 96 and 416, uneven M-slices with a
    partial last tile (M = 200, MS = 3), slab and atomic combine, fused bias
    column sums; accumulation into a non-zero bucket, pad rows untouched."""
    H, W, B = geom
    M = B * H * W
    g = gen(Cin + N + MS + M)
    a, cols, kc, kcp, gk = wgrad_inputs(g, act, src, Cin, H, W, B, M, N)
    dpre = draw(g, M, N, lo=-0.1, hi=0.1).to(DT[act])
    dW0, db0 = draw(g, kcp, N), draw(g, N)
    ad, dd = a.to(device), dpre.to(device)

    def run():
        dW, db = dW0.clone().to(device), db0.clone().to(device)
        part = (torch.full((MS * kcp * N,), float("nan"), device=device)
                if slab else EMPTY)
        _C.deep_wgrad_gemm(ad, dd, dW, M, kcp, N, MS, sh(),
                           imx=ad if src == "imp" else EMPTY, part=part,
                           db=db if with_db else EMPTY, **gk)
        torch.cuda.synchronize()
        return dW, db

    dW, db = run()
    want = cols.T @ mf(dpre)
    mag = cols.T.abs() @ mf(dpre).abs()
    inc = f64(dW) - f64(dW0)
    # M-long dot + MS combines + the add into the bucket
    bound = (M + 8) * U32 * mag + (MS + 2) * U32 * (f64(dW0).abs() + mag)
    tag = f"[{act},{src},KcP{kcp},N{N},MS{MS},slab{int(slab)}]"
    check("wgrad_dW" + tag, inc, want, bound)
    check_bits("wgrad_pad_rows" + tag, dW[kc:], dW0[kc:])
    if with_db:
        wdb = f64(dpre).sum(0)
        bdb = (M + MS + 10) * U32 * (f64(dpre).abs().sum(0) + f64(db0).abs())
        check("wgrad_db" + tag, f64(db) - f64(db0), wdb, bdb)
    else:
        check_bits("wgrad_db_untouched" + tag, db, db0)
    if slab:
        dW2, _ = run()
        check_bits("wgrad_slab_rerun" + tag, dW2, dW)


@pytest.mark.parametrize("act", ACTS)
def test_wgrad_multi_equals_singles(act, device):
    """Three stages of different shapes in one k_wgrad_multi launch (one
    materialized, two implicit) equal three deep_wgrad_gemm calls: bitwise
    at MS = 1 (one add per element), within the bound at MS = 3."""
    g = gen(77)
    spec = [("mat", 3, (8, 8, 2), 16, 1), ("imp", 8, (8, 8, 2), 32, 1),
            ("imp", 16, (4, 16, 3), 64, 3)]
    st = []
    for src, Cin, (H, W, B), N, MS in spec:
        M = B * H * W
        a, cols, kc, kcp, gk = wgrad_inputs(g, act, src, Cin, H, W, B, M, N)
        dpre = draw(g, M, N, lo=-0.1, hi=0.1).to(DT[act])
        st.append(dict(src=src, a=a.to(device), cols=cols, kc=kc, kcp=kcp,
                       gk=gk, dpre=dpre, dd=dpre.to(device), M=M, N=N, MS=MS,
                       dW0=draw(g, kcp, N), db0=draw(g, N), H=H, W=W, Cin=Cin))
    one = [(s["dW0"].clone().to(device), s["db0"].clone().to(device))
           for s in st]
    for s, (dW, db) in zip(st, one):
        _C.deep_wgrad_gemm(s["a"], s["dd"], dW, s["M"], s["kcp"], s["N"],
                           s["MS"], sh(),
                           imx=s["a"] if s["src"] == "imp" else EMPTY,
                           db=db, **s["gk"])
    multi = [(s["dW0"].clone().to(device), s["db0"].clone().to(device))
             for s in st]
    _C.deep_wgrad_multi(
        [s["a"] for s in st], [s["dd"] for s in st], [m[0] for m in multi],
        [m[1] for m in multi], [s["M"] for s in st], [s["kcp"] for s in st],
        [s["N"] for s in st], [s["MS"] for s in st],
        [int(s["src"] == "imp") for s in st], [s["H"] for s in st],
        [s["W"] for s in st], [s["Cin"] for s in st], [5] * 3, [2] * 3, sh())
    torch.cuda.synchronize()
    for i, (s, (dW1, db1), (dWm, dbm)) in enumerate(zip(st, one, multi)):
        M, MS = s["M"], s["MS"]
        want = s["cols"].T @ mf(s["dpre"])
        mag = s["cols"].T.abs() @ mf(s["dpre"]).abs()
        bound = (M + 8) * U32 * mag + (MS + 2) * U32 * (
            f64(s["dW0"]).abs() + mag)
        tag = f"[{act},stage{i}]"
        check("wgrad_multi_dW" + tag, f64(dWm) - f64(s["dW0"]), want, bound)
        wdb = f64(s["dpre"]).sum(0)
        bdb = (M + MS + 10) * U32 * (f64(s["dpre"]).abs().sum(0) +
                                     f64(s["db0"]).abs())
        check("wgrad_multi_db" + tag, f64(dbm) - f64(s["db0"]), wdb, bdb)
        if MS == 1:
            check_bits("wgrad_multi_vs_single_dW" + tag, dWm, dW1)
            check_bits("wgrad_multi_vs_single_db" + tag, dbm, db1)
        else:
            check("wgrad_multi_vs_single_dW" + tag, dWm, dW1, 2 * bound)
            check("wgrad_multi_vs_single_db" + tag, dbm, db1, 2 * bdb)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("slices", [1, 7, 512])
def test_colsum(act, N, slices, device):
    M = 200
    g = gen(N + slices)
    dpre = draw(g, M, N, lo=-0.1, hi=0.1).to(DT[act])
    db0 = draw(g, N)
    db = db0.clone().to(device)
    part = torch.zeros(slices * N, device=device)
    _C.deep_colsum(dpre.to(device), part, db, M, N, slices, sh())
    torch.cuda.synchronize()
    bound = (M + 10) * U32 * (f64(dpre).abs().sum(0) + f64(db0).abs())
    check(f"colsum[{act},N{N},G{slices}]", f64(db) - f64(db0),
          f64(dpre).sum(0), bound)


# -------------------------------------------------------------- pool kernels
def pool_data(g, act, B, H, W, C, K):
    a = torch.sigmoid(draw(g, B, H, W, C)).to(DT[act])
    d = draw(g, B, H // K, W // K, C, lo=-0.1, hi=0.1).to(DT[act])
    pw = draw(g, K * K + 1)
    dpw0 = draw(g, K * K + 1)
    a64, d64 = f64(a), f64(d)
    aw = a64.view(B, H // K, K, W // K, K, C)
    want_w = torch.einsum("bpqc,bpiqjc->ij", d64, aw).reshape(-1)
    mag_w = torch.einsum("bpqc,bpiqjc->ij", d64.abs(), aw.abs()).reshape(-1)
    want = torch.cat([want_w, d64.sum().reshape(1)])
    mag = torch.cat([mag_w, d64.abs().sum().reshape(1)])
    up = d64.repeat_interleave(K, 1).repeat_interleave(K, 2)
    pwm = f64(pw)[:K * K].view(K, K).repeat(H // K, W // K).view(1, H, W, 1)
    dapre = up * pwm * a64 * (1 - a64)
    return a, d, pw, dpw0, want, mag, dapre


def dpw_bound(mag, dpw0, want, items, G):
    # `items`-long sums + one add per workgroup into the bucket
    return (items + G + 8) * U32 * (mag + f64(dpw0).abs() + want.abs())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("G", [1, 64, 1000])
def test_pool_backward_vector_route(act, G, device):
    """deep_pool_bwd, deep_pool_wgrad (C = 16, K = 2: k_pool_wgrad8) and the
    fused deep_pool_wbwd: dapre and dpw (bias grad included) against float64
    and against each other, accumulating into a non-zero dpw.  G = 1 makes
    every thread loop, G = 1000 exceeds the 640 work items."""
    B, H, W, C, K = 5, 16, 16, 16, 2
    a, d, pw, dpw0, want, mag, dapre = pool_data(gen(G), act, B, H, W, C, K)
    ad, dd, pwd = a.to(device), d.to(device), pw.to(device)
    o1 = torch.zeros(B, H, W, C, dtype=DT[act], device=device)
    o2 = torch.zeros_like(o1)
    w1, w2 = dpw0.clone().to(device), dpw0.clone().to(device)
    _C.deep_pool_bwd(dd, ad, pwd, o1, B, H, W, C, K, sh())
    _C.deep_pool_wgrad(dd, ad, w1, B, H, W, C, K, G, sh())
    _C.deep_pool_wbwd(dd, ad, pwd, o2, w2, B, H, W, C, K, G, sh())
    torch.cuda.synchronize()
    tag = f"[{act},G{G}]"
    bd = 8 * U32 * dapre.abs() + store_bound(dapre, act)
    check("pool_bwd" + tag, o1, dapre, bd)
    check("pool_wbwd_dapre" + tag, o2, dapre, bd)
    check("pool_wbwd_vs_bwd" + tag, o2, o1, 2 * bd)
    bw = dpw_bound(mag, dpw0, want, d.numel(), G)
    check("pool_wgrad8" + tag, f64(w1) - f64(dpw0), want, bw)
    check("pool_wbwd_dpw" + tag, f64(w2) - f64(dpw0), want, bw)
    check("pool_wbwd_vs_wgrad" + tag, w2, w1, 2 * bw)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C,K", [(16, 4), (12, 2)])
@pytest.mark.parametrize("G", [1, 64, 5000])
def test_pool_wgrad_scalar_route(act, C, K, G, device):
    """k_pool_wgrad: K = 4, and C = 12 (no 8-channel vectors) through the
    raw binding."""
    B, H, W = 5, 16, 16
    a, d, pw, dpw0, want, mag, _ = pool_data(gen(C + K + G), act, B, H, W, C,
                                             K)
    w1 = dpw0.clone().to(device)
    _C.deep_pool_wgrad(d.to(device), a.to(device), w1, B, H, W, C, K, G, sh())
    torch.cuda.synchronize()
    check(f"pool_wgrad_scalar[{act},C{C},K{K},G{G}]", f64(w1) - f64(dpw0),
          want, dpw_bound(mag, dpw0, want, d.numel(), G))


# ---------------------------------------------------------------- fc kernels
def fc_data(g, act, B, FCIN):
    flat = torch.sigmoid(draw(g, B, FCIN)).to(DT[act])
    fw = draw(g, 10, FCIN) * (4.0 / FCIN)   # keeps y off saturation
    fb = draw(g, 10)
    labels = torch.tensor([0, 9, 3, 0, 9][:B] if B > 1 else [9],
                          dtype=torch.int32)
    x = f64(flat)
    z = x @ f64(fw).T + f64(fb)
    pre = (FCIN + 8) * U32 * (x.abs() @ f64(fw).T.abs()) + U32 * z.abs()
    y = torch.sigmoid(z)
    by = sig_bound(z, pre, "fp32")
    dz = F.one_hot(labels.long(), 10).double() - y
    return flat, fw, fb, labels, x, y, by, dz


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("FCIN", [256, 1000])
def test_fc_fwd_train(act, B, FCIN, device):
    """Mode 0: y, dz, the loss increment from a non-zero start and the fused
    dflat (against float64 and against deep_fc_bwd)."""
    flat, fw, fb, labels, x, y, by, dz = fc_data(gen(B + FCIN), act, B, FCIN)
    fd, fwd, fbd = flat.to(device), fw.to(device), fb.to(device)
    yd = torch.zeros(B, 10, device=device)
    dzd = torch.zeros(B, 10, device=device)
    loss = torch.full((1,), 2.5, device=device)
    corr = torch.full((1,), 7, dtype=torch.int32, device=device)
    dflat = torch.zeros(B, FCIN, dtype=DT[act], device=device)
    dflat2 = torch.zeros_like(dflat)
    _C.deep_fc_fwd(fd, fwd, fbd, labels.to(device), yd, dzd, loss, corr, B,
                   FCIN, 10, 0, sh(), dflat=dflat)
    _C.deep_fc_bwd(dzd, fd, fwd, dflat2, B, FCIN, 10, sh())
    torch.cuda.synchronize()
    tag = f"[{act},B{B},FCIN{FCIN}]"
    check("fc_y" + tag, yd, y, by)
    bdz = by + U32 * dz.abs()
    check("fc_dz" + tag, dzd, dz, bdz)
    wl = dz.norm(dim=1).sum()
    bl = bdz.norm(dim=1).sum() + (B + 12) * U32 * (2.5 + wl)
    check("fc_loss" + tag, f64(loss) - 2.5, wl.reshape(1), bl.reshape(1))
    assert int(corr.item()) == 7
    f = x * (1 - x)
    fw64 = f64(fw)
    want = (dz @ fw64) * f
    acc = 18 * U32 * (dz.abs() @ fw64.abs()) * f
    bfl = (bdz @ fw64.abs()) * f + acc + 4 * U32 * want.abs() + \
        store_bound(want, act)
    check("fc_dflat" + tag, dflat, want, bfl)
    check("fc_bwd" + tag, dflat2, want, bfl)
    own = acc + 4 * U32 * want.abs() + store_bound(want, act)
    check("fc_dflat_vs_bwd" + tag, dflat, dflat2, 2 * own)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("FCIN", [256, 1000])
def test_fc_fwd_eval_infer(act, B, FCIN, device):
    """Mode 1 counts correct predictions into a non-zero counter; mode 2
    writes y only."""
    flat, fw, fb, labels, x, y, by, dz = fc_data(gen(B * FCIN), act, B, FCIN)
    top2 = y.topk(2, dim=1).values
    assert ((top2[:, 0] - top2[:, 1]) > 4 * by.max()).all(), \
        "test data: argmax must not hinge on rounding"
    labels = y.argmax(1).to(torch.int32)
    labels[0] = (labels[0] + 1) % 10          # one wrong, the rest right
    fd, fwd, fbd = flat.to(device), fw.to(device), fb.to(device)
    for mode in (1, 2):
        yd = torch.zeros(B, 10, device=device)
        dzd = torch.full((B, 10), 4.0, device=device)
        loss = torch.full((1,), 2.5, device=device)
        corr = torch.full((1,), 7, dtype=torch.int32, device=device)
        _C.deep_fc_fwd(fd, fwd, fbd, labels.to(device), yd, dzd, loss, corr,
                       B, FCIN, 10, mode, sh())
        torch.cuda.synchronize()
        check(f"fc_y_mode{mode}[{act},B{B},FCIN{FCIN}]", yd, y, by)
        assert int(corr.item()) == 7 + (B - 1 if mode == 1 else 0)
        assert (dzd == 4.0).all() and loss.item() == 2.5


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("FS", [1, 3, 5])
def test_fc_wgrad(act, FS, device):
    B, FCIN = 5, 1000
    g = gen(FS)
    flat = torch.sigmoid(draw(g, B, FCIN)).to(DT[act])
    dz = draw(g, B, 10)
    gw0, gb0 = draw(g, 10 * FCIN), draw(g, 10)
    gw, gb = gw0.clone().to(device), gb0.clone().to(device)
    _C.deep_fc_wgrad(dz.to(device), flat.to(device), gw, gb, B, FCIN, 10, FS,
                     sh())
    torch.cuda.synchronize()
    want = (f64(dz).T @ f64(flat)).reshape(-1)
    mag = (f64(dz).T.abs() @ f64(flat).abs()).reshape(-1)
    bound = (B + FS + 8) * U32 * (mag + f64(gw0).abs())
    check(f"fc_wgrad_w[{act},FS{FS}]", f64(gw) - f64(gw0), want, bound)
    check(f"fc_wgrad_b[{act},FS{FS}]", f64(gb) - f64(gb0), f64(dz).sum(0),
          (B + FS + 8) * U32 * (f64(dz).abs().sum(0) + f64(gb0).abs()))


# ------------------------------------------------ 8-padded stage-0 route
@pytest.mark.parametrize("act", ACTS)
def test_pad8_route_matches_materialized(act, device):
    """Cin = 3 through the padded copy (pad_channels + implicit GEMM over
    wp8, implicit wgrad + remap_dw8) against float64 and against the
    materialized route (im2col + wbfT GEMM, cols wgrad)."""
    K, P, Cin, Cout, B, H, W = 5, 2, 3, 16, 2, 8, 8
    g = gen(38)
    s = cast_all(device, [(K, Cin, Cout, True)], g)[0]
    kc, kcp, M, k8 = s["kc"], s["kcp"], B * H * W, K * K * 8
    x = draw(g, B, H, W, Cin).to(DT[act])
    bias = draw(g, Cout)
    xd, Wd, bd = x.to(device), s["W"].to(device), bias.to(device)
    x8 = torch.zeros(M, 8, dtype=DT[act], device=device)
    cols = torch.zeros(M, kcp, dtype=DT[act], device=device)
    _C.deep_pad_channels(xd, x8, M, Cin, sh())
    _C.deep_im2col(xd, cols, B, H, W, Cin, K, P, kcp, sh())
    C8 = torch.zeros(M, Cout, dtype=DT[act], device=device)
    Cm = torch.zeros_like(C8)
    gemm(device, x8, Wd, bd, C8, M, k8, Cout, k8, Cout, 1, 1, Bpre=s["wp8"],
         imx=x8, XH=H, XW=W, XC=8, XK=K, XP=P)
    gemm(device, cols, Wd, bd, Cm, M, kcp, Cout, kcp, Cout, 1, 1,
         Bpre=s["wbfT"])
    xn = mf(x).permute(0, 3, 1, 2)
    wq = mf(s["w"])
    z = F.conv2d(xn, wq, f64(bias), padding=P)
    pre = (k8 + 8) * U32 * F.conv2d(xn.abs(), wq.abs(), None, padding=P) + \
        U32 * z.abs()
    want = torch.sigmoid(z).permute(0, 2, 3, 1).reshape(M, Cout)
    bound = sig_bound(z, pre, act).permute(0, 2, 3, 1).reshape(M, Cout)
    tag = f"[{act}]"
    check("pad8_fwd" + tag, C8, want, bound)
    check("pad8_fwd_materialized" + tag, Cm, want, bound)
    check("pad8_fwd_routes_agree" + tag, C8, Cm, 2 * bound)

    dpre = draw(g, M, Cout, lo=-0.1, hi=0.1).to(DT[act])
    dd = dpre.to(device)
    dW0 = draw(g, kcp, Cout)
    dw8 = torch.zeros(k8 * Cout, device=device)
    g8, gm = dW0.clone().to(device), dW0.clone().to(device)
    _C.deep_wgrad_gemm(x8, dd, dw8, M, k8, Cout, 2, sh(), imx=x8, XH=H, XW=W,
                       XC=8, XK=K, XP=P)
    _C.deep_remap_dw8(dw8, g8, K * K, Cin, Cout, sh())
    _C.deep_wgrad_gemm(cols, dd, gm, M, kcp, Cout, 2, sh())
    torch.cuda.synchronize()
    u = F.unfold(xn, K, padding=P).view(B, Cin, K * K, -1)
    c64 = torch.zeros(M, kcp, dtype=torch.float64)
    c64[:, :kc] = u.permute(0, 3, 2, 1).reshape(M, kc)
    wantw = c64.T @ mf(dpre)
    magw = c64.T.abs() @ mf(dpre).abs()
    bw = (M + 8) * U32 * magw + 5 * U32 * (f64(dW0).abs() + magw)
    check("pad8_wgrad" + tag, f64(g8) - f64(dW0), wantw, bw)
    check("pad8_wgrad_materialized" + tag, f64(gm) - f64(dW0), wantw, bw)
    check("pad8_wgrad_routes_agree" + tag, g8, gm, 2 * bw)
    assert (dw8 == 0).all(), "remap must leave the scratch zeroed"
