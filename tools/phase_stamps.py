"""Phase breakdown of the in-block training kernels (shader-clock stamps).

Builds csrc/hip/lenet_kernels.hip with -DPCNN_LENET_STAMPS into a shared
library of its own (tools/lenet_stamps.so; the shipped extension carries no
stamp), launches the cell kernel (k_fwdbwd<.., INBLOCK>) and the pair kernel
(k_fwdbwd_pair) once each on random data after a warm-up, and prints for
every segment between two stamp points the median over blocks, in shader
cycles.  A block's time at a stamp point is the LATEST wave's stamp, i.e.
the segment times add up to the block's critical path.

    python tools/phase_stamps.py --build-only     # compile (no GPU needed)
    python tools/phase_stamps.py [--batch 64] [--dtype bf16] [--json OUT]

The stamp build drains memory counters at three of the points and pins the
instruction schedule at every point, so it runs slower than the shipped
kernels (about 11 % for the stamps alone); it is never timed end to end.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "lenet_stamps.so")
SRC = os.path.join(ROOT, "csrc", "hip", "lenet_kernels.hip")
ST_N = 16
NAMES = ["entry", "loads landed", "conv+pool FMAs", "barrier 1",
         "fc phase", "barrier 2", "fc-bwd+pool-bwd", "wgrad FMAs",
         "LDS stores", "barrier 3", "owner sums", "last store"]


def build():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    arch = os.environ.get("PCNN_GFX_ARCH", "gfx950")
    cmd = [os.path.join(rocm, "bin", "hipcc"), f"--offload-arch={arch}",
           "-O3", "-std=c++17", "-fPIC", "-shared", "-DPCNN_LENET_STAMPS",
           SRC, "-o", LIB]
    print("[phase_stamps]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def segments(st, threads):
    """st: [B, 512, ST_N] int64 -> (per-segment medians, total median)."""
    import torch
    waves = threads // 64
    w = st[:, 0:threads:64, :len(NAMES)]          # [B, waves, points]
    assert w.shape[1] == waves
    big = torch.iinfo(torch.int64).max
    first = torch.where(w > 0, w, torch.full_like(w, big)).amin(dim=1)
    last = w.amax(dim=1)                          # latest wave per point
    t = last.clone()
    t[:, 0] = first[:, 0]                         # entry: the earliest wave
    seg = (t[:, 1:] - t[:, :-1]).double()
    total = (t[:, -1] - t[:, 0]).double()
    return seg.median(dim=0).values.tolist(), total.median().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="bf16",
                    choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.build_only or not os.path.exists(LIB):
        build()
        if a.build_only:
            return
    import torch
    sys.path.insert(0, ROOT)
    from parallel_cnn_amd.ops import shapes as S
    assert torch.cuda.is_available(), "phase_stamps needs a GPU"
    lib = ctypes.CDLL(LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.pcnn_stamp_set_buffer.argtypes = [vp, ci]
    lib.pcnn_launch_fwdbwd_inblock.argtypes = [vp] * 8 + [ci] * 5 + [vp]
    dev = "cuda:0"
    B = a.batch
    ad = {"bf16": torch.bfloat16, "fp16": torch.float16,
          "fp32": torch.float32}[a.dtype]
    flag = {"bf16": 1, "fp16": 2, "fp32": 0}[a.dtype]
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, S.IN_PIX, generator=g).to(dev, dtype=ad)
    labels = torch.randint(0, 10, (B,), generator=g).to(dev,
                                                        dtype=torch.int32)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=g)).to(dev)
    a2 = torch.empty(B, S.S1_OUT, dtype=ad, device=dev)
    y = torch.empty(B, S.FC_OUT, device=dev)
    dz = torch.empty(B, S.FC_OUT, device=dev)
    loss = torch.zeros(1, device=dev)
    slab = torch.zeros(B, S.GSLAB_LD, device=dev)
    stamps = torch.zeros(B, 512, ST_N, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    err = lib.pcnn_stamp_set_buffer(stamps.data_ptr(), B)
    assert err == 0, f"stamp buffer: hip error {err}"
    out = {"batch": B, "dtype": a.dtype, "points": NAMES}
    for name, variant, threads in (("cell", 0, 256), ("pair", 1, 512)):
        def launch():
            e = lib.pcnn_launch_fwdbwd_inblock(
                x.data_ptr(), params.data_ptr(), a2.data_ptr(), y.data_ptr(),
                dz.data_ptr(), labels.data_ptr(), loss.data_ptr(),
                slab.data_ptr(), B, flag, 0, 0, variant, None)
            assert e == 0, f"launch: hip error {e}"
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        stamps.zero_()
        torch.cuda.synchronize()
        launch()
        torch.cuda.synchronize()
        seg, total = segments(stamps.cpu(), threads)
        out[name] = {"segments": seg, "total": total}
        print(f"== {name} kernel, B={B}, {a.dtype}: median over blocks, "
              f"shader cycles")
        for i, v in enumerate(seg):
            print(f"  {NAMES[i]:>16s} -> {NAMES[i + 1]:<16s} {v:8.0f}")
        print(f"  {'entry':>16s} -> {'last store':<16s} {total:8.0f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
