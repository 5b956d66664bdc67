"""In-tree build of parallel_cnn_amd._C.

Compiles the gfx950 HIP kernels with hipcc (cross-compiles fine on a
GPU-less box) and links them into a torch CppExtension together with the
CPU reference ops.  Build with:

    python setup.py build_ext --inplace
"""
import glob
import os
import subprocess
import sys

from setuptools import setup

from torch.utils.cpp_extension import BuildExtension, CppExtension

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("PCNN_GFX_ARCH", "gfx950")
HERE = os.path.dirname(os.path.abspath(__file__))

HIP_SOURCES = [
    os.path.join(HERE, "csrc", "hip", "lenet_kernels.hip"),
    os.path.join(HERE, "csrc", "hip", "conv_kernels.hip"),
]


# Every header under csrc/: the launcher surface (pcnn_launch.h), the
# dimensions and the shared device headers.  An edit to any of them makes
# the HIP objects, the native CLI and the extension stale.
HEADERS = sorted(glob.glob(os.path.join(HERE, "csrc", "**", "*.h"),
                           recursive=True))

FORCE = os.environ.get("PCNN_FORCE_REBUILD") == "1"


def older_than(out, deps):
    return (not os.path.exists(out)
            or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps))


def compile_hip_objects():
    objs = []
    for src in HIP_SOURCES:
        obj = os.path.splitext(src)[0] + ".o"
        if FORCE or older_than(obj, [src] + HEADERS):
            cmd = [
                os.path.join(ROCM, "bin", "hipcc"),
                f"--offload-arch={ARCH}",
                "-O3",
                "-std=c++17",
                "-fPIC",
                "-c",
                src,
                "-o",
                obj,
            ]
            print("[pcnn build]", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        objs.append(obj)
    return objs


def build_native_cli(hip_objs):
    """Link the native CLI trainer (tools/pcnn_train) against the kernel
    objects.  Non-fatal: the binary is a parity artifact, not a build
    dependency."""
    src = os.path.join(HERE, "tools", "pcnn_train.cpp")
    out = os.path.join(HERE, "tools", "pcnn_train")
    try:
        if FORCE or older_than(out, [src] + HEADERS + hip_objs):
            obj = os.path.join(HERE, "tools", "pcnn_train.o")
            hipcc = os.path.join(ROCM, "bin", "hipcc")
            for cmd in ([hipcc, f"--offload-arch={ARCH}", "-O3",
                         "-std=c++17", "-c", src, "-o", obj],
                        [hipcc, f"--offload-arch={ARCH}", obj,
                         os.path.join(HERE, "csrc", "hip",
                                      "lenet_kernels.o"), "-o", out]):
                print("[pcnn build]", " ".join(cmd), flush=True)
                subprocess.check_call(cmd)
    except Exception as e:  # pragma: no cover
        print(f"[pcnn build] native CLI skipped: {e}", flush=True)


_hip_objs = compile_hip_objects()
build_native_cli(_hip_objs)

ext = CppExtension(
    name="parallel_cnn_amd._C",
    sources=["csrc/bindings.cpp", "csrc/cpu_ops.cpp"],
    depends=HEADERS,
    extra_objects=_hip_objs,
    libraries=["amdhip64"],
    library_dirs=[os.path.join(ROCM, "lib")],
    extra_compile_args=["-O3", "-std=c++17"],
    extra_link_args=[f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"],
)

setup(
    name="parallel_cnn_amd",
    version="0.1.0",
    description="MI355X-native CNN training framework "
    "(capability parity with Tamerkobba/Parallel-CNN)",
    packages=[
        "parallel_cnn_amd",
        "parallel_cnn_amd.data",
        "parallel_cnn_amd.models",
        "parallel_cnn_amd.ops",
        "parallel_cnn_amd.parallel",
        "parallel_cnn_amd.engine",
        "parallel_cnn_amd.utils",
    ],
    ext_modules=[ext],
    cmdclass={"build_ext": BuildExtension.with_options(no_python_abi_suffix=False)},
)
