"""In-tree builds of the native extensions.

Two extensions, built straight with the toolchain (no setuptools overhead),
.so files landing inside the package so they travel with a repo snapshot:

* ``demodel_amd/_native.so``  — CPU helpers (libcrypto cert minting,
  host zstd, the GIL-free socket loops of csrc/sock_io.h).
  Plain C++, no torch, builds and runs anywhere.
* ``demodel_amd/_hip.so``     — the GPU pipeline: pinned-ring allocator,
  HIP streams/events, and the CDNA4 kernels (SHA-256, scatter, GGUF and
  FP8 dequant, the zstd / snappy / inflate / LZ4 page codecs, parquet
  page decode).  Compiled with hipcc for gfx950 only; importable on a
  CPU-only box (calls fail until a GPU is present).
"""

from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")

GFX_ARCH = os.environ.get("DEMODEL_GFX_ARCH", "gfx950")


def _py_includes() -> list[str]:
    import pybind11

    return [
        "-I" + sysconfig.get_paths()["include"],
        "-I" + pybind11.get_include(),
    ]


def _newer(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    deps = list(sources) + [__file__]
    return all(os.path.getmtime(s) < t for s in deps if os.path.exists(s))


def _run(cmd: list[str]) -> None:
    print("[demodel-amd build]", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


NATIVE_SRCS = ["certs.cpp", "zstd_host.cpp", "sock_native.cpp"]

# in-tree headers each source includes (rebuild triggers); every source
# of NATIVE_SRCS and HIP_SRCS lists all of its own
HDRS = {
    "zstd_host.cpp": ["zstd_common.h"],
    "sock_native.cpp": ["sock_io.h"],
    "hip_core.cpp": ["resource_cache.h", "sock_io.h"],
    "zstd_kernel.hip": ["zstd_common.h"],
    "inflate.hip": ["lz_window.h"],
    "snappy.hip": ["lz_window.h"],
    "lz4.hip": ["lz_window.h"],
}


def _with_hdrs(src: str) -> list[str]:
    """A source's path followed by its in-tree headers' paths."""
    return [os.path.join(CSRC, f) for f in [src] + HDRS.get(src, [])]


def build_native(force: bool = False) -> str:
    out = os.path.join(PKG_DIR, "_native.so")
    srcs = [os.path.join(CSRC, s) for s in NATIVE_SRCS]
    if not force and _newer(out, [p for s in NATIVE_SRCS
                                  for p in _with_hdrs(s)]):
        return out
    cmd = (
        ["c++", "-O2", "-std=c++17", "-shared", "-fPIC",
         "-fvisibility=hidden"]
        + _py_includes()
        + srcs
        + ["-lcrypto", "-o", out]
    )
    _run(cmd)
    return out


HIP_SRCS = [
    "hip_core.cpp",
    "sha256.hip",
    "scatter.hip",
    "fp8_dequant.hip",
    "gguf_dequant.hip",
    "inflate.hip",
    "zstd_kernel.hip",
    "snappy.hip",
    "lz4.hip",
    "parquet_decode.hip",
]


def build_hip(force: bool = False) -> str:
    out = os.path.join(PKG_DIR, "_hip.so")
    names = [s for s in HIP_SRCS if os.path.exists(os.path.join(CSRC, s))]
    if not names:
        raise RuntimeError("no HIP sources present")
    if not force and _newer(out, [p for s in names for p in _with_hdrs(s)]):
        return out
    hipcc = os.environ.get("HIPCC", "hipcc")
    objs = []
    os.makedirs(os.path.join(PKG_DIR, "_build"), exist_ok=True)
    for name in names:
        src = os.path.join(CSRC, name)
        obj = os.path.join(PKG_DIR, "_build", name.rsplit(".", 1)[0] + ".o")
        if not _newer(obj, _with_hdrs(name)):
            cmd = (
                [hipcc, f"--offload-arch={GFX_ARCH}", "-O3", "-std=c++17",
                 "-fPIC", "-fvisibility=hidden", "-c", src, "-o", obj]
                + _py_includes()
            )
            _run(cmd)
        objs.append(obj)
    _run([hipcc, f"--offload-arch={GFX_ARCH}", "-shared", "-fPIC"]
         + objs + ["-lamdhip64", "-o", out])
    return out


def build_all(force: bool = False) -> None:
    build_native(force=force)
    if any(os.path.exists(os.path.join(CSRC, s)) for s in HIP_SRCS):
        build_hip(force=force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
