"""csrc/sock_io.h under sanitizers, on the CPU.

The header has no HIP and no Python includes, so a stand-alone driver
(sock_io_host_main.cpp) exercises it as a plain child process over
loopback TCP pairs, each receive case on a blocking and on an O_NONBLOCK
fd: a body arriving in many small writes, a peer closing mid-body (short
count + EOF status), a stalled peer (timeout status with the bytes so
far, stall limit 200 ms), a signal without SA_RESTART during the wait,
sendfile_exact against a slow reader behind a 4 KiB SO_SNDBUF, against a
reader that stops, and against a closed peer (error status, no SIGPIPE),
8 threads doing send/receive pairs at once, and the scatter-descriptor
expansion (sizes 0, 1, 2^20-1, 2^20, 2^20+1, 3*2^20+5; exact tiling;
capacity one record short writes nothing).  Built once with
AddressSanitizer+UBSan and once with ThreadSanitizer; a flavour whose
runtime the compiler cannot link and start is skipped."""

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "demodel_amd", "csrc")
MAIN = os.path.join(HERE, "sock_io_host_main.cpp")

FLAVOURS = {
    "asan_ubsan": "-fsanitize=address,undefined",
    "tsan": "-fsanitize=thread",
}


def _compile(cxx, flag, src, out):
    return subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fno-sanitize-recover=all", flag, "-pthread", "-I" + CSRC,
         src, "-o", out],
        capture_output=True, text=True)


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_sock_io_under_sanitizer(flavour, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") \
        or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    flag = FLAVOURS[flavour]

    # does this compiler have the sanitizer's runtime at all?
    probe_src = tmp_path / "probe.cpp"
    probe_src.write_text("int main() { return 0; }\n")
    probe = str(tmp_path / "probe")
    r = _compile(cxx, flag, str(probe_src), probe)
    if r.returncode != 0 or subprocess.run(
            [probe], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} lacks a working {flag} runtime")

    exe = str(tmp_path / f"sock_io_{flavour}")
    r = _compile(cxx, flag, MAIN, exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sock_io OK" in run.stdout
    # a sanitizer report that did not change the exit status still fails
    assert "Sanitizer" not in run.stderr, run.stderr
    assert "runtime error" not in run.stderr, run.stderr
