"""The count / fill protocol (csrc/asr_pending.h) without a GPU: tests/pending_protocol.cpp, a stand-alone program with
its own main, compiled by the host compiler with the address and undefined-behaviour sanitizers and run once."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pending_protocol(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pending_protocol")
    # the sanitizer runtimes are linked into the program (gcc's flags; clang links them statically anyway)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + static + [os.path.join(HERE, "pending_protocol.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode == 0 and run.stdout.decode().strip() == "ok", run.stderr.decode()
