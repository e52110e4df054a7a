"""The two g++ command lines of the CPU tests over tests/cpp/*.cpp, which
compile the host-compilable headers of csrc/ alone:

* run_check: a stand-alone check program (its own main) under ASan + UBSan,
  built once per directory and run; nothing is loaded into Python.
* shared_lib: a -fPIC -shared library of plain C functions, for ctypes.
"""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CPP = ROOT / "tests" / "cpp"
CSRC = ROOT / "lora-sdr-lightweight-standalone-library-clean_amd" / "csrc"

SANITIZED = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SHARED = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared"]


def run_check(source: str, tmp: Path, *args: str, define: str | None = None, skip_without_sanitizers: bool = False,
              timeout: float | None = None) -> str:
    """Stdout of tests/cpp/`source` built under the sanitizers (with -D`define`
    when given) and run with `args`; a failed compile or a non-zero exit
    fails the test.  skip_without_sanitizers: skip instead when the compile
    fails for want of the sanitizers' runtimes."""
    exe = tmp / (Path(source).stem + "_san")
    if not exe.exists():
        r = subprocess.run(["g++", *SANITIZED, *([f"-D{define}"] if define else []), "-I", str(CSRC), "-o", str(exe),
                            str(CPP / source)], capture_output=True, text=True)
        if skip_without_sanitizers and r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr):
            pytest.skip("g++ has no sanitizer runtimes here")
        assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def shared_lib(source: str, tmp: Path) -> ctypes.CDLL:
    """tests/cpp/`source` as a shared library; a failed compile raises."""
    so = tmp / f"lib{Path(source).stem}.so"
    subprocess.run(["g++", *SHARED, "-I", str(CSRC), "-o", str(so), str(CPP / source)], check=True)
    return ctypes.CDLL(str(so))
