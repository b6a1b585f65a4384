"""ASan + UBSan pass over the classical-MENT entry points: mentflow_amd/csrc/ment.hip (with api.hip, which carries the shared
error plumbing) and the fiber emulator compiled for the host with the sanitizer flags of tests/emu/build_sanitize.sh (read
from that script, so the two stay the same), linked with the driver tests/emu/sanitize_ment.cpp, which calls every mf_ment_*
entry point (see its header).  Any out-of-range LDS or global index, or undefined arithmetic, aborts the program."""
import os
import re
import subprocess

import pytest

from conftest import EMU_DIR, ROOT

CXX = "/opt/rocm/lib/llvm/bin/clang++"
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")


def _script_flags():
    """SAN and FLAGS of build_sanitize.sh, with $HERE / $SAN expanded."""
    text = open(os.path.join(EMU_DIR, "build_sanitize.sh")).read()
    san = re.search(r'^SAN="([^"]*)"', text, re.M).group(1)
    flags = re.search(r'^FLAGS="([^"]*)"', text, re.M).group(1)
    flags = flags.replace("$SAN", san).replace("$HERE", EMU_DIR)
    return san.split(), flags.split()


@pytest.fixture(scope="module")
def ment_sanitize_binary(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("needs the ROCm clang++ with the sanitizer runtimes")
    san, flags = _script_flags()
    assert "-fsanitize=address,undefined" in san and "-DMF_EMU" in flags
    out = tmp_path_factory.mktemp("ment_san")
    csrc = os.path.join(ROOT, "mentflow_amd", "csrc")
    jobs = [[CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "ment.hip"), "-o", str(out / "ment.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "api.hip"), "-o", str(out / "api.o")],
            [CXX, "-std=c++17", "-O1", "-g", "-fPIC", "-DMF_EMU", *san, "-c", os.path.join(EMU_DIR, "hip_emu.cpp"), "-o",
             str(out / "hip_emu.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(EMU_DIR, "sanitize_ment.cpp"), "-o", str(out / "main.o")]]
    procs = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, procs):
        text, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (" ".join(j), text[-3000:])
    binary = str(out / "sanitize_ment")
    subprocess.run([CXX, "-fsanitize=address,undefined", "-o", binary, *(str(out / f) for f in
                                                                         ("ment.o", "api.o", "hip_emu.o", "main.o"))],
                   check=True, capture_output=True, timeout=300)
    return binary


def test_ment_entry_points_are_clean_under_asan_and_ubsan(ment_sanitize_binary):
    r = subprocess.run([ment_sanitize_binary], env=ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE MENT OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_driver_calls_every_ment_entry_point():
    from test_abi import declared_symbols
    text = open(os.path.join(EMU_DIR, "sanitize_ment.cpp")).read()
    missing = [s for s in declared_symbols() if s.startswith("mf_ment_") and s + "(" not in text]
    assert not missing, missing
