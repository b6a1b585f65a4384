"""ASan + UBSan pass over the Metropolis-Hastings entry point: mentflow_amd/csrc/mcmc.hip (with api.hip, which carries the shared
error plumbing) and the fiber emulator compiled for the host with the sanitizer flags of tests/emu/build_sanitize.sh (read from
that script, so the two stay the same), linked with the driver tests/emu/sanitize_mcmc.cpp (see its header).  Any out-of-range
LDS or global index, or undefined arithmetic, aborts the program."""
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
def mcmc_sanitize_binary(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("needs the ROCm clang++ with the sanitizer runtimes")
    san, flags = _script_flags()
    assert "-fsanitize=address,undefined" in san and "-DMF_EMU" in flags
    out = tmp_path_factory.mktemp("mcmc_san")
    csrc = os.path.join(ROOT, "mentflow_amd", "csrc")
    jobs = [[CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "mcmc.hip"), "-o", str(out / "mcmc.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "api.hip"), "-o", str(out / "api.o")],
            [CXX, "-std=c++17", "-O1", "-g", "-fPIC", "-DMF_EMU", *san, "-c", os.path.join(EMU_DIR, "hip_emu.cpp"), "-o",
             str(out / "hip_emu.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(EMU_DIR, "sanitize_mcmc.cpp"), "-o", str(out / "main.o")]]
    procs = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, procs):
        text, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (" ".join(j), text[-3000:])
    binary = str(out / "sanitize_mcmc")
    subprocess.run([CXX, "-fsanitize=address,undefined", "-o", binary, *(str(out / f) for f in
                                                                         ("mcmc.o", "api.o", "hip_emu.o", "main.o"))],
                   check=True, capture_output=True, timeout=300)
    return binary


def test_mcmc_entry_point_is_clean_under_asan_and_ubsan(mcmc_sanitize_binary):
    r = subprocess.run([mcmc_sanitize_binary], env=ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE MCMC OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_driver_calls_every_mcmc_entry_point():
    from test_abi import declared_symbols
    text = open(os.path.join(EMU_DIR, "sanitize_mcmc.cpp")).read()
    names = [s for s in declared_symbols() if s.startswith("mf_mcmc_")]
    assert names == ["mf_mcmc_ment_steps"]
    missing = [s for s in names if s + "(" not in text]
    assert not missing, missing
