"""ASan + UBSan pass over the entropy-estimator entry points: mentflow_amd/csrc/entropy.hip (with api.hip, which carries the
shared error plumbing) and the fiber emulator compiled for the host with the sanitizer flags of tests/emu/build_sanitize.sh
(read from that script, so the two stay the same), linked with the driver tests/emu/sanitize_entropy.cpp, which calls every
mf_knn_entropy_* and mf_cov_entropy_* entry point (see its header: ragged N, k = 16, every chunking).  Any out-of-range LDS or
global index, or undefined arithmetic, aborts the program."""
import os
import subprocess

import pytest

from conftest import EMU_DIR, ROOT
from test_ment_sanitize import CXX, ENV, _script_flags


@pytest.fixture(scope="module")
def entropy_sanitize_binary(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("needs the ROCm clang++ with the sanitizer runtimes")
    san, flags = _script_flags()
    assert "-fsanitize=address,undefined" in san and "-DMF_EMU" in flags
    out = tmp_path_factory.mktemp("entropy_san")
    csrc = os.path.join(ROOT, "mentflow_amd", "csrc")
    jobs = [[CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "entropy.hip"), "-o", str(out / "entropy.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(csrc, "api.hip"), "-o", str(out / "api.o")],
            [CXX, "-std=c++17", "-O1", "-g", "-fPIC", "-DMF_EMU", *san, "-c", os.path.join(EMU_DIR, "hip_emu.cpp"), "-o",
             str(out / "hip_emu.o")],
            [CXX, *flags, "-x", "c++", "-c", os.path.join(EMU_DIR, "sanitize_entropy.cpp"), "-o", str(out / "main.o")]]
    procs = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, procs):
        text, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (" ".join(j), text[-3000:])
    binary = str(out / "sanitize_entropy")
    subprocess.run([CXX, "-fsanitize=address,undefined", "-o", binary, *(str(out / f) for f in
                                                                         ("entropy.o", "api.o", "hip_emu.o", "main.o"))],
                   check=True, capture_output=True, timeout=300)
    return binary


def test_entropy_entry_points_are_clean_under_asan_and_ubsan(entropy_sanitize_binary):
    r = subprocess.run([entropy_sanitize_binary], env=ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE ENTROPY OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_driver_calls_every_entropy_entry_point():
    from test_abi import declared_symbols
    text = open(os.path.join(EMU_DIR, "sanitize_entropy.cpp")).read()
    names = [s for s in declared_symbols() if s.startswith(("mf_knn_entropy_", "mf_cov_entropy_"))]
    assert len(names) == 6
    missing = [s for s in names if s + "(" not in text]
    assert not missing, missing
