"""SURVEY.md §5 "race detection / sanitizers" — the CPU pass (GPU-side ASan is not available on this pool).

tests/emu/build_sanitize.sh compiles the kernel sources for the host against the fiber emulator with AddressSanitizer
+ UndefinedBehaviorSanitizer (fiber switches annotated, dynamic LDS exactly sized and fenced by PROT_NONE pages) and
links the driver, every tests/emu/sanitize_*.cpp, into one binary: sanitize_main.cpp (main; flow, KDE and tail kernels:
both backward variants, every window variant of the KDE kernels, NaN / inf / out-of-range rows) and one section each in
sanitize_ment.cpp, sanitize_mcmc.cpp, sanitize_entropy.cpp and sanitize_swd.cpp, with sanitize_common.h for what they
share.  Together they call every compute entry point of include/mentflow_hip.h on small synthetic inputs, which
test_driver_calls_every_entry_point checks against the header.  Any out-of-range LDS or global index, or undefined
arithmetic, aborts the program."""
import glob
import os
import subprocess

import pytest

from conftest import EMU_DIR, ROOT

BIN = os.path.join(EMU_DIR, "sanitize_emu")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")


def _up_to_date():
    if not os.path.exists(BIN):
        return False
    t = os.path.getmtime(BIN)
    srcs = [os.path.join(ROOT, "mentflow_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "mentflow_amd", "csrc"))
            if f.endswith((".hip", ".h", ".inc"))]
    srcs += [os.path.join(EMU_DIR, f) for f in ("hip_emu.h", "hip_emu.cpp", "build_sanitize.sh")]
    srcs += glob.glob(os.path.join(EMU_DIR, "sanitize_*.cpp")) + glob.glob(os.path.join(EMU_DIR, "sanitize_*.h"))
    srcs.append(os.path.join(ROOT, "include", "mentflow_hip.h"))
    return all(os.path.getmtime(s) <= t for s in srcs)


@pytest.fixture(scope="module")
def sanitize_binary():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("needs the ROCm clang++ with the sanitizer runtimes")
    if not _up_to_date():
        subprocess.run(["bash", os.path.join(EMU_DIR, "build_sanitize.sh")], check=True, capture_output=True, timeout=1500)
    return BIN


def test_every_entry_point_is_clean_under_asan_and_ubsan(sanitize_binary):
    r = subprocess.run([sanitize_binary], env=ENV, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE OK" in r.stdout
    sections = r.stdout[:r.stdout.index("SANITIZE OK")]
    for marker in ("SANITIZE MENT OK", "SANITIZE MCMC OK", "SANITIZE ENTROPY OK", "SANITIZE SWD OK"):
        assert marker in sections, marker
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_lds_guard_catches_an_overflow(sanitize_binary):
    """Self-test of the guard: a kernel writing 64 bytes past its dynamic LDS block must die."""
    r = subprocess.run([sanitize_binary, "--provoke-lds-overflow"], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "NOT caught" not in r.stdout
    assert "AddressSanitizer" in r.stderr


# entry points that launch nothing and touch no caller buffer; everything else needs a call in the driver
EXEMPT = {
    "mf_abi_version": "returns a constant",
    "mf_flow_rqs_deriv_slot": "returns an index computed from its argument",
    "mf_prof_enable": "sets a process-wide switch",
}


def test_driver_calls_every_entry_point():
    """Every function declared in include/mentflow_hip.h is called somewhere in tests/emu/sanitize_*.cpp."""
    from test_abi import declared_symbols
    text = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(EMU_DIR, "sanitize_*.cpp"))))
    symbols = declared_symbols()
    assert set(EXEMPT) <= set(symbols), sorted(set(EXEMPT) - set(symbols))
    missing = [s for s in symbols if s not in EXEMPT and s + "(" not in text]
    assert not missing, missing
