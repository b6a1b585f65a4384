"""The weighted-projection section of the sanitizer driver (tests/emu/sanitize_wproj.cpp): the six entry points of
mentflow_amd/csrc/wproj.hip on the host build with AddressSanitizer + UndefinedBehaviorSanitizer.  It is part of the same
stand-alone binary as every other section (tests/test_sanitizers.py builds it); this module runs that binary and looks for the
section's own marker."""
import subprocess

from test_sanitizers import ENV, sanitize_binary  # noqa: F401  (the fixture builds tests/emu/sanitize_emu when it is out of date)


def test_wproj_section_is_clean_under_asan_and_ubsan(sanitize_binary):  # noqa: F811
    r = subprocess.run([sanitize_binary], env=ENV, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE WPROJ OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
