"""The annealed-importance-sampling section of the sanitizer driver (tests/emu/sanitize_ais.cpp): mf_ais_ment_steps of
mentflow_amd/csrc/ais.hip on the host build with AddressSanitizer + UndefinedBehaviorSanitizer.  It is part of the same stand-alone
binary as every other section (tests/test_sanitizers.py builds it); this module runs that binary and looks for the section's own
marker."""
import subprocess

from test_sanitizers import ENV, sanitize_binary  # noqa: F401  (the fixture builds tests/emu/sanitize_emu when it is out of date)


def test_ais_section_is_clean_under_asan_and_ubsan(sanitize_binary):  # noqa: F811
    r = subprocess.run([sanitize_binary], env=ENV, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SANITIZE AIS OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
