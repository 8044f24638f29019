"""What the programme bank's carried stages (resample, convolve, dynamics, the limiter) share on the host
(openmeters_amd/csrc/program/program_carried.hpp): the stand-alone check program under the sanitizers.  The stages' own CPU files hold
the streaming rule against their restatements; tests/test_gpu_program_carried.py drives the shared hand-over on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_program_is_clean_under_the_sanitizers(tmp_path):
    """tools/carried_ledger_check.cpp, a stand-alone host program with its own main, under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "carried_ledger_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "carried_ledger_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr
