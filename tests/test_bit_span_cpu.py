"""The arithmetic of the staging layer (bow_amd/csrc/bit_span.h) against a bit-by-bit model: a stand-alone program, built and run
under AddressSanitizer + UBSan.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_bit_span_program(tmp_path):
    exe = str(tmp_path / "test_bit_span")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "cpp", "test_bit_span.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.split() == ["cases", str(8 * 71 * 12)], p.stdout
