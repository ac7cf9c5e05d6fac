"""Runs the reference's "sparse bool" reducer cases through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp,
tests/cpp/test_bool_rolling.cpp): Boolean series in, Boolean series out, through the C ABI, on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_mirror_replays_the_sparse_bool_cases():
    exe = os.path.join(ROOT, "tests", "cpp", "test_bool_rolling")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failures" in p.stdout


def test_cpp_mirror_of_the_bool_cases_builds():
    # CPU: the test of the mirror's Boolean series compiles and links against libbowgpu.so
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_bool_rolling"))
