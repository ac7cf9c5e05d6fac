"""The pure host steps of a call over several devices (bow_amd/csrc/fan_host.h: who the fan-out serves, its row ranges, the
Interpolate edge exchange, a rank's bitmap placed in the frame's, the merge of the ranks' infos) as a stand-alone program under
AddressSanitizer + UBSan: tests/fan_host_check.cpp holds the models and links fan_host.cpp alone, so the arithmetic that a GPU and two
ranks were needed to reach runs here, on buffers of exactly the product's sizes.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sanitizers' runtimes are linked INTO the program: a dynamically linked one refuses to start unless it is the first library the
# process loads, which an environment that preloads anything of its own takes away
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_fan_host_steps_match_their_models_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "fan_host_check")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "fan_host_check.cpp"),
                                             os.path.join(ROOT, "bow_amd", "csrc", "fan_host.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:]
    assert "fan_host_check: ok" in run.stdout
