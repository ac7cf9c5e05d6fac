"""NewBowFromParquet of the C++ mirror (bow_amd/host/bow_rolling.hpp, tests/cpp/test_parquet_bool.cpp) on a pyarrow file that holds
Int64, Float64 and BOOLEAN columns: asked to (ParquetBooleans::Read), it makes the flag column a Boolean series, through the C ABI, on the GPU."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import parquet_bool_pages as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 3000   # past one trip of 2048 rows


@pytest.mark.gpu
def test_cpp_mirror_reads_a_file_with_a_flag_column(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "test_parquet_bool")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    r = np.arange(ROWS)
    path = str(tmp_path / "frame.parquet")
    # the rows tests/cpp/test_parquet_bool.cpp expects
    pb.write_pyarrow(path, r % 3 == 0, r % 7 != 2, "rle_v1", compression="snappy",
                     extra={"time": pa.array((10 * r).astype(np.int64)), "value": pa.array(r / 2.0, mask=r % 5 == 3)})
    p = subprocess.run([exe, path, str(ROWS), os.path.join(ROOT, "tests", "golden", "bow1-100-rows.parquet")], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failures" in p.stdout


def test_cpp_mirror_of_the_parquet_flag_column_builds():
    # CPU: the test of the mirror's Boolean Parquet path compiles and links against libbowgpu.so
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_parquet_bool"))
