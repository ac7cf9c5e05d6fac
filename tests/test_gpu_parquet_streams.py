"""The device Parquet loader (snappy_pages_kernel, dict_indices_kernel, page_scatter_kernel in parquet_decode.hip) on byte streams
no encoder emits: the files of tests/parquet_stream_cases.py, built element by element with tests/parquet_streams.py.  Snappy
copies of every (offset, length) around the 64-lane stride in every tag form, literals in every length form, preambles of 1 to 3
bytes; dictionary indices at bit widths 0 to 32 in alternating RLE / bit-packed runs; definition-level runs that end on the
2048-row batch edge of page_scatter_kernel; chunks that mix dictionary and PLAIN pages, lack dictionary_page_offset, or hold v2
pages stored inside a SNAPPY chunk.  The expectation is pyarrow's read of the same file, bit for bit, through check_file (both
residencies, validity, zeroed null slots, null count); tests/test_parquet_streams_cpu.py shows that pyarrow reads each file as the
column it was built from.  Every damaged file must come back as BOWGPU_ERR_ARG (-10), and a well-formed file must read correctly
right after it.

The two kinds of damage that went unreported before this file (its ten `ends_early` / `end_early` / `rle_count_0` cases failed with
"DID NOT RAISE" against the library of the commit before): a dictionary index stream that ends early came back with code 0 and the
indices an earlier call had left in the pool workspace (hence the undamaged twin that is read first), and definition levels that end
early came back with code 0 and the remaining rows null."""
import pytest

import parquet_stream_cases as cases
from bow_amd import capi
from test_parquet_loader import check_file

pytestmark = pytest.mark.gpu

GOOD = ["snappy_copy_form1", "snappy_copy_form2", "snappy_copy_form3", "snappy_copy_chains", "snappy_literals", "snappy_preambles"] + \
       ["indices_%s_%s_codec%d" % (t, o, c) for t in ("int64", "double") for o in ("required", "optional") for c in (0, 1)] + \
       ["levels_codec%d_v%d" % (c, v) for c in (0, 1) for v in (1, 2)] + \
       ["chunk_%s_codec%d_%s" % (n, c, o) for n in ("dict_then_plain", "no_dictionary_page_offset", "v2_stored_and_compressed")
        for c in (0, 1) for o in ("required", "optional")] + ["chunk_v2_nulls_only_codec%d" % c for c in (0, 1)]

DAMAGED = ["snappy_" + n for n in ("declared_smaller", "declared_larger", "offset_0", "offset_past_output", "copy_overruns_output",
                                   "literal_overruns_input", "offset_cut_off", "ends_short", "extra_element")] + \
          ["indices_%s_%s" % (n, o) for n in ("width_33", "index_equals_dictionary_size", "run_past_the_page", "rle_count_0", "ends_early_rle",
                                              "ends_early_bit_packed") for o in ("required", "optional")] + \
          ["levels_end_early_%s_%s" % (n, v) for n in ("rle", "bit_packed") for v in ("v1", "v2")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("streams")
    good = cases.good_files(d)
    bad, twins = cases.damaged_files(d)
    assert sorted(good) == sorted(GOOD) and sorted(bad) == sorted(DAMAGED)
    return good, bad, twins


@pytest.mark.parametrize("name", GOOD)
def test_hand_built_file_reads_like_pyarrow(files, name):
    assert check_file(files[0][name][0]) == 1


@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_file_is_refused(files, name):
    good, bad, twins = files
    path, twin = bad[name]
    if twin is not None:   # the same shape, undamaged: its indices then lie in the pool workspace the damaged read takes
        assert check_file(twin) == 1
    f = capi.ParquetFile(path)
    for res in (capi.HOST, capi.DEVICE):
        with pytest.raises(capi.BowGpuError) as e:
            f.read_column(0, out_residency=res)
        assert e.value.code == -10, (name, e.value)
    f.close()
    assert check_file(good["chunk_dict_then_plain_codec1_optional"][0]) == 1
