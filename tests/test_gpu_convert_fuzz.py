"""Seeded fuzz of bowgpu_convert against the numpy model (tests/convert_model.py, fuzz_case): random lists of (source, target)
pairs in one call, lengths from 0 to 70 001 that differ within a call, Arrow offsets, input and output residencies, null patterns
(no bitmap, all null, some null; the null count given or left to the library; null slots holding NaN, 1, set bits or whatever was
there), with every special value of the source type salted into a valid row and into a null slot.  Exact: every byte of both output
buffers, type, length and null count.  BOW_FUZZ_SEEDS=N runs N seeds instead of 64; what the default seeds cover is asserted without
a GPU by tests/test_convert_model_cpu.py."""
import os

import pytest

import convert_model as cm
from bow_amd import capi

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")))


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_convert(seed):
    case_cols, out_res = cm.fuzz_case(seed)
    cols = [cm.place(c.column(), c.residency) for c in case_cols]
    try:
        outs = capi.convert(cols, [c.to_t for c in case_cols], out_residency=out_res)
    finally:
        for c in cols:
            c.unpin()
    for k, (c, o) in enumerate(zip(case_cols, outs)):
        cm.compare((seed, k, cm.NAMES[c.from_t], cm.NAMES[c.to_t], len(c.slots), c.offset, c.residency, out_res), o, c.expected())
