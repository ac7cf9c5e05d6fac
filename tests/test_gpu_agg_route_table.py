"""Which kernel a Rolling.Aggregate call takes, for about four thousand calls on both sides of every routing threshold:
tests/agg_route_table.json (written by scratch/agg_route_table.py BEFORE the host path of api.cpp was folded, so it is that code's
behaviour).  A cell records capi.last_kernel_name(), whether info.long_windows is 0 / num_windows / something else, and whether the
general kernel took rows.  A routing change on purpose regenerates the table; anything else that moves a cell is a regression."""
import json
import os

import pytest

import agg_route_cells as cells

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "agg_route_table.json")) as _f:
    TABLE = json.load(_f)


@pytest.fixture(scope="module")
def data():
    return cells.Data(max(cells.rows_n(r) for r in set(cells.ROWS) | set(cells.ROWS_VARIANTS)))


@pytest.fixture(scope="module")
def big_data():
    return cells.Data(cells.BIG_N)


def test_the_table_holds_exactly_the_cells_of_the_spec():
    want = {k for col, rows in cells.groups() for k in cells.keys_of(col, rows)}
    assert set(TABLE["cells"]) == want
    assert all(len(v) == len(cells.REDUCER_SETS) for v in TABLE["cells"].values())
    assert TABLE["reducer_sets"] == [list(s) for s in cells.REDUCER_SETS]


@pytest.mark.parametrize("col,rows", cells.groups(), ids=lambda v: str(v))
def test_routes(col, rows, request):
    d = request.getfixturevalue("big_data" if rows == "big" else "data")
    names = list(TABLE["names"])
    wrong = []
    for suffix, n, interval, variants in cells.group_shapes(rows):
        for variant in variants:
            key = "%s|%s|%s" % (col, suffix, variant)
            want = TABLE["cells"][key]   # (a cell the table lacks fails here)
            for reducers, w in zip(cells.REDUCER_SETS, want):
                got = cells.run_cell(d, col, n, interval, variant, reducers, names)
                if got != w:
                    wrong.append((key, reducers, describe(got, names), describe(w, names)))
    assert not wrong, "%d cells left their route (cell, reducers, now, table): %s" % (len(wrong), wrong[:8])


def describe(code, names):
    if code < 0:
        return "error %d" % -code
    return "%s long=%s slow=%d" % (names[code // 6], ("none", "all", "some")[code // 2 % 3], code & 1)
