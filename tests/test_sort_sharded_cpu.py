"""bowgpu_sort_by_col_sharded without a GPU: everything the call decides about host-resident shards before it touches a device - the
errors bowgpu_sort_by_col gives for the concatenated frame (the reference's "nil values" message with the count summed over the
ranks, the type and column checks), the sharded frame's own (world, schema, lengths, capacities naming rank and size, the row limit
of a rank) - is answered on a box that has none, with the outputs untouched.  A frame of fewer than two rows is in order there too;
a valid call of two rows is BOWGPU_ERR_NO_DEVICE: the path has no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from bow_amd import capi

POISON = 0x5A5A5A5A5A5A5A5A


def _gpu_count():
    try:
        return capi.device_count()
    except capi.BowGpuError:
        return 0


def frame(keys, vals=None, key_type="int64"):
    """one rank: a key column and a Float64 value column (None: a null)"""
    vals = [float(i) for i in range(len(keys))] if vals is None else vals
    return [capi.Column.from_list(keys, key_type), capi.Column.from_list(vals, "float64")]


def fresh_outs(ranks, slots=None):
    return [[capi.OutColumn(cols[0].length if slots is None else slots[r]) for _ in cols] for r, cols in enumerate(ranks)]


def untouched(outs):
    for o_rank in outs:
        for o in o_rank:
            assert o.null_count == -1 and o.type == 0 and o.length == o.slots
            assert (o.values == POISON).all() and (o.validity == 0xA5).all()


def fails(ranks, key_col=0, ids=None, outs=None):
    outs = fresh_outs(ranks) if outs is None else outs
    with pytest.raises(capi.BowGpuError) as e:
        capi.sort_by_col_sharded(ranks, key_col, [0] * len(ranks) if ids is None else ids, outs=outs)
    untouched(outs)
    return e.value


def test_symbol_and_version():
    assert "bowgpu_sort_by_col_sharded" in capi.SYMBOLS and capi.ABI_VERSION == 14
    assert hasattr(capi.lib(), "bowgpu_sort_by_col_sharded")
    assert capi.MERGE_TILE_ROWS == 2048


def test_nulls_in_the_key_carry_the_count_summed_over_the_ranks():
    ranks = [frame([5, None, 3]), frame([]), frame([None, None, 1, 9]), frame([2, 4])]
    e = fails(ranks)
    assert e.code == -16 and e.message == "column to sort by has 3 nil values"
    # counted from the bitmaps when the caller says -1, a slice at an odd offset included
    k = capi.Column.from_list([5, None, 3, None, None, 1, 9], "int64")
    sl = capi.Column(k.values, k.validity, capi.INT64, offset=3, length=4, null_count=-1)
    v = capi.Column.from_list([1.0] * 7, "float64")
    vs = capi.Column(v.values, v.validity, capi.FLOAT64, offset=3, length=4, null_count=-1)
    e = fails([[sl, vs], frame([None, 7])])
    assert e.code == -16 and e.message == "column to sort by has 3 nil values"


def test_key_and_column_checks_of_the_one_device_call():
    good = frame([3, 1, 2])
    boolean = capi.Column.from_list([True, False, True], "bool")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    e = fails([[boolean, val], [boolean, val]])                       # key of a type Less is not served for
    assert e.code == -7
    for bad in (-1, 2, 7):
        e = fails([good, frame([9, 8])], key_col=bad)
        assert e.code == -6, bad
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3)
    for other in (boolean, string):                                   # a value column the device path does not move, on every rank
        e = fails([[good[0], other], [good[0], other]])
        assert e.code == -9
    e = fails([good, [capi.Column.from_list([1, 2], "int64"), capi.Column.from_list([1.0], "float64")]])   # a rank's columns differ in length
    assert e.code == -10 and "rank 1" in e.message


def test_schema_mismatch_between_ranks():
    a = frame([3, 1, 2])
    b = [capi.Column.from_list([3, 1], "int64"), capi.Column.from_list([4, 5], "int64")]
    e = fails([a, b])
    assert e.code == -10 and "rank 1" in e.message and "column 1" in e.message
    f = frame([2.0, 1.0], key_type="float64")                         # the key's own type differs
    e = fails([a, f])
    assert e.code == -10 and "rank 1" in e.message and "column 0" in e.message


def test_world_and_null_lists():
    one = frame([2, 1])
    L = capi.lib()
    unchanged = C.c_int32(0)
    ids = (C.c_int32 * 65)()
    carr = capi._cols(one)
    cptrs = (C.POINTER(capi.Col) * 65)(*[C.cast(carr, C.POINTER(capi.Col))] * 65)
    outs = [capi.OutColumn(2), capi.OutColumn(2)]
    oarr = (capi.Out * 2)(outs[0].c(), outs[1].c())
    optrs = (C.POINTER(capi.Out) * 65)(*[C.cast(oarr, C.POINTER(capi.Out))] * 65)
    for world in (0, 65, -3):
        rc = L.bowgpu_sort_by_col_sharded(cptrs, ids, world, 2, 0, optrs, C.byref(unchanged))
        assert rc == -10 and b"world" in L.bowgpu_last_error(), world
    for args in ((None, ids, 1, 2, 0, optrs, C.byref(unchanged)), (cptrs, None, 1, 2, 0, optrs, C.byref(unchanged)),
                 (cptrs, ids, 1, 2, 0, None, C.byref(unchanged)), (cptrs, ids, 1, 2, 0, optrs, None)):
        assert L.bowgpu_sort_by_col_sharded(*args) == -10
    holes = (C.POINTER(capi.Col) * 2)(C.cast(carr, C.POINTER(capi.Col)), None)       # a rank without a column array
    rc = L.bowgpu_sort_by_col_sharded(holes, ids, 2, 2, 0, optrs, C.byref(unchanged))
    assert rc == -10 and b"rank 1" in L.bowgpu_last_error()
    untouched([outs])


def test_capacity_names_rank_and_size():
    ranks = [frame([3, 1, 2]), frame([9, 8, 7, 6])]
    outs = fresh_outs(ranks, slots=[3, 3])
    e = fails(ranks, outs=outs)
    assert e.code == -10 and "rank 1" in e.message and "3 slots" in e.message and "4 needed" in e.message
    # capacity beyond the row count suffices (decided without a device: the next thing the call asks for is one)
    outs = fresh_outs([frame([]), frame([4])], slots=[0, 5])
    _, unchanged = capi.sort_by_col_sharded([frame([]), frame([4])], 0, [0, 0], outs=outs)
    assert unchanged
    untouched(outs)


def test_a_rank_of_two_to_the_31_rows_names_the_limit():
    big = [capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 2 ** 31), capi.Column(np.zeros(1, np.float64), None, capi.FLOAT64, 0, 2 ** 31)]
    outs = [[capi.OutColumn(2), capi.OutColumn(2)], [capi.OutColumn(1), capi.OutColumn(1)]]   # (the limit is reported before any capacity is looked at)
    e = fails([frame([2, 1]), big], outs=outs)
    assert e.code == -9 and "rank 1" in e.message and "2^31 = 2147483648" in e.message


def test_fewer_than_two_rows_are_in_order_without_a_device():
    for shards in ([[]], [[], []], [[7]], [[], [7], []], [[], [], [], [], [3.5]]):
        typ = "float64" if any(isinstance(x, float) for s in shards for x in s) else "int64"
        ranks = [frame(s, key_type=typ) for s in shards]
        outs, unchanged = capi.sort_by_col_sharded(ranks, 0, [0] * len(ranks))
        assert unchanged
        untouched(outs)


def test_two_rows_need_a_device_and_the_info_of_a_call_that_never_ran_is_empty():
    ranks = [frame([10]), frame([5])]
    outs = fresh_outs(ranks)
    if _gpu_count() == 0:            # (that one assertion: with a GPU the call is served - tests/test_gpu_sort_sharded.py)
        with pytest.raises(capi.BowGpuError) as e:
            capi.sort_by_col_sharded(ranks, 0, [0, 0], outs=outs)
        assert e.value.code == -11
        untouched(outs)
    fails([frame([5, None, 3]), frame([1])])
    info = capi.sort_by_col_sharded_info()
    assert (info.splitter_rounds, info.merge_rounds, info.sort_passes, info.merged_ranks) == (0, 0, 0, 0)
    assert info.local_sort_ms == info.splitter_ms == info.merge_ms == 0.0
    assert "bowgpu_sort_by_col_sharded_info" in capi.SYMBOLS


def test_unchanged_is_cleared_by_a_call_that_fails():
    ranks = [frame([3, None]), frame([1])]
    carrs = [capi._cols(r) for r in ranks]
    cptrs = (C.POINTER(capi.Col) * 2)(*[C.cast(a, C.POINTER(capi.Col)) for a in carrs])
    outs = fresh_outs(ranks)
    oarrs = [(capi.Out * 2)(*[o.c() for o in rank]) for rank in outs]
    optrs = (C.POINTER(capi.Out) * 2)(*[C.cast(a, C.POINTER(capi.Out)) for a in oarrs])
    unchanged = C.c_int32(1)
    ids = (C.c_int32 * 2)(0, 0)
    assert capi.lib().bowgpu_sort_by_col_sharded(cptrs, ids, 2, 2, 0, optrs, C.byref(unchanged)) == -16
    assert unchanged.value == 0
    if _gpu_count() == 0:            # a valid call that finds no device does not say "unchanged" either
        good = [capi._cols(frame([10])), capi._cols(frame([5]))]
        gptrs = (C.POINTER(capi.Col) * 2)(*[C.cast(a, C.POINTER(capi.Col)) for a in good])
        o1 = [[capi.OutColumn(1), capi.OutColumn(1)] for _ in range(2)]
        oa = [(capi.Out * 2)(*[o.c() for o in rank]) for rank in o1]
        op = (C.POINTER(capi.Out) * 2)(*[C.cast(a, C.POINTER(capi.Out)) for a in oa])
        unchanged = C.c_int32(1)
        assert capi.lib().bowgpu_sort_by_col_sharded(gptrs, ids, 2, 2, 0, op, C.byref(unchanged)) == -11
        assert unchanged.value == 0
