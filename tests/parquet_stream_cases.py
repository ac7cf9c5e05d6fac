"""The hand-built files and Snappy blocks of tests/test_parquet_streams_cpu.py (pyarrow reads / refuses them) and
tests/test_gpu_parquet_streams.py (the device loader reads / refuses the same ones), built with tests/parquet_streams.py.

good_files(dir)     name -> (path, values, valid): the intended column, one entry per row (null rows hold 0)
damaged_files(dir)  name -> (path, path of the undamaged twin or None)
good_blocks()       name -> Snappy builder (stream() and the intended bytes `out`)
damaged_blocks()    name -> (stream, declared uncompressed size)"""
import os

import numpy as np

import parquet_streams as ps

COPY_OFFSETS = (1, 2, 3, 7, 8, 63, 64, 65)
COPY_LENGTHS = (4, 11, 12, 63, 64)
LITERAL_LENGTHS = (1, 60, 61, 64, 65, 256, 257, 65537)
INDEX_WIDTHS = (0, 1, 7, 8, 9, 16, 17, 24, 25, 31, 32)
DICT_SIZE = 5


def _bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


# ---------------------------------------------------------------- Snappy blocks
def good_blocks():
    rng = np.random.default_rng(71)
    out = {}
    # every (off, len) in every form that can express it: once behind a prefix that is no multiple of 8, once more three bytes later
    for off in COPY_OFFSETS:
        for n in COPY_LENGTHS:
            for form in ps.copy_forms(off, n):
                s = ps.Snappy().literal(_bytes(rng, 65 + (off + n) % 7))
                s.copy(off, n, form).literal(_bytes(rng, 3)).copy(off, n, form)
                out["copy_form%d_off%d_len%d" % (form, off, n)] = s.pad_to(8, rng)
    # a copy whose offset equals the bytes written so far (it reaches byte 0), at three fill levels
    for k, form in ((13, 1), (64, 2), (333, 3)):
        s = ps.Snappy().literal(_bytes(rng, k))
        s.copy(k, 11, form).copy(k + 11, 11, form)
        out["copy_reaches_byte0_%d" % k] = s.pad_to(8, rng)
    # three copies, each reading only what the copy before it wrote; behind prefixes that are no multiples of 8 or 64
    for prefix in (5, 67, 129):
        for n in (5, 64):
            s = ps.Snappy().literal(_bytes(rng, prefix))
            s.copy(n if n <= prefix else prefix, n, 2).copy(n, n, 2).copy(n, n, 3).copy(n, n, 2)
            out["copy_chain_%d_%d" % (prefix, n)] = s.pad_to(8, rng)
        s = ps.Snappy().literal(_bytes(rng, prefix))
        s.copy(1, 64, 2).copy(63, 64, 2).copy(1, 7, 3).copy(7, 64, 2)   # overlapping ones: each source was just written
        out["copy_chain_overlap_%d" % prefix] = s.pad_to(8, rng)
    for n in LITERAL_LENGTHS:
        for form in ps.literal_forms(n):
            out["literal_%d_form%d" % (n, form)] = ps.Snappy().literal(_bytes(rng, n), form).pad_to(8, rng)
    s = ps.Snappy()
    for _ in range(200):
        s.literal(_bytes(rng, 1))
    out["one_byte_literals"] = s
    return out


def damaged_blocks():
    """every block should give 64 bytes, by its page's header"""
    rng = np.random.default_rng(72)
    lit = lambda n: ps.literal(_bytes(rng, n))   # noqa: E731
    pre = ps._uleb(64)
    return {
        "declared_smaller": (ps._uleb(56) + lit(64), 64),
        "declared_larger": (ps._uleb(72) + lit(64), 64),
        "offset_0": (pre + lit(56) + ps.copy(0, 8, 2), 64),
        "offset_past_output": (pre + lit(56) + ps.copy(57, 8, 2), 64),
        "copy_overruns_output": (pre + lit(60) + ps.copy(4, 8, 2), 64),
        "literal_overruns_input": (pre + lit(64)[:41], 64),
        "offset_cut_off": (pre + lit(56) + ps.copy(8, 8, 3)[:3], 64),
        "ends_short": (pre + lit(56), 64),
        "extra_element": (pre + lit(64) + lit(1), 64),
    }


# ---------------------------------------------------------------- files
def _values(rng, ptype, n):
    return rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64) if ptype == ps.INT64 else rng.standard_normal(n)


def _spread(rng, n_values, rows):
    valid = np.zeros(rows, dtype=bool)
    valid[rng.choice(rows, n_values, replace=False)] = True
    return valid


class _Files:
    def __init__(self, directory):
        self.dir, self.good, self.bad = str(directory), {}, {}

    def path(self, name):
        return os.path.join(self.dir, name + ".parquet")

    def add(self, name, pages, cols, **kw):
        """cols: per page (values per row, valid per row)"""
        ps.write_file(self.path(name), pages, **kw)
        vals = np.concatenate([c[0] for c in cols])
        valid = np.concatenate([np.ones(len(c[0]), dtype=bool) if c[1] is None else c[1] for c in cols])
        vals = vals.copy()
        vals[~valid] = 0
        self.good[name] = (self.path(name), vals, valid)

    def damaged(self, name, pages, twin=None, **kw):
        ps.write_file(self.path(name), pages, **kw)
        self.bad[name] = (self.path(name), self.good[twin][0] if twin else None)


def _snappy_files(F):
    groups = {}
    for name, s in good_blocks().items():
        group = name[:10] if name.startswith("copy_form") else "copy_chains" if name.startswith("copy_") else "literals"
        groups.setdefault("snappy_" + group, []).append(s)
    for name, blocks in groups.items():
        pages = [ps.Page(len(s.out) // 8, s.out, comp=s.stream()) for s in blocks]
        F.add(name, pages, [(np.frombuffer(bytes(s.out), dtype="<i8"), None) for s in blocks], codec=1)
    # the preamble (uncompressed length) in 1, 2 and 3 bytes
    rng = np.random.default_rng(73)
    vals = [_values(rng, ps.INT64, n) for n in (15, 16, 2047, 2048, 2049)]
    F.add("snappy_preambles", [ps.plain_page(v) for v in vals], [(v, None) for v in vals], codec=1)


def _index_page(rng, bw, ptype, dictionary, optional, form):
    """form 0: alternating RLE and bit-packed runs, the last group padded past the value count; 1: an RLE run longer than the
    values left; 2 / 3: a page of nulls only, without a values section / with the width byte alone"""
    top = min(1 << bw, DICT_SIZE)
    ix = lambda n: rng.integers(0, top, n)   # noqa: E731
    if form == 0:
        runs = [("rle", ix(1)[0], 9), ("bp", ix(16)), ("rle", ix(1)[0], 70), ("bp", ix(24)), ("rle", ix(1)[0], 3), ("bp", ix(5))]
        n = 127
    elif form == 1:
        runs, n = [("bp", ix(8)), ("rle", ix(1)[0], 1000)], 28
    else:
        runs, n = [], 0
    idx = ps.expand(runs, n)
    rows = n + n // 3 + 1 if optional else n
    if form >= 2:
        rows = 40
    valid = _spread(rng, n, rows) if optional else None
    full = np.zeros(rows, dtype=dictionary.dtype)
    full[valid if optional else slice(None)] = dictionary[idx]
    pg = ps.dict_page(runs, bw, rows, valid)
    if form == 2:
        pg.values = b""
    return pg, (full, valid)


def _index_files(F):
    rng = np.random.default_rng(74)
    for ptype, tname in ((ps.INT64, "int64"), (ps.DOUBLE, "double")):
        for optional in (False, True):
            for codec in (0, 1):
                dictionary = _values(rng, ptype, DICT_SIZE)
                pages, cols = [], []
                for bw in INDEX_WIDTHS:
                    for form in ((0, 1, 2, 3) if optional else (0, 1)):
                        pg, col = _index_page(rng, bw, ptype, dictionary, optional, form)
                        pages.append(pg)
                        cols.append(col)
                F.add("indices_%s_%s_codec%d" % (tname, "optional" if optional else "required", codec), pages, cols, ptype=ptype,
                      optional=optional, codec=codec, dictionary=dictionary)


def _level_page(rng, runs, rows, **kw):
    valid = ps.expand(runs, rows).astype(bool)
    assert len(valid) == rows
    vals = _values(rng, ps.INT64, rows)
    return ps.plain_page(vals, valid, level_runs=runs, **kw), (vals, valid)


def _level_files(F):
    rng = np.random.default_rng(75)
    rows = 2048 + 33
    for codec in (0, 1):
        for v2 in (False, True):
            pages, cols = [], []

            def add(runs, n):
                pg, col = _level_page(rng, runs, n, v2=v2)
                pages.append(pg)
                cols.append(col)
            for end in (2047, 2048, 2049):   # a run that ends just before, on and just behind the 2048-row batch edge
                add([("rle", 1, end), ("rle", 0, 7), ("rle", 1, rows - end - 7)], rows)
                add([("rle", 0, end), ("rle", 1, rows - end)], rows)
                add([("rle", end & 1, end - 2040), ("bp", rng.integers(0, 2, 2040)), ("rle", 1, 5), ("bp", rng.integers(0, 2, rows - end - 5))], rows)
            lens = (1, 31, 32, 33) * 3
            add([("rle", k & 1, n) for k, n in enumerate(lens)], sum(lens))
            add([("bp", rng.integers(0, 2, 32)), ("rle", 1, 1), ("rle", 0, 31), ("bp", rng.integers(0, 2, 8)), ("rle", 1, 33), ("bp", rng.integers(0, 2, 31))], 136)
            for n in (1, 31, 33, 70) * 2:   # small pages back to back: a page's first row falls inside a validity word
                add([("bp", rng.integers(0, 2, n))], n)
            F.add("levels_codec%d_v%d" % (codec, 2 if v2 else 1), pages, cols, optional=True, codec=codec)


def _chunk_files(F):
    rng = np.random.default_rng(76)
    for codec in (0, 1):
        for optional in (False, True):
            dictionary = _values(rng, ps.INT64, DICT_SIZE)
            tag = "codec%d_%s" % (codec, "optional" if optional else "required")

            def dict_pg():
                return _index_page(rng, 3, ps.INT64, dictionary, optional, 0)

            def plain_pg(n):
                vals = _values(rng, ps.INT64, n)
                valid = (rng.random(n) < 0.7) if optional else None
                return ps.plain_page(vals, valid), (vals, valid)

            def v2(item, stored=False):
                item[0].v2, item[0].stored = True, stored
                return item
            for name, items, kw in (
                    ("dict_then_plain", [dict_pg(), dict_pg(), plain_pg(77), dict_pg(), plain_pg(3)], {}),
                    ("no_dictionary_page_offset", [dict_pg(), plain_pg(9), dict_pg()], {"dictionary_page_offset": False}),
                    ("v2_stored_and_compressed", [v2(dict_pg(), True), v2(plain_pg(77), True), v2(dict_pg()), v2(plain_pg(50)), v2(plain_pg(9), True)], {})):
                F.add("chunk_%s_%s" % (name, tag), [it[0] for it in items], [it[1] for it in items], optional=optional, codec=codec,
                      dictionary=dictionary, **kw)
        # v2 pages of nulls only: no values section at all, compressed (an empty Snappy block) and stored
        nulls = (np.zeros(40, dtype=np.int64), np.zeros(40, dtype=bool))
        items = [(ps.plain_page(*nulls, level_runs=[("rle", 0, 40)], v2=True, stored=st), nulls) for st in (False, True)]
        some = _values(rng, ps.INT64, 21)
        items.insert(1, (ps.plain_page(some, np.ones(21, dtype=bool), v2=True), (some, None)))
        F.add("chunk_v2_nulls_only_codec%d" % codec, [it[0] for it in items], [it[1] for it in items], optional=True, codec=codec)


def good_files(directory):
    F = _Files(directory)
    _snappy_files(F)
    _index_files(F)
    _level_files(F)
    _chunk_files(F)
    return F.good


def damaged_files(directory):
    F = _Files(directory)
    rng = np.random.default_rng(77)
    vals64 = np.frombuffer(_bytes(rng, 64), dtype="<i8")
    for name, (stream, size) in damaged_blocks().items():
        F.damaged("snappy_" + name, [ps.Page(size // 8, vals64.tobytes(), comp=stream)], codec=1)
    # ---- dictionary indices
    dictionary = _values(rng, ps.INT64, DICT_SIZE)
    n = 300
    idx = rng.integers(0, DICT_SIZE, n)
    for optional in (False, True):
        tag = "optional" if optional else "required"
        rows = n + 100 if optional else n
        valid = _spread(rng, n, rows) if optional else None
        kw = dict(optional=optional, dictionary=dictionary)
        full = np.zeros(rows, dtype=np.int64)
        idx[160:200] = idx[160]
        whole = [("bp", idx[:160]), ("rle", idx[160], 40), ("bp", idx[200:])]
        full[valid if optional else slice(None)] = dictionary[idx]
        F.add("indices_twin_" + tag, [ps.dict_page(whole, 3, rows, valid)], [(full, valid)], **kw)
        for name, runs, wb in (
                ("width_33", whole, 33),
                ("index_equals_dictionary_size", [("bp", idx[:160]), ("rle", DICT_SIZE, 40), ("bp", idx[200:])], None),
                ("rle_count_0", [("rle", 1, 0)] + whole, None),
                ("ends_early_rle", [("bp", idx[:160]), ("rle", idx[160], 39)], None),
                ("ends_early_bit_packed", [("bp", idx[:160]), ("rle", idx[160], 40), ("bp", idx[200:280])], None)):
            F.damaged("indices_%s_%s" % (name, tag), [ps.dict_page(runs, 3, rows, valid, width_byte=wb)], twin="indices_twin_" + tag, **kw)
        pg = ps.dict_page([("bp", idx[:160])], 3, rows, valid)
        pg.values += ps._uleb((100_000 << 1) | 1) + b"\x55" * 12   # a bit-packed run of 300 000 bytes, 12 of them there
        F.damaged("indices_run_past_the_page_" + tag, [pg], twin="indices_twin_" + tag, **kw)
    # ---- definition levels that end before the page's rows do
    rows = 2048 + 300
    vals = _values(rng, ps.INT64, rows)
    lv = rng.integers(0, 2, rows)
    for v2 in (False, True):
        tag = "v2" if v2 else "v1"
        whole = [("bp", lv[:1600]), ("rle", 1, 500), ("bp", lv[2100:])]
        valid = ps.expand(whole, rows).astype(bool)
        F.add("levels_twin_" + tag, [ps.plain_page(vals, valid, level_runs=whole, v2=v2)], [(vals, valid)], optional=True)
        for name, runs in (("rle", [("bp", lv[:1600]), ("rle", 1, 480)]), ("bit_packed", [("bp", lv[:1600]), ("rle", 1, 500), ("bp", lv[2100:2300])])):
            short = ps.expand(runs).astype(bool)
            pg = ps.Page(rows, vals[:len(short)][short].view(np.uint64).astype("<u8").tobytes(), levels=ps.hybrid(runs, 1), v2=v2,
                         nulls=rows - int(short.sum()))
            F.damaged("levels_end_early_%s_%s" % (name, tag), [pg], twin="levels_twin_" + tag, optional=True)
    return F.bad, F.good
