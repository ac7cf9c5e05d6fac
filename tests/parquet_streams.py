"""Parquet byte streams built element by element, beside tests/parquet_pages.py: what no encoder can be asked to emit.  Snappy
blocks from explicit literals and copies in a chosen form; the RLE / bit-packed hybrid (definition levels, dictionary indices) from
explicit runs at any bit width from 0 to 32; and a one-column file whose pages take these bytes as they are - codec 0 or 1, a
dictionary page with or without dictionary_page_offset, data pages v1 / v2 (v2 also stored inside a SNAPPY chunk), PLAIN and
dictionary pages mixed.  The formats are restated from the Snappy format description and the Parquet format specification; pyarrow
reads the well-formed results back and refuses the damaged ones (tests/test_parquet_streams_cpu.py): that validates the builders."""
import struct

import numpy as np

from parquet_pages import DOUBLE, INT64, PLAIN, _Struct, _uleb   # noqa: F401  (re-exported for the tests)

RLE_DICTIONARY = 8


# ---------------------------------------------------------------- Snappy
def literal_forms(n):
    """the length forms (count of extra length bytes, 0 .. 4) that can hold a literal of n bytes"""
    return ([0] if n <= 60 else []) + [k for k in (1, 2, 3, 4) if n <= 1 << (8 * k)]


def copy_forms(off, n):
    """the copy forms (tag 1, 2, 3) that can express (off, n)"""
    return ([1] if 4 <= n <= 11 and off < 2048 else []) + ([2] if 1 <= n <= 64 and off < 65536 else []) + ([3] if 1 <= n <= 64 else [])


def literal(data, length_form=None):
    n = len(data)
    assert n >= 1
    form = literal_forms(n)[0] if length_form is None else length_form
    assert form in literal_forms(n), (n, form)
    if form == 0:
        return bytes([(n - 1) << 2]) + bytes(data)
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little") + bytes(data)


def copy(off, n, form):
    """the bytes of one copy element; nothing is checked beyond what the form can hold (damaged streams use it too)"""
    if form == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048
        return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 0xff])
    assert 1 <= n <= 64 and form in (2, 3)
    return bytes([form | ((n - 1) << 2)]) + off.to_bytes(2 if form == 2 else 4, "little")


class Snappy:
    """a Snappy block under construction: `out` is what it must decompress to, kept by the plain meaning of each element"""

    def __init__(self):
        self.elements, self.out = bytearray(), bytearray()

    def literal(self, data, length_form=None):
        self.elements += literal(data, length_form)
        self.out += bytes(data)
        return self

    def copy(self, off, n, form):
        assert 1 <= off <= len(self.out)
        self.elements += copy(off, n, form)
        for _ in range(n):
            self.out.append(self.out[-off])
        return self

    def pad_to(self, multiple, rng):
        """a closing literal that brings the output to a multiple of `multiple` bytes (a PLAIN page holds whole values)"""
        k = -len(self.out) % multiple
        return self.literal(bytes(rng.integers(0, 256, k, dtype=np.uint8))) if k else self

    def stream(self, declared=None):
        return _uleb(len(self.out) if declared is None else declared) + bytes(self.elements)


def one_literal(data, length_form=None):
    """`data` as a Snappy block of one literal (an empty block is its preamble alone)"""
    return _uleb(len(data)) + (literal(data, length_form) if data else b"")


class SnappyError(ValueError):
    pass


def snappy_decode(stream):
    """plain decoder of a raw Snappy block; SnappyError for every kind of damage"""
    size = sh = p = 0
    while True:
        if p >= len(stream) or sh > 28:
            raise SnappyError("preamble")
        c = stream[p]
        p += 1
        size |= (c & 0x7f) << sh
        sh += 7
        if not c & 0x80:
            break
    out = bytearray()
    while p < len(stream):
        tag, kind = stream[p], stream[p] & 3
        p += 1
        if kind == 0:
            n = (tag >> 2) + 1
            if n > 60:
                k = n - 60
                if p + k > len(stream):
                    raise SnappyError("literal length cut off")
                n = int.from_bytes(stream[p:p + k], "little") + 1
                p += k
            if p + n > len(stream):
                raise SnappyError("literal overruns the input")
            out += stream[p:p + n]
            p += n
        else:
            k = (1, 2, 4)[kind - 1]
            if p + k > len(stream):
                raise SnappyError("offset cut off")
            if kind == 1:
                n, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | stream[p]
            else:
                n, off = (tag >> 2) + 1, int.from_bytes(stream[p:p + k], "little")
            p += k
            if off == 0 or off > len(out):
                raise SnappyError("offset %d at output position %d" % (off, len(out)))
            for _ in range(n):
                out.append(out[-off])
        if len(out) > size:
            raise SnappyError("output overruns the declared length")
    if len(out) != size:
        raise SnappyError("%d bytes for a declared length of %d" % (len(out), size))
    return bytes(out)


# ---------------------------------------------------------------- RLE / bit-packed hybrid
def hybrid(runs, bw):
    """runs: ("rle", value, count) | ("bp", values): a bit-packed run is padded with zeros to whole groups of 8 values"""
    out = bytearray()
    for run in runs:
        if run[0] == "rle":
            out += _uleb(run[2] << 1) + int(run[1]).to_bytes((bw + 7) // 8, "little")
        else:
            vals = [int(v) for v in run[1]]
            groups = (len(vals) + 7) // 8
            acc = 0
            for k, v in enumerate(vals):
                assert 0 <= v < max(1 << bw, 1)
                acc |= v << (k * bw)
            out += _uleb((groups << 1) | 1) + acc.to_bytes(groups * bw, "little")
    return bytes(out)


def expand(runs, count=None):
    """the values the runs stand for, padding of bit-packed groups included, cut to `count`"""
    vals = []
    for run in runs:
        vals += [int(run[1])] * run[2] if run[0] == "rle" else [int(v) for v in run[1]] + [0] * (-len(run[1]) % 8)
    return np.array(vals[:count], dtype=np.int64)


# ---------------------------------------------------------------- pages and the file
class _S(_Struct):
    def bool(self, fid, v):
        self._hdr(fid, 1 if v else 2)
        return self


class Page:
    """One data page.  rows: num_values of the header; levels: the hybrid bytes of the definition levels (OPTIONAL columns; no
    length prefix - v1 pages get theirs here); values: the values section (a dictionary page: width byte + index bytes).
    comp: the compressed bytes of the page (v1: of prefix + levels + values; v2: of the values section), None = one literal in a
    SNAPPY chunk, the bytes themselves in an UNCOMPRESSED one.  stored: a v2 page with is_compressed = false."""

    def __init__(self, rows, values, encoding=PLAIN, levels=b"", v2=False, comp=None, stored=False, nulls=0, claim=None):
        self.rows, self.values, self.encoding, self.levels = rows, bytes(values), encoding, bytes(levels)
        self.v2, self.comp, self.stored, self.nulls = v2, comp, stored, nulls
        self.claim = claim   # a damaged header: the uncompressed_page_size it states instead of the true one
        assert not stored or v2


def _squeeze(data, codec, comp):
    if comp is not None:
        return bytes(comp)
    return one_literal(data) if codec == 1 else data


def write_file(path, pages, ptype=INT64, optional=False, codec=0, dictionary=None, dictionary_page_offset=True, name="c"):
    """dictionary: the chunk's dictionary values (a PLAIN dictionary page in front of the data pages), or None.  Without
    dictionary_page_offset the metadata's data_page_offset names the dictionary page, as the writers that leave the field out do."""
    out = bytearray(b"PAR1")
    raw_total = 0
    encs = {3}
    if dictionary is not None:
        body = np.ascontiguousarray(dictionary).view(np.uint64).astype("<u8").tobytes()
        comp = _squeeze(body, codec, None)
        hdr = _S().i32(1, 2).i32(2, len(body)).i32(3, len(comp)).struct(7, _S().i32(1, len(dictionary)).i32(2, PLAIN)).done()
        out += hdr + comp
        raw_total += len(hdr) + len(body)
        encs.add(PLAIN)
    data_off = len(out)
    rows = 0
    for pg in pages:
        if pg.v2:
            comp = pg.values if pg.stored else _squeeze(pg.values, codec, pg.comp)
            dph = (_S().i32(1, pg.rows).i32(2, pg.nulls).i32(3, pg.rows).i32(4, pg.encoding).i32(5, len(pg.levels)).i32(6, 0)
                   .bool(7, not pg.stored))
            raw = len(pg.levels) + len(pg.values)
            hdr = _S().i32(1, 3).i32(2, raw if pg.claim is None else pg.claim).i32(3, len(pg.levels) + len(comp)).struct(8, dph).done()
            out += hdr + pg.levels + comp
        else:
            body = (struct.pack("<I", len(pg.levels)) + pg.levels if optional else b"") + pg.values
            comp = _squeeze(body, codec, pg.comp)
            raw = len(body)
            dph = _S().i32(1, pg.rows).i32(2, pg.encoding).i32(3, 3).i32(4, 3)   # levels: RLE
            hdr = _S().i32(1, 0).i32(2, raw if pg.claim is None else pg.claim).i32(3, len(comp)).struct(5, dph).done()
            out += hdr + comp
        raw_total += len(hdr) + raw
        encs.add(pg.encoding)
        rows += pg.rows
    size = len(out) - 4
    meta = (_S().i32(1, ptype).list(2, 5, [_uleb(e << 1) for e in sorted(encs)]).list(3, 8, [_uleb(len(name)) + name.encode()])
            .i32(4, codec).i64(5, rows).i64(6, raw_total).i64(7, size))
    if dictionary is not None and dictionary_page_offset:
        meta.i64(9, data_off).i64(11, 4)
    else:
        meta.i64(9, 4)
    chunk = _S().i64(2, 4).struct(3, meta)
    group = _S().list(1, 12, [chunk.done()]).i64(2, raw_total).i64(3, rows)
    schema = [_S().string(4, "schema").i32(5, 1).done(), _S().i32(1, ptype).i32(3, 1 if optional else 0).string(4, name).done()]
    footer = _S().i32(1, 1).list(2, 12, schema).i64(3, rows).list(4, 12, [group.done()]).string(6, "parquet_streams.py").done()
    out += footer + struct.pack("<I", len(footer)) + b"PAR1"
    with open(path, "wb") as fh:
        fh.write(bytes(out))


# ---------------------------------------------------------------- pages from a column's values
def plain_page(values, valid=None, level_runs=None, **kw):
    """a PLAIN page of `values` (one per ROW); valid: the rows that are not null (OPTIONAL); level_runs: the runs that say so
    (default: one bit-packed run)"""
    values = np.asarray(values)
    if valid is None:
        return Page(len(values), values.view(np.uint64).astype("<u8").tobytes(), **kw)
    valid = np.asarray(valid, dtype=bool)
    runs = [("bp", valid.astype(int))] if level_runs is None else level_runs
    assert np.array_equal(expand(runs, len(valid)), valid.astype(np.int64))
    return Page(len(values), values[valid].view(np.uint64).astype("<u8").tobytes(), levels=hybrid(runs, 1),
                nulls=int((~valid).sum()), **kw)


def dict_page(index_runs, bw, rows, valid=None, level_runs=None, width_byte=None, **kw):
    """a dictionary-encoded page: the width byte and the hybrid of `index_runs`, one index per non-null row"""
    vals = bytes([bw if width_byte is None else width_byte]) + hybrid(index_runs, bw)
    if valid is None:
        return Page(rows, vals, encoding=RLE_DICTIONARY, **kw)
    valid = np.asarray(valid, dtype=bool)
    assert len(valid) == rows
    runs = [("bp", valid.astype(int))] if level_runs is None else level_runs
    return Page(rows, vals, encoding=RLE_DICTIONARY, levels=hybrid(runs, 1), nulls=int((~valid).sum()), **kw)
