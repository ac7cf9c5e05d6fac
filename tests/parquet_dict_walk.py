"""The pages of one column chunk of a Parquet file from the chunk's DICTIONARY page on, as they lie in the file (data page v1,
UNCOMPRESSED or SNAPPY): what tests/parquet_page_walk.py, which starts at data_page_offset, cannot see.  And the contract of
include/bowgpu.h for an RLE_DICTIONARY chunk restated in a few lines - expected_dictionary, expected_section - beside a decoder of
the RLE / bit-packed hybrid (restated from the Parquet format specification) that reads pyarrow's index sections as well."""
import struct

import numpy as np
import pyarrow as pa

from parquet_page_walk import _varint

DICT_MAX = 65536


def _skip(b, p, t):
    """the position behind a value of Thrift compact type t"""
    if t in (1, 2):
        return p
    if t == 3:
        return p + 1
    if t in (4, 5, 6):
        return _varint(b, p)[1]
    if t == 7:
        return p + 8
    if t == 8:
        n, p = _varint(b, p)
        return p + n
    if t in (9, 10):
        n, et = b[p] >> 4, b[p] & 15
        p += 1
        if n == 15:
            n, p = _varint(b, p)
        for _ in range(n):
            p = _skip(b, p, et)
        return p
    if t == 12:
        return _struct(b, p)[1]
    raise AssertionError("Thrift type %d" % t)


def _struct(b, p):
    """{field id: value} of the struct at b[p:] - i32 / i64 as ints, nested structs as dicts, whatever else a writer puts into a page
    header (pyarrow: statistics with binary fields, booleans) skipped - and the position behind its stop byte"""
    out, fid = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        if h >> 4:
            fid += h >> 4
        else:
            v, p = _varint(b, p)
            fid = (v >> 1) ^ -(v & 1)
        t = h & 15
        if t in (4, 5, 6):
            v, p = _varint(b, p)
            out[fid] = (v >> 1) ^ -(v & 1)
        elif t == 12:
            out[fid], p = _struct(b, p)
        else:
            p = _skip(b, p, t)


def chunk_pages(path, chunk):
    """chunk: pyarrow's ColumnChunkMetaData of an OPTIONAL INT64 / DOUBLE column.  Returns (dictionary, pages): the dictionary page's
    entries as uint64 (None: the chunk has no dictionary page) and per data page (num_values, encoding, level bytes without their
    4-byte length, value bytes).  The page headers and bodies fill total_compressed_size from the chunk's first page on, and header +
    uncompressed sizes sum to total_uncompressed_size."""
    start = chunk.dictionary_page_offset if chunk.has_dictionary_page else chunk.data_page_offset
    with open(path, "rb") as fh:
        fh.seek(start)
        b = fh.read(chunk.total_compressed_size)
    assert chunk.compression in ("UNCOMPRESSED", "SNAPPY"), chunk.compression
    codec = pa.Codec("snappy") if chunk.compression == "SNAPPY" else None
    dictionary, pages, p, raw = None, [], 0, 0
    while p < len(b):
        p0 = p
        h, p = _struct(b, p)
        comp, p = bytes(b[p:p + h[3]]), p + h[3]
        body = codec.decompress(comp, decompressed_size=h[2]).to_pybytes() if codec else comp
        assert len(body) == h[2], h
        raw += (p - p0) - h[3] + h[2]
        if h[1] == 2:   # DICTIONARY_PAGE: first in the chunk, once, PLAIN (pyarrow still says PLAIN_DICTIONARY = 2 there)
            assert dictionary is None and not pages and p0 == 0
            assert h[7][2] in (0, 2) and len(body) == 8 * h[7][1], h
            if chunk.has_dictionary_page:
                assert chunk.data_page_offset == start + p and chunk.data_page_offset - start >= 4
            dictionary = np.frombuffer(body, dtype=np.uint64)
        else:
            assert h[1] == 0, h   # DATA_PAGE
            (lv,) = struct.unpack_from("<I", body, 0)
            lv += 4
            pages.append((h[5][1], h[5][2], body[4:lv], body[lv:]))
    assert p == len(b) and raw == chunk.total_uncompressed_size, (p, len(b), raw, chunk.total_uncompressed_size)
    return dictionary, pages


# ------------------------------------------------------------------ the contract, restated
def expected_dictionary(dense):
    """the distinct 64-bit patterns of the chunk's non-null values, ascending as unsigned integers"""
    return np.unique(np.ascontiguousarray(dense).view(np.uint64))


def width_of(entries):
    return max(1, (entries - 1).bit_length())


def expected_section(dense_page, dictionary):
    """the width byte and, where the page has a value, ONE bit-packed run of its indices, LSB first, padded to a group of 8 values"""
    w, k = width_of(len(dictionary)), len(dense_page)
    if k == 0:
        return bytes([w])
    idx = np.searchsorted(dictionary, np.ascontiguousarray(dense_page).view(np.uint64)).astype(np.uint64)
    groups = (k + 7) // 8
    bits = np.zeros((8 * groups, w), dtype=np.uint8)
    bits[:k] = (idx[:, None] >> np.arange(w, dtype=np.uint64)) & 1
    head, v = b"", (groups << 1) | 1
    while v >= 0x80:
        head, v = head + bytes([(v & 0x7f) | 0x80]), v >> 7
    return bytes([w]) + head + bytes([v]) + np.packbits(bits.reshape(-1), bitorder="little").tobytes()


def decode_section(section, k):
    """the k indices of an RLE_DICTIONARY values section: any sequence of RLE and bit-packed runs"""
    w, p, out = section[0], 1, []
    assert 0 <= w <= 32
    while len(out) < k:
        h, p = _varint(section, p)
        if h & 1:
            n = 8 * (h >> 1)
            raw = np.frombuffer(section, dtype=np.uint8, count=(n * w + 7) // 8, offset=p)
            p += len(raw)
            bits = np.unpackbits(raw, bitorder="little")[:n * w].reshape(n, w).astype(np.uint64)
            out += (bits << np.arange(w, dtype=np.uint64)).sum(axis=1).tolist()
        else:
            nb = (w + 7) // 8
            out += [int.from_bytes(section[p:p + nb], "little")] * (h >> 1)
            p += nb
    return np.array(out[:k], dtype=np.int64), p
