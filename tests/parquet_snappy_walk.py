"""The data pages of one SNAPPY column chunk of a Parquet file, as they lie in the file (data page v1): what
tests/parquet_page_walk.py shows for an UNCOMPRESSED chunk, after pyarrow's Snappy decompressor, and the page's element stream
parsed here (restated from the Snappy format description): every literal and copy with its length, its distance and the position of
its first output byte."""
import struct

import pyarrow as pa

from parquet_page_walk import _struct, _varint

LITERAL, COPY = 0, 1


def elements(stream):
    """(uncompressed size by the preamble, [(kind, length, distance (0 for a literal), output position, bytes of the element's tag)])"""
    size, p = _varint(stream, 0)
    out, at = [], 0
    while p < len(stream):
        tag, kind = stream[p], stream[p] & 3
        if kind == 0:
            n, t = tag >> 2, 1
            if n >= 60:
                t = 1 + n - 59
                n = int.from_bytes(stream[p + 1:p + t], "little")
            n += 1
            out.append((LITERAL, n, 0, at, t))
            p += t + n
        elif kind == 1:
            n, d, t = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | stream[p + 1], 2
            out.append((COPY, n, d, at, t))
            p += t
        else:
            t = 3 if kind == 2 else 5
            n, d = 1 + (tag >> 2), int.from_bytes(stream[p + 1:p + t], "little")
            out.append((COPY, n, d, at, t))
            p += t
        at += n
    assert p == len(stream) and at == size, (p, len(stream), at, size)
    return size, out


def pages(path, chunk):
    """chunk: pyarrow's ColumnChunkMetaData of an OPTIONAL column.  Yields per data page (num_values, encoding, level bytes, value
    bytes, compressed section, elements): the level bytes without their 4-byte length, as parquet_page_walk.pages gives them."""
    with open(path, "rb") as fh:
        fh.seek(chunk.data_page_offset)
        b = fh.read(chunk.total_compressed_size)
    codec = pa.Codec("snappy")
    p = raw = 0
    while p < len(b):
        p0 = p
        h, p = _struct(b, p)
        assert h[1] == 0, h   # DATA_PAGE
        comp, p = bytes(b[p:p + h[3]]), p + h[3]
        size, els = elements(comp)
        assert size == h[2], (size, h)
        body = codec.decompress(comp, decompressed_size=h[2]).to_pybytes()
        assert len(body) == h[2]
        (lv,) = struct.unpack_from("<I", body, 0)
        lv += 4
        raw += (p - p0) - h[3] + h[2]
        yield h[5][1], h[5][2], body[4:lv], body[lv:], comp, els
    assert p == len(b) and raw == chunk.total_uncompressed_size, (p, len(b), raw, chunk.total_uncompressed_size)


def values_elements(els, levels_len):
    """the elements behind the levels literal(s), with positions counted from the first byte of the values section"""
    start, out = 4 + levels_len, []
    for kind, n, d, at, t in els:
        if at < start:
            assert kind == LITERAL and at + n <= start, "the levels section is not a literal of its own"
            continue
        out.append((kind, n, d, at - start, t))
    return out
