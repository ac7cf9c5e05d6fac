"""The data pages of one column chunk of a Parquet file, as they lie in the file: the read side of the Thrift compact protocol for
PageHeader / DataPageHeader (restated from the Parquet format specification), for data page v1 of an UNCOMPRESSED chunk.  What
pyarrow does not show: a page's level bytes and value bytes."""
import struct


def _varint(b, p):
    r = sh = 0
    while True:
        c = b[p]
        p += 1
        r |= (c & 0x7f) << sh
        sh += 7
        if not c & 0x80:
            return r, p


def _struct(b, p):
    """{field id: value} of the struct at b[p:] (i32 / i64 as ints, nested structs as dicts; other types are not expected in a
    v1 data page header) and the position behind its stop byte"""
    out, fid = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        assert h >> 4, "long-form field ids are not expected in a page header"
        fid += h >> 4
        if h & 15 in (5, 6):
            v, p = _varint(b, p)
            out[fid] = (v >> 1) ^ -(v & 1)
        elif h & 15 == 12:
            out[fid], p = _struct(b, p)
        else:
            raise AssertionError("field %d of Thrift type %d in a page header" % (fid, h & 15))


def pages(path, chunk, optional=True):
    """chunk: pyarrow's ColumnChunkMetaData (data_page_offset, total_compressed_size).  Yields per data page
    (num_values, encoding, level bytes, value bytes); the level bytes are the definition-level section without its 4-byte length
    (b"" for a REQUIRED column)."""
    with open(path, "rb") as fh:
        fh.seek(chunk.data_page_offset)
        b = fh.read(chunk.total_compressed_size)
    p = 0
    while p < len(b):
        h, p = _struct(b, p)
        assert h[1] == 0 and h[2] == h[3], h   # DATA_PAGE, uncompressed
        body, p = b[p:p + h[3]], p + h[3]
        lv = 0
        if optional:
            (lv,) = struct.unpack_from("<I", body, 0)
            lv += 4
        yield h[5][1], h[5][2], bytes(body[4:lv]) if optional else b"", bytes(body[lv:])
    assert p == len(b)
