"""Parquet files written page by page, by hand: what pyarrow cannot be asked to write - DELTA_BINARY_PACKED with a chosen block /
miniblock size (parquet-mr writes 128 / 4 for INT64, pyarrow 256 / 4), and a column chunk that changes its value encoding from
page to page.  One column (INT64 or DOUBLE, REQUIRED or OPTIONAL), one row group, UNCOMPRESSED, data page v1, Thrift compact
headers and footer restated from the Parquet format specification.  pyarrow reads these files back
(tests/test_parquet_encodings_cpu.py): that is what validates the writer."""
import struct

import numpy as np

PLAIN, DELTA_BINARY_PACKED, BYTE_STREAM_SPLIT = 0, 5, 9
INT64, DOUBLE = 2, 5   # Parquet physical types


# ---------------------------------------------------------------- values sections
def _uleb(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _zigzag(v):
    return _uleb(((v << 1) ^ (v >> 63)) & ((1 << 64) - 1))


def encode_plain(values):
    return np.ascontiguousarray(values).view(np.uint64).astype("<u8").tobytes()


def encode_byte_stream_split(values):
    b = np.ascontiguousarray(values).view(np.uint64).astype("<u8").view(np.uint8).reshape(-1, 8)
    return b.T.tobytes()   # stream k = byte k of every value


def encode_delta(values, block_size=128, miniblocks=4):
    """DELTA_BINARY_PACKED of int64 values: wrapping differences, per block the smallest one, per miniblock the width of the
    largest remainder; the last miniblock holding values is padded to full length, the ones after it keep only their width byte"""
    M = 1 << 64
    vals = [int(v) for v in np.asarray(values, dtype=np.int64)]
    per = block_size // miniblocks
    assert block_size % 128 == 0 and block_size % miniblocks == 0 and per % 32 == 0
    out = bytearray(_uleb(block_size) + _uleb(miniblocks) + _uleb(len(vals)) + _zigzag(vals[0] if vals else 0))
    signed = lambda d: ((d + (1 << 63)) % M) - (1 << 63)   # noqa: E731  (the difference as a wrapped int64)
    deltas = [signed(vals[k] - vals[k - 1]) for k in range(1, len(vals))]
    for b0 in range(0, len(deltas), block_size):
        blk = deltas[b0:b0 + block_size]
        mn = min(blk)
        rem = [(d - mn) % M for d in blk]
        out += _zigzag(mn)
        minis = [rem[m:m + per] for m in range(0, block_size, per)]
        out += bytes(max(r).bit_length() if r else 0 for r in minis)
        for r in minis:
            if not r:
                break
            w = max(r).bit_length()
            acc = 0
            for k, x in enumerate(r):
                acc |= x << (k * w)
            out += acc.to_bytes(per * w // 8, "little")
    return bytes(out)


ENCODERS = {PLAIN: lambda v, **kw: encode_plain(v), DELTA_BINARY_PACKED: encode_delta, BYTE_STREAM_SPLIT: lambda v, **kw: encode_byte_stream_split(v)}


# ---------------------------------------------------------------- Thrift compact protocol (write side)
class _Struct:
    def __init__(self):
        self.b, self.last = bytearray(), 0

    def _hdr(self, fid, typ):
        d = fid - self.last
        assert 0 < d < 16
        self.b.append((d << 4) | typ)
        self.last = fid

    def i32(self, fid, v):
        self._hdr(fid, 5)
        self.b += _uleb(((v << 1) ^ (v >> 31)) & 0xffffffff)
        return self

    def i64(self, fid, v):
        self._hdr(fid, 6)
        self.b += _zigzag(v)
        return self

    def string(self, fid, s):
        self._hdr(fid, 8)
        self.b += _uleb(len(s)) + s.encode()
        return self

    def struct(self, fid, st):
        self._hdr(fid, 12)
        self.b += st.done()
        return self

    def list(self, fid, etype, items):
        """items: already-encoded elements (structs: done(); i32: zigzag varints; strings: length + bytes)"""
        self._hdr(fid, 9)
        self.b += bytes([(len(items) << 4) | etype]) if len(items) < 15 else bytes([0xf0 | etype]) + _uleb(len(items))
        for it in items:
            self.b += it
        return self

    def done(self):
        return bytes(self.b) + b"\x00"


def _levels(valid):
    """definition levels of a v1 page (max level 1): 4-byte length + one bit-packed run of the RLE / bit-packed hybrid"""
    groups = (len(valid) + 7) // 8
    body = _uleb((groups << 1) | 1) + np.packbits(np.asarray(valid, dtype=bool), bitorder="little").tobytes().ljust(groups, b"\0")
    return struct.pack("<I", len(body)) + body


def write_file(path, pages, ptype=INT64, optional=False, name="c"):
    """pages: [(encoding, values, valid or None[, encoder keywords])]; `values` holds one entry per ROW (null rows: anything),
    `valid` the rows that are not null (OPTIONAL columns only).  `encoding` is what the page header claims and what encodes the
    values.  Returns (values, valid) of the whole column."""
    out = bytearray(b"PAR1")
    encs, rows, all_vals, all_valid = set(), 0, [], []
    for pg in pages:
        enc, vals, valid = pg[0], np.asarray(pg[1]), pg[2]
        kw = pg[3] if len(pg) > 3 else {}
        valid = np.ones(len(vals), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        assert optional or valid.all()
        body = (_levels(valid) if optional else b"") + ENCODERS[enc](vals[valid], **kw)
        dph = _Struct().i32(1, len(vals)).i32(2, enc).i32(3, 3).i32(4, 3)   # levels: RLE
        out += _Struct().i32(1, 0).i32(2, len(body)).i32(3, len(body)).struct(5, dph).done() + body
        encs.add(enc)
        rows += len(vals)
        all_vals.append(vals)
        all_valid.append(valid)
    size = len(out) - 4
    meta = (_Struct().i32(1, ptype).list(2, 5, [_uleb(e << 1) for e in sorted(encs | {3})]).list(3, 8, [_uleb(len(name)) + name.encode()])
            .i32(4, 0).i64(5, rows).i64(6, size).i64(7, size).i64(9, 4))
    chunk = _Struct().i64(2, 4).struct(3, meta)
    group = _Struct().list(1, 12, [chunk.done()]).i64(2, size).i64(3, rows)
    schema = [_Struct().string(4, "schema").i32(5, 1).done(), _Struct().i32(1, ptype).i32(3, 1 if optional else 0).string(4, name).done()]
    footer = _Struct().i32(1, 1).list(2, 12, schema).i64(3, rows).list(4, 12, [group.done()]).string(6, "parquet_pages.py").done()
    out += footer + struct.pack("<I", len(footer)) + b"PAR1"
    with open(path, "wb") as fh:
        fh.write(bytes(out))
    return np.concatenate(all_vals), np.concatenate(all_valid)
