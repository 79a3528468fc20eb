"""Streaming TFRecord reader without TensorFlow: the container the multi-object datasets ship in
(third_party/multi_object_datasets/*.py: tf.data.TFRecordDataset(path, compression_type='GZIP') of tf.Example protos).

The file is read and, when it is a GZIP stream, inflated in bounded chunks (zlib.decompressobj; zlib releases the GIL);
record framing, both CRC-32C checks, the tf.Example walk and the unpacking of one-byte-per-value byte lists are the host
functions of the C ABI (genesis_amd/csrc/gx_tfrecord.cpp: gx_tfrecord_scan, gx_tfexample_find_bytes_list,
gx_bytes_list_unpack), which need no GPU.  Nothing here touches a pixel in Python."""
import ctypes
import zlib

import numpy as np

from . import _lib
from ._lib import GenesisHipError, np_ptr as _ptr


class TFRecordError(GenesisHipError):
    """A truncated or corrupt TFRecord stream; the message names the record (0-based index in the file)."""


def crc32c(data):
    """CRC-32C (Castagnoli) of bytes / a uint8 array."""
    a = _lib.as_u8(data, 'tfrecord')
    return int(_lib.load().gx_crc32c(_ptr(a), a.size))


def masked_crc32c(data):
    """TFRecord's masked CRC-32C: ((c >> 15) | (c << 17)) + 0xa282ead8."""
    a = _lib.as_u8(data, 'tfrecord')
    return int(_lib.load().gx_crc32c_masked(_ptr(a), a.size))


def find_bytes_list(record, name):
    """(offset, length) of the BytesList payload of feature `name` inside one tf.Example `record` (uint8 array / bytes)."""
    a = _lib.as_u8(record, 'tfrecord')
    off, length = ctypes.c_longlong(), ctypes.c_longlong()
    _lib.call('gx_tfexample_find_bytes_list', _ptr(a), a.size, name.encode(), ctypes.byref(off), ctypes.byref(length))
    return off.value, length.value


def unpack_bytes_list(record, name, out):
    """Concatenates the values of bytes_list feature `name` of `record` into `out`, a writable C-contiguous uint8 array
    (any shape); raises unless they total exactly out.size bytes."""
    a = _lib.as_u8(record, 'tfrecord')
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise GenesisHipError('tfrecord: out must be a writable C-contiguous uint8 array')
    off, length = find_bytes_list(a, name)
    try:
        _lib.call('gx_bytes_list_unpack', _ptr(a, off), length, _ptr(out), out.size)
    except GenesisHipError as e:
        raise TFRecordError("feature '%s': %s" % (name, e)) from None
    return out


class TFRecordReader(object):
    """Iterates the records of a TFRecord file as uint8 arrays (views of the stream buffer, valid until the next record
    is asked for; copy to keep).  compression: 'GZIP', '' (none) or 'auto' (GZIP when the file starts with 1f 8b).
    `source` is a path or a binary file object.  `chunk_bytes` bounds both the compressed bytes read and the bytes
    inflated at a time, so odd sizes only change the chunking, never the records.

    Raises TFRecordError on a checksum mismatch (unless verify_crc=False), on a record cut short by the end of the file
    and on a GZIP stream that ends early; the message names the record index."""

    def __init__(self, source, compression='auto', verify_crc=True, chunk_bytes=1 << 22, max_scan=256):
        if compression not in ('auto', 'GZIP', ''):
            raise GenesisHipError("tfrecord: compression must be 'auto', 'GZIP' or '', not %r" % (compression,))
        self.source = source
        self.compression = compression
        self.verify_crc = bool(verify_crc)
        self.chunk_bytes = max(1, int(chunk_bytes))
        self.max_scan = max(1, int(max_scan))

    def _chunks(self, f):
        """Decompressed (or raw) byte chunks of at most chunk_bytes."""
        n = self.chunk_bytes
        head = f.read(2)
        gz = self.compression == 'GZIP' or (self.compression == 'auto' and head == b'\x1f\x8b')
        if not gz:
            data = head + f.read(max(0, n - len(head)))
            while data:
                yield data
                data = f.read(n)
            return
        d = zlib.decompressobj(16 + zlib.MAX_WBITS)
        data = head + f.read(n)
        while True:
            if not data:
                data = f.read(n)
                if not data:
                    break
            if d.eof:                            # a further GZIP member follows
                d = zlib.decompressobj(16 + zlib.MAX_WBITS)
            out = d.decompress(data, n)
            if out:
                yield out
            data = d.unused_data if d.eof else d.unconsumed_tail
        out = d.flush()
        if out:
            yield out
        if not d.eof:
            raise EOFError('the GZIP stream ends before its end-of-stream marker')

    def __iter__(self):
        if hasattr(self.source, 'read'):
            yield from self._records(self.source)
        else:
            with open(self.source, 'rb') as f:
                yield from self._records(f)

    def _records(self, f):
        offsets = np.zeros(self.max_scan, dtype=np.int64)
        lengths = np.zeros(self.max_scan, dtype=np.int64)
        nrec, consumed = ctypes.c_int(), ctypes.c_size_t()
        buf = np.zeros(0, dtype=np.uint8)
        index = 0
        chunks = self._chunks(f)
        while True:
            try:
                chunk = next(chunks, None)
            except (zlib.error, EOFError) as e:
                raise TFRecordError('tfrecord: the compressed stream is truncated or corrupt after %d complete records '
                                    '(while reading record %d): %s' % (index, index, e)) from None
            if chunk is None:
                break
            new = np.frombuffer(chunk, dtype=np.uint8)
            buf = np.concatenate([buf, new]) if buf.size else new
            pos = 0
            while True:
                try:
                    _lib.call('gx_tfrecord_scan', _ptr(buf, pos), buf.size - pos, int(self.verify_crc), index, self.max_scan,
                              _ptr(offsets), _ptr(lengths), ctypes.byref(nrec), ctypes.byref(consumed))
                except GenesisHipError as e:
                    raise TFRecordError('tfrecord: corrupt record: %s' % e) from None
                for k in range(nrec.value):
                    o = pos + int(offsets[k])
                    yield buf[o:o + int(lengths[k])]
                    index += 1
                pos += consumed.value
                if nrec.value < self.max_scan:
                    break
            buf = buf[pos:]
        if buf.size:
            raise TFRecordError('tfrecord: truncated file: record %d is cut short (%d trailing bytes after %d complete '
                                'records)' % (index, buf.size, index))
