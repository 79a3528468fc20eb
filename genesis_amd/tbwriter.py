"""A TensorBoard event-file writer: the import replacement of the reference's `from tensorboardX import SummaryWriter`
(train.py:28) for the calls its loop makes -- add_scalar, add_image, add_histogram, add_histogram_raw, flush, close -- with the two
host costs of tensorboardX's last hop moved to the device:

  pictures  tensorboardX's add_image copies each fp32 picture to the host and encodes it there.  Here every device picture of a
            logging event (`add_images_device`; `genesis_amd.visualise.visualise_outputs` uses it) is turned into its filtered PNG
            scanline stream by ONE gx_png_pack launch (include/genesis_hip.h) and fetched as bytes by ONE copy; the host only
            deflates (zlib) and frames.
  scalars   tensorboardX's add_scalar reads a device scalar with one blocking copy per call.  Here a one-element device tensor is
            snapshotted at call time, in stream order, by a small gx_scalar_snapshot launch into a device ring of fp64 slots; the
            call returns without reading the device.  The pending slots come to the host in ONE copy at flush() / close(), when the
            ring is full, or before a picture or histogram event is written.  (The snapshot is what makes deferring legal: the
            static outputs of a replayed step graph are overwritten by the next step.)

The file format is hand-encoded from the public TensorFlow definitions: an uncompressed TFRecord stream (u64 length, masked CRC-32C
of the length, data, masked CRC-32C of the data; gx_crc32c_masked) of `Event` protobuf messages.  No dependency beyond numpy, torch
and the standard library.  `read_events` reads such a file back.

Pictures: 8-bit PNG, colour type 0 (C = 1) or 2 (C = 3), one IDAT; per row the filter with the smallest sum of |signed byte| (ties:
the lowest filter number).  The bytes of a float picture are trunc(clamp(x, 0, 1) * 255.0f), NaN -> 0: for in-range input what
tensorboardX publishes ((tensor * 255.0).astype(uint8)) -- not the rounding of `visualise.save_png`'s sheets.  The host path (numpy,
in this file) and the device path write the same bytes: a file does not depend on where its pictures were packed.

Not verified: tensorboardX and TensorBoard are not installed where this project is built, so neither the byte rule nor the files
were checked against them; conformance rests on the format definitions and on the independent decoders of the tests.

Not here: add_text / add_graph / add_embedding / add_video and the other tensorboardX calls the reference does not make, a writer
thread (events are written by the calling thread), `max_bins`."""
import ctypes
import os
import os.path as osp
import socket
import struct
import time
import zlib

import numpy as np
import torch

from . import _lib
from . import histogram as _hist
from ._lib import GenesisHipError
from .visualise import _chunk

# kinds, descriptor words and bounds of gx_png_pack and gx_scalar_snapshot (tests/test_tbwriter_cpu.py holds them against
# include/genesis_hip.h)
PNGPACK_FP32, PNGPACK_U8, PNGPACK_I64 = range(3)
(PNGPACK_D_SRC, PNGPACK_D_KIND, PNGPACK_D_C, PNGPACK_D_H, PNGPACK_D_W, PNGPACK_D_PIX_STRIDE, PNGPACK_D_ROW_STRIDE,
 PNGPACK_D_CH_STRIDE, PNGPACK_D_DST, PNGPACK_D_ROW0) = range(10)
PNGPACK_DESC_WORDS = 12
PNGPACK_MAX_DIM = 4096
SCALAR_FP32, SCALAR_FP64, SCALAR_I32, SCALAR_I64 = range(4)
SCALAR_MAX_REFS = 32

_SCALAR_DTYPES = {torch.float32: SCALAR_FP32, torch.float64: SCALAR_FP64, torch.int32: SCALAR_I32, torch.int64: SCALAR_I64}
_PACK_KINDS = {torch.float32: PNGPACK_FP32, torch.uint8: PNGPACK_U8, torch.int64: PNGPACK_I64}


class _ScalarRefs(ctypes.Structure):      # gx_scalar_refs
    _fields_ = [('ptr', ctypes.c_void_p * SCALAR_MAX_REFS), ('dtype', ctypes.c_int * SCALAR_MAX_REFS)]


# ---- TFRecord framing and protobuf wire format -------------------------------------------------------------------------------------
def _masked_crc(data):
    return int(_lib.load().gx_crc32c_masked(data, len(data))) & 0xffffffff


def _record(data):
    head = struct.pack('<Q', len(data))
    return head + struct.pack('<I', _masked_crc(head)) + data + struct.pack('<I', _masked_crc(data))


def _varint(v):
    v = int(v) & 0xffffffffffffffff      # (a negative int64 is its two's complement: ten bytes)
    out = bytearray()
    while v > 0x7f:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _len_field(number, payload):
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def _double_field(number, v):
    return _varint(number << 3 | 1) + struct.pack('<d', v)


def _event(wall_time, step, file_version=None, values=()):
    """Event: wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary: value = 1, repeated)."""
    out = _double_field(1, float(wall_time))
    if step:
        out += _varint(2 << 3) + _varint(step)
    if file_version is not None:
        out += _len_field(3, file_version.encode())
    if values:
        out += _len_field(5, b''.join(_len_field(1, v) for v in values))
    return out


def _scalar_value(tag, value):
    """Summary.Value: tag = 1, simple_value = 2 (float, wire type 5)."""
    return _len_field(1, tag.encode()) + _varint(2 << 3 | 5) + struct.pack('<f', value)


def _image_value(tag, H, W, C, png):
    """Summary.Value: image = 4 (Summary.Image: height = 1, width = 2, colorspace = 3, encoded_image_string = 4)."""
    image = _varint(1 << 3) + _varint(H) + _varint(2 << 3) + _varint(W) + _varint(3 << 3) + _varint(C) + _len_field(4, png)
    return _len_field(1, tag.encode()) + _len_field(4, image)


def _histogram_value(tag, mn, mx, num, sm, sq, limits, counts):
    """Summary.Value: histo = 5 (HistogramProto: min = 1 .. sum_squares = 5 doubles, bucket_limit = 6, bucket = 7 packed doubles)."""
    histo = b''.join(_double_field(i + 1, float(v)) for i, v in enumerate((mn, mx, num, sm, sq)))
    histo += _len_field(6, np.asarray(limits, '<f8').tobytes()) + _len_field(7, np.asarray(counts, '<f8').tobytes())
    return _len_field(1, tag.encode()) + _len_field(5, histo)


# ---- the reader ------------------------------------------------------------------------------------------------------------------
def _fields(buf):
    """One protobuf message -> [(field number, wire type, value)]: varints as unsigned ints, the other types as bytes."""
    pos, n = 0, len(buf)

    def varint():
        nonlocal pos
        v = shift = 0
        while True:
            if pos >= n or shift > 63:
                raise GenesisHipError('read_events: a varint runs past its message')
            b = buf[pos]
            pos += 1
            v |= (b & 0x7f) << shift
            shift += 7
            if b < 0x80:
                return v
    out = []
    while pos < n:
        key = varint()
        number, wire = key >> 3, key & 7
        if wire == 0:
            out.append((number, wire, varint()))
            continue
        size = {1: 8, 5: 4}.get(wire)
        if wire == 2:
            size = varint()
        if size is None or pos + size > n:
            raise GenesisHipError('read_events: wire type %d or a length that runs past its message' % wire)
        out.append((number, wire, bytes(buf[pos:pos + size])))
        pos += size
    return out


def _int64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def read_events(path):
    """Yields one dict per event of an event file, in file order: 'wall_time' (float), 'step' (int), and either 'file_version' (str)
    or the event's summary values as lists of (tag, value) in their order: 'scalars' (value: numpy.float32), 'images' (value: dict of
    height, width, colorspace, encoded_image_string) and 'histograms' (value: dict of min, max, num, sum, sum_squares, bucket_limit,
    bucket).  Both checksums of every record are verified; a mismatch or a truncated record raises GenesisHipError naming the record."""
    with open(path, 'rb') as f:
        data = f.read()
    pos, index = 0, 0
    while pos < len(data):
        if pos + 12 > len(data):
            raise GenesisHipError('read_events: %s: record %d is truncated' % (path, index))
        head = data[pos:pos + 8]
        size = struct.unpack('<Q', head)[0]
        if struct.unpack('<I', data[pos + 8:pos + 12])[0] != _masked_crc(head):
            raise GenesisHipError('read_events: %s: record %d: the checksum of the length does not match' % (path, index))
        if pos + 16 + size > len(data):
            raise GenesisHipError('read_events: %s: record %d is truncated' % (path, index))
        body = data[pos + 12:pos + 12 + size]
        if struct.unpack('<I', data[pos + 12 + size:pos + 16 + size])[0] != _masked_crc(body):
            raise GenesisHipError('read_events: %s: record %d: the checksum of the data does not match' % (path, index))
        pos += 16 + size
        index += 1
        event = dict(wall_time=0.0, step=0)
        for number, wire, v in _fields(body):
            if number == 1 and wire == 1:
                event['wall_time'] = struct.unpack('<d', v)[0]
            elif number == 2 and wire == 0:
                event['step'] = _int64(v)
            elif number == 3 and wire == 2:
                event['file_version'] = v.decode()
            elif number == 5 and wire == 2:
                event.update(scalars=[], images=[], histograms=[])
                for n1, w1, value in _fields(v):
                    if n1 == 1 and w1 == 2:
                        _read_value(value, event)
        yield event


def _read_value(buf, event):
    tag = ''
    for number, wire, v in _fields(buf):
        if number == 1 and wire == 2:
            tag = v.decode()
        elif number == 2 and wire == 5:
            event['scalars'].append((tag, np.frombuffer(v, '<f4')[0]))
        elif number == 4 and wire == 2:
            image = dict(height=0, width=0, colorspace=0, encoded_image_string=b'')
            for n1, w1, x in _fields(v):
                if w1 == 0 and n1 in (1, 2, 3):
                    image[('height', 'width', 'colorspace')[n1 - 1]] = _int64(x)      # (a negative int32 is ten bytes too)
                elif n1 == 4 and w1 == 2:
                    image['encoded_image_string'] = x
            event['images'].append((tag, image))
        elif number == 5 and wire == 2:
            histo = dict(min=0.0, max=0.0, num=0.0, sum=0.0, sum_squares=0.0, bucket_limit=[], bucket=[])
            for n1, w1, x in _fields(v):
                if w1 == 1 and 1 <= n1 <= 5:
                    histo[('min', 'max', 'num', 'sum', 'sum_squares')[n1 - 1]] = struct.unpack('<d', x)[0]
                elif n1 in (6, 7) and w1 == 2:      # packed
                    histo['bucket_limit' if n1 == 6 else 'bucket'].extend(np.frombuffer(x, '<f8').tolist())
                elif n1 in (6, 7) and w1 == 1:      # one by one, as a proto2 writer would
                    histo['bucket_limit' if n1 == 6 else 'bucket'].append(struct.unpack('<d', x)[0])
            event['histograms'].append((tag, histo))


# ---- pictures on the host: the same bytes as gx_png_pack ---------------------------------------------------------------------------
def _quantise_host(a, dataformats):
    """A host array in `dataformats` -> uint8 [H, W, C] by the byte rule."""
    if dataformats == 'CHW':
        a = a.transpose(1, 2, 0)
    elif dataformats == 'HW':
        a = a[:, :, None]
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    if a.dtype.kind in 'iub':
        return np.clip(a.astype(np.int64) if a.dtype.kind == 'b' else a, 0, 255).astype(np.uint8)
    x = a.astype(np.float32)
    with np.errstate(invalid='ignore'):
        x = np.where(np.isnan(x), np.float32(0.0), np.minimum(np.maximum(x, np.float32(0.0)), np.float32(1.0)))
        return (x.astype(np.float32) * np.float32(255.0)).astype(np.uint8)


def pack_rows_host(u8, force_filter=None):
    """uint8 [H, W, C] -> the scanline stream of gx_png_pack as bytes: per row the filter byte and the filtered bytes, the filter
    with the smallest sum of |signed byte| (ties: the lowest number); force_filter: that filter for every row."""
    H, W, C = u8.shape
    cur = u8.reshape(H, W * C).astype(np.int32)
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    left = np.zeros_like(cur)
    left[:, C:] = cur[:, :-C]
    upleft = np.zeros_like(cur)
    upleft[:, C:] = up[:, :-C]
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cand = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]) & 255      # [5, H, W C]
    if force_filter is None:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)
        best = np.argmin(cost, axis=0)      # (the first minimum: the lowest filter number)
    else:
        best = np.full(H, int(force_filter))
    rows = np.empty((H, 1 + W * C), np.uint8)
    rows[:, 0] = best
    rows[:, 1:] = cand[best, np.arange(H)]
    return rows.tobytes()


def _png(stream, H, W, C, level):
    return (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2 if C == 3 else 0, 0, 0, 0))
            + _chunk(b'IDAT', zlib.compress(stream, level)) + _chunk(b'IEND', b''))


def _geometry(shape, dataformats, what):
    """The shape of a picture in `dataformats` -> (C, H, W), or GenesisHipError naming the argument."""
    if dataformats not in ('CHW', 'HWC', 'HW'):
        raise GenesisHipError("%s: dataformats=%r; 'CHW', 'HWC' and 'HW' are supported" % (what, dataformats))
    if len(shape) != len(dataformats):
        raise GenesisHipError('%s: img of shape %s is not %s' % (what, tuple(shape), dataformats))
    dims = dict(zip(dataformats, shape))
    C, H, W = int(dims.get('C', 1)), int(dims['H']), int(dims['W'])
    if C not in (1, 3):
        raise GenesisHipError('%s: img of shape %s in %s: C = %d is neither 1 nor 3' % (what, tuple(shape), dataformats, C))
    if not (1 <= H <= PNGPACK_MAX_DIM and 1 <= W <= PNGPACK_MAX_DIM):
        raise GenesisHipError('%s: img of shape %s in %s: H = %d, W = %d outside [1, %d]'
                              % (what, tuple(shape), dataformats, H, W, PNGPACK_MAX_DIM))
    return C, H, W


def _tag(tag, what):
    if not isinstance(tag, str) or not tag:
        raise GenesisHipError('%s: tag=%r; expected a non-empty string' % (what, tag))
    return tag


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class SummaryWriter(object):
    """SummaryWriter(logdir=None, comment='', filename_suffix='', compress_level=6, device_pack=True, scalar_slots=4096).
    logdir: created; None: runs/<time>_<hostname><comment>.  The file is events.out.tfevents.<unix time>.<hostname><filename_suffix>;
    an existing file is never truncated ('.1', '.2', ... is appended to the name until it is free).  compress_level: zlib's, for
    the pictures.  device_pack=False packs device pictures on the host from their fp32 / integer copy (the same bytes).
    scalar_slots: fp64 slots of the device ring of pending scalars.  Every add_* takes global_step=None (step 0) and walltime=None
    (the time of the call); events are in the file in call order.  `stats`: what this writer itself launched, copied and wrote."""

    def __init__(self, logdir=None, comment='', filename_suffix='', compress_level=6, device_pack=True, scalar_slots=4096):
        if isinstance(scalar_slots, bool) or not isinstance(scalar_slots, int) or not 1 <= scalar_slots < 1 << 31:
            raise GenesisHipError('SummaryWriter: scalar_slots=%r; expected an integer in [1, 2^31)' % (scalar_slots,))
        if isinstance(compress_level, bool) or not isinstance(compress_level, int) or not -1 <= compress_level <= 9:
            raise GenesisHipError('SummaryWriter: compress_level=%r; expected an integer in [-1, 9]' % (compress_level,))
        host, now = socket.gethostname(), time.time()
        if logdir is None:
            logdir = osp.join('runs', time.strftime('%b%d_%H-%M-%S', time.localtime(now)) + '_' + host + comment)
        self.logdir = str(logdir)
        os.makedirs(self.logdir, exist_ok=True)
        base = osp.join(self.logdir, 'events.out.tfevents.%010d.%s%s' % (int(now), host, filename_suffix))
        self.path, self._file, k = base, None, 0
        while self._file is None:
            try:
                self._file = open(self.path, 'xb')
            except FileExistsError:
                k += 1
                self.path = '%s.%d' % (base, k)
        self.compress_level, self.device_pack, self.scalar_slots = compress_level, bool(device_pack), scalar_slots
        self.stats = dict(pack_launches=0, snapshot_launches=0, d2h_copies=0, d2h_bytes=0, events=0, file_bytes=0)
        self._rings = {}                   # device -> fp64 [scalar_slots]
        self._pending = []                 # (tag, step, wall time, ring slot or None, host value or None) in call order
        self._used, self._device, self._streams = 0, None, []
        self._write(_event(now, 0, file_version='brain.Event:2'))

    # -- plumbing ------------------------------------------------------------------------------------------------------------------
    def _open(self, what):
        if self._file is None:
            raise GenesisHipError('%s: the writer is closed' % what)

    def _write(self, event):
        data = _record(event)
        self._file.write(data)
        self.stats['events'] += 1
        self.stats['file_bytes'] += len(data)

    def _drain(self):
        """Brings the pending scalars to the host in one copy and writes them, in call order."""
        if not self._pending:
            return
        host = None
        if self._used:
            with torch.cuda.device(self._device):
                now = torch.cuda.current_stream(self._device)
                for s in self._streams:      # (a snapshot queued on another stream is not ordered before this copy)
                    if s != now:
                        s.synchronize()
                host = self._rings[self._device][:self._used].cpu().numpy()
            self.stats['d2h_copies'] += 1
            self.stats['d2h_bytes'] += 8 * self._used
        pending, self._pending, self._used, self._streams = self._pending, [], 0, []
        for tag, step, wall, slot, value in pending:
            self._write_scalar(tag, host[slot] if slot is not None else value, step, wall)

    def _write_scalar(self, tag, value, step, wall):
        with np.errstate(over='ignore'):
            self._write(_event(wall, step, values=[_scalar_value(tag, np.float32(value))]))

    def _snapshot(self, entries, what):
        """entries: [(tag, one-element device tensor, step, wall time)], already checked -> queued, one launch per 32 of them."""
        device = entries[0][1].device
        if self._device is not None and device != self._device:
            self._drain()
        self._device = device
        per_launch = min(SCALAR_MAX_REFS, self.scalar_slots)
        with torch.cuda.device(device):
            if device not in self._rings:
                self._rings[device] = torch.empty(self.scalar_slots, dtype=torch.float64, device=device)
            ring, stream = self._rings[device], torch.cuda.current_stream(device)
            for i in range(0, len(entries), per_launch):
                group = entries[i:i + per_launch]
                if self._used + len(group) > self.scalar_slots:      # the ring is full
                    self._drain()
                refs = _ScalarRefs()
                for j, (_, t, _, _) in enumerate(group):
                    refs.ptr[j], refs.dtype[j] = t.data_ptr(), _SCALAR_DTYPES[t.dtype]
                _lib.call('gx_scalar_snapshot', ctypes.byref(refs), len(group), ctypes.c_void_p(ring.data_ptr()), self.scalar_slots,
                          self._used, ctypes.c_void_p(stream.cuda_stream))
                self.stats['snapshot_launches'] += 1
                if stream not in self._streams:
                    self._streams.append(stream)
                for j, (tag, _, step, wall) in enumerate(group):
                    self._pending.append((tag, step, wall, self._used + j, None))
                self._used += len(group)

    def _scalar(self, tag, value, what):
        """-> ('device', tensor) for a one-element device tensor, else ('host', number)."""
        if torch.is_tensor(value):
            if value.numel() != 1:
                raise GenesisHipError('%s: value of shape %s for %r; expected one element' % (what, tuple(value.shape), tag))
            if value.is_cuda:
                if value.dtype not in _SCALAR_DTYPES:
                    raise GenesisHipError('%s: value of dtype %s for %r; a device scalar is float32, float64, int32 or int64'
                                          % (what, value.dtype, tag))
                return 'device', value.detach()
            value = value.detach().item()
        elif isinstance(value, np.ndarray):
            if value.size != 1:
                raise GenesisHipError('%s: value of shape %s for %r; expected one element' % (what, value.shape, tag))
            value = value.reshape(()).item()
        if isinstance(value, (bool, int, float, np.number, np.bool_)):
            try:
                return 'host', float(value)
            except OverflowError:      # a Python int beyond double range
                return 'host', float('inf') if value > 0 else float('-inf')
        raise GenesisHipError('%s: value=%r for %r; expected a number or a one-element tensor or array' % (what, value, tag))

    def _add_scalars(self, items, global_step, walltime, what):
        self._open(what)
        step, wall = int(global_step or 0), time.time() if walltime is None else float(walltime)
        checked = [(_tag(tag, what),) + self._scalar(tag, value, what) for tag, value in items]
        if any(where == 'device' for _, where, _ in checked) and _capturing():
            raise GenesisHipError('%s: value: the current stream is being captured; a snapshot launch would become part of the graph '
                                  'and the file would never see it.  Log outside the capture' % what)
        run = []      # consecutive device values share their launches
        for tag, where, value in checked + [(None, None, None)]:
            if where == 'device' and (not run or run[0][1].device == value.device):
                run.append((tag, value, step, wall))
                continue
            if run:
                self._snapshot(run, what)
                run = []
            if where == 'device':
                run.append((tag, value, step, wall))
            elif where == 'host':
                if self._pending:      # behind the pending ones: call order
                    self._pending.append((tag, step, wall, None, value))
                else:
                    self._write_scalar(tag, value, step, wall)
        if run:
            self._snapshot(run, what)

    # -- scalars -------------------------------------------------------------------------------------------------------------------
    def add_scalar(self, tag, value, global_step=None, walltime=None):
        """value: a Python or numpy number, a one-element host tensor or array, or a one-element device tensor (fp32, fp64, int32,
        int64), which is snapshotted now, in stream order, and read later.  simple_value is numpy.float32(value)."""
        self._add_scalars([(tag, value)], global_step, walltime, 'add_scalar')

    def add_scalars_dict(self, sdict, tag, global_step=None, walltime=None):
        """utils/misc.py:77-79 log_scalars: add_scalar('<tag>/<key>', value, global_step) per item, the device values of the dict
        snapshotted by one launch per 32."""
        self._add_scalars([('%s/%s' % (tag, key), val) for key, val in sdict.items()], global_step, walltime, 'add_scalars_dict')

    # -- pictures ------------------------------------------------------------------------------------------------------------------
    def _write_image(self, tag, stream, C, H, W, step, wall):
        self._drain()
        self._write(_event(wall, step, values=[_image_value(tag, H, W, C, _png(stream, H, W, C, self.compress_level))]))

    def add_image(self, tag, img, global_step=None, walltime=None, dataformats='CHW'):
        """img: a host or device tensor or an ndarray in `dataformats` ('CHW', 'HWC' or 'HW'; C = 1 or 3).  Floats go through
        trunc(clamp(x, 0, 1) * 255.0f) (NaN -> 0), uint8 is taken as bytes, other integers as byte values clamped to 0..255."""
        if torch.is_tensor(img) and img.is_cuda:
            return self.add_images_device([(tag, img, dataformats)], global_step, walltime, what='add_image')
        self._open('add_image')
        _tag(tag, 'add_image')
        a = img.detach().numpy() if torch.is_tensor(img) else np.asarray(img)
        if a.dtype.kind not in 'fiub':
            raise GenesisHipError('add_image: img of dtype %s for %r; expected floats or integers' % (a.dtype, tag))
        C, H, W = _geometry(a.shape, dataformats, 'add_image')
        wall = time.time() if walltime is None else float(walltime)
        self._write_image(tag, pack_rows_host(_quantise_host(a, dataformats)), C, H, W, int(global_step or 0), wall)

    def add_images_device(self, items, global_step=None, walltime=None, what='add_images_device'):
        """items: [(tag, device tensor, dataformats)].  All pictures are packed by ONE gx_png_pack launch and fetched by ONE copy;
        one event per picture, in list order.  fp32, uint8 and int64 are read in place; other dtypes are converted on the device
        first (floats to fp32, integers to int64)."""
        self._open(what)
        step, wall = int(global_step or 0), time.time() if walltime is None else float(walltime)
        pictures, device = [], None
        for tag, t, dataformats in items:
            _tag(tag, what)
            if not torch.is_tensor(t) or not t.is_cuda:
                raise GenesisHipError('%s: items: %r is not a device tensor' % (what, tag))
            if device is not None and t.device != device:
                raise GenesisHipError('%s: items: %r is on %s, the pictures before it on %s' % (what, tag, t.device, device))
            device = t.device
            C, H, W = _geometry(t.shape, dataformats, what)
            if t.dtype.is_complex or t.dtype == torch.bool:
                raise GenesisHipError('%s: img of dtype %s for %r; expected floats or integers' % (what, t.dtype, tag))
            if not t.is_contiguous():
                raise GenesisHipError('%s: img for %r of shape %s with strides %s is not contiguous' % (what, tag, tuple(t.shape), t.stride()))
            pictures.append((tag, t.detach(), dataformats, C, H, W))
        if not pictures:
            return
        if _capturing():
            raise GenesisHipError('%s: the current stream is being captured; log outside the capture' % what)
        if not self.device_pack:
            streams = []
            for tag, t, dataformats, C, H, W in pictures:
                a = t.cpu().numpy()
                self.stats['d2h_copies'] += 1
                self.stats['d2h_bytes'] += a.nbytes
                streams.append(pack_rows_host(_quantise_host(a, dataformats)))
        else:
            streams = self._pack_device(pictures, device)
        for (tag, _, _, C, H, W), stream in zip(pictures, streams):
            self._write_image(tag, stream, C, H, W, step, wall)

    def _pack_device(self, pictures, device):
        table = np.zeros((len(pictures), PNGPACK_DESC_WORDS), np.int64)
        keep, dst, row0 = [], 0, 0
        with torch.cuda.device(device):
            for i, (_, t, dataformats, C, H, W) in enumerate(pictures):
                if t.dtype not in _PACK_KINDS:
                    t = t.to(torch.float32 if t.dtype.is_floating_point else torch.int64)
                keep.append(t)
                pix, row, ch = (C, W * C, 1) if dataformats == 'HWC' else (1, W, H * W if C == 3 else 0)
                table[i, :PNGPACK_D_ROW0 + 1] = (t.data_ptr(), _PACK_KINDS[t.dtype], C, H, W, pix, row, ch, dst, row0)
                dst += H * (1 + W * C)
                row0 += H
            dev_table = torch.from_numpy(table).to(device)
            out = torch.empty(dst, dtype=torch.uint8, device=device)
            _lib.call('gx_png_pack', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(dev_table.data_ptr()), table.size, len(pictures),
                      ctypes.c_void_p(out.data_ptr()), dst, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
            host = out.cpu().numpy()
        self.stats['pack_launches'] += 1
        self.stats['d2h_copies'] += 1
        self.stats['d2h_bytes'] += dst
        streams = []
        for i in range(len(pictures)):
            first = int(table[i, PNGPACK_D_DST])
            H, W, C = (int(table[i, k]) for k in (PNGPACK_D_H, PNGPACK_D_W, PNGPACK_D_C))
            streams.append(host[first:first + H * (1 + W * C)].tobytes())
        return streams

    # -- histograms ------------------------------------------------------------------------------------------------------------------
    def add_histogram(self, tag, values, global_step=None, bins='tensorflow', walltime=None, max_bins=None):
        """A device tensor goes through genesis_amd.histogram.Histograms (one gx_hist_multi call); a host tensor or array through
        numpy.histogram over the same edge table and the same trimming."""
        self._open('add_histogram')
        _tag(tag, 'add_histogram')
        if torch.is_tensor(values) and values.is_cuda:
            if _capturing():
                raise GenesisHipError('add_histogram: the current stream is being captured; log outside the capture')
            h = _hist.Histograms(bins, max_bins)
            h.add(tag, values)
            r = h.compute()[0]
            return self.add_histogram_raw(tag, r.min, r.max, r.num, r.sum, r.sum_squares, r.bucket_limits, r.bucket_counts, global_step,
                                          walltime)
        if max_bins is not None:
            raise GenesisHipError('max_bins=%r is not supported: the buckets are not subsampled' % (max_bins,))
        edges = _hist._edges(bins)
        v = (values.detach().numpy() if torch.is_tensor(values) else np.asarray(values)).reshape(-1)
        if v.size == 0 or v.dtype.kind not in 'fiu':
            raise GenesisHipError('add_histogram: values of dtype %s with %d elements for %r; expected at least one number'
                                  % (v.dtype, v.size, tag))
        v = v.astype(np.float64)
        counts, _ = np.histogram(v, bins=edges)
        limits, kept = _hist.trim(counts, edges)
        with np.errstate(invalid='ignore', over='ignore'):
            self.add_histogram_raw(tag, float(v.min()), float(v.max()), int(v.size), float(v.sum()), float(v.dot(v)), limits, kept,
                                   global_step, walltime)

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None, walltime=None):
        self._open('add_histogram_raw')
        _tag(tag, 'add_histogram_raw')
        if len(bucket_limits) != len(bucket_counts):
            raise GenesisHipError('add_histogram_raw: bucket_limits has %d entries, bucket_counts %d' % (len(bucket_limits), len(bucket_counts)))
        wall = time.time() if walltime is None else float(walltime)
        self._drain()
        self._write(_event(wall, int(global_step or 0),
                           values=[_histogram_value(tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts)]))

    # -- the end -----------------------------------------------------------------------------------------------------------------------
    def flush(self):
        self._open('flush')
        self._drain()
        self._file.flush()

    def close(self):
        if self._file is None:
            return
        try:
            self._drain()
        finally:
            self._file.close()
            self._file = None
            self._rings = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
