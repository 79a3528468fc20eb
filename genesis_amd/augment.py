"""Augmentation of cached training batches on the device: flip, scale crop and gain in the resident gather.

A split that data_cache.CachedLoader keeps resident is shown to the model again every epoch, pixel for pixel.  With an
`Augment` the resident epochs' batches come from ONE launch of gx_cache_gather_aug instead of the two plain gathers: every
frame is mirrored left to right with probability `flip`, cropped to a window whose side is a uniformly drawn fraction
`min_side` .. 1 of the frame's (aspect ratio kept) and resampled back to H x W, bilinear for the frame and nearest for its
label map, and scaled by a gain of 1 +- `brightness` times a per-channel gain of 1 +- `colour`.  The exact transform
("augment v1") is written down in include/genesis_hip.h; tests/augment_restatement.py restates it in numpy.

Every random quantity is a pure function of (seed, resident epoch, cache row) through Philox4x32-10: a run is reproducible
and can be resumed (CachedLoader.set_epoch) whatever the batch size, the epoch's order or the rank layout.

Switching it on: `cfg.augment` (an attribute, like cfg.cache_on_device) or the environment variable GENESIS_AUGMENT, a text
such as 'flip=0.5,min_side=0.6,brightness=0.2,colour=0.1' (Augment.parse) or an Augment: data_cache.wrap_loaders."""
import ctypes
import math
import os

import numpy as np
import torch

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError

ENV = 'GENESIS_AUGMENT'
KEYS = ('flip', 'min_side', 'brightness', 'colour')
PARAM_FIELDS = ('flip', 'x0', 'y0', 'w', 'h', 'g0_bits', 'g1_bits', 'g2_bits')      # a row of `params`
MAX_CHANNELS = 3


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
        raise GenesisHipError('augment: %s must be a number, not %r' % (name, v))
    return float(v)


class Augment(object):
    """flip: the probability of a left-right mirror, [0, 1].  min_side: the smallest crop window's side as a fraction of the
    frame's, (0, 1]; 1 = no crop.  brightness, colour: the half-widths of the frame's and the channels' gains, [0, 1); 0 = none.
    seed: any integer; its low 64 bits key the generator."""

    def __init__(self, flip=0.5, min_side=1.0, brightness=0.0, colour=0.0, seed=0):
        self.flip = _number('flip', flip)
        self.min_side = _number('min_side', min_side)
        self.brightness = _number('brightness', brightness)
        self.colour = _number('colour', colour)
        if not 0.0 <= self.flip <= 1.0:
            raise GenesisHipError('augment: flip must be a probability in [0, 1], not %r' % (flip,))
        if not 0.0 < self.min_side <= 1.0:
            raise GenesisHipError('augment: min_side must be in (0, 1], not %r' % (min_side,))
        for name in ('brightness', 'colour'):
            v = getattr(self, name)
            # (the kernel takes them as float32: a value that rounds up to 1.0f is refused here, with the argument's name)
            if not (0.0 <= v and float(np.float32(v)) < 1.0):
                raise GenesisHipError('augment: %s must be in [0, 1), not %r' % (name, v))
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise GenesisHipError('augment: seed must be an integer, not %r' % (seed,))
        self.seed = seed & ((1 << 64) - 1)

    @property
    def flip_t(self):
        """The flip threshold on a word's 24-bit integer: round(flip * 2^24)."""
        return int(round(self.flip * (1 << 24)))

    def wmin(self, W):
        """The narrowest crop window of a frame W wide: max(1, ceil(min_side * W))."""
        return min(int(W), max(1, int(math.ceil(self.min_side * int(W)))))

    @classmethod
    def parse(cls, text, seed=0):
        """'flip=0.5,min_side=0.6,brightness=0.2,colour=0.1' -> Augment; a bare `flip` means flip=0.5, a key left out keeps
        its off value (flip 0, min_side 1, brightness 0, colour 0).  Unknown keys and an empty text are refused."""
        if not isinstance(text, str):
            raise GenesisHipError('augment: expected a text such as %r, not %r' % ('flip,min_side=0.6', text))
        values = dict(flip=0.0, min_side=1.0, brightness=0.0, colour=0.0)
        seen = set()
        for item in (p.strip() for p in text.split(',')):
            key, eq, val = (s.strip() for s in item.partition('='))
            if key not in KEYS:
                raise GenesisHipError('augment: unknown key %r in %r (known: %s)' % (key, text, ', '.join(KEYS)))
            if key in seen:
                raise GenesisHipError('augment: %s is given twice in %r' % (key, text))
            seen.add(key)
            if not eq:
                if key != 'flip':
                    raise GenesisHipError('augment: %s needs a value in %r (only a bare flip has one: 0.5)' % (key, text))
                values[key] = 0.5
                continue
            try:
                values[key] = float(val)
            except ValueError:
                raise GenesisHipError('augment: %s=%r in %r is no number' % (key, val, text))
        return cls(seed=seed, **values)

    def __repr__(self):
        return 'Augment(flip=%g, min_side=%g, brightness=%g, colour=%g, seed=%d)' % (
            self.flip, self.min_side, self.brightness, self.colour, self.seed)


def requested(cfg):
    """The Augment that cfg.augment or GENESIS_AUGMENT ask for (the variable first), seeded with cfg.seed; None without
    either.  An Augment given as cfg.augment is taken as it is, its own seed included."""
    text = os.environ.get(ENV, '').strip()
    value = text if text else getattr(cfg, 'augment', None)
    if value is None or value is False or (isinstance(value, str) and not value.strip()):
        return None
    if isinstance(value, Augment):
        return value
    return Augment.parse(value, seed=int(getattr(cfg, 'seed', 0) or 0))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def gather(frames_store, labels_store, shape, aug, epoch, idx=None, first=0, B=None, mode=0, return_params=False):
    """-> (input fp32 [B, C, H, W], instances int64 [B, 1, H, W] or None[, params int32 [B, 8]]): the rows
    idx[first : first + B] of a frame store and (labels_store not None) of a label store, (C, H, W) = shape, augmented as
    `aug` says for resident epoch `epoch`.  One launch of gx_cache_gather_aug on the current stream and nothing else.  A row
    of params is PARAM_FIELDS.  As with data_cache.gather_frames the values of idx are the caller's to check."""
    from genesis_amd import data_cache
    if not isinstance(aug, Augment):
        raise GenesisHipError('augment: aug must be an Augment, not %r' % (aug,))
    C, H, W = (int(v) for v in shape)
    if C > MAX_CHANNELS:
        raise GenesisHipError('augment: frames of %d channels: there is one colour gain for each of at most %d' % (C, MAX_CHANNELS))
    data_cache._check_store(frames_store, C * H * W)
    if labels_store is not None:
        data_cache._check_store(labels_store, 2 * H * W)
        if labels_store.shape[0] != frames_store.shape[0] or labels_store.device != frames_store.device:
            raise GenesisHipError('augment: the label store (%d rows on %s) does not go with the frame store (%d rows on %s)'
                                  % (labels_store.shape[0], labels_store.device, frames_store.shape[0], frames_store.device))
    first, B, pidx, nidx = data_cache._gather_args(frames_store, idx, first, B)
    dev = frames_store.device
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    out_labels = None if labels_store is None else torch.empty(B, 1, H, W, dtype=torch.int64, device=dev)
    params = torch.empty(B, 8, dtype=torch.int32, device=dev) if return_params else None
    _lib.call('gx_cache_gather_aug', _ptr(frames_store), int(frames_store.shape[1]), _ptr(labels_store),
              0 if labels_store is None else int(labels_store.shape[1]), int(frames_store.shape[0]), pidx, nidx, first, int(mode),
              aug.seed, int(epoch), aug.flip_t, aug.wmin(W), aug.brightness, aug.colour, _ptr(out), _ptr(out_labels), _ptr(params),
              B, C, H, W, data_cache._stream(frames_store))
    return (out, out_labels, params) if return_params else (out, out_labels)
