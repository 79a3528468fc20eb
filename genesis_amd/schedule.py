"""Learning-rate schedules that the optimiser launch evaluates on the device (gx_adam_step_pair_ex / gx_optimiser_step_pair_ex,
include/genesis_hip.h): the rate is a function of the device step counter, so a captured HIP graph follows a warm-up, a decay or a
rule of the host's own without being captured again.

`LRSchedule.value(k, base)` is the closed form the kernel evaluates, in Python floats and in the kernel's operation order: the rate
of the optimiser step that makes the step counter k + 1 (torch: `param_groups[0]['lr']` at `last_epoch = k` of
`SequentialLR([LinearLR(warmup_start, 1, warmup_iters), X], [warmup_iters])`).  One difference from torch: the cosine is HELD at
`min_lr` once `decay_iters` steps have passed; torch's CosineAnnealingLR is periodic and climbs again."""
import math

import numpy as np

# descriptor words of the schedule and byte offsets of the tail record (tests/test_lr_ema_cpu.py holds them against
# include/genesis_hip.h)
CONSTANT, COSINE, EXPONENTIAL, STEP, DEVICE = range(5)
KIND, BASE, WARMUP, START, T, ETA_MIN, GAMMA, N_MILESTONES, MILESTONE0 = range(9)
MAX_MILESTONES = 8
WORDS = 16
TAIL_LR, TAIL_DECAY, TAIL_BYTES = 0, 8, 16

KINDS = {'constant': CONSTANT, 'cosine': COSINE, 'exponential': EXPONENTIAL, 'step': STEP, 'device': DEVICE}


def _whole(value, name, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < least:
        raise ValueError('%s must be an integer >= %d, got %r' % (name, least, value))
    return int(value)


def _number(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(float(value)):
        raise ValueError('%s must be a finite number, got %r' % (name, value))
    return float(value)


class LRSchedule(object):
    """kind: 'constant'; 'cosine' (decay_iters steps from the base rate down to min_lr, then held); 'exponential' (times gamma per
    step); 'step' (times gamma at each of at most 8 ascending `milestones`); 'device' (the rate is a device scalar that
    TrainStep.set_lr writes; no warm-up).  warmup_iters > 0: the first warmup_iters steps ramp linearly from warmup_start times the
    base rate to the base rate, and decay_iters / milestones count from the end of the ramp."""

    def __init__(self, kind='constant', warmup_iters=0, warmup_start=1.0 / 3.0, decay_iters=None, min_lr=0.0, gamma=0.1,
                 milestones=()):
        if kind not in KINDS:
            raise ValueError('kind must be one of %s, got %r' % (sorted(KINDS), kind))
        self.kind = kind
        self.warmup_iters = _whole(warmup_iters, 'warmup_iters', 0)
        self.warmup_start = _number(warmup_start, 'warmup_start')
        if not 0.0 < self.warmup_start <= 1.0:
            raise ValueError('warmup_start must lie in (0, 1], got %r' % (warmup_start,))
        if kind == 'device' and self.warmup_iters:
            raise ValueError("warmup_iters does not apply to kind='device' (the host writes the rate it wants)")
        if kind == 'cosine':
            if decay_iters is None:
                raise ValueError("decay_iters is needed by kind='cosine'")
            self.decay_iters = _whole(decay_iters, 'decay_iters', 1)
        else:
            self.decay_iters = None if decay_iters is None else _whole(decay_iters, 'decay_iters', 1)
        self.min_lr = _number(min_lr, 'min_lr')
        self.gamma = _number(gamma, 'gamma')
        if not self.gamma > 0.0:
            raise ValueError('gamma must be positive, got %r' % (gamma,))
        try:
            ms = list(milestones)
        except TypeError:
            raise ValueError('milestones must be a sequence of integers, got %r' % (milestones,))
        self.milestones = tuple(_whole(m, 'milestones', 0) for m in ms)
        if len(self.milestones) > MAX_MILESTONES:
            raise ValueError('milestones: at most %d are held, got %d' % (MAX_MILESTONES, len(self.milestones)))
        if any(a > b for a, b in zip(self.milestones, self.milestones[1:])):
            raise ValueError('milestones must be in ascending order, got %r' % (self.milestones,))

    def value(self, k, base):
        """The rate of the step with index k >= 0 (the step counter is k + 1 after it).  kind='device' has no closed form."""
        if self.kind == 'device':
            raise ValueError("kind='device' has no closed form: the rate is what set_lr wrote")
        k, W = float(int(k)), float(self.warmup_iters)
        base = float(base)
        if k < W:
            return base * (self.warmup_start + ((1.0 - self.warmup_start) * k) / W)
        j = k - W
        if self.kind == 'cosine':
            Tn = float(self.decay_iters)
            if j >= Tn:
                return self.min_lr
            return self.min_lr + ((base - self.min_lr) * (1.0 + math.cos((math.pi * j) / Tn))) / 2.0
        if self.kind == 'exponential':
            return base * _pow(self.gamma, j)
        if self.kind == 'step':
            return base * _pow(self.gamma, float(sum(1 for m in self.milestones if float(m) <= j)))
        return base

    def words(self, base):
        """The GX_SCHED_WORDS fp64 words of the C ABI for the base rate `base` (a numpy array the caller keeps alive)."""
        w = np.zeros(WORDS, np.float64)
        w[KIND], w[BASE], w[WARMUP], w[START] = KINDS[self.kind], float(base), self.warmup_iters, self.warmup_start
        w[T], w[ETA_MIN], w[GAMMA] = (self.decay_iters or 0), self.min_lr, self.gamma
        w[N_MILESTONES] = len(self.milestones)
        w[MILESTONE0:MILESTONE0 + len(self.milestones)] = self.milestones
        return w

    def state_dict(self):
        """The settings as a plain dict (what a checkpoint records); LRSchedule(**d) rebuilds the schedule."""
        return dict(kind=self.kind, warmup_iters=self.warmup_iters, warmup_start=self.warmup_start, decay_iters=self.decay_iters,
                    min_lr=self.min_lr, gamma=self.gamma, milestones=list(self.milestones))

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.state_dict() == other.state_dict()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return 'LRSchedule(%s)' % ', '.join('%s=%r' % kv for kv in self.state_dict().items())


def _pow(x, y):
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf


def check_ema_decay(value, name='ema_decay'):
    """None, or a number in [0, 1) -> float; anything else: ValueError naming the argument."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not 0.0 <= float(value) < 1.0:
        raise ValueError('%s must be a number in [0, 1) (or None: no averaged weights), got %r' % (name, value))
    return float(value)


def ema_decay_at(decay, t, warmup):
    """decay_t of the update that leaves the step counter at t >= 1, as the kernels form it in fp64."""
    return min(decay, (1.0 + float(t)) / (10.0 + float(t))) if warmup else decay
