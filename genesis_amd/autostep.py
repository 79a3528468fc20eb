"""The reference's training loop UNCHANGED (train.py:223-263: optimiser.zero_grad(); model(x); ...; loss.backward();
optimiser.step()) on the step machinery of `TrainStep`, without the loop knowing.

`TrainStep` gets its speed from three things the plain autograd path does not have: every conv weight is packed ONCE per iteration
(gx_weight_cache_*: one launch instead of one per conv call), the weight gradients of a backward pass run as ONE stream-K launch and
their split-K / GroupNorm-affine reductions as one batched launch each (gx_defer_*), and parameter gradients are written straight
into their buffers (no per-parameter accumulation launch).  None of this needs the loop's cooperation:

  * `arm(model)` -- called by the model's own forward() in training mode with autograd on -- refreshes (first time: records) the
    model's packed-weight cache and remembers the model;
  * the first HIP autograd node of the following backward pass (`begin_backward`, from functions.ctx_bound) -- if every parameter's
    .grad is None, which is what `optimiser.zero_grad()` leaves -- gives the parameters zeroed gradient views of ONE flat buffer (one
    fill launch), switches the Functions to direct gradient writes + deferred reductions, and queues an end-of-backward callback on
    the autograd engine (the hook DistributedDataParallel finalises its buckets with);
  * that callback (`end_backward`) flushes the queued launches, releases the weight cache and switches everything off again.

After `loss.backward()` returns, every parameter has its .grad exactly as the plain path would have left it (up to the summation
order of the split-K slabs: the stream-K launch cuts the tile line differently from per-layer launches), and `torch.optim.*.step()`
consumes them as usual.  Anything unusual -- gradients already present (accumulation over several backward passes), a forward
without a backward, an exception inside backward -- falls back to the plain path: the state is reset at the next arm().
`GENESIS_AUTOSTEP=0` switches the whole mechanism off (the plain per-call path).  Measured on the metric configuration
(tools/ref_loop_time.py): see DESIGN.md section 7."""
import os
import threading
import weakref

import torch
from torch.nn.parallel import DistributedDataParallel as _DDP

from . import _lib
from . import hip_ops as _hip
from . import precision as _precision

ENABLED = os.environ.get('GENESIS_AUTOSTEP', '1') != '0'


class _State(object):
    __slots__ = ('models', 'in_pass', 'direct', 'cache_on', 'recording', 'ctx')

    def __init__(self):
        self.models = []          # weak references to the models armed since the last backward pass
        self.in_pass = False      # a backward pass is running under this mechanism
        self.direct = False       # ... with direct gradient writes + deferred reductions
        self.cache_on = None      # id of the weight cache that is serving / recording
        self.recording = False
        self.ctx = 0


_STATE = _State()

# Per-model bookkeeping lives HERE, keyed weakly by the model -- not in model.__dict__, which copy.deepcopy / torch.save /
# nn.DataParallel's replicate() would duplicate together with the native cache id it holds (two models aliasing one cache, a
# finalizer destroying a live one).  A copy of a model simply starts without an entry.
_BOOK = weakref.WeakKeyDictionary()      # model -> {'cache': [id, recorded, key] | None, 'params': [...], 'grads': (...) | None}


def _book(model):
    b = _BOOK.get(model)
    if b is None:
        b = {'cache': None, 'params': None, 'grads': None}
        _BOOK[model] = b
    return b


def _fn():
    from . import functions
    return functions


def _reset():
    """Back to the plain path: whatever an unfinished pass left behind is dropped."""
    st = _STATE
    if st.direct:
        s = _fn().step_state()
        s.direct_param_grads = False
        _hip.defer_state().on = False
        _hip.defer_discard()
    if st.cache_on is not None:
        if st.recording:
            _lib.call('gx_weight_cache_record', st.cache_on, 0)
        else:
            _lib.call('gx_weight_cache_release')
    st.models, st.in_pass, st.direct, st.cache_on, st.recording = [], False, False, None, False


def _wrapped_or_threaded(model):
    """The callers this mechanism must leave alone.
    * nn.DataParallel (train.py --multi_gpu, train.py:153-155) runs REPLICAS on worker threads: a replica has no parameters() and
      the packed-weight cache tables of a library context are not made for concurrent recording -- replicas and any forward off
      the main thread take the plain per-call path, which touches no shared state.
    * DistributedDataParallel copies p.grad into its bucket from the AccumulateGrad post-hooks, i.e. DURING the backward pass,
      while this mechanism only finalises the conv-weight / GroupNorm-affine gradients in its end-of-backward callback: the bucket
      would carry zeros and be copied back over the flushed gradients.  Under a DDP forward the plain path runs."""
    if getattr(model, '_is_replica', False) or threading.current_thread() is not threading.main_thread():
        return True
    return getattr(_DDP, '_active_ddp_module', None) is not None


def arm(model, x=None):
    """Top of a model's forward().  No-op unless: enabled, training mode, autograd on, not inside a stream capture, not a
    DataParallel replica / DDP-wrapped forward, and no TrainStep (or other owner of the library's step switches) active in this
    library context.  Whatever an earlier, unfinished pass left behind (a training forward that never got its backward, a
    backward that raised) is dropped FIRST, also by forwards that do not arm -- an evaluation forward must not be served packed
    weights that were cached before an in-place weight update."""
    if not ENABLED:
        return
    st = _STATE
    if (st.in_pass or st.cache_on is not None or st.direct) and threading.current_thread() is threading.main_thread() \
            and not torch.cuda.is_current_stream_capturing():
        prev = _lib.current_ctx()
        if prev != st.ctx:
            _lib.make_current(st.ctx)
        try:
            _reset()
        finally:
            if prev != st.ctx:
                _lib.make_current(prev)
    if not model.training or not torch.is_grad_enabled() or _wrapped_or_threaded(model):
        return
    if _lib.current_ctx() != 0 or _fn().step_state().direct_param_grads and not _STATE.direct:
        return                                         # a TrainStep owns this thread's step state
    if torch.cuda.is_current_stream_capturing():
        return
    st.ctx = _lib.current_ctx()
    book = _book(model)
    cache = book['cache']
    key = (_param_key(model), _precision.key())
    if cache is not None and cache[2] != key:
        # the parameters moved (a TrainStep re-homed them into its flat bucket, .to(), load of another state) or the matmul
        # precision / tap-conv mode changed (the packings are laid out per level and mode): the recorded (weight pointer, layout)
        # pairs are stale -- start over
        _lib.call('gx_weight_cache_destroy', cache[0])
        cache[0], cache[1], cache[2] = int(_lib.query('gx_weight_cache_create')), False, key
    if cache is None:
        cache = [int(_lib.query('gx_weight_cache_create')), False, key]     # [id, recorded, parameter key]
        book['cache'] = cache
        weakref.finalize(model, _destroy_cache, cache)
    if not cache[1]:
        _lib.call('gx_weight_cache_record', cache[0], 1)
        st.recording = True
    else:
        _lib.call('gx_weight_cache_refresh', cache[0], _hip._stream())
        st.recording = False
    st.cache_on = cache[0]
    st.models = [weakref.ref(model)]
    if x is not None:
        note_eager_iteration(model, x)


def _params(model):
    """The model's parameters, listed once (walking the module tree costs ~0.2 ms per call at 78 parameters: more than the
    launches this mechanism saves would cost on the host) as (owning module, name, parameter) and re-validated by identity on
    every use (78 dictionary look-ups): a parameter that was replaced (`module.weight = nn.Parameter(...)`) rebuilds the list."""
    book = _book(model)
    ent = book['params']
    if ent is not None:
        for mod, name, p in ent:
            if mod._parameters.get(name) is not p:
                ent = None
                break
    if ent is None:
        ent, seen = [], set()
        for mod in model.modules():
            for name, p in mod._parameters.items():
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    ent.append((mod, name, p))
        book['params'] = ent
        book['plist'] = [e[2] for e in ent]
        book['grads'] = None
    return book['plist']


def _param_key(model):
    ps = _params(model)
    return tuple((id(p), p.data_ptr()) for p in ps)


def _destroy_cache(cache):
    try:
        if _STATE.cache_on == cache[0]:
            _reset()
        _lib.call('gx_weight_cache_destroy', cache[0])
    except Exception:       # noqa: BLE001  (interpreter shutdown)
        pass


def begin_backward():
    """From the first HIP autograd node of a backward pass (functions.ctx_bound)."""
    st = _STATE
    if not st.models or st.in_pass:
        return
    st.in_pass = True
    models = [m() for m in st.models]
    params = [p for m in models if m is not None for p in _params(m) if p.requires_grad]
    if params and all(p.grad is None for p in params):
        owner = _book(models[0])
        flat = owner['grads']
        key = tuple(id(p) for p in params) + (params[0].device,)
        if flat is None or flat[0] != key:
            # one flat buffer per dtype, every parameter's gradient a 64-byte-aligned view of it (built once per model)
            views, bufs = [], {}
            for dt in sorted({p.dtype for p in params}, key=str):
                ps = [p for p in params if p.dtype == dt]
                al = 64 // ps[0].element_size()
                offs, n = [], 0
                for p in ps:
                    offs.append(n)
                    n += (p.numel() + al - 1) // al * al
                buf = torch.zeros(n, dtype=dt, device=ps[0].device)
                bufs[dt] = buf
                views.extend((p, buf[o:o + p.numel()].view(p.shape)) for p, o in zip(ps, offs))
            flat = (key, list(bufs.values()), views)
            owner['grads'] = flat
        else:
            for b in flat[1]:
                b.zero_()
        for p, v in flat[2]:
            p.grad = v
        s = _fn().step_state()
        s.direct_param_grads = True
        _fn().begin_direct_grads()
        _hip.defer_state().on = True
        st.direct = True
    torch.autograd.Variable._execution_engine.queue_callback(end_backward)


def flat_grad_buffers(grads):
    """The flat gradient buffers begin_backward built (one per dtype; the padding between two views stays zero) if `grads` are
    exactly the gradient views of one model in them (a subset would drag the other parameters' gradients along), else None --
    genesis_amd.clip_grad_norm_ then reduces a few long segments instead of one per parameter."""
    got = sorted((g.data_ptr(), g.numel()) for g in grads)
    for book in list(_BOOK.values()):
        flat = book.get('grads')
        if flat is None or len(grads) > len(flat[2]):
            continue
        if got == sorted((v.data_ptr(), v.numel()) for _, v in flat[2] if v.numel()):
            return list(flat[1])
    return None


def end_backward():
    st = _STATE
    if not st.in_pass:
        return
    prev = _lib.current_ctx()
    if prev != st.ctx:
        _lib.make_current(st.ctx)
    try:
        if st.direct:
            _fn().join_side_stream()
            _hip.defer_flush()
            s = _fn().step_state()
            s.direct_param_grads = False
            _hip.defer_state().on = False
            st.direct = False
        if st.cache_on is not None:
            if st.recording:
                _lib.call('gx_weight_cache_record', st.cache_on, 0)
                for m in st.models:
                    m = m()
                    c = _BOOK.get(m, {}).get('cache') if m is not None else None
                    if c is not None and c[0] == st.cache_on:
                        c[1] = True
            else:
                _lib.call('gx_weight_cache_release')
            st.cache_on, st.recording = None, False
    finally:
        st.models, st.in_pass = [], False
        if prev != st.ctx:
            try:
                _lib.make_current(prev)
            except Exception:       # noqa: BLE001
                pass


# ---------------------------------------------------------------------------------------------------------------------------
# The unchanged loop as two replayed HIP graphs (round 6).  With the mechanism above the unchanged train.py loop is bound by the
# HOST: ~170 ctypes launches + autograd bookkeeping per iteration issue more slowly than the GPU executes them.
# From the third iteration of a steady loop on -- same input shape, same parameters, no injected noise -- the model therefore
#   * captures its forward pass (the packed-weight refresh included) into ONE HIP graph on a private copy of the input and, in every
#     later iteration, copies x in, replays it and returns the SAME static output tensors; every one that required grad at capture
#     (the loss terms, mu, sigma, z, the masks, recon, x_r, log_m_r, ...) is re-wrapped as an output of one autograd node
#     (`_ReplayFn`) -- to the loop they are ordinary tensors that require grad;
#   * captures, at the first `loss.backward()` that reaches that node (normally with gradients for the loss terms only: err, the
#     KL terms, train.py:226-242), the whole backward pass for that set of outputs -- zeroed flat gradient buffer, direct gradient writes, ONE stream-K weight-gradient
#     launch, batched reductions -- into a second graph, and replays it from then on after copying the incoming gradients into
#     static buffers.  p.grad are views of the flat buffer, as above; `torch.optim.*.step()` consumes them as usual.
# The loop's contract is untouched: `optimiser.zero_grad(); model(x); ...; loss.backward(); optimiser.step()`.  What differs from the
# eager path and is documented here: the returned tensors are overwritten by the next forward (train.py reads what it logs before
# that: `.item()`, train.py:266-270).  Everything else falls back -- and stays correct: gradients already present at backward
# time (accumulation) or a set of outputs with gradients other than the captured one (a loss that also reads `recon` or
# `comp_stats.z_k`) run the ordinary autograd backward of the captured forward's own (retained) graph from those outputs, on the
# static tensors; a changed input shape, moved / replaced / frozen parameters, a changed scalar setting (_SETTINGS, the attention
# kernel), eval mode, no_grad, injected noise, dynamic_K, a TrainStep in the same context, DataParallel / DDP wrappers take the eager
# path above.
# GENESIS_AUTOSTEP_GRAPH=0 switches this stage off.
GRAPH = os.environ.get('GENESIS_AUTOSTEP_GRAPH', '1') != '0'
_STABLE_ITERS = 2          # eager (armed) iterations with the same key before the capture


class _GraphState(object):
    __slots__ = ('key', 'stable', 'F', 'B', 'static_x', 'tensors', 'meta', 'roots', 'root_names', 'static_grads', 'bpattern',
                 'cache_id', 'flat', 'params', 'dummy', 'replays', 'bwd_replays', 'bwd_fallbacks', 'failed')

    def __init__(self):
        self.key, self.stable, self.F, self.B = None, 0, None, None
        self.replays = self.bwd_replays = self.bwd_fallbacks = 0
        self.failed = False


def _gstate(model):
    b = _book(model)
    g = b.get('graph')
    if g is None:
        g = b['graph'] = _GraphState()
    return g


def graph_stats(model):
    """(forward replays, backward replays, backward fallbacks) of the model's captured loop -- tests / bench."""
    g = _BOOK.get(model, {}).get('graph')
    return (g.replays, g.bwd_replays, g.bwd_fallbacks) if g is not None else (0, 0, 0)


# The model's scalar settings a captured forward bakes in (read by _compute, _decode, _component_kl as Python values).
_SETTINGS = ('klm_loss', 'detach_mr_in_klm', 'pixel_bound', 'autoreg_prior', 'std')


def _graph_key(model, x):
    # the parameters with their requires_grad flags (the captured backward writes a gradient for every parameter it captured),
    # the settings above, the attention kernel, and the matmul precision level and tap-conv mode (a graph captured under others
    # holds their kernels and packings)
    ap = getattr(model, 'att_process', None)
    return (tuple(x.shape), x.dtype, x.device, tuple((id(p), p.data_ptr(), p.requires_grad) for p in _params(model)),
            tuple(getattr(model, k, None) for k in _SETTINGS), getattr(ap, 'kernel', None), getattr(ap, 'semiconv', None),
            _precision.key())


def _drop_graph(g):
    g.F = g.B = None
    g.static_x = g.tensors = g.roots = g.static_grads = None
    g.stable = 0


class _ReplayFn(torch.autograd.Function):
    """Every captured output that required grad (the loss terms, mu, sigma, z, the masks, the decoder outputs, ...) as the outputs
    of ONE autograd node; its backward is the captured backward graph, or the retained-graph fallback for another pattern."""

    @staticmethod
    def forward(ctx, dummy, g):
        ctx.g = g
        ctx.level = _precision.key()
        ctx.set_materialize_grads(False)
        return tuple(t.detach() for t in g.roots)

    @staticmethod
    def backward(ctx, *grads):
        _precision.check_backward_key(ctx.level)
        _graph_backward(ctx.g, grads)
        return None, None


def graph_forward(model, x):
    """From model.forward(x) (no injected noise).  Returns the dict of output tensors for model._assemble, or None: the eager path."""
    if not (ENABLED and GRAPH) or not model.training or not torch.is_grad_enabled() or _wrapped_or_threaded(model):
        return None
    if getattr(model, 'dynamic_K', False) or getattr(model, 'noise', None) is not None:
        return None
    if _lib.current_ctx() != 0 or _fn().step_state().direct_param_grads or torch.cuda.is_current_stream_capturing():
        return None
    g = _gstate(model)
    if g.failed:
        return None
    key = _graph_key(model, x)
    if g.key != key:
        _drop_graph(g)
        g.key = key
        return None                                    # (this iteration and the next: eager, armed)
    if g.F is None:
        book = _book(model)
        cache = book.get('cache')
        if g.stable < _STABLE_ITERS or cache is None or not cache[1] or book.get('grads') is None:
            return None
        st = _STATE
        if st.in_pass or st.cache_on is not None or st.direct:
            _reset()
        try:
            _capture_forward(model, x, g, cache[0], book)
        except Exception:       # noqa: BLE001  (whatever the capture raised: the eager path is always valid)
            _drop_graph(g)
            g.failed = True
            torch.cuda.synchronize()
            return None
    else:
        g.static_x.data.copy_(x)      # (.data: the captured forward's autograd graph saved static_x -- no version bump)
        g.F.replay()
    g.replays += 1
    outs = _ReplayFn.apply(g.dummy, g)
    t = {k: v.detach() for k, v in g.tensors.items()}
    t.update(g.meta)
    for name, o in zip(g.root_names, outs):
        t[name] = o
    return t


def note_eager_iteration(model, x):
    """From arm(): one more eager iteration with this (shape, parameters) key completed its forward."""
    if not GRAPH:
        return
    g = _gstate(model)
    key = _graph_key(model, x) if x is not None else None
    if g.key == key and g.F is None:
        g.stable += 1


def _same(t):
    return t


def _capture_forward(model, x, g, cache_id, book):
    g.static_x = x.clone()
    g.cache_id = cache_id
    g.params = [p for p in _params(model) if p.requires_grad]
    g.flat = book['grads']
    g.dummy = g.params[0]
    F = torch.cuda.CUDAGraph()
    # (identity saved-tensor hooks: the captured forward's autograd graph outlives optimiser steps -- parameters it saved are
    #  updated in place between its replays, which is exactly what is wanted: a backward pass through it reads the CURRENT static
    #  activations and the CURRENT weights; tensors that come back through an unpack hook carry no version check)
    with torch.cuda.graph(F, capture_error_mode='thread_local'), torch.autograd.graph.saved_tensors_hooks(_same, _same):
        _lib.call('gx_weight_cache_refresh', cache_id, _hip._stream())
        try:
            t = model._compute(g.static_x)
        finally:
            _lib.call('gx_weight_cache_release')
    g.meta = {k: v for k, v in t.items() if not torch.is_tensor(v)}
    g.tensors = {k: v for k, v in t.items() if torch.is_tensor(v)}
    # (every output a gradient can reach: one left out would come back detached and its gradient would be lost)
    g.root_names = [k for k, v in g.tensors.items() if v.requires_grad]
    g.roots = [g.tensors[k] for k in g.root_names]
    g.F, g.B, g.bpattern = F, None, None
    F.replay()                      # (a capture executes nothing)


def _graph_backward(g, grads):
    pattern = tuple(x is not None for x in grads)
    clean = all(p.grad is None for p in g.params)
    if clean and (g.B is not None and pattern == g.bpattern):
        for p, v in g.flat[2]:
            p.grad = v
        for sg, x in zip(g.static_grads, grads):
            if sg is not None:
                sg.copy_(x)
        g.B.replay()
        g.bwd_replays += 1
        return
    if clean and g.B is None and any(pattern):
        try:
            _capture_backward(g, grads, pattern)
            g.bwd_replays += 1
            return
        except Exception:       # noqa: BLE001
            g.B = None
            g.failed = True         # (the forward graph stays valid for this iteration; later ones run eagerly)
            torch.cuda.synchronize()
            for p in g.params:
                p.grad = None
    # the ordinary autograd backward of the captured forward's own graph, on the static tensors: gradient accumulation over
    # several backward passes, gradients for outputs other than the captured pattern
    g.bwd_fallbacks += 1
    roots = [r for r, x in zip(g.roots, grads) if x is not None]
    if roots:
        torch.autograd.backward(roots, [x for x in grads if x is not None], retain_graph=True)


def _capture_backward(g, grads, pattern):
    g.static_grads = [x.clone() if x is not None else None for x in grads]
    for p, v in g.flat[2]:
        p.grad = v
    roots = [r for r, x in zip(g.roots, grads) if x is not None]
    sgr = [x for x in g.static_grads if x is not None]
    B = torch.cuda.CUDAGraph()
    s = _fn().step_state()
    with torch.cuda.graph(B, pool=g.F.pool(), capture_error_mode='thread_local'):
        for b in g.flat[1]:
            b.zero_()
        s.direct_param_grads = True
        _fn().begin_direct_grads()
        _hip.defer_state().on = True
        _lib.call('gx_weight_cache_activate', g.cache_id)
        try:
            torch.autograd.backward(roots, sgr, retain_graph=True)
            _fn().join_side_stream()
            _hip.defer_flush()
        finally:
            s.direct_param_grads = False
            _hip.defer_state().on = False
            _hip.defer_discard()
            _lib.call('gx_weight_cache_release')
    g.B, g.bpattern = B, pattern
    B.replay()
