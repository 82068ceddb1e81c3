"""What every packer behind the optimizer loop shares (theseus_amd/packed.py: PackedPoseGraph, theseus_amd/ba.py: PackedBA,
theseus_amd/generic.py: PackedState and its subclasses): who owns the state buffer, and -- for the two fused packers, whose buffers
are built from thousands of Variables -- whether somebody changed a variable behind the packer's back.

``StateOwner``: the state the loop moves around lives in buffers of the packer; the Variable objects are in one of three states
(DESIGN.md, 2.2):
  * they VIEW the state (``_state_exposed``): whoever holds their tensors holds the buffer, which is never recycled;
  * the state is PRIVATE and they are behind it (``_vars_stale``): the loop recycles its buffers, ``flush_variables`` catches up;
  * they KEEP the caller's graph-carrying tensors (neither flag): the packed copy is private, the values are the same.
``TrackedVariables(StateOwner)``: update counters and deep stamps of every variable the buffers are built from, and the endings of
a re-packing ``sync``.
"""
import operator

import torch

from .core import Variable
from .kernels import default_kernels

_GET_TENSOR = {True: operator.attrgetter("_tensor"), False: operator.attrgetter("tensor")}   # own Variable: skip the property
_DATA_PTR, _VERSION, _NUM_UPDATES = operator.methodcaller("data_ptr"), operator.attrgetter("_version"), operator.attrgetter("_num_updates")

# one C++ loop over a list of tensors instead of 33 k method calls (torch's cudagraph trees check their static inputs with it)
_PTRS_EQUAL = getattr(torch._C, "_tensors_data_ptrs_at_indices_equal", None)


class _AuxDeepStamp:
    """Deep stamp of the AUXILIARY variables' tensors (measurements, weights, ... -- 33 k of them in a bundle-adjustment objective):
    has anybody replaced a tensor object, swapped the storage under one (``var.tensor.data = other`` / ``set_()``: object and
    version counter stay), or edited one in place (``var.tensor.mul_()``: only the autograd version counter moves)?  The reference
    re-reads ``var.tensor`` at every evaluation (core/objective.py:813-830) and sees all three.

    Three flat comparisons instead of a 3-tuple per tensor (12 ms at 33 k tensors):
      * the tuple of object ids (0.9 ms; the tensors are kept referenced here, so an id cannot be recycled);
      * the storage pointers, in one C++ call against the cached list (2 ms; a Python pass of ``data_ptr()`` calls: 4.3 ms);
      * the version counters of one REPRESENTATIVE per group of tensors that share one: views share their base's counter
        (``feat[:, k]`` for 32768 observations is one counter), so an in-place edit through ANY of them moves the representative's.
        A tensor's ``_base`` is fixed at creation: the grouping holds for as long as the ids do."""

    def __init__(self):
        self.refs = self.ids = self.ptrs = self.ptrs_t = self.reps = self.idx = None

    def stamp(self, ts):
        ids = tuple(map(id, ts))
        if ids != self.ids:
            self.refs, self.ids = ts, ids
            self.ptrs = list(map(_DATA_PTR, ts))
            self.ptrs_t = tuple(self.ptrs)
            self.idx = list(range(len(ts)))
            groups = {}
            for t in ts:
                base = t._base
                groups.setdefault(id(base) if base is not None else id(t), t)
            self.reps = list(groups.values())
        else:
            same = None
            if _PTRS_EQUAL is not None and ts:
                try:
                    same = _PTRS_EQUAL(ts, self.ptrs, self.idx)
                except TypeError:      # (a private torch symbol: another signature in another release -> the Python pass)
                    same = None
            if same is None:
                same = list(map(_DATA_PTR, ts)) == self.ptrs
            if not same:
                self.ptrs = list(map(_DATA_PTR, ts))
                self.ptrs_t = tuple(self.ptrs)
        return ids, self.ptrs_t, tuple(map(_VERSION, self.reps))


def _opt_deep_stamp(ts):
    """Deep stamp of the optimisation variables' tensors: storage pointer + version counter (they are views of the packed state:
    holding the objects would pin a state buffer), as two flat tuples."""
    return tuple(map(_DATA_PTR, ts)), tuple(map(_VERSION, ts))


def _views_deep_stamp(buffers):
    """``_opt_deep_stamp`` of variables that were JUST re-pointed at ``buf.unbind(0)`` of these buffers, without touching the 8.7 k
    view objects: view k starts ``k * stride(0)`` elements into its buffer and shares the buffer's version counter."""
    ptrs, vers = (), ()
    for buf in buffers:
        n, step = buf.shape[0], buf.stride(0) * buf.element_size()
        base = buf.data_ptr()
        ptrs += tuple(range(base, base + n * step, step)) if step else (base,) * n
        vers += (buf._version,) * n
    return ptrs, vers


def _each(f, state):
    """``f`` over the buffers of a state: one tensor, or a tuple of them (bundle adjustment: (cams, points))."""
    return tuple(map(f, state)) if isinstance(state, tuple) else f(state)


class StateOwner:
    """The life cycle of the optimisation state.  A subclass says what the state is -- ``_get_state()`` / ``_set_state(new)``: one
    tensor, or a tuple of tensors -- and implements ``_repoint_variables()``: make every optimisation variable's tensor a view of the
    state, clear ``_vars_stale``, set ``_state_exposed``.  ``_vars_stale`` is only ever set while a state exists."""

    def __init__(self, objective, kernels=None):
        self.objective = objective
        self.K = kernels or default_kernels()
        self._vars_stale = False
        self._state_exposed = False
        self._keep_graph_tensors = False   # set by the optimizer around an optimize() that differentiates from the initial tensors
        self._defer_repoint = False        # set by the optimizer around its first sync (TrackedVariables._finish_sync)
        self._bufs = {}

    @property
    def state(self):
        return self._get_state()

    @property
    def device(self):
        state = self._get_state()
        return (state[0] if isinstance(state, tuple) else state).device

    def alloc_state(self):
        return _each(torch.empty_like, self._get_state())

    def clone_state(self):
        return _each(torch.clone, self._get_state())

    def privatize_state(self):
        """Called at the start of ``optimize()``: if the state buffer is the one the variables' tensors view (i.e. what the
        previous ``optimize()`` / ``forward()`` handed to the user, possibly carrying an autograd graph), continue on a
        private copy -- the loop recycles its two state buffers through raw-pointer kernels and must never write into a
        tensor somebody else holds."""
        if self._state_exposed:
            with torch.no_grad():
                self._set_state(_each(lambda t: t.detach().clone(), self._get_state()))
            self._state_exposed = False
            self._vars_stale = True

    def swap_state(self, new, repoint: bool = False):
        """Adopt ``new`` as the current state (after an accepted step); returns the previous buffer(s) for re-use.  Without
        ``repoint`` the O(#variables) Python re-pointing of the Variable objects is deferred (the optimiser loop flushes before
        anybody can look: callbacks, loop exit)."""
        old = self._get_state()
        self._set_state(new)
        if repoint:
            self._repoint_variables()
        else:
            self._vars_stale = True
        return old

    def flush_variables(self):
        if self._vars_stale:
            self._repoint_variables()

    @staticmethod
    def _mask_u8(ignore_mask):
        return ignore_mask if ignore_mask is None or ignore_mask.dtype == torch.uint8 else ignore_mask.to(torch.uint8)

    def _buf(self, key, shape, dtype=None):
        """Scratch tensor ``key``, re-allocated when shape, dtype or device moved."""
        t = self._bufs.get(key)
        dt, dev = dtype or self.objective.dtype, self.device
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != dev:
            t = torch.empty(*shape, dtype=dt, device=dev)
            self._bufs[key] = t
        return t


class TrackedVariables(StateOwner):
    """Change detection for packers whose buffers (``self.tensors``, None until the first sync) are copies of the variables' tensors.
    A subclass provides ``_walk_tracked()`` -- every variable the buffers are built from, the optimisation variables
    (``optim_variables``) first -- and ``_state_groups()`` -- [(variables, the state buffer whose ``unbind(0)`` they view)]; it calls
    ``_start_tracking()`` at the end of its constructor."""

    defers_repoint = True   # honour the optimizer's ``_defer_repoint`` (PackedBA does not: its inputs are re-pointed twice per forward)

    def _start_tracking(self):
        """The objective is frozen once an optimizer holds it (Optimizer.optimize checks its version): the walk over the cost
        functions is done once, every later stamp is one pass over the cached list (7 k variables at the headline size)."""
        seen, self._tracked_list = set(), []   # each variable ONCE: a cost weight shared by 1024 edges is one entry
        for v in self._walk_tracked():
            if id(v) not in seen:
                seen.add(id(v))
                self._tracked_list.append(v)
        self._n_opt = len(self.optim_variables)
        # the O(1) "nothing changed" test relies on theseus_amd.core.Variable's global update counter
        self._own_variables = all(isinstance(v, Variable) for v in self._tracked_list)
        self._stamp = None
        self._deep_stamp = None
        self._aux_stamp = _AuxDeepStamp()
        self._global_stamp = -1

    def tracked_list(self):
        """Every variable the packed buffers are built from, each once, the optimisation variables first."""
        return self._tracked_list

    def _counters_unchanged(self) -> bool:
        return self._own_variables and self._stamp is not None and Variable._global_updates == self._global_stamp

    def _current_stamp(self, deep: bool = False):
        if deep:
            # (optimisation part, auxiliary part): catches IN-PLACE edits of a variable's tensor that never go through
            # Variable.update() (an nn.Parameter stepped by a torch optimizer, ``var.tensor.mul_()``), ``var.tensor = other`` and
            # ``var.tensor.data = other`` -- see _AuxDeepStamp.
            ts = list(map(_GET_TENSOR[self._own_variables], self._tracked_list))
            return _opt_deep_stamp(ts[:self._n_opt]), self._aux_stamp.stamp(ts[self._n_opt:])
        return tuple(map(_NUM_UPDATES, self._tracked_list))

    @staticmethod
    def _stack(ts, B):
        """list of (b_k, ...) with b_k in {1,B} -> (len, 1|B, ...) contiguous."""
        if not ts:
            return None
        if all(t.shape[0] == ts[0].shape[0] for t in ts):
            return torch.stack(ts, dim=0).contiguous()
        return torch.stack([t.expand(B, *t.shape[1:]) for t in ts], dim=0).contiguous()

    def _changed(self, force: bool, deep: bool):
        """What ``sync(force, deep)`` has to re-pack: None (nothing), else (optimisation part changed, auxiliary part changed,
        stamp, deep stamp | None) -- the stamps this look computed, for ``_finish_sync``.  ``deep`` also looks for in-place edits of
        the variables' tensors (storage pointer + version counter): the optimizers ask for it once per ``optimize()``, the
        inner-loop calls keep the O(1) test; with the reference's own Variable class (theseus_amd/plugin.py) every call is deep --
        there is no global update counter to lean on."""
        deep = deep or not self._own_variables
        packed = self.tensors is not None
        if packed and not force and not deep and Variable._global_updates == self._global_stamp:
            return None  # nobody called Variable.update()/to() since the last look: O(1) fast path
        # (nobody called Variable.update() / to() since the last look: the update counters -- the shallow stamp -- are what they
        #  were; a pass over 42 k variables of a bundle-adjustment objective is ~10 ms of host time per optimize())
        # (the reference's Variable: the deep stamp -- storage + version of every tensor -- is the only one looked at: a
        #  Variable.update() that changes neither is not a change.  One pass per call instead of two.)
        shallow = self._own_variables or self._stamp is None
        stamp = self._stamp if (self._counters_unchanged() or not shallow) else self._current_stamp()
        dstamp = self._current_stamp(deep=True) if deep else None
        if force or not packed:
            return True, True, stamp, dstamp
        n = self._n_opt
        opt = (shallow and stamp[:n] != self._stamp[:n]) or (deep and dstamp[0] != self._deep_stamp[0])
        aux = (shallow and stamp[n:] != self._stamp[n:]) or (deep and dstamp[1] != self._deep_stamp[1])
        if not (opt or aux):
            self._global_stamp = Variable._global_updates
            return None
        return opt, aux, stamp, dstamp

    def _finish_sync(self, stamp, dstamp, adopted: bool = False):
        """After a re-pack (``stamp``, ``dstamp``: what ``_changed`` handed back): where do the variables stand?"""
        # (the auxiliary entries of the deep stamp: what this call saw -- _repoint_variables patches the optimisation variables')
        self._deep_stamp = dstamp if dstamp is not None else self._current_stamp(deep=True)
        if adopted:   # the variables hold views of this very buffer already (PackedPoseGraph.buffer_of): only the stamps move
            stale, exposed = False, True
        elif (not any(buf.requires_grad for _, buf in self._state_groups())
              and (self._keep_graph_tensors or not self._own_variables)
              and any(v.tensor.requires_grad for v in self.optim_variables)):
            # packed under no_grad from tensors that carry autograd history (the values the caller passed in, about to be
            # differentiated through: backward_mode="unroll"): re-pointing the variables to views of this graph-less copy would cut
            # them off -- they keep their tensors (same values), the copy is private.  Only where that is needed: theseus_amd's
            # own loop says so for the optimize() calls that captured the initial tensors (``_keep_graph_tensors``: everywhere
            # else the variables view the packed state, also inside callbacks and after an exception); under the reference's
            # loop (its Variable class), which re-assigns every variable every iteration anyway.
            stale, exposed = False, False
        elif self.defers_repoint and self._defer_repoint and self._own_variables:
            # the optimizer's sync at the start of optimize(): the loop is about to continue on a PRIVATE state buffer and re-points
            # the variables when it is done (or before anybody can look: callbacks, exceptions -- flush_variables) -- re-pointing
            # them to views of THIS buffer first was 5 ms of host time per optimize() at 4096 poses in front of the first kernel,
            # for views nobody ever read.  The variables keep the tensors they hold (the same values) until then.
            stale, exposed = True, False
        else:
            self._repoint_variables()
            return
        self._stamp = stamp
        self._global_stamp = Variable._global_updates
        self._vars_stale, self._state_exposed = stale, exposed

    def remember_views(self, buf: torch.Tensor, views):
        """Hook of ``_repoint_variables`` for a packer that recognises a list of its own views as one buffer (PackedPoseGraph)."""

    def _repoint_variables(self):
        """Make every optimisation variable's tensor a view of its state buffer."""
        groups = self._state_groups()
        # the optimiser calls this under no_grad; after the implicit last step the state carries a graph and the per-variable
        # views must stay attached to it
        with torch.set_grad_enabled(any(buf.requires_grad for _, buf in groups)):
            attr = "_tensor" if self._own_variables else "tensor"   # (own Variable: no update count for a re-pointing, core.py)
            for variables, buf in groups:
                views = buf.unbind(0)  # one call builds all the views
                for v, t in zip(variables, views):
                    setattr(v, attr, t)
                self.remember_views(buf, views)
        if not self._counters_unchanged():
            self._stamp = self._current_stamp()
        # deep stamp: only the optimisation variables were re-pointed here -- the auxiliary variables' entries (the bulk: 1 k
        # measurements of a pose graph, 33 k features of a bundle-adjustment problem) are still the ones sync() looked at
        if self._deep_stamp is not None:
            self._deep_stamp = (_views_deep_stamp([buf for _, buf in groups]), self._deep_stamp[1])
        else:
            self._deep_stamp = self._current_stamp(deep=True)
        self._global_stamp = Variable._global_updates
        self._vars_stale = False
        self._state_exposed = True   # the variables (and whoever holds their tensors) now view the state buffer
