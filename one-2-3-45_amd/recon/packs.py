"""Parameter reads and packed-operand caches that also work on ``nn.DataParallel`` replicas of the mirror modules.

``torch.nn.parallel.replicate`` (run by ``DataParallel.forward`` on EVERY forward once more than one device is given) builds each replica with
``_replicate_for_data_parallel``: a shallow copy of the module's ``__dict__`` with ``_parameters == {}``, the broadcast copies of the parameters set as
plain attributes, and ``state_dict()`` without parameter keys.  So

* ``param(module, name)`` reads a parameter from ``_parameters`` when the module owns it and falls back to the attribute on a replica;
* ``PackCache`` holds the kernel packings of one mirror module per device.  It is created in the mirror's ``__init__``, so the source module and every
  replica of it share the SAME object (the shallow ``__dict__`` copy).  Entries are keyed by the SOURCE module's parameters (object, storage, version
  counter) -- a replica's tensors are new on every forward and would never hit -- plus whatever else the packing depends on (precision, resolution).
  A second forward with unchanged weights packs nothing on any device; an optimiser step, ``load_state_dict`` or an in-place update of the source
  re-packs once per device.  The first packing on a device also loads the library's code objects there (``ops.preload``).

Thread safety: ``DataParallel`` runs its replicas on one host thread per device (``parallel_apply``).  Building and inserting an entry happens under a
per-slot lock, so each (kind, device, slot) is packed exactly once and no thread sees a half-built entry (entries are inserted as complete tuples).
The cache is not part of ``state_dict()`` and ``.to()`` does not touch it; ``copy.deepcopy`` and ``pickle`` give the copy its own, EMPTY cache bound to
the copy (``__reduce__``: the locks are never copied)."""
import threading
import weakref

import torch

_STATS = {}                         # (kind, device) -> number of packings built in this process (pack_stats)
_STATS_LOCK = threading.Lock()


def param(module, name):
    """The parameter ``name`` of ``module``: ``_parameters[name]`` when the module owns it, else the attribute (an ``nn.DataParallel`` replica holds its
    broadcast copy as a plain attribute and has ``_parameters == {}``)."""
    return module._parameters[name] if name in module._parameters else getattr(module, name)


def params_key(ps):
    """Identity of a parameter list (objects, storages, version counters): changes with any load / assignment / in-place update."""
    return tuple((id(p), p.data_ptr(), p._version) for p in ps)


def pack_stats():
    """{(kind, device): packings built in this process} for every kind of packed operand of the mirrors ("sdf_blob", "sdf_grid", "costreg", "colour",
    "conv", "lattice"), plus ("preload", device): 1 for every device whose code objects were loaded.  "Packed once per device" is visible here: a second
    forward of an unchanged model -- replicated or not -- adds nothing."""
    from .. import ops
    with _STATS_LOCK:
        out = dict(_STATS)
    for d in list(ops._preloaded):
        out[("preload", str(d))] = 1
    return out


def _count(kind, device):
    with _STATS_LOCK:
        k = (kind, str(device))
        _STATS[k] = _STATS.get(k, 0) + 1


class PackCache:
    """Per-device packed operands of ONE mirror module, shared by the module and all of its ``nn.DataParallel`` replicas (see the module docstring)."""

    def __init__(self, owner=None):
        self._owner = weakref.ref(owner) if owner is not None else None
        self._entries = {}                 # (kind, device, slot) -> (key, value)
        self._locks = {}                   # (kind, device, slot) -> threading.Lock
        self._guard = threading.Lock()

    def __reduce__(self):
        # deepcopy / pickle: an EMPTY cache bound to the copy of the owner (the owner is memoised before its __dict__ is copied)
        return (PackCache, (self.owner(),))

    def owner(self):
        return self._owner() if self._owner is not None else None

    def source(self, module):
        """The module whose parameters key the entries: the source module for a replica, ``module`` itself otherwise."""
        if getattr(module, "_is_replica", False):
            o = self.owner()
            if o is not None:
                return o
        return module

    def get(self, kind, device, key, make, slot=None):
        """The entry (kind, device, slot) if it was built for ``key``; else ``make()`` -- exactly once across threads -- stored and returned."""
        if not isinstance(device, torch.device):
            device = torch.device(device)
        s = (kind, device, slot)
        e = self._entries.get(s)
        if e is not None and e[0] == key:
            return e[1]
        with self._guard:
            lock = self._locks.setdefault(s, threading.Lock())
        with lock:
            e = self._entries.get(s)
            if e is not None and e[0] == key:
                return e[1]
            if device.type == "cuda":
                from .. import ops
                ops.preload(device)        # the first use on a device loads every code object there (not inside the first kernel call)
            val = make()
            self._entries[s] = (key, val)
            _count(kind, device)
            return val

    def discard(self, kind, device, slot=None):
        self._entries.pop((kind, torch.device(device), slot), None)

    def clear(self):
        """Drop every entry (featurenet.invalidate_packed: parameter updates through ``.data`` bump no version counter)."""
        self._entries.clear()

    def __len__(self):
        return len(self._entries)
