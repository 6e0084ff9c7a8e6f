"""The reference's answers without the reference: every call a test makes on the reference sampler
(oracle/_ref, built only where the reference sources are) is keyed by its inputs and its answer
is stored in tests/golden/ref_replay.json.gz.

  * oracle/_ref built: the call runs live; an answer already stored for the same key must equal
    it; with EULER_REF_RECORD=1 the answers are (re)written to the file at the end of the session.
  * oracle/_ref absent: the stored answer is returned; a call with no stored answer fails.

A reference graph is identified by the digest of what built it (build_raw's arrays, the feature
lists pushed into it), so the same call on two graphs has two keys.

An answer array of more than SMALL elements is stored as a Digest (SHA-256 of its shape and
bytes, its dtype) unless the tests read its values (FULL); same(a, b) compares either form bit
for bit, and a Digest passed back into a reference call keys it as the array it stands for."""
import atexit
import base64
import gzip
import hashlib
import json
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ref_replay.json.gz")
RECORD = os.environ.get("EULER_REF_RECORD") == "1"

SMALL = 64                   # answer arrays up to this many elements are stored whole
FULL = ("node_order",)       # ... and these answers, whose values the tests use as inputs

_stored = None
_recorded = {}


def _bytes_digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()[:32]


class Digest:
    """Stands for a large array of the reference's answer: its dtype, shape and bytes' digest."""

    def __init__(self, dtype, shape, hexdigest):
        self.dtype, self.shape, self.hex = np.dtype(dtype), tuple(shape), hexdigest

    def __len__(self):
        return self.shape[0]

    def view(self, dtype):
        assert np.dtype(dtype).itemsize == self.dtype.itemsize
        return Digest(dtype, self.shape, self.hex)


def same(a, b):
    """np.array_equal, where either side may be a Digest (then: bit for bit, b cast to a's dtype)"""
    if isinstance(b, Digest) and not isinstance(a, Digest):
        a, b = b, a
    if isinstance(a, Digest):
        if isinstance(b, Digest):
            return a.shape == b.shape and a.hex == b.hex
        b = np.asarray(b)
        return a.shape == b.shape and a.hex == _bytes_digest(b.astype(a.dtype, copy=False))
    return np.array_equal(a, b)


def _digest_into(h, x):
    if isinstance(x, Digest) or (isinstance(x, np.ndarray) and x.size > SMALL):
        d = x if isinstance(x, Digest) else None
        h.update(b"D%s%s" % ((d.dtype if d else x.dtype).str.encode(),
                             (d.hex if d else _bytes_digest(x)).encode()))
    elif isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        h.update(b"A%s%r" % (a.dtype.str.encode(), a.shape))
        h.update(a.tobytes())
    elif isinstance(x, (list, tuple)):
        h.update(b"L%d[" % len(x))
        for y in x:
            _digest_into(h, y)
        h.update(b"]")
    elif isinstance(x, dict):
        for k in sorted(x):
            h.update(repr(k).encode())
            _digest_into(h, x[k])
    elif isinstance(x, (str, bytes, int, float, bool, type(None), np.generic)):
        h.update(b"S" + repr(x.item() if isinstance(x, np.generic) else x).encode())
    elif hasattr(x, "__dict__"):          # DenseFeatures / SparseFeatures: their arrays
        h.update(type(x).__name__.encode())
        _digest_into(h, {k: v for k, v in vars(x).items() if not k.startswith("_")})
    else:
        raise TypeError("cannot key a reference call on %r" % type(x))


def _key(*parts):
    h = hashlib.sha256()
    _digest_into(h, parts)
    return h.hexdigest()[:32]


def _pack(value, full=False):
    """value -> JSON structure: arrays inline (dtype, shape, base64 of the bytes), large ones as a Digest"""
    if isinstance(value, np.ndarray) and value.size > SMALL and not full:
        return {"d": [value.dtype.str, list(value.shape), _bytes_digest(value)]}
    if isinstance(value, np.ndarray):
        a = np.ascontiguousarray(value)
        return {"a": [a.dtype.str, list(a.shape), base64.b64encode(a.tobytes()).decode()]}
    if isinstance(value, (list, tuple)):
        return {"t" if isinstance(value, tuple) else "l": [_pack(v, full) for v in value]}
    if isinstance(value, np.generic):
        value = value.item()
    if hasattr(value, "__dict__"):        # a CSR: its fields
        return {"o": {k: _pack(v, full) for k, v in vars(value).items()}}
    return {"v": value}


def _unpack(s):
    if "a" in s:
        dt, shape, b = s["a"]
        return np.frombuffer(base64.b64decode(b), dtype=dt).reshape(shape).copy()
    if "d" in s:
        return Digest(*s["d"])
    if "t" in s:
        return tuple(_unpack(v) for v in s["t"])
    if "l" in s:
        return [_unpack(v) for v in s["l"]]
    if "o" in s:
        return types.SimpleNamespace(**{k: _unpack(v) for k, v in s["o"].items()})
    return s["v"]


def _load():
    global _stored
    if _stored is None:
        _stored = {}
        if os.path.exists(PATH):
            with gzip.open(PATH, "rt") as f:
                _stored = json.load(f)
    return _stored


def _same(a, b):
    if isinstance(a, Digest) or isinstance(b, Digest):
        return same(a, b) and (a.dtype == b.dtype)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if hasattr(a, "__dict__") and hasattr(b, "__dict__"):
        return vars(a).keys() == vars(b).keys() and all(_same(v, vars(b)[k]) for k, v in vars(a).items())
    return a == b


def answer(live, key, what, full=False):
    """live: a callable running the reference, or None where it is absent"""
    stored = _load()
    if live is None:
        if key not in stored:
            raise AssertionError("no stored reference answer for %s (key %s): rerun the tests where "
                                 "oracle/_ref is built with EULER_REF_RECORD=1" % (what, key))
        return _unpack(stored[key])
    value = live()
    if key in stored:
        assert _same(value, _unpack(stored[key])), \
            "the reference's answer to %s differs from the stored one" % what
    if RECORD:
        _recorded[key] = _pack(value, full)
    return value


@atexit.register
def _save():
    """Write the answers recorded in this session (EULER_REF_RECORD=1) next to the stored ones."""
    if RECORD and _recorded:
        merged = dict(_load())
        merged.update(_recorded)
        with open(PATH, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, compresslevel=9) as f:
            f.write(json.dumps(merged, sort_keys=True, separators=(",", ":")).encode())


def call(O, name, *args):
    """A module-level function of oracle.py that runs the reference (e.g. ref_umap_iteration_order)."""
    live = (lambda: getattr(O, name)(*args)) if O.have_ref() else None
    return answer(live, _key("fn", name, args), name)


_MUTATORS = ("add_edges_from_adjacency",)


class RefReplay:
    """Stands for an O.RefGraph: method calls are answered live or from the stored answers."""

    def __init__(self, O, graph, ident):
        self._O, self._graph, self._ident = O, graph, ident

    @classmethod
    def build_raw(cls, O, *args, **kw):
        graph = O.RefGraph.build_raw(*args, **kw) if O.have_ref() else None
        return cls(O, graph, _key("build_raw", args, kw))

    def __getattr__(self, name):
        def method(*args, **kw):
            live = (lambda: getattr(self._graph if self._graph is not None else self._O.RefGraph, name)(*args, **kw)) \
                if self._O.have_ref() else None
            if name.startswith("set_"):       # the graph's state changes: so does its identity
                self._ident = _key(self._ident, name, args, kw)
                return live() if live else None
            value = answer(live, _key(self._ident, name, args, kw), "RefGraph." + name, name in FULL)
            if name in _MUTATORS:
                self._ident = _key(self._ident, name, args, kw)
            return value
        return method
