"""Stored reference calls: the reference-parity tests without the reference tree.

The tests that pin this package to the reference call its functions through the ``ref`` fixture (``ref.<module>.<function>``)
or through ``oracle.reference_loader`` (``load_function`` / ``load_distributed_utils`` / ``load_trajectory_builder``).  Where the
reference tree is readable they run against it, live.  Where it is not, the calls are answered from
``tests/golden/reference_calls/<test module>.pt.xz``: per test, in call order, a fingerprint of the call's inputs, the outputs the
reference returned, and what it changed in place in its tensor / dict arguments.  A replayed call whose inputs no longer match
the recorded fingerprint fails the test: the recording is out of date.  A test that uses the reference in a way that cannot be
stored (its classes, objects that do not pickle) skips as before.

Recording (where the reference tree exists):  RLX_RECORD_REFERENCE=1 python -m pytest tests -m "not gpu"
"""

from __future__ import annotations

import builtins
import io
import lzma
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "reference_calls")
RECORD = os.environ.get("RLX_RECORD_REFERENCE", "0") not in ("", "0")

_recorded: dict = {}  # record mode: test module -> {nodeid: [call, ...]}
_stores: dict = {}    # replay mode: test module -> {nodeid: [call, ...]}


class NotStorable(Exception):
    pass


def _fingerprint(x):
    """Inputs, reduced to something small that still tells a changed input from the recorded one."""
    if torch.is_tensor(x):
        t = x.detach().cpu()
        d = t.double()
        finite = torch.isfinite(d)
        v = torch.where(finite, d, torch.zeros_like(d)).reshape(-1)
        w = torch.arange(1, v.numel() + 1, dtype=torch.float64).remainder(97) + 1
        return ("T", str(t.dtype), tuple(t.shape), float(v.sum()), float(v.abs().sum()), float((v * w).sum()),
                int((~finite).sum()))
    if isinstance(x, dict):
        return ("D", tuple((str(k), _fingerprint(v)) for k, v in sorted(x.items(), key=lambda kv: str(kv[0]))))
    if isinstance(x, (list, tuple)):
        return ("L", tuple(_fingerprint(v) for v in x))
    if isinstance(x, (bool, int, float, str, type(None))):
        return x
    if isinstance(x, torch.dtype):
        return str(x)
    if callable(x):
        return "callable"
    return type(x).__name__


def _close(a, b) -> bool:
    if isinstance(a, float) and isinstance(b, float):
        return a == b or abs(a - b) <= 1e-6 * max(abs(a), abs(b)) + 1e-9
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(_close(x, y) for x, y in zip(a, b))
    return a == b


def _tensors(x):
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    return []


def _plain(x) -> bool:
    """Data a stored call can hand back: tensors, numbers, strings and containers of them (functions too, as arguments).  Modules,
    optimizers and other objects are held by identity and changed in place where a replay cannot follow."""
    if torch.is_tensor(x) or isinstance(x, (bool, int, float, str, type(None), torch.dtype)):
        return True
    if isinstance(x, dict):
        return all(_plain(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_plain(v) for v in x)
    return callable(x) and not isinstance(x, torch.nn.Module)


def _flat_args(args, kwargs):
    return list(args) + [kwargs[k] for k in sorted(kwargs)]


def _snapshot(args):
    """Clones of every tensor / dict argument, to find what the call changed in place."""
    out = []
    for a in args:
        if torch.is_tensor(a):
            out.append(a.detach().clone())
        elif isinstance(a, dict):
            out.append(_fingerprint(a))
        else:
            out.append(None)
    return out


def _freeze(x) -> bytes:
    """The value as torch.save bytes, taken at once (the test may change the object afterwards)."""
    buf = io.BytesIO()
    try:
        torch.save(x, buf)
    except Exception as e:  # noqa: BLE001 -- e.g. an object of a reference class
        raise NotStorable(f"{type(e).__name__}: {e}") from e
    return buf.getvalue()


def _thaw(b: bytes):
    return torch.load(io.BytesIO(b), weights_only=False)


class _Call:
    """One callable of the reference (a module function, or a function a reference function returned)."""

    def __init__(self, session, name: str, real=None):
        self.session, self.name, self.real = session, name, real

    def __call__(self, *args, **kwargs):
        return self.session.call(self, args, kwargs)


class _Module:
    def __init__(self, session, name: str, real=None):
        self._session, self._name, self._real = session, name, real

    def __getattr__(self, attr):
        real = None if self._real is None else getattr(self._real, attr)
        if real is not None and (isinstance(real, type) or not callable(real)):
            self._session.storable = False  # a class / a constant of the reference: the test cannot run from a recording
            return real
        if real is None and self._session.mode == "replay" and attr[:1].isupper():
            pytest.skip(f"reference tree not present on this machine ({self._name}.{attr} is a class of the reference)")
        return _Call(self._session, f"{self._name}.{attr}", real)


class Session:
    """The reference as one test sees it: live, recording, or replaying that test's stored calls."""

    def __init__(self, nodeid: str, module: str, mode: str, real=None, calls=None):
        self.nodeid, self.module, self.mode, self.real = nodeid, module, mode, real
        self.calls = [] if calls is None else calls
        self.i = 0
        self.storable = True
        self.depth = 0  # > 0 inside a recorded call: what the reference calls from there is part of that call

    def __getattr__(self, name):
        real = None if self.real is None else getattr(self.real, name)
        return _Module(self, name, real)

    def call(self, fn: _Call, args, kwargs):
        flat = _flat_args(args, kwargs)
        if self.mode == "replay":
            if self.i >= len(self.calls):
                pytest.fail(f"{fn.name}: more reference calls than recorded for {self.nodeid} (re-record with RLX_RECORD_REFERENCE=1)")
            rec = self.calls[self.i]
            self.i += 1
            if rec["name"] != fn.name or not _close(rec["inputs"], _fingerprint(flat)):
                pytest.fail(f"{fn.name}: inputs differ from the recorded call {self.i} of {self.nodeid} (recorded: {rec['name']}); "
                            "re-record with RLX_RECORD_REFERENCE=1")
            for k, after in _thaw(rec["in_place"]).items():
                a = flat[k]
                if torch.is_tensor(a):
                    a.copy_(after)
                else:
                    a.clear()
                    a.update(after)
            if rec["out"][0] == "raise":
                raise _thaw(rec["out"][1])
            return self._wrap_out(rec["out"], fn.name)
        if self.depth:
            return fn.real(*args, **kwargs)
        if not _plain(flat) or any(a.requires_grad for a in _tensors(flat)):
            self.storable = False  # an object the call may change, or a test that differentiates through the reference
        before, inputs = _snapshot(flat), _fingerprint(flat)
        self.depth += 1
        try:
            out = fn.real(*args, **kwargs)
        except Exception as e:
            try:
                self.calls.append({"name": fn.name, "inputs": inputs, "in_place": _freeze({}), "out": ("raise", _freeze(e))})
            except NotStorable:
                self.storable = False
            raise
        finally:
            self.depth -= 1
        if not (_plain(out) or callable(out)) or any(t.requires_grad for t in _tensors([out])):
            self.storable = False
        in_place = {}
        for k, (a, b) in enumerate(zip(flat, before)):
            if torch.is_tensor(a) and not (a.shape == b.shape and torch.equal(a.detach(), b)):
                in_place[k] = a.detach().clone()
            elif isinstance(a, dict) and _fingerprint(a) != b:
                in_place[k] = dict(a)
        rec = {"name": fn.name, "inputs": inputs, "in_place": b"", "out": None}
        self.calls.append(rec)
        try:
            rec["in_place"] = _freeze(in_place)
            if callable(out) and not torch.is_tensor(out):
                rec["out"] = ("callable",)
                return _Call(self, f"{fn.name}()", out)
            rec["out"] = ("value", _freeze(out))
        except NotStorable:
            self.storable = False
        return out

    def _wrap_out(self, out, name):
        if out[0] == "callable":
            return _Call(self, f"{name}()")
        return _thaw(out[1])

    def finish(self):
        if self.mode == "record" and self.storable and self.calls:
            _recorded.setdefault(self.module, {})[self.nodeid] = self.calls


def _store(module: str) -> dict:
    if module not in _stores:
        path = os.path.join(GOLDEN, module + ".pt.xz")
        if os.path.exists(path):
            with open(path, "rb") as f:
                _stores[module] = _thaw(lzma.decompress(f.read()))
        else:
            _stores[module] = {}
    return _stores[module]


class Dispatch:
    """``ref`` while recording or replaying: attribute access goes to the running test's Session; outside a test (a fixture of
    wider scope) to the live reference, or the test skips where there is none."""

    def __init__(self, live):
        self.live, self.current = live, None

    def __getattr__(self, name):
        if self.current is not None:
            return getattr(self.current, name)
        if self.live is None:
            pytest.skip("reference tree not present on this machine")
        return getattr(self.live, name)


def session(request, live) -> Session | None:
    """Record (``live`` is the loaded reference) or replay this test's calls.  None: no reference and nothing recorded."""
    module = request.node.module.__name__.split(".")[-1]
    if live is not None:
        return Session(request.node.nodeid, module, "record", real=live)
    calls = _store(module).get(request.node.nodeid)
    if calls is None:
        return None
    return Session(request.node.nodeid, module, "replay", calls=calls)


def loader_hooks(sess: Session, reference_loader, monkeypatch):
    """Route oracle.reference_loader's function loaders through the session (record / replay).  While recording, any other way
    into the reference tree (its other loaders, reading its files) marks the test as one that cannot be stored."""
    real = {name: getattr(reference_loader, name) for name in ("load_function", "load_distributed_utils", "load_trajectory_builder")}
    routed = [0]

    def load_function(rel_path, name, **globs):
        if sess.mode == "replay":
            return _Call(sess, f"{rel_path}:{name}")
        routed[0] += 1
        try:
            return _Call(sess, f"{rel_path}:{name}", real["load_function"](rel_path, name, **globs))
        finally:
            routed[0] -= 1

    def module_loader(tag):
        def load():
            if sess.mode == "replay":
                return _Module(sess, tag)
            routed[0] += 1
            try:
                return _Module(sess, tag, real[tag]())
            finally:
                routed[0] -= 1
        return load

    monkeypatch.setattr(reference_loader, "load_function", load_function)
    for tag in ("load_distributed_utils", "load_trajectory_builder"):
        monkeypatch.setattr(reference_loader, tag, module_loader(tag))
    if sess.mode != "record":
        return

    def unstorable(fn):
        def wrapped(*args, **kwargs):
            if not routed[0]:
                sess.storable = False
            return fn(*args, **kwargs)
        return wrapped

    for name in ("load", "load_class", "load_weight_syncer", "load_models_registry", "_exec"):
        monkeypatch.setattr(reference_loader, name, unstorable(getattr(reference_loader, name)))
    root = os.path.realpath(reference_loader.REFERENCE_ROOT)
    real_open = builtins.open

    def open_(file, *args, **kwargs):
        if isinstance(file, (str, os.PathLike)) and os.path.realpath(file).startswith(root + os.sep) and not routed[0]:
            sess.storable = False
        return real_open(file, *args, **kwargs)

    monkeypatch.setattr(builtins, "open", open_)


def write_recordings():
    if not RECORD or not _recorded:
        return
    os.makedirs(GOLDEN, exist_ok=True)
    for module, tests in sorted(_recorded.items()):
        with open(os.path.join(GOLDEN, module + ".pt.xz"), "wb") as f:
            f.write(lzma.compress(_freeze(dict(sorted(tests.items())))))
