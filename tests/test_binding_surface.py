"""CPU, no library needed: the ctypes binding is a package of modules behind one façade, and from outside it is still the flat
module it was split from.

tests/binding_surface.json and tests/binding_record.json were written by tools/binding_snapshot.py in a checkout of the last
commit that had the binding in one file (libsrcnn_amd/__init__.py, 1811 lines).  They are the yardstick: the public names with
their signatures, struct layouts and values, and -- with a recorder in place of the loaded library -- the exact arguments
every thin wrapper hands to C for a full and a minimal argument set.  Regenerating them from a later tree proves nothing."""
import importlib.util
import json
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")


def _load(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


SURFACE = _load("binding_surface.json")
RECORD = _load("binding_record.json")


@pytest.fixture(scope="module")
def snap():
    spec = importlib.util.spec_from_file_location("binding_snapshot", os.path.join(ROOT, "tools", "binding_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def S():
    import libsrcnn_amd
    return libsrcnn_amd


def _without_doc(entry):
    if isinstance(entry, dict):
        return {k: _without_doc(v) for k, v in entry.items() if k != "doc"}
    return entry


def _documented(entry, path):
    """The paths of everything the snapshot saw a docstring on."""
    if isinstance(entry, dict):
        if entry.get("doc") is True:
            yield path
        for k, v in entry.items():
            yield from _documented(v, path + (k,))


def test_public_names_are_the_parents(S, snap):
    """No public name lost, none gained -- but for the modules the binding now consists of."""
    assert snap.public_names(S) == sorted(SURFACE)
    extra = [n for n, v in vars(S).items() if not n.startswith("_") and n not in SURFACE and n not in snap.SKIP]
    strangers = [n for n in extra if not (isinstance(getattr(S, n), types.ModuleType) and getattr(S, n).__name__ == "libsrcnn_amd." + n)]
    assert not strangers, strangers


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_public_name_matches_the_snapshot(S, snap, name):
    """Kind, signature (methods of a class included), Structure fields and size, value of a constant or list."""
    got = json.loads(json.dumps(snap.surface(S)[name]))
    assert _without_doc(got) == _without_doc(SURFACE[name])
    lost = [path for path in _documented(SURFACE[name], (name,)) if path not in set(_documented(got, (name,)))]
    assert not lost, "docstring lost: %r" % (lost,)


def test_every_documented_function_still_has_its_docstring(S):
    for name, entry in SURFACE.items():
        if entry["kind"] == "function" and entry["doc"]:
            assert (getattr(S, name).__doc__ or "").strip(), name


def test_abi_table_is_the_symbol_lists(S):
    """One table: every exported C function once, and every *_SYMBOLS list read off it in the parent's order."""
    symbols = [symbol for _group, symbol, _res, _args in S.abi.ABI_TABLE]
    assert len(symbols) == len(set(symbols)) == 127
    assert set(symbols) == set(S.C_ABI_SYMBOLS)
    lists = [n for n in SURFACE if n.endswith("_SYMBOLS")]
    assert len(lists) == 18                                   # sixteen headers, C_ABI_SYMBOLS, CXX_SYMBOLS
    for n in lists:
        assert getattr(S, n) == SURFACE[n]["value"], n
    per_header = [n for n in lists if n not in ("C_ABI_SYMBOLS", "CXX_SYMBOLS")]
    assert sorted(S.C_ABI_SYMBOLS) == sorted(s for n in per_header for s in getattr(S, n))
    for _group, _symbol, _res, args in S.abi.ABI_TABLE:
        assert isinstance(args, list)


def test_table_declares_every_symbol(S):
    """declare() leaves no function of the table with ctypes' default int arguments; an older build loaded for an A/B run may
    lack entry points of the extensions, never of the stable ABI."""
    class Fn:
        restype, argtypes = "unset", "unset"

    class Lib:
        def __init__(self, missing=()):
            self.fns, self.missing = {}, set(missing)

        def __getattr__(self, name):
            if name.startswith("__") or name in self.missing:
                raise AttributeError(name)
            return self.fns.setdefault(name, Fn())

    full = Lib()
    S.abi.declare(full, older_build=False)
    assert set(full.fns) == set(S.C_ABI_SYMBOLS) | set(S.CXX_SYMBOLS)
    assert all(fn.argtypes != "unset" and fn.restype != "unset" for fn in full.fns.values())
    older = Lib(missing=S.RGB_DELTA_SYMBOLS)
    S.abi.declare(older, older_build=True)
    assert set(older.fns) == (set(S.C_ABI_SYMBOLS) | set(S.CXX_SYMBOLS)) - set(S.RGB_DELTA_SYMBOLS)
    with pytest.raises(AttributeError):
        S.abi.declare(Lib(missing=S.RGB_DELTA_SYMBOLS), older_build=False)
    with pytest.raises(AttributeError):
        S.abi.declare(Lib(missing=["srcnn_trim"]), older_build=True)


@pytest.fixture(scope="module")
def record(S, snap):
    return json.loads(json.dumps(snap.record(S)))


def test_record_drives_the_same_cases(record):
    assert sorted(record) == sorted(RECORD)


@pytest.mark.parametrize("case", sorted(RECORD))
def test_wrapper_hands_c_what_the_parent_handed_it(record, case):
    """Symbol by symbol and argument by argument: float32-rounded factors, NULL-padded plane arrays, NULL for None, the n /
    item_size / struct_size overrides unaltered, the bytes of the item arrays, and what the wrapper returned or raised."""
    assert record[case] == RECORD[case]
