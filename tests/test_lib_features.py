"""The binding's feature table (`_lib.FEATURES`), one case per optional feature: the built library has it, a library just below it loads
without it and names the rebuild, a library that has it gets its symbols declared.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binding_stub import stub  # noqa: E402

from ml_fastvlm_amd import _lib  # noqa: E402

SINCE = dict(sampling=502, w8=504, beam=505, processors=506, lookup=507, gemm_plan=508, extend=509)     # include/fvhd.h's history, pinned
PROBED = ["score", "w4", "logprobs", "constraint", "lookup_sample", "guidance"]                         # added under 510
NAMES = list(_lib.FEATURES)


def _below(monkeypatch, name):
    """a library one step older than the feature: the version before it, or 510 without its probe symbol"""
    f = _lib.FEATURES[name]
    return stub(monkeypatch, f.since - 1, []) if f.probe is None else stub(monkeypatch, 510, [], without=(f.probe,))


def test_the_table_holds_the_pinned_versions_and_probes():
    assert NAMES == list(SINCE) + PROBED
    for name, f in _lib.FEATURES.items():
        assert (f.since, f.probe is None) == (SINCE.get(name), name in SINCE) and (f.probe is None or f.probe in f.sig), name
        assert f.needs is None or NAMES.index(f.needs) < NAMES.index(name), name
        assert callable(getattr(_lib, name + "_lib")), name
    assert [getattr(_lib, n.upper() + "_VERSION") for n in SINCE] == list(SINCE.values())
    assert (_lib.ABI_VERSION, _lib.WIDE_BATCH_VERSION) == (501, 503) and _lib.FEATURES["lookup_sample"].needs == "lookup"
    sigs = [n for f in _lib.FEATURES.values() for n in f.sig] + list(_lib.BASE_SIGNATURES)
    assert len(sigs) == len(set(sigs))                              # no symbol under two features


@pytest.mark.parametrize("name", NAMES)
def test_the_built_library_has_it(name):
    lib, f = _lib.load(), _lib.FEATURES[name]
    assert lib.fvhd_version() >= (f.since or 510) and (f.probe is None or lib.fvhd_version() == 510)
    assert _lib.has(name) and _lib.require(name) is lib and getattr(_lib, name + "_lib")() is lib
    for n in f.sig:
        assert getattr(lib, n).argtypes is not None, n


@pytest.mark.parametrize("name", NAMES)
def test_a_library_just_below_it_loads_and_names_the_rebuild(name, monkeypatch):
    f = _lib.FEATURES[name]
    lib = _below(monkeypatch, name)
    version = lib.fvhd_version()
    assert version == (f.since - 1 if f.probe is None else 510) and _lib.load() is lib
    assert not set(f.sig) & set(vars(lib))                          # declared only when the library has them
    for other, g in _lib.FEATURES.items():                          # everything older is still granted
        if other != name and g.needs != name and (g.since or 510) <= version:
            assert _lib.has(other) and _lib.require(other) is lib and set(g.sig) <= set(vars(lib)), other
    assert not _lib.has(name)
    what = f"needs {f.since}" if f.probe is None else f"built before {f.phrase}"
    for gate in (lambda: _lib.require(name), getattr(_lib, name + "_lib")):
        with pytest.raises(_lib.FvhdError, match="rebuild the library") as e:
            gate()
        assert what in str(e.value) and f"ABI version {version}" in str(e.value) and f.phrase in str(e.value) and f.names in str(e.value)


@pytest.mark.parametrize("name", NAMES)
def test_a_library_that_has_it_gets_it_declared(name, monkeypatch):
    f = _lib.FEATURES[name]
    lib = stub(monkeypatch, f.since or 510, [])
    assert _lib.has(name) and _lib.require(name) is lib and getattr(_lib, name + "_lib")() is lib
    for n, (res, args) in f.sig.items():
        assert n in vars(lib) and (getattr(lib, n).restype, getattr(lib, n).argtypes) == (res, args), n


@pytest.mark.parametrize("name", NAMES)
def test_the_gate_finds_load_through_the_module(name, monkeypatch):
    """what `monkeypatch.setattr(_lib, "load", ...)` puts there is what the gate asks: a library with a version number and nothing else"""
    f = _lib.FEATURES[name]

    class Old:
        def fvhd_version(self):
            return f.since - 1 if f.probe is None else 510

    monkeypatch.setattr(_lib, "load", lambda: Old())
    with pytest.raises(_lib.FvhdError, match=f"needs {f.since} - rebuild" if f.probe is None else f"built before {f.phrase}"):
        getattr(_lib, name + "_lib")()
    assert not _lib.has(name)


def test_lookup_sample_without_lookup_is_refused_with_lookups_message(monkeypatch):
    lib = stub(monkeypatch, _lib.LOOKUP_VERSION - 1, [])           # exports fvhd_llm_set_verify_sampling, as the stub exports everything
    assert not _lib.has("lookup_sample") and not set(_lib.FEATURES["lookup_sample"].sig) & set(vars(lib))
    with pytest.raises(_lib.FvhdError, match="prompt-lookup decoding \\(fvhd_llm_spec_reserve.* needs 507 - rebuild"):
        _lib.lookup_sample_lib()
