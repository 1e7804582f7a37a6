"""The one loader behind the eleven HIP libraries (gaussianavatars_amd/_lib.py: LibSpec, _load, _register, LIBS): every library's description
agrees with its include/<tag>.h and with the file that is built, the three ways a load can fail are reported the same way for all of them,
build() checks exactly this table, and a bare import maps none of them.  Loading works without a GPU: nothing here launches."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from gaussianavatars_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["gsr", "gab", "gls", "gmr", "gop", "grl", "gdc", "gev", "gfs", "gms", "glp"]
EXTRA_HEADERS = {"gmr": ["gmr_overlay"]}   # gmr.h includes it; _lib mirrors it in GMR_OVERLAY_SYMBOLS
UNORDERED = {"gsr"}   # GSR_SYMBOLS lists gsr_mark_visible after the bound entries, gsr.h before them; every other description is in header order


def _header(tag):
    txt = "".join(open(os.path.join(ROOT, "include", h + ".h")).read() for h in [tag] + EXTRA_HEADERS.get(tag, []))
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    names = re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % tag, code)
    abi = int(re.search(r"#define\s+%s_ABI_VERSION\s+(\d+)" % tag.upper(), txt).group(1))
    return names, abi


def test_the_table_lists_the_eleven_libraries():
    assert list(_lib.LIBS) == TAGS
    for tag, spec in _lib.LIBS.items():
        assert spec.tag == tag and spec.path == _lib._lib_path(tag, {"gsr": "GSR_LIB", "gab": "GAB_LIB"}.get(tag))
        assert spec.abi == getattr(_lib, tag.upper() + "_ABI_VERSION")
        if tag == "gmr":
            assert list(spec.symbols) == list(_lib.GMR_SYMBOLS) + list(_lib.GMR_OVERLAY_SYMBOLS)
            assert all(spec.symbols[n] is d[n] for d in (_lib.GMR_SYMBOLS, _lib.GMR_OVERLAY_SYMBOLS) for n in d)
        else:
            assert spec.symbols is getattr(_lib, tag.upper() + "_SYMBOLS")
    assert (_lib.GSR_LIB_PATH, _lib.GAB_LIB_PATH, _lib.GLS_LIB_PATH) == tuple(_lib.LIBS[t].path for t in ("gsr", "gab", "gls"))


def test_the_per_library_shims_follow_from_the_table():
    for tag, spec in _lib.LIBS.items():
        assert getattr(_lib, tag + "_error").func is _lib.last_error and getattr(_lib, tag + "_error").args == (tag,)
        if tag + "_profile_collect" in spec.symbols:   # csrc/launch_prof.h's exports
            assert set(_lib._profile_symbols(tag)) <= set(spec.symbols)
            enable, read = getattr(_lib, tag + "_profile_enable"), getattr(_lib, tag + "_profile_read")
            assert enable.func is _lib.profile_enable and read.func is _lib.profile_read and enable.args == read.args == ((tag,),)
    assert [t for t in TAGS if t + "_profile_collect" not in _lib.LIBS[t].symbols] == ["gsr", "gmr"]
    assert _lib.gsr_profile_enable.__module__ == _lib.gsr_profile_read.__module__ == _lib.__name__   # libgsr's slot-based functions, not partials
    assert _lib.launch_profile_enable.args == _lib.launch_profile_read.args == (("gab", "gls"),)


@pytest.mark.parametrize("tag", TAGS)
def test_description_header_and_library_agree(tag):
    spec = _lib.LIBS[tag]
    names, abi = _header(tag)
    assert len(names) == len(set(names)) and set(names) == set(spec.symbols), sorted(set(names) ^ set(spec.symbols))
    if tag not in UNORDERED:
        assert list(spec.symbols) == names
    assert abi == spec.abi
    lib = getattr(_lib, tag)()
    assert getattr(lib, tag + "_abi_version")() == abi == spec.abi
    assert _lib.handle(tag) is lib and getattr(_lib, tag)() is lib
    assert isinstance(_lib.last_error(tag), str)
    assert "raises (never falls back)" in getattr(_lib, tag).__doc__


@pytest.mark.parametrize("tag", TAGS)
def test_load_failures_read_the_same_for_every_library(tag):
    spec = _lib.LIBS[tag]
    real = getattr(_lib, tag)()

    missing = os.path.join(ROOT, "no_such_dir", "lib%s_hip.so" % tag)
    with pytest.raises(RuntimeError) as e:
        _lib._load(spec._replace(path=missing))
    assert missing in str(e.value) and "build()" in str(e.value)

    with pytest.raises(RuntimeError) as e:   # a stale file after an ABI bump
        _lib._load(spec._replace(abi=spec.abi + 1))
    assert str(e.value) == "%s ABI version %d != %d" % (tag, spec.abi, spec.abi + 1)

    with pytest.raises(AttributeError):      # a symbol the header gained and the file does not have
        _lib._load(spec._replace(symbols={**spec.symbols, tag + "_no_such_entry": (C.c_int, [])}))

    # the throw-away descriptions left the real handle, its prototypes and the table alone
    assert getattr(_lib, tag)() is real and _lib.gmr() is _lib.gmr()
    assert _lib.LIBS[tag] is spec and tag + "_no_such_entry" not in spec.symbols
    for name, (res, args) in spec.symbols.items():
        fn = getattr(real, name)
        assert fn.restype is res and list(fn.argtypes or []) == list(args), name


def test_build_checks_exactly_this_table():
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "for tag in _lib.LIBS:" in entry and set(re.findall(r"_lib\.(\w*LIBS)\b", entry)) == {"LIBS"}
    assert [n for n in dir(_lib) if n.endswith("LIBS")] == ["LIBS"]


def test_bare_import_maps_no_lazily_loaded_library():
    """Each library is mapped by the first call of its loader and by nothing before it: after a bare import none of the eleven is in the
    process, and handle(tag) brings in that one file.  (A fresh interpreter: other tests of this session have loaded them.)"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "mapped = lambda: [t for t in _lib.LIBS if ('lib%%s_hip.so' %% t) in open('/proc/self/maps').read()]\n"
            "print('MAPPED', mapped())\n"
            "for t in ('grl', 'gop', 'gmr'):\n"
            "    _lib.handle(t)\n"
            "    print('AFTER', t, mapped())\n"
            "for t in _lib.LIBS:\n"
            "    _lib.handle(t)\n"
            "print('ALL', mapped())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MAPPED []" in r.stdout and "ALL %r" % TAGS in r.stdout, r.stdout
    assert "AFTER grl ['grl']" in r.stdout and "AFTER gop ['gop', 'grl']" in r.stdout and "AFTER gmr ['gmr', 'gop', 'grl']" in r.stdout, r.stdout
