"""The one loader behind the six HIP libraries (gaussianavatars_amd/_lib.py: LibSpec, _load, LIBS): every library's description agrees with
its include/<tag>.h and with the file that is built, the three ways a load can fail are reported the same way for all of them, and the three
libraries only their own module maps stay unmapped on a bare import.  Loading works without a GPU: nothing here launches."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from gaussianavatars_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["gsr", "gab", "gls", "gmr", "gop", "grl"]


def _header(tag):
    txt = open(os.path.join(ROOT, "include", tag + ".h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    names = set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % tag, code))
    abi = int(re.search(r"#define\s+%s_ABI_VERSION\s+(\d+)" % tag.upper(), txt).group(1))
    return names, abi


def test_the_table_lists_the_six_libraries():
    assert list(_lib.LIBS) == TAGS
    for tag, spec in _lib.LIBS.items():
        assert spec.tag == tag and spec.path == getattr(_lib, tag.upper() + "_LIB_PATH")
        assert spec.symbols is getattr(_lib, tag.upper() + "_SYMBOLS") and spec.abi == getattr(_lib, tag.upper() + "_ABI_VERSION")


@pytest.mark.parametrize("tag", TAGS)
def test_description_header_and_library_agree(tag):
    spec = _lib.LIBS[tag]
    names, abi = _header(tag)
    assert names == set(spec.symbols), sorted(names ^ set(spec.symbols))
    assert abi == spec.abi
    lib = getattr(_lib, tag)()
    assert getattr(lib, tag + "_abi_version")() == abi == spec.abi
    assert _lib.handle(tag) is lib
    assert isinstance(_lib.last_error(tag), str)


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


def test_bare_import_maps_no_lazily_loaded_library():
    """mesh_raster.py, optim.py and loss.splat_regularizers are the only things that map libgmr, libgop and libgrl.  (A fresh interpreter:
    other tests of this session have loaded them.)"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "print('CACHE', _lib._gmr, _lib._gop, _lib._grl)\n"
            "print('MAPPED', [t for t in ('gmr', 'gop', 'grl') if ('lib%%s_hip.so' %% t) in open('/proc/self/maps').read()])\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CACHE None None None" in r.stdout and "MAPPED []" in r.stdout, r.stdout
