"""ctypes loader for the HIP shared libraries (C ABI of include/*.h).

There is deliberately NO fallback: if the library is missing or does not export a symbol the
import-time error says so.  The CPU oracle under oracle/ is test infrastructure and is never
reachable from here.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partial
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))


# ---- host-side fast paths (the frame loop is ~0.7 ms of Python; these run a dozen times per frame) -----------------
def raw_stream(dev):
    """torch's current stream on `dev` as a c_void_p, without building a torch.cuda.Stream object."""
    import torch

    try:
        return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    except AttributeError:   # very old / very new torch: the public route
        return torch.cuda.current_stream(dev).cuda_stream


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOCTX = _NoCtx()


def on_device(dev):
    """Context that makes `dev` the current device for the native call; free when it already is (the usual case)."""
    import torch

    global _ONE_DEVICE
    if _ONE_DEVICE is None:
        _ONE_DEVICE = torch.cuda.device_count() == 1
    if _ONE_DEVICE or dev.index is None or torch.cuda.current_device() == dev.index:
        return _NOCTX
    return torch.cuda.device(dev)


_ONE_DEVICE = None   # a process that sees one GPU never switches devices


# ---- the loader: one description per library, one _load() for all of them -------------------------------------------
class LibSpec(NamedTuple):
    """What _load() needs to map lib<tag>_hip.so and hold it to include/<tag>.h."""
    tag: str        # prefix of every export: <tag>_abi_version, <tag>_last_error, ...
    path: str
    symbols: dict   # every symbol include/<tag>.h declares -> (restype, argtypes)
    abi: int        # <TAG>_ABI_VERSION of the header this file mirrors


#: tag -> LibSpec of every HIP library the package ships; the module-level function of the same name (gsr(), gab(), ...) loads it
LIBS = {}


def _lib_path(tag, env=None):
    """The in-tree build of a library, or the file the environment variable `env` names (a variant built side by side, such as
    `make timeline`'s libgsr_timeline.so).  An override that does not exist is an error, never a fallback."""
    return (env and os.environ.get(env)) or os.path.join(_HERE, f"lib{tag}_hip.so")


def _torch_first():
    """The libraries take raw device pointers of torch tensors and launch on torch's streams, so they have to share torch's HIP
    runtime: torch is imported before the first library is mapped.  (Mapped first -- e.g. build() followed by smoke() in one
    process -- they pull in /opt/rocm's libamdhip64 ahead of the copy torch ships, and the first runtime call that needs the
    device fails with 'no ROCm-capable device is detected'.)"""
    import torch  # noqa: F401


def _load(spec):
    """Map one library and check it against its description; raises (never falls back) when it is not built, lacks a symbol or is stale.
    The caller keeps the handle: the loaders _register() returns each cache theirs."""
    if not os.path.exists(spec.path):
        raise RuntimeError(
            f"{spec.path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    _torch_first()
    lib = C.CDLL(spec.path)
    for name, (res, args) in spec.symbols.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    have = getattr(lib, spec.tag + "_abi_version")()
    if have != spec.abi:
        raise RuntimeError(f"{spec.tag} ABI version {have} != {spec.abi}")
    return lib


def _register(tag, symbols, abi, env=None):
    """Enter lib<tag>_hip.so into LIBS and return its loader <tag>(): the first call maps and checks the file, later calls return the same
    handle.  The handle is a cell of the closure, so the warm path is a cell load and a test."""
    LIBS[tag] = LibSpec(tag, _lib_path(tag, env), symbols, abi)
    lib = None

    def loader():
        nonlocal lib
        if lib is None:
            lib = _load(LIBS[tag])
        return lib

    loader.__name__ = loader.__qualname__ = tag
    loader.__doc__ = f"lib{tag}_hip.so, mapped and checked at the first call; raises (never falls back) when it is not built."
    return loader


def _profile_symbols(tag):
    """The four exports csrc/launch_prof.h's LPROF_EXPORTS(tag) emits, in the order the headers declare them."""
    return {
        tag + "_profile_enable": (C.c_int, [C.c_int]),
        tag + "_profile_collect": (C.c_int, []),
        tag + "_profile_entry": (C.c_int, [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
        tag + "_profile_reset": (C.c_int, []),
    }


def handle(tag):
    """The loaded library of a tag, through its module-level loader (and that loader's cache)."""
    return globals()[tag]()


def last_error(tag) -> str:
    return getattr(handle(tag), tag + "_last_error")().decode("utf-8", "replace")


def profile_enable(tags, on: bool) -> None:
    """Event pairs around every launch of the libraries `tags` (csrc/launch_prof.h: <tag>_profile_*), each from an empty table;
    libgsr's slot-based twin is gsr_profile_enable."""
    for tag in tags:
        lib = handle(tag)
        getattr(lib, tag + "_profile_enable")(1 if on else 0)
        if on:
            getattr(lib, tag + "_profile_reset")()


def profile_read(tags) -> dict:
    """{kernel name: (total_ms, launches)} of the launches of the libraries `tags` since profile_enable(tags, True)."""
    out = {}
    for tag in tags:
        lib = handle(tag)
        for i in range(getattr(lib, tag + "_profile_collect")()):
            name, ms, k = C.c_char_p(), C.c_double(), C.c_int64()
            if getattr(lib, tag + "_profile_entry")(i, C.byref(name), C.byref(ms), C.byref(k)) == 0:
                out[name.value.decode()] = (ms.value, k.value)
    return out


# ------------------------------------------------------------------------------------------------
# libgsr_hip.so : the splat rasterizer (include/gsr.h)
# ------------------------------------------------------------------------------------------------
GSR_OK = 0
GSR_ABI_VERSION = 12
GSR_E_CAPACITY = 1
GSR_COUNT_SLOTS = 128   # include/gsr.h: persistent instance-count slots of the deferred forwards


class GsrSettings(C.Structure):
    """include/gsr.h: GsrSettings"""
    _fields_ = [
        ("image_height", C.c_int32),
        ("image_width", C.c_int32),
        ("tanfovx", C.c_float),
        ("tanfovy", C.c_float),
        ("bg", C.c_void_p),
        ("scale_modifier", C.c_float),
        ("viewmatrix", C.c_void_p),
        ("projmatrix", C.c_void_p),
        ("sh_degree", C.c_int32),
        ("campos", C.c_void_p),
        ("prefiltered", C.c_int32),
        ("debug", C.c_int32),
        ("tile_culling", C.c_int32),
        ("forward_only", C.c_int32),
        ("deterministic", C.c_int32),
        ("exact_scale_grad", C.c_int32),
        ("deferred_count", C.c_int32),
        ("fast_blend", C.c_int32),
    ]


class GsrGeomLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in
                ("depths", "grec", "cov3D", "rect", "tiles_touched", "clamped", "visible", "brec", "acc64", "acc", "shjac", "total")]


class GsrBinningLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in
                ("keys", "point_list", "qlist", "qpos", "qcount", "qstart", "ranges", "tile_count", "tile_start", "tile_cursor", "tile_order",
                 "block_hist", "dkeys", "dtmp", "order", "bcount", "bstart", "bcursor", "border", "bhist", "qhist", "qprefix", "qmask", "ranks", "rank", "rank_over", "srect", "sspan", "pstat", "tdesc", "obs", "bandcnt", "path", "chunks", "nb", "nbands", "band_rows",
                 "total")]


class GsrBound(C.Structure):
    """include/gsr.h: GsrBound -- the per-face frames of a mesh-bound model for the rasterizer's bound entry"""
    _fields_ = [("binding", C.c_void_p), ("binding_is_i64", C.c_int32), ("F", C.c_int32), ("face_R", C.c_void_p), ("face_scale", C.c_void_p),
                ("face_center", C.c_void_p), ("face_quat", C.c_void_p), ("slot", C.c_void_p), ("rows", C.c_void_p)]


class GsrImageLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("final_T", "n_contrib", "n_contrib_q", "c_final", "ck", "gmax", "units", "total")]


#: every symbol include/gsr.h declares -> (restype, argtypes)
GSR_SYMBOLS = {
    "gsr_abi_version": (C.c_int, []),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_count_slot_read": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gsr_count_slot_overflow": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "gsr_last_forward_seq": (C.c_int64, []),
    "gsr_count_slot_wait": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "gsr_geom_layout": (C.c_int, [C.c_int32, C.POINTER(GsrGeomLayout)]),
    "gsr_binning_layout": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(GsrBinningLayout)]),
    "gsr_image_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(GsrImageLayout)]),
    "gsr_forward": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32] + [C.c_void_p] * 7 +
                    [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                     C.POINTER(C.c_int64), C.c_void_p]),
    "gsr_backward": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32] + [C.c_void_p] * 6 +
                     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] +
                     [C.c_void_p] * 8 + [C.c_void_p]),
    "gsr_forward_ex": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32] + [C.c_void_p] * 8 +
                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                        C.POINTER(C.c_int64), C.c_void_p]),
    "gsr_backward_ex": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32] + [C.c_void_p] * 7 +
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] +
                        [C.c_void_p] * 9 + [C.c_void_p]),
    "gsr_forward_bound": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32, C.POINTER(GsrBound)] + [C.c_void_p] * 6 +
                          [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "gsr_backward_bound": (C.c_int, [C.POINTER(GsrSettings), C.c_int32, C.c_int32, C.POINTER(GsrBound)] + [C.c_void_p] * 6 +
                           [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] +
                           [C.c_void_p] * 8 + [C.c_void_p]),
    "gsr_mark_visible": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_profile_enable": (C.c_int, [C.c_int]),
    "gsr_profile_read": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "gsr_kernel_name": (C.c_char_p, [C.c_int]),
    "gsr_wait_stats": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}
GSR_NUM_KERNELS = 12


def gsr_profile_enable(on: bool) -> None:
    gsr().gsr_profile_enable(1 if on else 0)


def gsr_profile_read() -> dict:
    """{kernel name: (total_ms, launches)} accumulated since the last read."""
    ms = (C.c_double * GSR_NUM_KERNELS)()
    n = (C.c_int64 * GSR_NUM_KERNELS)()
    rc = gsr().gsr_profile_read(ms, n)
    if rc != GSR_OK:
        raise RuntimeError(f"gsr_profile_read failed: {gsr().gsr_last_error().decode()}")
    return {gsr().gsr_kernel_name(i).decode(): (ms[i], n[i]) for i in range(GSR_NUM_KERNELS)}

def gsr_wait_stats():
    """(total host wait in ms, number of waits) since the last call -- see include/gsr.h."""
    ms, n = C.c_double(), C.c_int64()
    gsr().gsr_wait_stats(C.byref(ms), C.byref(n))
    return ms.value, n.value


gsr = _register("gsr", GSR_SYMBOLS, GSR_ABI_VERSION, "GSR_LIB")
GSR_LIB_PATH = LIBS["gsr"].path   # bench.py and _host.py read it


# ------------------------------------------------------------------------------------------------
# libgab_hip.so : FLAME / face-frame / splat binding kernels (include/gab.h)
# ------------------------------------------------------------------------------------------------
GAB_FLAME_WS_FLOATS = 512
GAB_BIND_ROW_FLOATS = 20   # include/gab.h: floats per splat of the two-pass CSR backward's scratch
_P = C.c_void_p


class GabRig(C.Structure):
    """include/gab.h: GabRig"""
    _fields_ = [("V", C.c_int32), ("n_shape", C.c_int32), ("n_expr", C.c_int32), ("v_template", _P), ("shapedirs", _P),
                ("posedirs", _P), ("J_regressor", _P), ("lbs_weights", _P), ("parents", C.c_int32 * 5)]


GAB_SYMBOLS = {
    "gab_abi_version": (C.c_int, []),
    "gab_last_error": (C.c_char_p, []),
    "gab_flame_forward": (C.c_int, [C.POINTER(GabRig)] + [_P] * 8 + [_P, _P, _P, _P]),
    "gab_flame_backward": (C.c_int, [C.POINTER(GabRig)] + [_P] * 8 + [_P, _P, _P, _P] + [_P] * 8 + [_P] +
                           [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _P]),
    "gab_flame_prepared_floats": (C.c_int64, [C.POINTER(GabRig)]),
    "gab_flame_prepare": (C.c_int, [C.POINTER(GabRig), _P, _P, _P, _P]),
    "gab_flame_forward_prepared": (C.c_int, [C.POINTER(GabRig), _P] + [_P] * 6 + [_P, _P, _P, _P]),
    "gab_blend_sequence": (C.c_int, [C.POINTER(GabRig), _P, _P, C.c_int32, _P, _P]),
    "gab_flame_forward_sequence": (C.c_int, [C.POINTER(GabRig), _P, _P] + [_P] * 6 + [_P, _P, _P, _P]),
    "gab_flame_backward_prepared": (C.c_int, [C.POINTER(GabRig), _P] + [_P] * 4 + [_P, _P, _P] + [_P] * 6 + [_P] +
                                    [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _P]),
    "gab_mesh_backward_prepared": (C.c_int, [C.POINTER(GabRig), _P] + [_P] * 4 + [_P, _P, _P, _P, _P] + [_P] * 5 + [_P] * 6 + [_P] +
                                   [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _P]),
    "gab_face_frames_forward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "gab_face_frames_backward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "gab_bind_forward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gab_bind_backward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gab_bind_backward_csr": (C.c_int, [C.c_int32, C.c_int32] + [_P] * 22),
    "gab_bind_backward_faces": (C.c_int, [C.c_int32, _P, _P, _P, _P]),
    "gab_zero_buffers": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _P]),
    "gab_feed_row": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    **_profile_symbols("gab"),
}
GAB_ABI_VERSION = 5

gab = _register("gab", GAB_SYMBOLS, GAB_ABI_VERSION, "GAB_LIB")
GAB_LIB_PATH = LIBS["gab"].path   # bench.py and _host.py read it

#: every symbol include/gab_landmarks.h declares -> (restype, argtypes): additive exports of the same library (gab.h's list is frozen at ABI 5)
GAB_LANDMARK_SYMBOLS = {
    "gab_landmarks_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "gab_landmarks_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "gab_root_joint": (C.c_int, [C.POINTER(GabRig), _P, _P, _P]),
    "gab_root_center": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P]),
    "gab_root_center_backward": (C.c_int, [C.POINTER(GabRig), _P, _P, _P, _P]),
}
_gab_landmarks = None


def gab_landmarks():
    """libgab_hip.so -- gab()'s handle -- with the entries of include/gab_landmarks.h resolved and typed at the first call; raises (never falls
    back) when the file that is built does not export them."""
    global _gab_landmarks
    if _gab_landmarks is None:
        lib = gab()
        for name, (res, args) in GAB_LANDMARK_SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError: a library built before these entries
            fn.restype = res
            fn.argtypes = args
        _gab_landmarks = lib
    return _gab_landmarks


# ------------------------------------------------------------------------------------------------
# libgls_hip.so : fused L1 + SSIM loss and densification statistics (include/gls.h)
# ------------------------------------------------------------------------------------------------
GLS_SYMBOLS = {
    "gls_abi_version": (C.c_int, []),
    "gls_last_error": (C.c_char_p, []),
    "gls_partial_floats": (C.c_int64, [C.c_int32] * 4),
    "gls_l1_ssim_forward": (C.c_int, [C.c_int32] * 4 + [_P, _P, C.c_float] + [_P] * 4),
    "gls_l1_ssim_backward": (C.c_int, [C.c_int32] * 4 + [_P] * 4 + [C.c_float, _P, _P]),
    "gls_l1_ssim_backward_split": (C.c_int, [C.c_int32] * 4 + [_P] * 5 + [C.c_int32, C.c_float, _P, _P]),
    "gls_l1_forward": (C.c_int, [C.c_int64, _P, _P, C.c_float, _P, _P, _P]),
    "gls_l1_forward_grad": (C.c_int, [C.c_int64, _P, _P, C.c_float, _P, _P, _P, _P]),
    "gls_l1_backward": (C.c_int, [C.c_int64, _P, _P, _P, C.c_float, _P, _P]),
    "gls_densification_stats": (C.c_int, [C.c_int32] + [_P] * 6),
    "gls_add_densification_stats": (C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, _P, _P]),
    **_profile_symbols("gls"),
}
GLS_ABI_VERSION = 4

gls = _register("gls", GLS_SYMBOLS, GLS_ABI_VERSION)
GLS_LIB_PATH = LIBS["gls"].path   # bench.py and _host.py read it


# ------------------------------------------------------------------------------------------------
# libgmr_hip.so : the mesh overlay's triangle rasterizer and antialias (include/gmr.h).  Loaded only by mesh_raster.py and
# mesh_renderer.py: the splat path never maps it.
# ------------------------------------------------------------------------------------------------
GMR_SYMBOLS = {
    "gmr_abi_version": (C.c_int, []),
    "gmr_last_error": (C.c_char_p, []),
    "gmr_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "gmr_rasterize": (C.c_int, [C.c_int32] * 5 + [_P, _P, _P, _P, _P]),
    "gmr_antialias": (C.c_int, [C.c_int32] * 6 + [_P] * 7),
}
GMR_ABI_VERSION = 2
GMR_MAX_TRIANGLES = (1 << 24) - 1   # include/gmr.h: triangle_id + 1 is stored as an exact float

# ABI 2, include/gmr_overlay.h (which gmr.h includes): the shaded overlay of mesh_renderer.py.  One dict per header; the library is
# registered with their union, so a file built before these entries raises at load time
GMR_LIGHT_CONSTANT, GMR_LIGHT_FRONT = 0, 1   # include/gmr_overlay.h
GMR_MAT_ROWS, GMR_MAT_CAMERA = 0, 1
GMR_MAX_MAPS = 4


class GmrMap(C.Structure):
    """include/gmr_overlay.h: GmrMap"""
    _fields_ = [("src", _P), ("dst", _P), ("C", C.c_int32)]


GMR_OVERLAY_SYMBOLS = {
    "gmr_mesh_prepare": (C.c_int, [C.c_int32] * 3 + [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "gmr_mesh_shade": (C.c_int, [C.c_int32] * 4 + [_P, _P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P]),
    "gmr_resize_flip": (C.c_int, [C.c_int32] * 6 + [C.POINTER(GmrMap), _P]),
    "gmr_compose_overlay": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_float, C.c_float, _P, _P, _P]),
}

gmr = _register("gmr", {**GMR_SYMBOLS, **GMR_OVERLAY_SYMBOLS}, GMR_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgop_hip.so : the fused Adam step (include/gop.h).  Loaded only by optim.py, at the first step on device tensors.
# ------------------------------------------------------------------------------------------------
GOP_ABI_VERSION = 1
GOP_MAX_TENSORS = 32   # include/gop.h: tensors per launch
GOP_SLAB = 2048        # include/gop.h: elements per workgroup


class GopAdamTensor(C.Structure):
    """include/gop.h: GopAdamTensor"""
    _fields_ = [("param", _P), ("grad", _P), ("exp_avg", _P), ("exp_avg_sq", _P), ("n", C.c_int64), ("step_size", C.c_float),
                ("bias_correction2_sqrt", C.c_float)]


GOP_SYMBOLS = {
    "gop_abi_version": (C.c_int, []),
    "gop_last_error": (C.c_char_p, []),
    "gop_adam_step": (C.c_int, [C.c_int32, C.POINTER(GopAdamTensor), C.c_float, C.c_float, C.c_float, _P]),
    "gop_adam_step_ex": (C.c_int, [C.c_int32, C.POINTER(GopAdamTensor)] + [C.c_float] * 5 + [_P]),
    **_profile_symbols("gop"),
}

gop = _register("gop", GOP_SYMBOLS, GOP_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgrl_hip.so : the fused splat regularisers (include/grl.h).  Loaded only by loss.splat_regularizers, at the first call on device tensors.
# ------------------------------------------------------------------------------------------------
GRL_ABI_VERSION = 1
GRL_SLAB = 1024               # include/grl.h: splats per workgroup
GRL_MAX_SPLATS = 1 << 24      # include/grl.h: P must stay below this (the count is an exact float)

GRL_SYMBOLS = {
    "grl_abi_version": (C.c_int, []),
    "grl_last_error": (C.c_char_p, []),
    "grl_scratch_bytes": (C.c_int64, [C.c_int32]),
    "grl_forward": (C.c_int, [C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P]),
    "grl_backward": (C.c_int, [C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P]),
    **_profile_symbols("grl"),
}

grl = _register("grl", GRL_SYMBOLS, GRL_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgdc_hip.so : adaptive density control (include/gdc.h).  Loaded only by densify.py and knn.py, at the first call on device tensors.
# ------------------------------------------------------------------------------------------------
GDC_ABI_VERSION = 2
GDC_CHUNK = 256                # include/gdc.h: splats per workgroup of the scan
GDC_MAX_TENSORS = 24           # include/gdc.h: tensors one gather launch moves
GDC_MAX_SPLATS = 1 << 30       # include/gdc.h: P must stay below this
GDC_KNN_CHUNK = 32             # include/gdc.h: sorted points per box of the nearest-neighbour search
GDC_COPY, GDC_MOMENT, GDC_ZERO, GDC_XYZ, GDC_SCALING = range(5)   # include/gdc.h: GdcTensor.kind


class GdcParams(C.Structure):
    """include/gdc.h: GdcParams"""
    _fields_ = [("max_grad", C.c_float), ("min_opacity", C.c_float), ("extent", C.c_float), ("percent_dense", C.c_float),
                ("max_screen_size", C.c_float)]


class GdcTensor(C.Structure):
    """include/gdc.h: GdcTensor"""
    _fields_ = [("src", _P), ("dst", _P), ("row_floats", C.c_int32), ("kind", C.c_int32)]


GDC_SYMBOLS = {
    "gdc_abi_version": (C.c_int, []),
    "gdc_last_error": (C.c_char_p, []),
    "gdc_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "gdc_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(GdcParams), _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "gdc_emit": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(GdcTensor), _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P,
                           _P, _P]),
    "gdc_order_workspace_bytes": (C.c_int64, [C.c_int32]),
    "gdc_morton_order": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "gdc_permute": (C.c_int, [C.c_int32, _P, C.c_int32, C.POINTER(GdcTensor), _P]),
    "gdc_knn_workspace_bytes": (C.c_int64, [C.c_int32]),
    "gdc_knn3_dist2": (C.c_int, [C.c_int32, _P, _P, _P, _P]),
    **_profile_symbols("gdc"),
}

gdc = _register("gdc", GDC_SYMBOLS, GDC_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgev_hip.so : evaluation and export (include/gev.h).  Loaded only by evaluate.py, at the first call on device tensors.
# ------------------------------------------------------------------------------------------------
GEV_ABI_VERSION = 1
GEV_F32_PLANAR, GEV_U8_INTERLEAVED = 0, 1          # include/gev.h: layout of one image of a pair
GEV_RAW, GEV_CLAMP, GEV_PNG8 = 0, 1, 2             # include/gev.h: load transform of a planar fp32 image
GEV_PSNR_PER_CHANNEL, GEV_PSNR_PER_IMAGE = 0, 1    # include/gev.h: how an image's PSNR is formed from its planes

_GEV_PAIR = [C.c_int32] * 4 + [_P, C.c_int32, _P, C.c_int32, C.c_int32]   # B, C, H, W, a, a_layout, b, b_layout, transform
GEV_SYMBOLS = {
    "gev_abi_version": (C.c_int, []),
    "gev_last_error": (C.c_char_p, []),
    "gev_partial_floats": (C.c_int64, [C.c_int32] * 4),
    "gev_pair_stats": (C.c_int, _GEV_PAIR + [_P, _P, _P]),
    "gev_accumulate": (C.c_int, _GEV_PAIR + [C.c_int32, _P, _P, _P, C.c_int32, _P, _P]),
    "gev_to_u8": (C.c_int, [C.c_int32] * 4 + [_P, _P, _P, _P, _P]),
    **_profile_symbols("gev"),
}

gev = _register("gev", GEV_SYMBOLS, GEV_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgfs_hip.so : the resident frame store (include/gfs.h).  Loaded only by frames.py, at the first ingest or fetch on device tensors.
# ------------------------------------------------------------------------------------------------
GFS_ABI_VERSION = 2
GFS_E_RANGE = -3               # include/gfs.h: a host index outside the store
GFS_TABLE_ENTRIES = 256        # include/gfs.h: floats of the byte-to-float table
GFS_MAX_BATCH = 65535          # include/gfs.h: frames per gfs_fetch_batch / gfs_compose launch
GFS_FLAG_RANGE = 1             # include/gfs.h: bit of the device flag word

GFS_SYMBOLS = {
    "gfs_abi_version": (C.c_int, []),
    "gfs_last_error": (C.c_char_p, []),
    "gfs_frame_stride": (C.c_int64, [C.c_int32, C.c_int32]),
    "gfs_compose": (C.c_int, [C.c_int32, C.c_int32, _P, C.POINTER(C.c_double), _P, C.c_int64, C.c_int64, C.c_int32, _P]),
    "gfs_resample_tmp_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gfs_resample": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P,
                               C.c_int64, C.c_int64, C.c_int32, _P]),
    "gfs_fetch": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, _P]),
    "gfs_fetch_indexed": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "gfs_fetch_batch": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int32, _P, _P, _P, _P]),
    **_profile_symbols("gfs"),
}

gfs = _register("gfs", GFS_SYMBOLS, GFS_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libgms_hip.so : the fused metric-space regularisers (include/gms.h).  Loaded only by loss.metric_regularizers, at the first call on device
# tensors.
# ------------------------------------------------------------------------------------------------
GMS_ABI_VERSION = 1
GMS_SLAB = 1024               # include/gms.h: splats per workgroup
GMS_MAX_SPLATS = 1 << 24      # include/gms.h: P must stay below this (the count is an exact float)
GMS_ROW_BYTES = 8             # include/gms.h: bytes per splat of the backward's parked face contributions

GMS_SYMBOLS = {
    "gms_abi_version": (C.c_int, []),
    "gms_last_error": (C.c_char_p, []),
    "gms_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "gms_forward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_float, C.c_float, _P, _P, _P]),
    "gms_backward": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_float, C.c_float] + [_P] * 10),
    **_profile_symbols("gms"),
}

gms = _register("gms", GMS_SYMBOLS, GMS_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# libglp_hip.so : LPIPS for evaluation (include/glp.h).  Loaded only by lpips.py, at the first call on device tensors.
# ------------------------------------------------------------------------------------------------
GLP_ABI_VERSION = 1
GLP_NET_ALEX, GLP_NET_VGG = 0, 1   # include/glp.h: the two backbones
GLP_TAPS = 5                       # include/glp.h: taps of either net
GLP_MAX_CONVS = 13                 # include/glp.h: convolutions of the larger net
GLP_TILE = 64                      # include/glp.h: output channels per workgroup of glp_conv2d (Cout is a multiple)
GLP_KBLOCK = 16                    # include/glp.h: packed weights are zero-padded to a multiple of this many reduction rows
GLP_HEAD_BLOCKS = 256              # include/glp.h: most partials of one glp_head launch
GLP_OUT_FLOATS = 6                 # include/glp.h: five per-tap terms and their sum

GLP_SYMBOLS = {
    "glp_abi_version": (C.c_int, []),
    "glp_last_error": (C.c_char_p, []),
    "glp_net_convs": (C.c_int, [C.c_int32]),
    "glp_packed_floats": (C.c_int64, [C.c_int32] * 3),
    "glp_pack_weights": (C.c_int, [C.c_int32] * 3 + [_P, _P, _P]),
    "glp_conv2d": (C.c_int, [C.c_int32] * 8 + [_P, _P, _P, C.c_int32, _P, _P]),
    "glp_maxpool": (C.c_int, [C.c_int64] + [C.c_int32] * 4 + [_P, _P, _P]),
    "glp_zscore": (C.c_int, [C.c_int32] * 3 + [_P, _P, _P, _P]),
    "glp_head_blocks": (C.c_int32, [C.c_int32] * 3),
    "glp_head": (C.c_int, [C.c_int32] * 4 + [_P, _P, _P, _P]),
    "glp_finish": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P]),
    "glp_workspace_bytes": (C.c_int64, [C.c_int32] * 4),
    "glp_forward": (C.c_int, [C.c_int32] * 4 + [_P, _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P, _P, _P]),
    **_profile_symbols("glp"),
}

glp = _register("glp", GLP_SYMBOLS, GLP_ABI_VERSION)


# ------------------------------------------------------------------------------------------------
# per-library shims, made from the table: <tag>_error() for every library, <tag>_profile_enable(on) / <tag>_profile_read() for every one that
# exports csrc/launch_prof.h's entries (libgsr does not: gsr_profile_enable / gsr_profile_read above are its slot-based twins)
# ------------------------------------------------------------------------------------------------
for _tag, _spec in LIBS.items():
    globals()[_tag + "_error"] = partial(last_error, _tag)
    if _tag + "_profile_collect" in _spec.symbols:
        globals()[_tag + "_profile_enable"] = partial(profile_enable, (_tag,))
        globals()[_tag + "_profile_read"] = partial(profile_read, (_tag,))
del _tag, _spec

# libgab's and libgls's launches together: what bench.py's roofline.all_kernels is built from
launch_profile_enable = partial(profile_enable, ("gab", "gls"))
launch_profile_read = partial(profile_read, ("gab", "gls"))
