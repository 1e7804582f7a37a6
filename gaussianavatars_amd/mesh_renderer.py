"""The shaded mesh overlay: the reference's NVDiffRenderer.render_from_camera / render_mesh (mesh_renderer/__init__.py) on the HIP
kernels of include/gmr.h and include/gmr_overlay.h, and the viewer's blend of the mesh over the splat image (train.py's network loop).
Forward only.

    MeshRenderer(use_opengl=False, lighting_type='constant')
        .render_from_camera(verts, faces, cam, background_color=[1, 1, 1], face_colors=None)
        .render_mesh(verts, faces, RT, full_proj, image_size, background_color=[1, 1, 1], face_colors=None)
            -> {'albedo', 'normal', 'diffuse': (B, H, W, 3), 'rgba': (B, H, W, 4)}, row 0 at the top of the image
    compose_overlay(splat_image, rgba_mesh, mesh_opacity, as_bytes=False)
    resize_flip(image, size)

One frame is six launches -- gmr_mesh_prepare, gmr_rasterize (setup + raster), gmr_mesh_shade, gmr_antialias, gmr_resize_flip -- and no host
wait once the topology is known: the int32 triangles, their index range and the edge adjacency are kept per `faces` tensor (topology()).
The contract is DESIGN.md section 16.  Every argument is checked before any launch and a CUDA tensor is required last, so the checks run
on host tensors too.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, mesh_raster

LIGHTING = {"constant": _lib.GMR_LIGHT_CONSTANT, "front": _lib.GMR_LIGHT_FRONT}
MAX_RENDER_SIDE = 2048      # the non-OpenGL branch of render_from_camera renders at 2048 x 2048 when either side of the image exceeds this
TOPOLOGY_CACHE_ENTRIES = 8  # `faces` tensors remembered (least recently used goes first)


# ---- the size rule ---------------------------------------------------------------------------------------------------------------------
def render_size(image_height: int, image_width: int, use_opengl: bool = False):
    """(H, W) render_from_camera rasterizes at: the image itself with use_opengl; otherwise both sides rounded down to a multiple of 8, or
    2048 x 2048 when either side exceeds 2048 (the result is resized back to the image)."""
    H, W = int(image_height), int(image_width)
    if H < 1 or W < 1:
        raise ValueError(f"the image must be at least 1 x 1, got ({H}, {W})")
    if use_opengl:
        return H, W
    if H > MAX_RENDER_SIDE or W > MAX_RENDER_SIDE:
        return MAX_RENDER_SIDE, MAX_RENDER_SIDE
    h, w = H // 8 * 8, W // 8 * 8
    if h < 1 or w < 1:
        raise ValueError(f"an image of ({H}, {W}) rounds down to a render of ({h}, {w}): both sides must be at least 8 without use_opengl")
    return h, w


# ---- topology cache --------------------------------------------------------------------------------------------------------------------
class _Topology:
    __slots__ = ("faces", "tri", "neighbours", "lo", "hi")


_TOPOLOGY: "OrderedDict[tuple, _Topology]" = OrderedDict()


def _build_adjacency(tri: torch.Tensor, num_vertices: int) -> torch.Tensor:
    """The edge adjacency of a topology (mesh_raster.edge_neighbours); the one place the cache builds it."""
    return mesh_raster.edge_neighbours(tri, num_vertices)


def _topology_key(faces: torch.Tensor):
    return (faces.data_ptr(), faces._version, tuple(faces.shape), faces.dtype, faces.device)


def topology(faces: torch.Tensor) -> _Topology:
    """What the kernels need of a `faces` tensor (F, 3), built once per tensor: the contiguous int32 triangles, their index range (the one
    host read) and the edge adjacency for gmr_antialias.  Keyed on (data_ptr, _version, shape, dtype, device); the entry holds `faces`
    itself, so its storage cannot be handed to another tensor while the entry lives.  An in-place edit (a new _version) or another tensor
    is another entry."""
    key = _topology_key(faces)
    hit = _TOPOLOGY.get(key)
    if hit is not None and hit.faces is faces:
        _TOPOLOGY.move_to_end(key)
        return hit
    t = _Topology()
    t.faces = faces
    t.tri = faces.detach().to(torch.int32).contiguous()
    if t.tri.shape[0] > 0:
        lo, hi = torch.aminmax(faces.detach())
        t.lo, t.hi = int(lo), int(hi)
    else:
        t.lo, t.hi = 0, -1
    t.neighbours = _build_adjacency(t.tri, t.hi + 1) if t.lo >= 0 else None
    _TOPOLOGY[key] = t
    _TOPOLOGY.move_to_end(key)
    while len(_TOPOLOGY) > TOPOLOGY_CACHE_ENTRIES:
        _TOPOLOGY.popitem(last=False)
    return t


def clear_topology_cache() -> None:
    _TOPOLOGY.clear()


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def _float_tensor(name, x, rank):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {x.dtype}")
    if x.dim() != rank:
        raise ValueError(f"{name} must have rank {rank}, got shape {tuple(x.shape)}")


def _check_mesh(verts, faces, face_colors):
    _float_tensor("verts", verts, 3)
    if verts.shape[2] != 3:
        raise ValueError(f"verts must be (B, V, 3), got {tuple(verts.shape)}")
    if verts.shape[0] < 1:
        raise ValueError("verts must hold at least one batch element")
    if not isinstance(faces, torch.Tensor) or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be an int32 or int64 torch.Tensor, got {getattr(faces, 'dtype', type(faces).__name__)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be (F, 3), got {tuple(faces.shape)}")
    B, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    if F > mesh_raster.MAX_TRIANGLES:
        raise ValueError(f"faces holds {F} triangles; at most {mesh_raster.MAX_TRIANGLES} (2^24 - 1) are supported")
    if face_colors is not None:
        _float_tensor("face_colors", face_colors, 3)
        if tuple(face_colors.shape) != (B, F, 3):
            raise ValueError(f"face_colors must be (B, F, 3) = {(B, F, 3)}, got {tuple(face_colors.shape)}")
    topo = topology(faces)
    if F > 0 and (topo.lo < 0 or topo.hi >= V):
        raise ValueError(f"faces indexes vertices in [{topo.lo}, {topo.hi}], outside [0, {V}) of verts")
    return topo


def _check_background(background_color, B, H, W):
    """(three floats, None) for a constant colour, (None, image) for a (B, H, W, 3) image."""
    if isinstance(background_color, torch.Tensor):
        _float_tensor("background_color", background_color, 4)
        if tuple(background_color.shape) != (B, H, W, 3):
            raise ValueError(f"a background image must be (B, H, W, 3) = {(B, H, W, 3)} at the render size, got {tuple(background_color.shape)}")
        return None, background_color
    if isinstance(background_color, (list, tuple)):
        if len(background_color) != 3:
            raise ValueError(f"a constant background is three numbers, got {len(background_color)}")
        return tuple(float(np.float32(c)) for c in background_color), None
    raise ValueError(f"Unknown background type: {type(background_color)}")


def _check_matrix(name, M, B, rows):
    _float_tensor(name, M, 3)
    if M.shape[0] != B or M.shape[1] not in rows or M.shape[2] != 4:
        raise ValueError(f"{name} must be (B, {' or '.join(str(r) for r in rows)}, 4) with B = {B}, got {tuple(M.shape)}")


def _check_device(**tensors):
    dev = None
    for name, x in tensors.items():
        if x is None:
            continue
        if not x.is_cuda:
            raise ValueError(f"{name} must be a CUDA (HIP) tensor: the mesh renderer has no CPU path")
        if dev is None:
            dev = x.device
        elif x.device != dev:
            raise ValueError(f"{name} is on {x.device}, expected {dev}")
    return dev


def _lighting(lighting_type):
    if lighting_type not in LIGHTING:
        raise NotImplementedError(f"Unknown lighting type: {lighting_type}")
    return LIGHTING[lighting_type]


# ---- launches --------------------------------------------------------------------------------------------------------------------------
def _ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None and x.numel() > 0 else None


def _fail(what):
    raise RuntimeError(f"{what} failed: {_lib.gmr_error()}")


def _prepare(verts, tri, rt, mvp, mat_mode, dev, stream):
    lib = _lib.gmr()
    B, V, F = verts.shape[0], verts.shape[1], tri.shape[0]
    pos_clip = torch.empty((B, V, 4), dtype=torch.float32, device=dev)
    normals = torch.empty((B, F, 3), dtype=torch.float32, device=dev)
    if lib.gmr_mesh_prepare(B, V, F, _ptr(verts), _ptr(tri), _ptr(rt), rt.shape[1], _ptr(mvp), mat_mode, _ptr(pos_clip), _ptr(normals),
                            stream) != 0:
        _fail("gmr_mesh_prepare")
    return pos_clip, normals


def _shade(rast, normals, face_colors, lighting, bg, bg_image, dev, stream):
    lib = _lib.gmr()
    B, H, W = rast.shape[:3]
    maps = [torch.empty((B, H, W, c), dtype=torch.float32, device=dev) for c in (3, 3, 3, 4)]
    r, g, b = bg if bg is not None else (0.0, 0.0, 0.0)
    if lib.gmr_mesh_shade(B, normals.shape[1], H, W, _ptr(rast), _ptr(normals), _ptr(face_colors), lighting, r, g, b, _ptr(bg_image),
                          *(_ptr(m) for m in maps), stream) != 0:
        _fail("gmr_mesh_shade")
    return maps


def _antialias(color, rast, pos, tri, neighbours, dev, stream):
    lib = _lib.gmr()
    B, H, W, Cn = color.shape
    out = torch.empty_like(color)
    if lib.gmr_antialias(B, pos.shape[1], tri.shape[0], H, W, Cn, _ptr(color), _ptr(rast), _ptr(pos), _ptr(tri), _ptr(neighbours), _ptr(out),
                         stream) != 0:
        _fail("gmr_antialias")
    return out


def _resize_flip(images, H, W, dev, stream):
    lib = _lib.gmr()
    B, h, w = images[0].shape[:3]
    outs = [torch.empty((B, H, W, x.shape[3]), dtype=torch.float32, device=dev) for x in images]
    table = (_lib.GmrMap * len(images))(*(_lib.GmrMap(x.data_ptr(), o.data_ptr(), x.shape[3]) for x, o in zip(images, outs)))
    if lib.gmr_resize_flip(B, h, w, H, W, len(images), table, stream) != 0:
        _fail("gmr_resize_flip")
    return outs


class _ForwardOnly(torch.autograd.Function):
    """Hangs the outputs off a node whose backward refuses: the overlay has no gradient, and it must never come back silently wrong or
    silently missing."""

    @staticmethod
    def forward(ctx, run, *inputs):
        return run()

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the mesh overlay (gaussianavatars_amd.mesh_renderer: render_mesh / render_from_camera / resize_flip / "
                                  "compose_overlay) is forward-only: it has no gradient with respect to its inputs")


def _through_node(run, *inputs):
    live = [x for x in inputs if isinstance(x, torch.Tensor) and x.requires_grad]
    if torch.is_grad_enabled() and live:
        return _ForwardOnly.apply(run, *live)
    return run()


KEYS = ("albedo", "normal", "diffuse", "rgba")


def _render(verts, topo, rt, mvp, mat_mode, render_hw, out_hw, bg, bg_image, face_colors, lighting, dev):
    """prepare -> rasterize -> shade -> antialias -> flip (+ resize): the four maps at out_hw, row 0 at the top."""
    h, w = render_hw
    H, W = out_hw
    stream = C.c_void_p(_lib.raw_stream(dev))
    verts_c = verts.detach().contiguous()
    colors_c = None if face_colors is None else face_colors.detach().contiguous()
    bg_c = None if bg_image is None else bg_image.detach().contiguous()
    with _lib.on_device(dev):
        pos_clip, normals = _prepare(verts_c, topo.tri, rt, mvp, mat_mode, dev, stream)
        rast, _ = mesh_raster._rasterize(pos_clip, topo.tri, h, w, dev)
        albedo, normal, diffuse, rgba = _shade(rast, normals, colors_c, lighting, bg, bg_c, dev, stream)
        rgba_aa = _antialias(rgba, rast, pos_clip, topo.tri, topo.neighbours, dev, stream)
        return tuple(_resize_flip([albedo, normal, diffuse, rgba_aa], H, W, dev, stream))


class MeshRenderer(torch.nn.Module):
    """NVDiffRenderer's public surface on this package's kernels.  `use_opengl` only selects render_from_camera's size rule (there is no
    GL context): True renders at the image size, False at render_size() and resizes back, as the reference's CUDA-context branch does."""

    def __init__(self, use_opengl: bool = False, lighting_type: str = "constant", lighting_space: str = "camera"):
        super().__init__()
        _lighting(lighting_type)
        if lighting_space != "camera":
            raise NotImplementedError(f"lighting_space {lighting_space!r}: the face normals are shaded in camera space only")
        self.use_opengl = use_opengl
        self.lighting_type = lighting_type
        self.lighting_space = lighting_space

    def render_from_camera(self, verts, faces, cam, background_color=[1.0, 1.0, 1.0], face_colors=None):
        """Renders the mesh as `cam` sees it: {'albedo', 'normal', 'diffuse' (B, H, W, 3), 'rgba' (B, H, W, 4)} at the camera's image size.
        cam.world_view_transform and cam.full_proj_transform are read as the camera stores them (the y and z flips to OpenGL axes
        happen inside gmr_mesh_prepare)."""
        return render_from_camera(verts, faces, cam, background_color, face_colors, lighting_type=self.lighting_type, use_opengl=self.use_opengl)

    def render_mesh(self, verts, faces, RT, full_proj, image_size, background_color=[1.0, 1.0, 1.0], face_colors=None):
        """Renders verts (B, V, 3) / faces (F, 3) with RT (B, 3 or 4, 4) world-to-camera and full_proj (B, 4, 4) world-to-clip (OpenGL axes)
        at image_size = (H, W)."""
        return render_mesh(verts, faces, RT, full_proj, image_size, background_color, face_colors, lighting_type=self.lighting_type)


def _camera_matrix(name, M, verts):
    if isinstance(M, np.ndarray):
        M = torch.from_numpy(M)
    if not isinstance(M, torch.Tensor) or tuple(M.shape) != (4, 4):
        raise ValueError(f"cam.{name} must be a (4, 4) tensor, got {getattr(M, 'shape', type(M).__name__)}")
    return M.detach().to(device=verts.device, dtype=verts.dtype).contiguous()[None]


def render_from_camera(verts, faces, cam, background_color=[1.0, 1.0, 1.0], face_colors=None, lighting_type="constant", use_opengl=False):
    lighting = _lighting(lighting_type)
    topo = _check_mesh(verts, faces, face_colors)
    if verts.shape[0] != 1:
        raise ValueError(f"render_from_camera draws one camera: verts must be (1, V, 3), got {tuple(verts.shape)}")
    H, W = int(cam.image_height), int(cam.image_width)
    h, w = render_size(H, W, use_opengl)
    mesh_raster._check_image(1, max(h, H), max(w, W))
    bg, bg_image = _check_background(background_color, 1, h, w)
    rt = _camera_matrix("world_view_transform", cam.world_view_transform, verts)
    mvp = _camera_matrix("full_proj_transform", cam.full_proj_transform, verts)
    dev = _check_device(verts=verts, faces=faces, face_colors=face_colors, background_color=bg_image)
    out = _through_node(lambda: _render(verts, topo, rt, mvp, _lib.GMR_MAT_CAMERA, (h, w), (H, W), bg, bg_image, face_colors, lighting, dev),
                        verts, face_colors, bg_image)
    return dict(zip(KEYS, out))


def render_mesh(verts, faces, RT, full_proj, image_size, background_color=[1.0, 1.0, 1.0], face_colors=None, lighting_type="constant"):
    lighting = _lighting(lighting_type)
    topo = _check_mesh(verts, faces, face_colors)
    B = verts.shape[0]
    try:
        H, W = (int(s) for s in image_size)
    except (TypeError, ValueError):
        raise ValueError(f"image_size must be (H, W), got {image_size!r}") from None
    mesh_raster._check_image(B, H, W)
    if isinstance(RT, np.ndarray):
        RT = torch.from_numpy(RT).to(verts.device)
    if isinstance(full_proj, np.ndarray):
        full_proj = torch.from_numpy(full_proj).to(verts.device)
    _check_matrix("RT", RT, B, (3, 4))
    _check_matrix("full_proj", full_proj, B, (4,))
    bg, bg_image = _check_background(background_color, B, H, W)
    dev = _check_device(verts=verts, faces=faces, RT=RT, full_proj=full_proj, face_colors=face_colors, background_color=bg_image)
    rt, mvp = RT.detach().contiguous(), full_proj.detach().contiguous()
    out = _through_node(lambda: _render(verts, topo, rt, mvp, _lib.GMR_MAT_ROWS, (H, W), (H, W), bg, bg_image, face_colors, lighting, dev),
                        verts, face_colors, bg_image, RT, full_proj)
    return dict(zip(KEYS, out))


# ---- the two stand-alone pieces ----------------------------------------------------------------------------------------------------------
def resize_flip(image, size):
    """image (B, h, w, C) float32 -> (B, H, W, C): the vertical flip followed by F.interpolate(..., size, mode='bilinear',
    align_corners=False) of the reference, in one pass; with size == (h, w) the flip alone, bit for bit."""
    _float_tensor("image", image, 4)
    try:
        H, W = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    B, h, w, Cn = image.shape
    if B < 1 or Cn < 1:
        raise ValueError(f"image must hold at least one batch element and one channel, got {tuple(image.shape)}")
    mesh_raster._check_image(B, h, w)
    mesh_raster._check_image(B, H, W)
    dev = _check_device(image=image)
    x = image.detach().contiguous()

    def run():
        with _lib.on_device(dev):
            return _resize_flip([x], H, W, dev, C.c_void_p(_lib.raw_stream(dev)))[0]

    return _through_node(run, image)


def compose_overlay(splat_image, rgba_mesh, mesh_opacity, as_bytes=False):
    """The viewer's blend of the mesh over the splat image (the reference's train.py network loop), one launch:

        net = rgb * alpha * mesh_opacity + splat_image * (alpha * (1 - mesh_opacity) + (1 - alpha))      (rgb alone without a splat image)

    with the bits of that torch expression.  splat_image: (3, H, W) float32 or None; rgba_mesh: (H, W, 4) or (1, H, W, 4) as render_from_camera
    returns it.  Returns (3, H, W) float32, or with as_bytes the (H, W, 3) uint8 image network_gui.send puts on the wire
    (clamp to [0, 1], times 255, truncated)."""
    if not isinstance(rgba_mesh, torch.Tensor) or rgba_mesh.dtype != torch.float32:
        raise ValueError(f"rgba_mesh must be a float32 torch.Tensor, got {getattr(rgba_mesh, 'dtype', type(rgba_mesh).__name__)}")
    if rgba_mesh.dim() == 4 and rgba_mesh.shape[0] == 1:
        rgba_mesh = rgba_mesh[0]
    if rgba_mesh.dim() != 3 or rgba_mesh.shape[2] != 4:
        raise ValueError(f"rgba_mesh must be (H, W, 4) or (1, H, W, 4), got {tuple(rgba_mesh.shape)}")
    H, W = rgba_mesh.shape[:2]
    mesh_raster._check_image(1, H, W)
    if splat_image is not None:
        _float_tensor("splat_image", splat_image, 3)
        if tuple(splat_image.shape) != (3, H, W):
            raise ValueError(f"splat_image must be (3, H, W) = {(3, H, W)}, got {tuple(splat_image.shape)}")
    try:
        op = float(mesh_opacity)
    except (TypeError, ValueError):
        raise ValueError(f"mesh_opacity must be a number, got {mesh_opacity!r}") from None
    dev = _check_device(rgba_mesh=rgba_mesh, splat_image=splat_image)
    rgba_c = rgba_mesh.detach().contiguous()
    splat_c = None if splat_image is None else splat_image.detach().contiguous()

    def run():
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if as_bytes else torch.empty((3, H, W), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.gmr().gmr_compose_overlay(H, W, _ptr(splat_c), _ptr(rgba_c), op, 1 - op, None if as_bytes else _ptr(out),
                                                _ptr(out) if as_bytes else None, C.c_void_p(_lib.raw_stream(dev)))
        if rc != 0:
            _fail("gmr_compose_overlay")
        return out

    if as_bytes:
        return run()
    return _through_node(run, rgba_mesh, splat_image)
