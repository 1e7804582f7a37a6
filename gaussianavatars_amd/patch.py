"""Zero-edit model-side boundary: rebinds the per-frame methods of the reference's OWN classes to
the fused MI355X path, so train.py / render.py / fps_benchmark_*.py run unchanged.

    import gaussianavatars_amd.patch as P;  P.patch_reference()          # from inside a reference checkout
    python -m gaussianavatars_amd.run fps_benchmark_demo.py --point_path ...   # the same, as a launcher

What is rebound (attribute names, lazy initialisation and autograd connectivity preserved):

    FlameGaussianModel.select_mesh_by_timestep   scene/flame_gaussian_model.py:117-135  -> gab_flame_* + gab_face_frames_* (one node)
    FlameGaussianModel.update_mesh_properties    scene/flame_gaussian_model.py:137-154  -> gab_face_frames_*
    FlameHead.forward (batch 1, no landmarks)    flame_model/flame.py:485-558           -> gab_flame_*  (update_mesh_by_param_dict, :91-115)
    GaussianModel.get_xyz / get_scaling / get_rotation / get_opacity   scene/gaussian_model.py:113-160 -> gab_bind_* (one launch for all four)
    GaussianModel.get_features_split (new)       the two SH leaf tensors, read in place by gsr_forward_ex (no per-frame cat, :152-156)
    gaussian_renderer.render (optional)          gaussian_renderer/__init__.py:19-101   -> the mirror with the split-SH / leaf fast paths
    GaussianModel.densify_and_prune              scene/gaussian_model.py:501-515        -> gdc_plan + gdc_emit (densify.py; GAA_FUSED_DENSIFY=0 opts out)
    NVDiffRenderer.render_mesh / render_from_camera   mesh_renderer/__init__.py:183-274   -> mesh_renderer.py (include/gmr_overlay.h; GAA_FUSED_OVERLAY=0 opts out)
    utils.image_utils.psnr                       utils/image_utils.py:18-20              -> evaluate.psnr (include/gev.h; GAA_FUSED_EVAL=0 opts out)
    scene.Scene.getTrainCameras                  scene/__init__.py:159-160               -> frames.ResidentCameraDataset over a FrameStore (include/gfs.h; GAA_FRAME_STORE=0 opts out)

`patch_classes` works on any class pair with the reference's attribute names; the repository's own mirror classes
(gaussianavatars_amd/gaussian_model.py) are written in composed torch like the reference and go through the very same
patch, which is how the GPU tests exercise it (the reference checkout does not travel to the GPU box).

There is no CPU fallback: a patched method called on host tensors raises the binding library's "no CPU implementation"
error.  `obj.binding_impl = "unfused"` on an instance is an explicit opt-out that runs the original composed-torch methods
(the A/B leg of bench.py and of the parity tests).
"""
from __future__ import annotations

import os
import sys

import torch

from . import binding as fused

_ORIG: dict = {}   # (class, attribute) -> the original attribute, for unpatch() and the "unfused" opt-out


def _default_impl() -> str:
    """GAA_BINDING_IMPL=unfused: objects that do not say otherwise keep the reference's composed-torch methods (CPU tensors, A/B runs)."""
    return os.environ.get("GAA_BINDING_IMPL", "fused")


def _fused(self) -> bool:
    return getattr(self, "binding_impl", _default_impl()) != "unfused"


# ------------------------------------------------------------------------------------------------
# bound accessors: one evaluation per (mesh update, leaf versions), shared by the four properties
# ------------------------------------------------------------------------------------------------
class _BoundCache:
    __slots__ = ("leaves", "versions", "faces", "binding", "binding_version", "grad", "out")


def _same(cache, leaves, faces, binding, grad) -> bool:
    # identity + version of objects the cache itself keeps alive: no id() reuse, no stale hit after densification
    return (cache is not None and cache.grad == grad and cache.binding is binding and cache.binding_version == binding._version
            and all(a is b for a, b in zip(cache.leaves, leaves)) and all(a is b for a, b in zip(cache.faces, faces))
            and cache.versions == tuple(t._version for t in leaves + faces))


def binding_csr_cached(self, num_faces: int):
    """The per-face CSR of `self.binding` for the atomic-free bind backward; rebuilt whenever the binding tensor is
    replaced (densification: cat / prune), modified in place, or the face count changes."""
    b = self.binding
    hit = getattr(self, "_gaa_csr", None)
    if hit is None or hit[0] is not b or hit[1] != b._version or hit[2] != num_faces or hit[3][0].numel() != b.shape[0]:
        hit = (b, b._version, num_faces, fused.binding_csr(b, num_faces))
        self._gaa_csr = hit
    return hit[3]


def bound(self):
    """(get_xyz, get_scaling, get_rotation, get_opacity) of a mesh-bound model from ONE launch.  The reference recomputes
    each accessor on every call (get_xyz twice per render(), gaussian_renderer/__init__.py:27,54); the values only change
    when the mesh, the binding or a leaf does, so they are cached on exactly that.  The shared autograd node keeps its
    inputs for its whole life (binding._Keep), so it can be walked by several backward passes like the reference's
    per-call graphs can."""
    leaves = (self._xyz, self._scaling, self._rotation, self._opacity)
    faces = (self.face_orien_mat, self.face_scaling, self.face_center, self.face_orien_quat)
    grad = torch.is_grad_enabled()
    cache = getattr(self, "_gaa_bound", None)
    if not _same(cache, leaves, faces, self.binding, grad):
        cache = _BoundCache()
        cache.leaves, cache.faces, cache.binding, cache.grad = leaves, faces, self.binding, grad
        cache.binding_version = self.binding._version
        cache.versions = tuple(t._version for t in leaves + faces)
        csr = binding_csr_cached(self, self.face_center.shape[0])
        cache.out = fused.bind_splats(self._xyz, self._scaling, self._rotation, self.binding, self.face_orien_mat, self.face_scaling,
                                      self.face_center, self.face_orien_quat, csr=csr, opacity_logit=self._opacity)
        self._gaa_bound = cache
    return cache.out


def _leaves_complete(self) -> bool:
    """The four leaves the one-launch bind reads all hold N rows.  Not so in the middle of GaussianModel.create_from_pcd
    (scene/gaussian_model.py:185-206 reads `self.get_xyz.shape[0]` after setting `_xyz` and before `_scaling` / `_rotation` / `_opacity` exist):
    such a call takes the reference's own per-accessor code, once, at initialisation."""
    n = self._xyz.shape[0]
    return n > 0 and self._scaling.shape[0] == n and self._rotation.shape[0] == n and self._opacity.shape[0] == n


def _make_accessor(cls, name: str, index: int, mesh_attr: str):
    orig = _ORIG[(cls, name)]

    def getter(self):
        if self.binding is None or not _fused(self) or not _leaves_complete(self):
            return orig.fget(self)
        if getattr(self, mesh_attr) is None:          # same lazy initialisation as the reference (:119-120,131-132,146-147)
            self.select_mesh_by_timestep(0)
        return bound(self)[index]

    getter.__name__ = name
    getter.__doc__ = f"fused {name} (gaussianavatars_amd.patch); original: {cls.__module__}.{cls.__name__}.{name}"
    return property(getter)


def _make_opacity(cls):
    orig = _ORIG[(cls, "get_opacity")]

    def get_opacity(self):
        if self.binding is None or not _fused(self) or self.face_center is None or not _leaves_complete(self):
            return orig.fget(self)
        return bound(self)[3]   # sigmoid(_opacity) rides in the bind kernel (same values, one launch fewer)

    return property(get_opacity)


def _get_features_split(self):
    """(dc (N,1,3), rest (N,K,3)): the two SH leaf tensors for the rasterizer's split-SH entry (None without a rest block)."""
    return (self._features_dc, self._features_rest) if self._features_rest.shape[1] > 0 else None


# ------------------------------------------------------------------------------------------------
# mesh update
# ------------------------------------------------------------------------------------------------
def _select_mesh_by_timestep(self, timestep, original=False):
    if not _fused(self):
        return _ORIG[(type(self)._gaa_patched_base, "select_mesh_by_timestep")](self, timestep, original)
    self.timestep = timestep
    fp = self.flame_param_orig if original and self.flame_param_orig is not None else self.flame_param
    faces = self.flame_model.faces
    verts, verts_cano, c, R, s, q = fused.mesh_frames_timestep(_prepared(self.flame_model), fp, timestep, faces)
    self.face_center, self.face_orien_mat, self.face_scaling, self.face_orien_quat = c, R, s, q
    self.verts, self.faces, self.verts_cano = verts, faces, verts_cano


def _update_mesh_properties(self, verts, verts_cano):
    if not _fused(self):
        return _ORIG[(type(self)._gaa_patched_base, "update_mesh_properties")](self, verts, verts_cano)
    faces = self.flame_model.faces
    c, R, s, q = fused.face_frames(verts.squeeze(0), faces)
    self.face_center, self.face_orien_mat, self.face_scaling, self.face_orien_quat = c, R, s, q
    self.verts, self.faces, self.verts_cano = verts, faces, verts_cano


def _prepared(head):
    """The kernels read the rig buffers in place: make sure they are contiguous fp32 (they are for the reference's FlameHead;
    a re-registered copy otherwise) and that the head carries the `n_shape_params` the rig struct is built from."""
    if getattr(head, "_gaa_prepared", False):
        return head
    for name in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        b = getattr(head, name)
        if b.dtype != torch.float32 or not b.is_contiguous():
            head.register_buffer(name, b.float().contiguous(), persistent=name in head.state_dict())
    head._gaa_prepared = True
    return head


def _device_f32(head, *tensors) -> bool:
    """Device fp32 throughout (what the landmark / root-centring kernels take; anything else is the composed-torch statement's)."""
    return head.v_template.is_cuda and all(t is None or (t.is_cuda and t.dtype is torch.float32) for t in tensors)


def _make_flame_forward(cls):
    orig = _ORIG[(cls, "forward")]

    def forward(self, shape, expr, rotation, neck, jaw, eyes, translation, zero_centered_at_root_node=False,
                return_landmarks=True, return_verts_cano=False, static_offset=None, dynamic_offset=None):
        fusable = (getattr(self, "impl", _default_impl()) != "unfused" and not zero_centered_at_root_node and not return_landmarks
                   and shape.shape[0] == 1)
        if (not fusable and (zero_centered_at_root_node or return_landmarks) and getattr(self, "impl", _default_impl()) != "unfused"
                and shape.shape[0] == 1 and (not return_landmarks or getattr(self, "full_lmk_faces_idx", None) is not None)
                and _device_f32(self, shape, expr, rotation, neck, jaw, eyes, translation, static_offset)):
            # the two other switches (flame.py:532-553) on the kernels: include/gab_landmarks.h
            return fused.flame_head_outputs(_prepared(self), shape, expr, rotation, neck, jaw, eyes, translation, static_offset,
                                            zero_centered_at_root_node, return_landmarks, return_verts_cano)
        if not fusable:
            kw = dict(zero_centered_at_root_node=zero_centered_at_root_node, return_landmarks=return_landmarks,
                      return_verts_cano=return_verts_cano, static_offset=static_offset, dynamic_offset=dynamic_offset)
            return orig(self, shape, expr, rotation, neck, jaw, eyes, translation, **kw)
        verts, v_shaped = fused.flame_forward(_prepared(self), shape, expr, rotation, neck, jaw, eyes, translation, static_offset)
        return [verts, v_shaped] if return_verts_cano else verts

    return forward


# ------------------------------------------------------------------------------------------------
def _hook_spatial_order(G) -> None:
    """Keeps the splats of a model of the REFERENCE's class in Morton order of their positions (gaussian_model.spatial_order_default:
    GAA_SPATIAL_SORT=0 opts out): after `load_ply` (scene/gaussian_model.py:282-332; the reference's FlameGaussianModel.load_ply calls it
    through super()) and after every `densify_and_prune` (:501-515, called from train.py:197-206), which appends its new splats at the end.
    The order is a layout choice -- images and gradients do not depend on it -- that lets a workgroup of the binning pass meet a compact set
    of tiles.  gaussian_model.spatial_resort moves the six leaves, their Adam moments, the densification statistics and
    the binding together: on the device for a model of fp32 device tensors (include/gdc.h ABI 2), through the model's
    own _prune_optimizer anywhere else.  Classes whose load_ply takes `spatial_sort` itself (this package's mirror) are left alone."""
    import inspect

    load = G.__dict__.get("load_ply")
    if load is not None and "spatial_sort" not in inspect.signature(load).parameters:
        _ORIG[(G, "load_ply")] = load

        def load_ply(self, *a, **k):
            out = load(self, *a, **k)
            from .gaussian_model import spatial_order_default, spatial_resort

            if getattr(self, "_xyz", None) is not None:
                self._gaa_order = torch.arange(self._xyz.shape[0], device=self._xyz.device)   # row i of the model = row i of the file, so far
                self._gaa_order_lost = False
            if spatial_order_default() and getattr(self, "_xyz", None) is not None and self._xyz.shape[0] > 1:
                spatial_resort(self)
            return out

        load_ply.__doc__ = load.__doc__
        G.load_ply = load_ply
    # `_gaa_order` (row i of the model = row _gaa_order[i] of the loaded file, -1 for splats born since) follows the rows through the reference's
    # own pruning and appending (scene/gaussian_model.py:371-399, :426-444); a row count that changed any other way drops it (None) instead of
    # leaving a permutation that points at the wrong rows
    prune = G.__dict__.get("prune_points")
    if prune is not None:
        _ORIG[(G, "prune_points")] = prune

        def prune_points(self, mask):
            order, n = getattr(self, "_gaa_order", None), self._xyz.shape[0]
            out = prune(self, mask)        # (narrows `mask` in place to the splats it really removes: every face keeps one)
            tracked = isinstance(order, torch.Tensor) and order.shape[0] == n and mask.shape[0] == n
            self._gaa_order = order.to(mask.device)[~mask] if tracked else None
            if self._gaa_order is None or self._gaa_order.shape[0] != self._xyz.shape[0]:
                self._gaa_order, self._gaa_order_lost = None, True
            return out

        prune_points.__doc__ = prune.__doc__
        G.prune_points = prune_points
    postfix = G.__dict__.get("densification_postfix")
    if postfix is not None:
        _ORIG[(G, "densification_postfix")] = postfix

        def densification_postfix(self, *a, **k):
            order, n = getattr(self, "_gaa_order", None), self._xyz.shape[0]
            out = postfix(self, *a, **k)   # (appends the new splats behind the old ones)
            grown = self._xyz.shape[0] - n
            if isinstance(order, torch.Tensor) and order.shape[0] == n and grown >= 0:
                self._gaa_order = torch.cat([order, torch.full((grown,), -1, dtype=order.dtype, device=order.device)])
            else:
                self._gaa_order, self._gaa_order_lost = None, True
            return out

        densification_postfix.__doc__ = postfix.__doc__
        G.densification_postfix = densification_postfix
    dens = G.__dict__.get("densify_and_prune")
    if dens is not None:
        _ORIG[(G, "densify_and_prune")] = dens

        def densify_and_prune(self, *a, **k):
            # the fused entry (densify.py: include/gdc.h) with the class's own method as what runs outside the kernels' domain; a class whose
            # method already is that entry (this package's mirror) is called as it is
            if getattr(dens, "_gaa_fused", False):
                out = dens(self, *a, **k)
            else:
                from . import densify

                out = densify.densify_and_prune(self, *a, fallback=dens, **k)
            from .gaussian_model import spatial_order_default, spatial_resort

            if spatial_order_default() and self._xyz.shape[0] > 1:
                # a reference class takes spatial_resort's device path (include/gdc.h, ABI 2) where it applies; the mirror's own entry keeps the
                # host statement: its densify_and_prune is pinned to the five gdc launches of the density control itself
                # (tests/test_densify_gpu.py counts them with the order hook on)
                spatial_resort(self, fused=False if getattr(dens, "_gaa_fused", False) else None)
            return out

        densify_and_prune.__doc__ = dens.__doc__
        G.densify_and_prune = densify_and_prune


def patch_classes(gaussian_model_cls, flame_gaussian_model_cls=None, flame_head_cls=None) -> None:
    """Rebinds the per-frame methods of classes shaped like the reference's (idempotent)."""
    G = gaussian_model_cls
    if not getattr(G, "_gaa_patched", False):
        for name in ("get_xyz", "get_scaling", "get_rotation", "get_opacity"):
            _ORIG[(G, name)] = G.__dict__[name]
        G.get_xyz = _make_accessor(G, "get_xyz", 0, "face_center")
        G.get_scaling = _make_accessor(G, "get_scaling", 1, "face_scaling")
        G.get_rotation = _make_accessor(G, "get_rotation", 2, "face_orien_quat")
        G.get_opacity = _make_opacity(G)
        if "get_features_split" not in G.__dict__:
            G.get_features_split = property(_get_features_split)
        _hook_spatial_order(G)
        G._gaa_patched = True
    F = flame_gaussian_model_cls
    if F is not None and not F.__dict__.get("_gaa_patched_flame", False):
        for name in ("select_mesh_by_timestep", "update_mesh_properties"):
            _ORIG[(F, name)] = F.__dict__[name]
        F._gaa_patched_base = F
        F.select_mesh_by_timestep = _select_mesh_by_timestep
        F.update_mesh_properties = _update_mesh_properties
        F._gaa_patched_flame = True
    H = flame_head_cls
    if H is not None and not H.__dict__.get("_gaa_patched_head", False):
        _ORIG[(H, "forward")] = H.__dict__["forward"]
        H.forward = _make_flame_forward(H)
        H._gaa_patched_head = True


def unpatch_classes(*classes) -> None:
    for (cls, name), orig in list(_ORIG.items()):
        if cls in classes:
            setattr(cls, name, orig)
            del _ORIG[(cls, name)]
    for cls in classes:
        for flag in ("_gaa_patched", "_gaa_patched_flame", "_gaa_patched_head", "_gaa_patched_base", "_gaa_patched_stats", "_gaa_patched_optimizer",
                     "_gaa_patched_overlay", "_gaa_patched_eval", "_gaa_orig_psnr", "_gaa_patched_frames", "_gaa_patched_lpips"):
            if flag in cls.__dict__:
                delattr(cls, flag)
        if isinstance(cls.__dict__.get("get_features_split"), property) and cls.__dict__["get_features_split"].fget is _get_features_split:
            delattr(cls, "get_features_split")


def patch_reference(reference_root: str | None = None, fast_render: bool = True, stub_torchvision: bool = True, pin: bool = True) -> dict:
    """Makes a checkout of the reference run on MI355X without editing it.

    1. registers the import shims the reference's unconditional imports need (gaussianavatars_amd.shims) and puts this
       repository's root on sys.path so that `diff_gaussian_rasterization` resolves to the HIP rasterizer;
    2. imports the reference's `scene.gaussian_model`, `scene.flame_gaussian_model`, `flame_model.flame` and rebinds their
       per-frame methods (patch_classes);
    3. with fast_render, replaces `gaussian_renderer.render` by the mirror with the same signature and return dict
       (split-SH read in place, screen-space leaf without the zeros_like + 0 + retain_grad round trip).
    4. with pin (default; GAA_PIN=0 opts out), moves the process next to its GPU (frame_parallel.pin_host_process: the host conditions
       bench.py measures under -- the frame loop is host-paced; forked DataLoader workers keep the original CPU mask).
    5. (GAA_LOSS_SEED=0 opts out) installs loss.install_backward_seed: train.py's `loss.backward()` seeds the backward pass with a cached
       device 1 instead of a one-element fill launch.
    6. (GAA_FUSED_LOSS=0 opts out) patch_loss_and_stats: `utils.loss_utils.l1_loss` / `ssim` and `GaussianModel.add_densification_stats`
       -> the fused kernels of include/gls.h (train.py:131-132,198 unchanged).
    7. (GAA_FUSED_ADAM=0 opts out) patch_optimizer: the torch.optim.Adam that `training_setup` builds becomes an optim.FusedAdam, so
       train.py:209's `gaussians.optimizer.step()` is one launch of include/gop.h.
    8. (GAA_FUSED_OVERLAY=0 opts out) adopt_mesh_overlay: `NVDiffRenderer.render_mesh` / `render_from_camera` (render.py --render_mesh, the
       viewers' show_mesh) run on mesh_renderer.py: six launches instead of the composed torch around rasterize and antialias.
    9. (GAA_FUSED_EVAL=0 opts out) adopt_evaluation: `utils.image_utils.psnr` (train.py:287, metrics.py:73) -> evaluate.psnr, two launches of
       include/gev.h.
    10. (GAA_FRAME_STORE=0 opts out) adopt_frame_store: `scene.Scene.getTrainCameras` returns a frames.ResidentCameraDataset: the ground truth and
       the cameras of the training frames stay in HBM (include/gfs.h), train.py:55's DataLoader workers pass placeholders on and train.py:128's
       `.cuda()` is one launch instead of a 5.3 MB pageable upload.
    11. (GAA_FUSED_LPIPS=0 opts out) adopt_lpips: with LPIPS weights configured (lpips.weights_available: load_weights or GAA_LPIPS_DIR),
       `lpipsPyTorch.lpips` (train.py:26,296, metrics.py:18,74) -> lpips.lpips on the kernels of include/glp.h, so the evaluation pass needs
       neither torchvision nor a download; without weights nothing is touched.
    Returns {'shims': [...], 'classes': [...], 'render': bool, 'pinned_cpus': [...] | None, 'backward_seed': bool, 'loss': [...],
    'optimizer': [...], 'overlay': [...], 'evaluation': [...], 'frames': [...], 'lpips': [...]}.  Call it before the entry script imports
    `render`."""
    from . import shims

    repo_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo_root not in sys.path:
        sys.path.insert(0, repo_root)
    if reference_root is not None and reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    served = shims.install(stub_torchvision=stub_torchvision)
    import importlib

    gm = importlib.import_module("scene.gaussian_model")
    fgm = importlib.import_module("scene.flame_gaussian_model")
    flame = importlib.import_module("flame_model.flame")
    patch_classes(gm.GaussianModel, fgm.FlameGaussianModel, flame.FlameHead)
    did_render = False
    if fast_render:
        gr = importlib.import_module("gaussian_renderer")
        from .gaussian_renderer import render as fast

        if gr.render is not fast:
            _ORIG[(gr, "render")] = gr.render
            gr.render = fast
        did_render = True
    pinned = None
    if pin:
        from .frame_parallel import pin_host_process

        pinned = pin_host_process()
    seeded = False
    if os.environ.get("GAA_LOSS_SEED", "1") != "0":
        from .loss import install_backward_seed

        install_backward_seed()
        seeded = True
    fused_loss = patch_loss_and_stats(gm.GaussianModel) if os.environ.get("GAA_FUSED_LOSS", "1") != "0" else []
    fused_adam = patch_optimizer(gm.GaussianModel, fgm.FlameGaussianModel) if os.environ.get("GAA_FUSED_ADAM", "1") != "0" else []
    overlay = adopt_mesh_overlay() if os.environ.get("GAA_FUSED_OVERLAY", "1") != "0" else []
    evaluation = adopt_evaluation() if os.environ.get("GAA_FUSED_EVAL", "1") != "0" else []
    frames = adopt_frame_store() if os.environ.get("GAA_FRAME_STORE", "1") != "0" else []
    fused_lpips = adopt_lpips() if os.environ.get("GAA_FUSED_LPIPS", "1") != "0" else []
    return dict(shims=served, classes=[gm.GaussianModel, fgm.FlameGaussianModel, flame.FlameHead], render=did_render, pinned_cpus=pinned,
                backward_seed=seeded, loss=fused_loss, optimizer=fused_adam, overlay=overlay, evaluation=evaluation, frames=frames, lpips=fused_lpips)


def _make_resident_getter(orig, name, device):
    def getter(self, scale=1.0):
        from . import frames as FR

        dataset = orig(self, scale)
        if not FR.fused_default() or not hasattr(dataset, "cameras"):
            return dataset
        cache = self.__dict__.setdefault("_gaa_frame_stores", {})
        hit = cache.get((name, scale))
        if hit is None or hit[0] is not dataset.cameras:   # (built on the first call, in the process that makes it: before train.py:55 forks its workers)
            dev = device if device is not None else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            hit = cache[(name, scale)] = (dataset.cameras, FR.FrameStore.from_cameras(dataset.cameras, dev, resample=FR.resize_default()))
        return FR.ResidentCameraDataset(dataset.cameras, hit[1], fallback=dataset)

    getter.__name__ = name
    getter.__doc__ = orig.__doc__
    return getter


def adopt_frame_store(scene_cls=None, device=None) -> list:
    """The training frames behind the zero-edit boundary: wraps `getTrainCameras` of the reference's `scene.Scene` (scene/__init__.py:159-160; or of
    `scene_cls`, any class whose getters return a dataset with a `cameras` list) so that it returns a frames.ResidentCameraDataset over a
    frames.FrameStore on `device` (default: the current GPU; the host without one).  The store is built at the first call -- train.py:55, in the
    main process, before the DataLoader forks its workers -- and kept on the Scene object, one per (getter, scale); train.py and its DataLoader
    line stay unedited.  Frames the store does not hold (budget, a size other than the file's) run the reference's own `__getitem__`; under
    GAA_FRAME_STORE_RESIZE=1 (read when the store is built) frames of another size than their file's are held too, resized as PIL resizes them.
    `getValCameras` / `getTestCameras` are wrapped only under GAA_FRAME_STORE_EVAL=1.  GAA_FRAME_STORE=0 (read at every call of the getter, and
    by patch_reference()) gives the reference's dataset.  Without an importable `scene.Scene` nothing is rebound.  Idempotent; undone by
    unpatch_classes.  Returns the names rebound."""
    cls = scene_cls
    if cls is None:
        import importlib

        try:
            cls = importlib.import_module("scene").Scene
        except (ImportError, AttributeError):
            return []
    if cls.__dict__.get("_gaa_patched_frames", False):
        return []
    names = ["getTrainCameras"] + (["getValCameras", "getTestCameras"] if os.environ.get("GAA_FRAME_STORE_EVAL", "0") == "1" else [])
    done = []
    for name in names:
        if name not in cls.__dict__:
            continue
        _ORIG[(cls, name)] = cls.__dict__[name]
        setattr(cls, name, _make_resident_getter(cls.__dict__[name], name, device))
        done.append(f"{cls.__name__}.{name}")
    cls._gaa_patched_frames = True
    return done


def adopt_lpips(module=None) -> list:
    """LPIPS behind the zero-edit boundary: when weights of either net are configured (lpips.weights_available) and GAA_FUSED_LPIPS is not 0,
    rebinds `lpipsPyTorch.lpips` (or that of `module`, any module with an `lpips`) to lpips.lpips BEFORE train.py:26 / metrics.py:18 bind it --
    the same signature and (1,1,1,1) result, on the kernels of include/glp.h for device fp32 images.  A net whose weights are not configured
    raises, naming the files it wants.  Without weights, or without an importable `lpipsPyTorch`, nothing is touched.  Idempotent; undone by
    unpatch_classes(module).  Returns the names rebound."""
    from . import lpips as L

    if not L.fused_default() or not (L.weights_available("alex") or L.weights_available("vgg")):
        return []
    mod = module
    if mod is None:
        import importlib

        try:
            mod = importlib.import_module("lpipsPyTorch")
        except ImportError:
            return []
    if getattr(mod, "_gaa_patched_lpips", False) or not hasattr(mod, "lpips"):
        return []
    _ORIG[(mod, "lpips")] = mod.lpips
    mod.lpips = L.lpips
    mod._gaa_patched_lpips = True
    return [f"{getattr(mod, '__name__', 'lpipsPyTorch')}.lpips"]


def adopt_evaluation(image_utils=None) -> list:
    """Evaluation behind the zero-edit boundary: rebinds `utils.image_utils.psnr` (utils/image_utils.py:18-20; or that of `image_utils`, any
    module with a `psnr`) to evaluate.psnr BEFORE the entry script imports it (train.py:23, metrics.py:21): a device pair of fp32 images of one
    shape, 3-D or 4-D, takes two launches of include/gev.h instead of about six; anything else -- host tensors, other dtypes, other ranks,
    shapes that broadcast -- keeps the reference's own function, kept on the module as `_gaa_orig_psnr`.  Without an importable
    `utils.image_utils` nothing is rebound.  Idempotent; undone by unpatch_classes(module); GAA_FUSED_EVAL=0 keeps patch_reference() from
    calling it.  Returns the names rebound.  (l1_loss / ssim keep their paired rebinding of patch_loss_and_stats.)"""
    iu = image_utils
    if iu is None:
        import importlib

        try:
            iu = importlib.import_module("utils.image_utils")
        except ImportError:
            return []
    if getattr(iu, "_gaa_patched_eval", False) or not hasattr(iu, "psnr"):
        return []
    from . import evaluate as E

    orig = iu.psnr
    _ORIG[(iu, "psnr")] = orig

    def psnr(img1, img2):
        if not (isinstance(img1, torch.Tensor) and img1.is_cuda and img1.dtype is torch.float32 and img1.dim() in (3, 4)
                and isinstance(img2, torch.Tensor) and img2.is_cuda and img2.dtype is torch.float32 and img1.shape == img2.shape):
            return orig(img1, img2)
        return E.psnr(img1, img2)

    psnr.__doc__ = E.psnr.__doc__
    iu._gaa_orig_psnr = orig
    iu.psnr = psnr
    iu._gaa_patched_eval = True
    return [f"{getattr(iu, '__name__', 'utils.image_utils')}.psnr"]


def _overlay_render_mesh(self, verts, faces, RT, full_proj, image_size, background_color=[1.0, 1.0, 1.0], face_colors=None):
    from . import mesh_renderer as M

    return M.render_mesh(verts, faces, RT, full_proj, image_size, background_color, face_colors, lighting_type=self.lighting_type)


def _overlay_render_from_camera(self, verts, faces, cam, background_color=[1.0, 1.0, 1.0], face_colors=None):
    from . import mesh_renderer as M

    return M.render_from_camera(verts, faces, cam, background_color, face_colors, lighting_type=self.lighting_type,
                                use_opengl=self.use_opengl)


def adopt_mesh_overlay(renderer_cls=None) -> list:
    """The mesh overlay behind the zero-edit boundary: rebinds `render_mesh` and `render_from_camera` of the reference's
    `mesh_renderer.NVDiffRenderer` (mesh_renderer/__init__.py:183-274; or of `renderer_cls`, any class with its `lighting_type` and
    `use_opengl` attributes) to gaussianavatars_amd.mesh_renderer, which honours both attributes of the instance.  Same arguments, same dict
    of four maps; forward only, device tensors only (a host tensor raises ValueError: there is no CPU path).  Without an importable
    `mesh_renderer` module nothing is rebound.  Idempotent; undone by unpatch_classes; GAA_FUSED_OVERLAY=0 keeps patch_reference() from
    calling it.  Returns the names rebound."""
    cls = renderer_cls
    if cls is None:
        import importlib

        try:
            cls = importlib.import_module("mesh_renderer").NVDiffRenderer
        except (ImportError, AttributeError):
            return []
    if cls.__dict__.get("_gaa_patched_overlay", False):
        return []
    done = []
    for name, fn in (("render_mesh", _overlay_render_mesh), ("render_from_camera", _overlay_render_from_camera)):
        _ORIG[(cls, name)] = cls.__dict__[name]
        setattr(cls, name, fn)
        done.append(f"{cls.__name__}.{name}")
    cls._gaa_patched_overlay = True
    return done


def patch_optimizer(gaussian_model_cls, flame_gaussian_model_cls=None) -> list:
    """The optimizer step behind the zero-edit boundary: wraps `training_setup` of the classes that define it (scene/gaussian_model.py:208-226,
    scene/flame_gaussian_model.py:174-208) so that, after the original has returned, `self.optimizer = optim.adopt(self.optimizer)`: the very
    torch.optim.Adam object the reference built -- its six named groups, and the three FlameGaussianModel adds with add_param_group -- steps
    through include/gop.h (optim.FusedAdam: same state, same state_dict, torch's own step outside the kernel's domain, e.g. on CPU tensors).
    `restore()` goes through `training_setup` (scene/gaussian_model.py:96) and is covered by the same wrap.  Idempotent; undone by
    unpatch_classes; GAA_FUSED_ADAM=0 keeps patch_reference() from calling it.  Returns the names rebound.

    This package's own mirror classes (gaussian_model.py) adopt the optimizer inside their own `training_setup`."""
    from . import optim

    done = []
    for cls in (gaussian_model_cls, flame_gaussian_model_cls):
        if cls is None or "training_setup" not in cls.__dict__ or cls.__dict__.get("_gaa_patched_optimizer", False):
            continue
        orig = cls.__dict__["training_setup"]
        _ORIG[(cls, "training_setup")] = orig
        cls.training_setup = _make_training_setup(orig, optim)
        cls._gaa_patched_optimizer = True
        done.append(f"{cls.__name__}.training_setup")
    return done


def _make_training_setup(orig, optim):
    def training_setup(self, *a, **k):
        out = orig(self, *a, **k)
        if getattr(self, "optimizer", None) is not None:
            self.optimizer = optim.adopt(self.optimizer)
        return out

    training_setup.__name__ = getattr(orig, "__name__", "training_setup")
    training_setup.__doc__ = orig.__doc__
    return training_setup


def patch_loss_and_stats(gaussian_model_cls=None, loss_utils=None) -> list:
    """SURVEY.md 8(f) N3 behind the zero-edit boundary: the training-step neighbours of the render path, rebound BEFORE the entry script
    imports them (train.py:22 `from utils.loss_utils import l1_loss, ssim`):

        utils.loss_utils.l1_loss / ssim              utils/loss_utils.py:17-18,36-63 -> loss.l1_loss_paired / loss.ssim_paired: train.py:131-132's two
                                                     calls on the same (image, gt) become ONE fused pass (gls_l1_ssim_*) from the second iteration on
        GaussianModel.add_densification_stats        scene/gaussian_model.py:517-519 (train.py:198) -> gls_add_densification_stats, one launch

    Host tensors / other dtypes / other window sizes keep the reference's own functions (kept on the module as `_gaa_orig_*`).  GAA_FUSED_LOSS=0
    opts out.  Returns the names rebound (idempotent)."""
    import importlib

    from . import loss as L

    done = []
    lu = loss_utils if loss_utils is not None else importlib.import_module("utils.loss_utils")
    if not getattr(lu, "_gaa_patched", False):
        orig_l1, orig_ssim = lu.l1_loss, lu.ssim
        _ORIG[(lu, "l1_loss")], _ORIG[(lu, "ssim")] = orig_l1, orig_ssim

        def l1_loss(network_output, gt):
            if not (isinstance(network_output, torch.Tensor) and network_output.is_cuda and network_output.dtype is torch.float32
                    and isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype is torch.float32):
                return orig_l1(network_output, gt)
            return L.l1_loss_paired(network_output, gt)

        def ssim(img1, img2, window_size=11, size_average=True):
            if not (window_size == 11 and isinstance(img1, torch.Tensor) and img1.is_cuda and img1.dtype is torch.float32 and img1.dim() in (3, 4)
                    and isinstance(img2, torch.Tensor) and img2.is_cuda and img2.dtype is torch.float32 and img1.shape == img2.shape):
                return orig_ssim(img1, img2, window_size, size_average)
            return L.ssim_paired(img1, img2, window_size, size_average)

        l1_loss.__doc__, ssim.__doc__ = L.l1_loss_paired.__doc__, L.ssim_paired.__doc__
        lu._gaa_orig_l1_loss, lu._gaa_orig_ssim = orig_l1, orig_ssim
        lu.l1_loss, lu.ssim = l1_loss, ssim
        lu._gaa_patched = True
        done += ["utils.loss_utils.l1_loss", "utils.loss_utils.ssim"]
    G = gaussian_model_cls
    if G is not None and "add_densification_stats" in G.__dict__ and not G.__dict__.get("_gaa_patched_stats", False):
        _ORIG[(G, "add_densification_stats")] = G.__dict__["add_densification_stats"]
        G.add_densification_stats = L.add_densification_stats
        G._gaa_patched_stats = True
        done.append(f"{G.__name__}.add_densification_stats")
    return done
