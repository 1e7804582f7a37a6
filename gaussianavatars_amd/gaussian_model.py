"""Host-side mirror of the model half of the hot path: the accessors of
scene/gaussian_model.py:113-163 and the mesh update of scene/flame_gaussian_model.py:91-154, with
the same names, attributes and lazy-init behaviour, so a caller written against the reference
(`render()`, train.py's inner loop, fps_benchmark_demo.py) reads the same.

The classes below state the per-frame methods in COMPOSED TORCH, the way the reference's own classes do, and then go
through `gaussianavatars_amd.patch.patch_classes` at the bottom of this file -- the very call that rebinds the
reference's classes in a checkout (`patch_reference()`).  `binding_impl="unfused"` on an instance opts out of the
fused kernels (the A/B leg of bench.py and the parity tests).  /root/reference does not travel to the GPU box; these
stand-ins are what the GPU tests and bench.py drive, through the same patched methods.

Beside the per-frame path the classes carry the training surface a loop needs to run on this package alone: `training_setup` (the
reference's group names, learning rates and `percent_dense`, scene/gaussian_model.py:208-226 and scene/flame_gaussian_model.py:174-207;
the optimizer is an optim.FusedAdam unless GAA_FUSED_ADAM=0), `update_learning_rate`, `densify_and_prune` (densify.py: include/gdc.h on
device tensors, its composed-torch statement anywhere else), `prune_points`, `reset_opacity` and `_prune_optimizer` (what spatial_resort
moves the Adam moments with).  Dataset loading stays with the reference's own files.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from . import unfused


class _TrainingSetup:
    """scene/gaussian_model.py:208-234 for the mirror classes: the optimizer of a training run and the position group's schedule.  A base of its
    own: patch.patch_optimizer wraps the `training_setup` a class itself defines (the reference's), and this one adopts its optimizer itself."""

    def training_setup(self, training_args):
        """The six splat groups of the reference, by name, with its learning rates; `percent_dense`; fresh densification statistics."""
        import os

        from . import optim

        n, dev = self._xyz.shape[0], self._xyz.device
        self.percent_dense = training_args.percent_dense
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        scale = getattr(self, "spatial_lr_scale", 1.0)
        groups = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
        ]
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        if os.environ.get("GAA_FUSED_ADAM", "1") != "0":
            self.optimizer = optim.adopt(self.optimizer)
        self._xyz_lr = (training_args.position_lr_init * scale, training_args.position_lr_final * scale,
                        getattr(training_args, "position_lr_delay_mult", 1.0), getattr(training_args, "position_lr_max_steps", 1000000))

    def update_learning_rate(self, iteration):
        """The position group's rate: log-linear from position_lr_init to position_lr_final over position_lr_max_steps (no delay ramp unless
        position_lr_delay_mult < 1 is combined with delay steps, which the reference never sets)."""
        lr_init, lr_final, _, max_steps = self._xyz_lr
        if iteration < 0 or (lr_init == 0.0 and lr_final == 0.0):
            lr = 0.0
        else:
            t = min(max(iteration / max_steps, 0.0), 1.0)
            lr = float(np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = lr
        return lr


class GaussianModel(_TrainingSetup):
    """Accessor surface of the reference GaussianModel (scene/gaussian_model.py:52-163)."""

    def __init__(self, sh_degree: int, binding_impl: str = "fused"):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        # mesh binding (reference :64-72)
        self.face_center = None
        self.face_scaling = None
        self.face_orien_mat = None
        self.face_orien_quat = None
        self.binding = None
        self.binding_counter = None
        self.timestep = None
        self.num_timesteps = 1
        if binding_impl not in ("fused", "unfused"):
            raise ValueError("binding_impl must be 'fused' or 'unfused'")
        self.binding_impl = binding_impl

    # ---- parameter loading: arrays, a point cloud (create_from_pcd), a PLY ----------------
    def load_arrays(self, arrs: Dict[str, np.ndarray], device="cuda", requires_grad: bool = True):
        """arrs uses the reference's leaf names (_xyz, _features_dc, _features_rest, _scaling, _rotation,
        _opacity, optional binding).  Like load_ply (:323) this activates the full SH degree."""
        for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
            src = arrs[k]
            if isinstance(src, np.ndarray) and not src.flags.writeable:   # (io.load_ply maps the file read-only: a host tensor must not alias it)
                src = np.array(src)
            t = torch.as_tensor(src, dtype=torch.float32, device=device).contiguous()
            setattr(self, k, nn.Parameter(t.requires_grad_(requires_grad)))
        if arrs.get("binding") is not None:
            self.binding = torch.as_tensor(arrs["binding"], device=device)
            nf = int(self.binding.max().item()) + 1
            self.binding_counter = torch.bincount(self.binding.long(), minlength=nf).int()
        self.active_sh_degree = self.max_sh_degree
        self.max_radii2D = torch.zeros((self._xyz.shape[0]), device=device)
        # densification statistics, as training_setup allocates them (scene/gaussian_model.py:210-211)
        self.xyz_gradient_accum = torch.zeros((self._xyz.shape[0], 1), device=device)
        self.denom = torch.zeros((self._xyz.shape[0], 1), device=device)

    def create_from_pcd(self, pcd, spatial_lr_scale: float, device="cuda"):
        """scene/gaussian_model.py:172-206: a model from nothing.  Un-bound: `pcd` has `.points` and `.colors` (N, 3); the DC colours are
        RGB2SH(colors) and every scale is log sqrt of the mean squared distance to the point's 3 nearest neighbours (knn.dist2_knn3: the exact
        search of include/gdc.h on device tensors), clamped at 1e-7.  Bound (`pcd is None`, a model with a binding): one splat per entry of
        `binding` at the face's origin, colours from the GLOBAL numpy stream as the reference draws them (np.random.random / 255: a seeded run
        matches), scales log 1.  Both: identity rotations, opacity inverse_sigmoid(0.1), zero higher SH, zero max_radii2D; the leaves have the
        layouts of load_arrays and `training_setup` works on the result.  `active_sh_degree` is left as it is (0 on a fresh model)."""
        from . import knn

        self.spatial_lr_scale = spatial_lr_scale
        if pcd is None:
            if self.binding is None:
                raise ValueError("create_from_pcd(None, ...) needs a model with a binding")
            n = self.binding.shape[0]
            xyz = torch.zeros((n, 3), dtype=torch.float32, device=device)
            color = torch.tensor(np.random.random((n, 3)) / 255.0).float()
        else:
            xyz = torch.tensor(np.asarray(pcd.points)).float().to(device)
            color = (torch.tensor(np.asarray(pcd.colors)).float() - 0.5) / 0.28209479177387814   # utils/sh_utils.py: RGB2SH
            n = xyz.shape[0]
        # (the colours and the opacity constant are rounded on the host, once: a device divides by a scalar as a multiplication by its reciprocal
        # and has its own log, and a model must not start an ulp away from where the same call puts it on the CPU)
        color = color.to(device)
        tenth = torch.full((1,), 0.1, dtype=torch.float32)
        logit = float(torch.log(tenth / (1 - tenth)))   # utils/general_utils.py: inverse_sigmoid
        if self.binding is None:
            dist2 = torch.clamp_min(knn.dist2_knn3(xyz), 0.0000001)
            scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        else:
            scales = torch.zeros((n, 3), dtype=torch.float32, device=device)
        rots = torch.zeros((n, 4), dtype=torch.float32, device=device)
        rots[:, 0] = 1
        leaves = {"_xyz": xyz, "_features_dc": color[:, None, :].contiguous(),
                  "_features_rest": torch.zeros((n, (self.max_sh_degree + 1) ** 2 - 1, 3), dtype=torch.float32, device=device),
                  "_scaling": scales, "_rotation": rots, "_opacity": torch.full((n, 1), logit, dtype=torch.float32, device=device)}
        for k, t in leaves.items():
            setattr(self, k, nn.Parameter(t.contiguous().requires_grad_(True)))
        self.max_radii2D = torch.zeros((n,), device=device)
        self.xyz_gradient_accum = torch.zeros((n, 1), device=device)
        self.denom = torch.zeros((n, 1), device=device)

    def load_ply(self, path, device="cuda", spatial_sort: Optional[bool] = None, face_centers=None, **kwargs):
        """scene/gaussian_model.py:282-332: leaf tensors from the reference's PLY (binding -> int32).  `spatial_sort` (round 4: ON by
        default, `GAA_SPATIAL_SORT=0` or `spatial_sort=False` keep the file's order): the splats in Morton order of their positions
        (io.spatial_sort; a bound model passes the template's face centres) -- same images, every per-splat tensor permuted the same way
        (row i is then NOT the file's row i), the binning pass of large models ~1.6 x faster because a workgroup's consecutive splats share
        tiles.  save_ply writes whatever order the model is in."""
        from . import io as gio

        arrs = gio.load_ply(str(path), self.max_sh_degree)
        if spatial_sort is None:
            spatial_sort = spatial_order_default()
        self._gaa_order = None
        if spatial_sort:
            arrs, order = gio.spatial_sort(arrs, face_centers, return_order=True)
            self._gaa_order = torch.as_tensor(np.asarray(order), dtype=torch.long)   # row i of the model = row _gaa_order[i] of the file (the permutation is kept)
        self.load_arrays(arrs, device=device)

    def save_ply(self, path):
        """scene/gaussian_model.py:253-275"""
        from . import io as gio

        arrs = {k: getattr(self, k).detach().cpu().numpy() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
        if self.binding is not None:
            arrs["binding"] = self.binding.detach().cpu().numpy()
        gio.save_ply(str(path), arrs)

    # ---- accessors (scene/gaussian_model.py:113-160, composed torch; rebound to the fused kernels below) ----------
    @property
    def get_scaling(self):
        if self.binding is None:
            return torch.exp(self._scaling)
        if self.face_scaling is None:
            self.select_mesh_by_timestep(0)
        return unfused.bind_scaling(self._scaling, self.binding, self.face_scaling)

    @property
    def get_rotation(self):
        if self.binding is None:
            return torch.nn.functional.normalize(self._rotation)
        if self.face_orien_quat is None:
            self.select_mesh_by_timestep(0)
        return unfused.bind_rotation(self._rotation, self.binding, self.face_orien_quat)

    @property
    def get_xyz(self):
        if self.binding is None:
            return self._xyz
        if self.face_center is None:
            self.select_mesh_by_timestep(0)
        return unfused.bind_xyz(self._xyz, self.binding, self.face_orien_mat, self.face_scaling, self.face_center)

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        # python cov3D path (pipe.compute_cov3D_python, default off): like the reference (:162-163) it
        # uses the LOCAL rotation, which is only right for un-bound splats.
        s = scaling_modifier * self.get_scaling
        q = self._rotation / self._rotation.norm(dim=1, keepdim=True)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
        L = R * s[:, None, :]
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)

    def select_mesh_by_timestep(self, timestep):
        raise NotImplementedError

    def update_densification_stats(self, viewspace_point_tensor, radii):
        """The two statistics lines of a training iteration, train.py:197-198, as one launch (include/gls.h):
            self.max_radii2D[vis] = max(self.max_radii2D[vis], radii[vis])          # train.py:197
            self.add_densification_stats(viewspace_point_tensor, vis)              # gaussian_model.py:517-519
        with vis = radii > 0 (render()'s visibility_filter)."""
        from .loss import densification_stats

        if viewspace_point_tensor.grad is None:
            raise RuntimeError("viewspace_point_tensor has no .grad: call backward() first")
        densification_stats(radii, viewspace_point_tensor.grad, self.max_radii2D, self.xyz_gradient_accum, self.denom)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- optimiser surgery and densification (scene/gaussian_model.py:277-280, 349-398, 501-515; training_setup: _TrainingSetup above) ----
    def _prune_optimizer(self, mask):
        from . import densify

        return densify.prune_optimizer(self.optimizer, mask)

    def prune_points(self, mask):
        from . import densify

        densify.prune_points(self, mask)

    def reset_opacity(self):
        from . import densify

        densify.reset_opacity(self)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, noise=None):
        """scene/gaussian_model.py:501-515 through densify.densify_and_prune: five launches and one host read on device tensors."""
        from . import densify

        densify.densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, noise=noise)

    densify_and_prune._gaa_fused = True   # patch._hook_spatial_order: already the fused entry, only the re-sort is added


class FlameHead(nn.Module):
    """Buffers + forward of the reference FlameHead (flame_model/flame.py:83-184, 485-558) on a rig given
    as arrays (the licensed flame2023.pkl is not available; gaussianavatars_amd.synthetic.flame_rig
    produces the same schema)."""

    def __init__(self, rig: Dict[str, np.ndarray], impl: str = "fused"):
        super().__init__()
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
            self.register_buffer(k, torch.as_tensor(rig[k], dtype=torch.float32).contiguous())
        self.register_buffer("parents", torch.as_tensor(rig["parents"], dtype=torch.long))
        self.register_buffer("faces", torch.as_tensor(rig["faces"], dtype=torch.long), persistent=False)
        self.n_shape_params = 300
        self.n_expr_params = self.shapedirs.shape[2] - 300
        self.impl = impl
        if "full_lmk_faces_idx" in rig and "full_lmk_bary_coords" in rig:
            self.attach_landmarks(rig["full_lmk_faces_idx"], rig["full_lmk_bary_coords"])

    def attach_landmarks(self, lmk_faces_idx, lmk_bary_coords):
        """The landmark embedding of flame.py:131-143 (landmark_embedding_with_eyes.npy: `full_lmk_faces_idx`, `full_lmk_bary_coords`), as
        (L,) / (L,3) or in the reference's (1,L) / (1,L,3): checked against `faces` here, on the host, once, and registered as the two
        buffers the reference registers -- (L,) long and (L,3) fp32."""
        from .binding import check_landmark_embedding

        idx, bary = check_landmark_embedding(self.faces, lmk_faces_idx, lmk_bary_coords)
        dev = self.faces.device
        self.register_buffer("full_lmk_faces_idx", idx.to(dev))
        self.register_buffer("full_lmk_bary_coords", bary.to(dev))
        return self

    def forward(self, shape, expr, rotation, neck, jaw, eyes, translation, zero_centered_at_root_node=False,
                return_landmarks=True, return_verts_cano=False, static_offset=None, dynamic_offset=None):
        rig = dict(v_template=self.v_template, shapedirs=self.shapedirs, posedirs=self.posedirs,
                   J_regressor=self.J_regressor, lbs_weights=self.lbs_weights, parents=self.parents)
        if not (zero_centered_at_root_node or return_landmarks):   # the per-frame call of GaussianAvatars
            verts, v_shaped = unfused.flame_forward(rig, shape, expr, rotation, neck, jaw, eyes, translation, static_offset)
            return [verts, v_shaped] if return_verts_cano else verts
        if return_landmarks and getattr(self, "full_lmk_faces_idx", None) is None:
            raise ValueError("return_landmarks=True (the default) needs a landmark embedding: call attach_landmarks(lmk_faces_idx, "
                             "lmk_bary_coords) first, or pass return_landmarks=False")
        verts, v_shaped = unfused.flame_forward(rig, shape, expr, rotation, neck, jaw, eyes, translation, static_offset,
                                                zero_centered_at_root_node=zero_centered_at_root_node)
        ret = [verts]                                               # flame.py:539-558: [vertices, (v_shaped), (landmarks)]
        if return_verts_cano:
            ret.append(v_shaped)
        if return_landmarks:
            ret.append(unfused.landmarks(verts, self.faces, self.full_lmk_faces_idx, self.full_lmk_bary_coords))
        return ret if len(ret) > 1 else ret[0]


class FlameGaussianModel(GaussianModel):
    """Mesh-update surface of scene/flame_gaussian_model.py:22-41,91-154."""

    def __init__(self, sh_degree: int, rig: Dict[str, np.ndarray], disable_flame_static_offset=False,
                 not_finetune_flame_params=False, n_shape=300, n_expr=100, binding_impl: str = "fused", device="cuda"):
        super().__init__(sh_degree, binding_impl=binding_impl)
        self.disable_flame_static_offset = disable_flame_static_offset
        self.not_finetune_flame_params = not_finetune_flame_params
        self.n_shape, self.n_expr = n_shape, n_expr
        self.flame_model = FlameHead(rig, impl=binding_impl).to(device)
        self.flame_param = None
        self.flame_param_orig = None
        if self.binding is None:
            nf = len(self.flame_model.faces)
            self.binding = torch.arange(nf, device=device)
            self.binding_counter = torch.ones(nf, dtype=torch.int32, device=device)

    def training_setup(self, training_args):
        """scene/flame_gaussian_model.py:174-207: the splat groups plus the pose, translation and expression groups of the FLAME parameters."""
        super().training_setup(training_args)
        if self.not_finetune_flame_params:
            return
        fp = self.flame_param
        for k in ("rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation", "expr"):
            fp[k].requires_grad = True
        self.optimizer.add_param_group({"params": [fp["rotation"], fp["neck_pose"], fp["jaw_pose"], fp["eyes_pose"]],
                                        "lr": training_args.flame_pose_lr, "name": "pose"})
        self.optimizer.add_param_group({"params": [fp["translation"]], "lr": training_args.flame_trans_lr, "name": "trans"})
        self.optimizer.add_param_group({"params": [fp["expr"]], "lr": training_args.flame_expr_lr, "name": "expr"})

    def load_flame_param(self, arrs: Dict[str, np.ndarray], device="cuda", requires_grad: bool = False):
        """flame_param.npz schema (scene/flame_gaussian_model.py:61-71,229-237)."""
        fp = {k: torch.as_tensor(v, dtype=torch.float32, device=device) for k, v in arrs.items()}
        if requires_grad:  # the rows train.py puts in Adam groups (:186-207)
            for k in ("rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation", "expr"):
                fp[k].requires_grad_(True)
        self.flame_param = fp
        self.num_timesteps = fp["expr"].shape[0]

    def load_ply(self, path, device="cuda", spatial_sort: Optional[bool] = None, **kwargs):
        """scene/flame_gaussian_model.py:226-269: the PLY plus the flame_param.npz stored next to it.  `spatial_sort`: as GaussianModel.load_ply
        (default on), by the template centre of each splat's face.  `motion_path` (:239-258): an npz whose seven per-timestep entries replace
        the dynamic FLAME parameters, `shape` and `static_offset` staying.  `disable_fid` (:260-269): the splats bound to the listed faces are
        dropped -- from the leaves and the binding like the reference, and from everything else that has a row per splat."""
        import os

        from . import io as gio

        if spatial_sort is None:
            spatial_sort = spatial_order_default()
        super().load_ply(path, device=device, spatial_sort=spatial_sort, face_centers=template_face_centers(self) if spatial_sort else None)
        if not kwargs.get("has_target", False):
            self.load_flame_param(gio.load_flame_param(os.path.join(os.path.dirname(str(path)), "flame_param.npz")), device=device)
        if kwargs.get("motion_path") is not None:
            motion = gio.load_flame_param(str(kwargs["motion_path"]))
            fp = {k: self.flame_param[k] for k in ("shape", "static_offset")}
            for k in ("translation", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "expr", "dynamic_offset"):
                fp[k] = torch.as_tensor(motion[k], dtype=torch.float32, device=device)
            self.flame_param = fp
            self.num_timesteps = fp["expr"].shape[0]
        disable_fid = kwargs.get("disable_fid")
        if disable_fid is not None and len(disable_fid) > 0:
            fid = torch.as_tensor(disable_fid, device=self.binding.device).reshape(-1).to(self.binding.dtype)
            keep = (self.binding[:, None] != fid[None, :]).all(-1)
            n = keep.shape[0]
            for attr in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
                p = getattr(self, attr)
                setattr(self, attr, nn.Parameter(p.detach()[keep].contiguous().requires_grad_(p.requires_grad)))
            self.binding = self.binding[keep]
            self.binding_counter = torch.bincount(self.binding.long(), minlength=self.binding_counter.shape[0]).to(self.binding_counter.dtype)
            # what prune_points keeps in step with the leaves (densify.prune_points), and the file-row permutation of the spatial order
            self.xyz_gradient_accum, self.denom, self.max_radii2D = self.xyz_gradient_accum[keep], self.denom[keep], self.max_radii2D[keep]
            order = getattr(self, "_gaa_order", None)
            if isinstance(order, torch.Tensor):
                self._gaa_order = order[keep.to(order.device)] if order.shape[0] == n else None

    def save_ply(self, path):
        """scene/flame_gaussian_model.py:219-224"""
        import os

        from . import io as gio

        super().save_ply(path)
        gio.save_flame_param(os.path.join(os.path.dirname(str(path)), "flame_param.npz"),
                             {k: v.detach().cpu().numpy() for k, v in self.flame_param.items()})

    def update_mesh_by_param_dict(self, flame_param):
        shape = flame_param["shape"] if "shape" in flame_param else self.flame_param["shape"]
        static_offset = flame_param["static_offset"] if "static_offset" in flame_param else self.flame_param["static_offset"]
        dev = self.flame_model.v_template.device
        verts, verts_cano = self.flame_model(
            shape[None, ...], flame_param["expr"].to(dev), flame_param["rotation"].to(dev), flame_param["neck"].to(dev),
            flame_param["jaw"].to(dev), flame_param["eyes"].to(dev), flame_param["translation"].to(dev),
            zero_centered_at_root_node=False, return_landmarks=False, return_verts_cano=True, static_offset=static_offset)
        self.update_mesh_properties(verts, verts_cano)

    def select_mesh_by_timestep(self, timestep, original=False):
        self.timestep = timestep
        fp = self.flame_param_orig if original and self.flame_param_orig is not None else self.flame_param
        verts, verts_cano = self.flame_model(
            fp["shape"][None, ...], fp["expr"][[timestep]], fp["rotation"][[timestep]], fp["neck_pose"][[timestep]],
            fp["jaw_pose"][[timestep]], fp["eyes_pose"][[timestep]], fp["translation"][[timestep]],
            zero_centered_at_root_node=False, return_landmarks=False, return_verts_cano=True,
            static_offset=fp["static_offset"], dynamic_offset=fp["dynamic_offset"][[timestep]])
        self.update_mesh_properties(verts, verts_cano)

    def update_mesh_properties(self, verts, verts_cano):
        faces = self.flame_model.faces
        c, R, s, q = unfused.face_frames(verts.squeeze(0), faces)
        self.face_center, self.face_orien_mat, self.face_scaling, self.face_orien_quat = c, R, s, q
        self.verts = verts
        self.faces = faces
        self.verts_cano = verts_cano


# The same rebinding `patch_reference()` applies to the reference's classes (gaussianavatars_amd/patch.py).
from .patch import patch_classes as _patch_classes  # noqa: E402

_patch_classes(GaussianModel, FlameGaussianModel, FlameHead)


def spatial_order_default() -> bool:
    """Whether loaders (and the densification hook of patch.py) keep the splats in Morton order of their positions: yes unless
    GAA_SPATIAL_SORT=0.  A layout choice -- the rasterizer's outputs do not depend on the order of the splats -- that decides how far apart in
    time the binning pass writes the entries of one tile (492 -> 141 MB written per frame at 2 M splats)."""
    import os

    return os.environ.get("GAA_SPATIAL_SORT", "1") != "0"


def template_face_centers(model):
    """(F,3) numpy: centres of the faces of the model's template mesh (flame_model.v_template / .faces), None for a model without a mesh."""
    fm = getattr(model, "flame_model", None)
    if fm is None or not hasattr(fm, "v_template") or not hasattr(fm, "faces"):
        return None
    v = fm.v_template.detach().cpu().numpy().reshape(-1, 3)
    f = fm.faces.detach().cpu().numpy().astype(np.int64).reshape(-1, 3)
    return v[f].mean(1)


def _device_face_centers(model, dev):
    """template_face_centers as an (F, 3) fp32 tensor on `dev`, built and uploaded once per template and kept with the model; None for a model
    without a mesh, or whose template is not fp32 (the host statement then computes the positions in another precision)."""
    fm = getattr(model, "flame_model", None)
    if fm is None or not hasattr(fm, "v_template") or not hasattr(fm, "faces"):
        return None
    key = (fm.v_template.data_ptr(), fm.v_template._version, fm.faces.data_ptr(), fm.faces._version, str(dev))
    held = getattr(model, "_gaa_face_centers", None)
    if held is None or held[0] != key:
        centers = template_face_centers(model)
        held = (key, torch.from_numpy(np.ascontiguousarray(centers)).to(dev) if centers.dtype == np.float32 else None)
        model._gaa_face_centers = held
    return held[1]


def _spatial_resort_fused(model):
    """spatial_resort on the kernels of include/gdc.h (ABI 2) when the model is inside their domain, else None: one densify.morton_permutation
    and one densify.permute_rows over the six leaves, the moments the optimizer holds for them, the three statistics, `binding` and a tracked
    `_gaa_order` (23 tensors at most), installed the way densify._install and densify.prune_optimizer do.  Nothing is copied to the host and
    nothing synchronises."""
    import os

    from . import _lib, densify

    if os.environ.get("GAA_FUSED_RESORT", "1") == "0":
        return None
    xyz = getattr(model, "_xyz", None)
    if not isinstance(xyz, torch.Tensor) or xyz.device.type != "cuda" or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] >= _lib.GDC_MAX_SPLATS:
        return None
    dev, P = xyz.device, xyz.shape[0]
    if torch.cuda.is_current_stream_capturing():
        return None
    attrs = tuple(densify.SPLAT_GROUPS.values())
    if not all(densify._dense(getattr(model, a, None), dev) and getattr(model, a).shape[0] == P for a in attrs):
        return None
    binding = getattr(model, "binding", None)
    centers = None
    if binding is not None:
        if not isinstance(binding, torch.Tensor) or binding.dtype not in (torch.int32, torch.int64) or not densify._dense(binding, dev, binding.dtype) \
                or binding.shape != (P,):
            return None
        fm = getattr(model, "flame_model", None)
        if fm is not None and hasattr(fm, "v_template") and hasattr(fm, "faces"):
            centers = _device_face_centers(model, dev)
            if centers is None:
                return None
    optimizer = getattr(model, "optimizer", None)
    groups = None
    if optimizer is not None:
        groups = densify._splat_groups(optimizer)
        if groups is None or any(g["params"][0] is not getattr(model, a) for a, g in groups.items()):
            return None
    names, tensors = [], []
    for a in attrs:
        names.append(a)
        tensors.append(getattr(model, a).detach())
        state = optimizer.state.get(getattr(model, a)) if groups is not None else None
        if state:
            # Adam's two moments and nothing else per row: any other state (another optimizer's buffers, amsgrad's maximum) is the host path's
            if "exp_avg" not in state or "exp_avg_sq" not in state:
                return None
            if any(isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == P for k, v in state.items() if k not in ("exp_avg", "exp_avg_sq")):
                return None
            for key in ("exp_avg", "exp_avg_sq"):
                if not densify._dense(state[key], dev) or state[key].shape != getattr(model, a).shape:
                    return None
                names.append((a, key))
                tensors.append(state[key])
    for aux in ("xyz_gradient_accum", "denom", "max_radii2D"):
        t = getattr(model, aux, None)
        if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == P:
            if not densify._dense(t, dev):
                return None
            names.append(aux)
            tensors.append(t)
    if binding is not None:
        names.append("binding")
        tensors.append(binding)
    prev = getattr(model, "_gaa_order", None)
    tracked = isinstance(prev, torch.Tensor) and prev.shape[0] == P
    if tracked:
        if prev.dtype not in (torch.int32, torch.int64) or prev.dim() != 1:
            return None
        names.append("_gaa_order")
        tensors.append(prev.to(dev).contiguous())
    with torch.no_grad():
        perm32 = densify._morton_i32(xyz, binding if centers is not None else None, centers)
        moved = dict(zip(names, densify.permute_rows(tensors, perm32)))
        perm = perm32.long()
        for a in attrs:
            old = getattr(model, a)
            p = nn.Parameter(moved[a], requires_grad=old.requires_grad)
            if groups is not None:
                state = optimizer.state.get(old)
                if state is not None:
                    del optimizer.state[old]
                    if (a, "exp_avg") in moved:
                        state["exp_avg"], state["exp_avg_sq"] = moved[(a, "exp_avg")], moved[(a, "exp_avg_sq")]
                    optimizer.state[p] = state
                groups[a]["params"][0] = p
            setattr(model, a, p)
        for aux in ("xyz_gradient_accum", "denom", "max_radii2D", "binding"):
            if aux in moved:
                setattr(model, aux, moved[aux])
        if tracked:
            model._gaa_order = moved["_gaa_order"]
        elif prev is None and not getattr(model, "_gaa_order_lost", False):
            model._gaa_order = perm.clone()
        else:
            model._gaa_order = None
            model._gaa_order_lost = True
    return perm


def spatial_resort(model, fused: Optional[bool] = None) -> torch.Tensor:
    """Puts the splats of a LIVE model -- this package's classes or the reference's own -- into Morton order of their positions
    (io.spatial_sort) and returns the permutation.  Densification appends its new splats (scene/gaussian_model.py:426-515), so a model that
    was loaded in order drifts out of it; this is the re-sort.  Everything that is indexed by splat moves together: the six leaf
    parameters, with an optimiser attached their Adam moments too -- through the reference's own `_prune_optimizer` (:349-371), which indexes
    parameters and moments with whatever it is given: a permutation instead of a keep-mask --, the densification statistics
    (xyz_gradient_accum, denom, max_radii2D) and the binding.  Recorded steps (graphs.py) must be captured again afterwards.

    A model of contiguous fp32 device tensors (binding / `_gaa_order` integer) takes the kernels of include/gdc.h instead -- the same
    permutation and the same rows, bit for bit, without a copy to the host or a synchronisation (_spatial_resort_fused);
    GAA_FUSED_RESORT=0 or `fused=False` keep the host statement below, which is also what runs anywhere outside that domain."""
    if fused is None or fused:
        perm = _spatial_resort_fused(model)
        if perm is not None:
            return perm
    from . import io as gio

    with torch.no_grad():
        binding = getattr(model, "binding", None)
        arrs = {"_xyz": model._xyz.detach().cpu().numpy(), "binding": None if binding is None else binding.detach().cpu().numpy()}
        centers = template_face_centers(model) if binding is not None else None
        pos = arrs["_xyz"] if centers is None else centers[arrs["binding"].astype(np.int64)] + 1e-3 * arrs["_xyz"]
        perm = torch.as_tensor(gio.morton_order(pos), dtype=torch.long, device=model._xyz.device)
        names = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
        if getattr(model, "optimizer", None) is not None and hasattr(model, "_prune_optimizer"):
            moved = model._prune_optimizer(perm)
            for group, attr in names.items():
                setattr(model, attr, moved[group])
        else:
            for attr in names.values():
                p = getattr(model, attr)
                setattr(model, attr, nn.Parameter(p.detach()[perm].contiguous().requires_grad_(p.requires_grad)))
        n = perm.shape[0]
        for aux in ("xyz_gradient_accum", "denom", "max_radii2D"):
            t = getattr(model, aux, None)
            if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == n:
                setattr(model, aux, t[perm])
        if binding is not None:
            model.binding = binding[perm]
        # the order is recorded: row i of the model is row `_gaa_order[i]` of what was loaded (composed over every re-sort since; densification's new
        # splats get -1), so that tools matching splats by index across PLYs / checkpoints can undo it
        # (`inv = torch.empty_like(o); inv[o] = arange`: row j of the file is row inv[j] of the model)
        prev = getattr(model, "_gaa_order", None)
        if isinstance(prev, torch.Tensor) and prev.shape[0] == n:
            model._gaa_order = prev.to(perm.device)[perm]
        elif prev is None and not getattr(model, "_gaa_order_lost", False):
            model._gaa_order = perm.clone()          # first sort of a freshly loaded model: the file's order is the order it had until now
        else:
            # the row count changed without the rows being followed (patch._hook_spatial_order follows the reference's prune_points /
            # densification_postfix; anything else does not): no permutation is better than one that names the wrong rows
            model._gaa_order = None
            model._gaa_order_lost = True
    return perm
