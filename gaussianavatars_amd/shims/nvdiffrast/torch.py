"""Contexts construct (NVDiffRenderer() is built at import time of train.py / render.py); `rasterize` and `antialias` run on the HIP
mesh rasterizer (gaussianavatars_amd.mesh_raster, include/gmr.h) in the form NVDiffRenderer.render_mesh calls them: instanced mode,
forward only, rast_db empty.  `interpolate` and `texture` raise: no reference caller uses them."""


class _Ctx:
    def __init__(self, *a, **k):
        pass


class RasterizeCudaContext(_Ctx):
    pass


class RasterizeGLContext(_Ctx):
    pass


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    from gaussianavatars_amd import mesh_raster

    return mesh_raster.rasterize(glctx, pos, tri, resolution, ranges=ranges, grad_db=grad_db)


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    from gaussianavatars_amd import mesh_raster

    return mesh_raster.antialias(color, rast, pos, tri, topology_hash=topology_hash, pos_gradient_boost=pos_gradient_boost)


rasterize.__doc__ = "nvdiffrast.torch.rasterize on gaussianavatars_amd.mesh_raster.rasterize (see there)."
antialias.__doc__ = "nvdiffrast.torch.antialias on gaussianavatars_amd.mesh_raster.antialias (see there)."


def _unavailable(name):
    def f(*a, **k):
        raise RuntimeError(f"nvdiffrast.torch.{name}: not provided by this stand-in (only rasterize and antialias, which the mesh "
                           "overlay uses, are); it needs the real nvdiffrast, which is CUDA-only")
    f.__name__ = name
    return f


interpolate = _unavailable("interpolate")
texture = _unavailable("texture")
