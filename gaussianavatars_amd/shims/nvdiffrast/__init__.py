"""`nvdiffrast` stand-in: the reference imports it eagerly (mesh_renderer/__init__.py:10, instantiated at train.py:40 and
render.py:33) but uses it only for the mesh overlay (`--render_mesh`, the viewers' `show_mesh`), which is off the splat hot path: `rasterize` and
`antialias` run on gaussianavatars_amd.mesh_raster."""
from . import torch  # noqa: F401
