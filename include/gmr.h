/*
 * gmr.h -- C ABI of the mesh rasterizer ("Gaussian avatars mesh rasterizer"): the triangle rasterizer and the analytic
 * antialias behind the FLAME mesh overlay (mesh_renderer/__init__.py: NVDiffRenderer.render_mesh, which calls
 * nvdiffrast's rasterize and antialias).  Forward only: no caller of the overlay needs a gradient.
 *
 *   gmr_rasterize   instanced mode: pos (B,V,4) clip space, tri (F,3) -> rast (B,H,W,4) = (u, v, z/w, triangle_id + 1),
 *                   zeros where nothing covers.  Pixel (x, y) samples NDC ((2x+1)/W - 1, (2y+1)/H - 1): row 0 is NDC y = -1.
 *   gmr_antialias   analytic silhouette blending of color (B,H,W,C) along the id boundaries of rast (Laine et al. 2020).
 *
 * The contract (barycentrics, fragment test, depth order, the blend) is DESIGN.md section 10.  Conventions as gls.h:
 * DEVICE pointers, fp32 / int32, contiguous; 0 / <0 return codes with gmr_last_error(); everything is enqueued on `stream`,
 * nothing synchronises.  No float atomics and no order-dependent reduction: results are bitwise reproducible.
 * The caller validates tri indices against [0, V) (the kernels also treat an out-of-range index as an empty triangle).
 */
#ifndef GMR_H
#define GMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMR_ABI_VERSION 2   /* 2: the shaded overlay of gmr_overlay.h, included below */
#define GMR_OK 0
#define GMR_E_ARG (-1)
#define GMR_E_HIP (-2)
#define GMR_MAX_TRIANGLES 16777215   /* 2^24 - 1: triangle_id + 1 is stored as an exact float */

int gmr_abi_version(void);
const char* gmr_last_error(void);

/* bytes of `workspace` gmr_rasterize needs for B batch elements of F triangles (per-triangle setup records); >= 0 */
int64_t gmr_workspace_bytes(int32_t B, int32_t F);

/* pos: (B,V,4) float; tri: (F,3) int32; rast: (B,H,W,4) float, fully written; workspace: gmr_workspace_bytes(B, F) bytes,
 * 16-byte aligned (may be NULL when that is 0).  F may be 0 (rast is all zeros).  B*H*W < 2^31. */
int gmr_rasterize(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float* pos, const int32_t* tri, float* rast,
                  void* workspace, void* stream);

/* color: (B,H,W,C) float; rast: (B,H,W,4) as gmr_rasterize writes it (an id outside [1, F] counts as empty); pos, tri as above;
 * neighbours: (F,3) int32, for edge k = (tri[f][k], tri[f][(k+1)%3]) of triangle f the other triangle on that edge, -1 for a
 * boundary edge, -2 for an edge of more than two triangles; out: (B,H,W,C), fully written (must not alias color). */
int gmr_antialias(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, int32_t C, const float* color, const float* rast,
                  const float* pos, const int32_t* tri, const int32_t* neighbours, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#include "gmr_overlay.h"   /* ABI 2: prepare, shade, resize / flip and compose, the rest of the overlay around the two calls above */

#endif /* GMR_H */
