/*
 * gmr_overlay.h -- the shaded half of the mesh overlay, ABI 2 of libgmr_hip.so (included by gmr.h): everything
 * NVDiffRenderer.render_from_camera / render_mesh (mesh_renderer/__init__.py) does around rasterize and antialias, and the viewer's
 * blend of the mesh over the splat image.  Forward only.  Conventions as gmr.h: DEVICE pointers, fp32 / int32, contiguous, 0 / <0
 * return codes with gmr_last_error(), everything enqueued on `stream`, nothing synchronises, no float atomics: bitwise reproducible.
 * (A header of its own: tests/test_mesh_raster_cpu.py pins the declarations of gmr.h itself to the five of ABI 1.)
 *
 *   gmr_mesh_prepare      verts (B,V,3) world space -> pos_clip (B,V,4) for gmr_rasterize and the camera-space face normals (B,F,3)
 *   gmr_mesh_shade        rast -> albedo, normal, diffuse (B,H,W,3) and the pre-antialias rgba (B,H,W,4), background included
 *   gmr_resize_flip       up to GMR_MAX_MAPS images (B,h,w,C) -> (B,H,W,C): vertical flip, then bilinear resize, in one pass
 *   gmr_compose_overlay   mesh rgba over the splat image, as floats (3,H,W) or as the bytes (H,W,3) the viewer receives
 */
#ifndef GMR_OVERLAY_H
#define GMR_OVERLAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMR_LIGHT_CONSTANT 0   /* diffuse = 1 */
#define GMR_LIGHT_FRONT 1      /* diffuse = clamp(normal.z, 0, 1): a light at the camera */
#define GMR_MAT_ROWS 0         /* rt (B,rt_rows,4), mvp (B,4,4) row-major, applied to column vectors: out[j] = sum_k M[j][k] p[k] */
#define GMR_MAT_CAMERA 1       /* rt, mvp are a camera's world_view_transform / full_proj_transform as it stores them (B,4,4), for row
                                  vectors; the y and z axes of the view and the y axis of the projection are negated while loading:
                                  M[j][k] = s_j * stored[k][j], s = (1,-1,-1,1) for rt and (1,-1,1,1) for mvp */
#define GMR_MAX_MAPS 4

typedef struct GmrMap {
    const float* src;   /* (B,h,w,C) */
    float* dst;         /* (B,H,W,C), fully written, must not alias src */
    int32_t C;          /* >= 1 */
} GmrMap;

/* Per vertex p = (x, y, z, 1): pos_clip = mvp p, each component fma(1, m3, fma(z, m2, fma(y, m1, x * m0))) in fp32, the order of an fp32
 * GEMM.  Per face: n = cross(c1 - c0, c2 - c0) of its camera-space vertices c = (rt p).xyz, then n / sqrt(max(n.n, 1e-20)), in fp32.
 * A face with an index outside [0, V) gets a zero normal.  rt_rows is 3 or 4 (only three rows are read).  V or F may be 0. */
int gmr_mesh_prepare(int32_t B, int32_t V, int32_t F, const float* verts, const int32_t* tri, const float* rt, int32_t rt_rows,
                     const float* mvp, int32_t mat_mode, float* pos_clip, float* face_normals, void* stream);

/* Per pixel, with id = rast.w: fg = clamp(id, 0, 1) != 0, f = min(max((int)id - 1, 0), F - 1);  albedo = face_colors[b][f] (ones when
 * face_colors is NULL or F == 0), whether fg or not;  d = 1 or clamp(face_normals[b][f].z, 0, 1);  the background is (bg_r, bg_g, bg_b),
 * or bg_image[b][H - 1 - y][x] when bg_image (B,H,W,3) is not NULL.  fg: normal = face_normals[b][f], diffuse = (d, d, d),
 * rgba = (albedo * d, 1);  otherwise normal = diffuse = background, rgba = (background, 0).  With F == 0 nothing is fg. */
int gmr_mesh_shade(int32_t B, int32_t F, int32_t H, int32_t W, const float* rast, const float* face_normals, const float* face_colors,
                   int32_t lighting, float bg_r, float bg_g, float bg_b, const float* bg_image, float* albedo, float* normal,
                   float* diffuse, float* rgba, void* stream);

/* dst[b][Y][X] = bilinear sample (align_corners = false: source coordinate max(scale * (i + 0.5) - 0.5, 0), scale = in / out, the
 * neighbour index clamped at the border) of the vertically flipped source, src[b][h - 1 - y][x].  With h == H and w == W it is the flip
 * alone, copied bit for bit.  All n_maps (1 .. GMR_MAX_MAPS) images share B, h, w, H, W and go in one launch; `maps` is HOST memory. */
int gmr_resize_flip(int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, int32_t n_maps, const GmrMap* maps, void* stream);

/* rgba: (H,W,4) mesh image; splat: (3,H,W) or NULL.  net = (rgb * a) * opacity + splat * (a * one_minus_opacity + (1 - a)), every
 * operation rounded once in fp32 in that order (one_minus_opacity is passed, not derived: the caller forms 1 - opacity in double);
 * net = rgb when splat is NULL.  Exactly one of out (3,H,W) float and out_bytes (H,W,3) uint8 is not NULL; the bytes are
 * (uint8)(min(max(net, 0), 1) * 255), truncating. */
int gmr_compose_overlay(int32_t H, int32_t W, const float* splat, const float* rgba, float opacity, float one_minus_opacity, float* out,
                        uint8_t* out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GMR_OVERLAY_H */
