// gmr_overlay.h -- the shaded half of the mesh overlay (include/gmr_overlay.h); part of gmr_kernels.hip's
// translation unit (-ffp-contract=off: the roundings are the ones the header lists).
//
// k_mesh_prepare    one thread per vertex and per face of a batch element: clip-space position; camera-space face normal
// k_mesh_shade      one pixel per lane: a float4 load of rast, three 3-channel maps and one float4 store of rgba
// k_resize_flip     one output pixel per lane, blockIdx.y = the map: flip + bilinear resize (or the bitwise flip at equal sizes)
// k_compose_overlay one pixel per lane: a float4 load of the mesh rgba, three planar loads of the splat image
//
// Streaming kernels: no LDS, no scratch, no atomics; every index is bounded by the launch shape or clamped before it is used.
#pragma once

namespace gmr {

// rows 0..2 of the matrix of batch element b in GMR_MAT_ROWS form, whatever form it is stored in (uniform over the workgroup)
__device__ __forceinline__ void load_rows(const float* __restrict__ M, int b, int rows, int mode, float s1, float s2, float out[][4], int n)
{
    const float* p = M + (size_t)b * (mode == GMR_MAT_CAMERA ? 16 : rows * 4);
    for (int j = 0; j < n; ++j) {
        const float s = j == 1 ? s1 : (j == 2 ? s2 : 1.f);
        for (int k = 0; k < 4; ++k) out[j][k] = mode == GMR_MAT_CAMERA ? s * p[k * 4 + j] : p[j * 4 + k];
    }
}

// row . (x, y, z, 1) as an fp32 GEMM accumulates it: one product, then a fused multiply-add per further term, in index order (the bits of
// torch.bmm on the host; explicit fmaf, this TU does not contract on its own)
__device__ __forceinline__ float row_dot(const float r[4], float x, float y, float z)
{
    return fmaf(1.f, r[3], fmaf(z, r[2], fmaf(y, r[1], x * r[0])));
}

__global__ __launch_bounds__(NT) void k_mesh_prepare(int32_t V, int32_t F, const float* __restrict__ verts, const int32_t* __restrict__ tri,
                                                     const float* __restrict__ rt, int32_t rt_rows, const float* __restrict__ mvp,
                                                     int32_t mode, float4* __restrict__ pos_clip, float* __restrict__ face_normals)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < V) {
        float P[4][4];
        load_rows(mvp, b, 4, mode, -1.f, 1.f, P, 4);
        const float* p = verts + ((size_t)b * V + i) * 3;
        const float x = p[0], y = p[1], z = p[2];
        pos_clip[(size_t)b * V + i] = make_float4(row_dot(P[0], x, y, z), row_dot(P[1], x, y, z), row_dot(P[2], x, y, z), row_dot(P[3], x, y, z));
    }
    if (i < F) {
        float R[3][4];
        load_rows(rt, b, rt_rows, mode, -1.f, -1.f, R, 3);
        const int i0 = tri[3 * (size_t)i], i1 = tri[3 * (size_t)i + 1], i2 = tri[3 * (size_t)i + 2];
        float n[3] = {0.f, 0.f, 0.f};
        if (in_range(i0, V) && in_range(i1, V) && in_range(i2, V)) {
            float c[3][3];
            const int idx[3] = {i0, i1, i2};
            for (int k = 0; k < 3; ++k) {
                const float* p = verts + ((size_t)b * V + idx[k]) * 3;
                for (int j = 0; j < 3; ++j) c[k][j] = row_dot(R[j], p[0], p[1], p[2]);
            }
            const float ax = c[1][0] - c[0][0], ay = c[1][1] - c[0][1], az = c[1][2] - c[0][2];
            const float bx = c[2][0] - c[0][0], by = c[2][1] - c[0][1], bz = c[2][2] - c[0][2];
            const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const float len = sqrtf(fmaxf((nx * nx + ny * ny) + nz * nz, 1e-20f));
            n[0] = nx / len;
            n[1] = ny / len;
            n[2] = nz / len;
        }
        float* o = face_normals + ((size_t)b * F + i) * 3;
        o[0] = n[0];
        o[1] = n[1];
        o[2] = n[2];
    }
}

__device__ __forceinline__ void store3(float* __restrict__ p, float a, float b, float c)
{
    p[0] = a;
    p[1] = b;
    p[2] = c;
}

__global__ __launch_bounds__(NT) void k_mesh_shade(int32_t B, int32_t F, int32_t H, int32_t W, const float4* __restrict__ rast,
                                                   const float* __restrict__ face_normals, const float* __restrict__ face_colors,
                                                   int32_t lighting, float bg_r, float bg_g, float bg_b, const float* __restrict__ bg_image,
                                                   float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ diffuse,
                                                   float4* __restrict__ rgba)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= (int64_t)B * HW) return;
    const int b = (int)(g / HW);
    const int y = (int)((g % HW) / W), x = (int)(g % W);
    const float id = rast[g].w;
    const bool fg = F > 0 && fminf(fmaxf(id, 0.f), 1.f) != 0.f;
    // (int)id - 1 clamped to [0, F - 1]; the comparison form keeps a NaN or a huge id from reaching the conversion
    const int f = id >= 2.f ? (id < (float)F ? (int)id - 1 : F - 1) : 0;
    float ar = 1.f, ag = 1.f, ab = 1.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (F > 0) {
        const float* n = face_normals + ((size_t)b * F + f) * 3;
        nx = n[0];
        ny = n[1];
        nz = n[2];
        if (face_colors) {
            const float* c = face_colors + ((size_t)b * F + f) * 3;
            ar = c[0];
            ag = c[1];
            ab = c[2];
        }
    }
    const float d = lighting == GMR_LIGHT_FRONT ? fminf(fmaxf(nz, 0.f), 1.f) : 1.f;
    float br = bg_r, bgg = bg_g, bb = bg_b;
    if (bg_image && !fg) {
        const float* q = bg_image + (((size_t)b * H + (H - 1 - y)) * W + x) * 3;
        br = q[0];
        bgg = q[1];
        bb = q[2];
    }
    store3(albedo + g * 3, ar, ag, ab);
    if (fg) {
        store3(normal + g * 3, nx, ny, nz);
        store3(diffuse + g * 3, d, d, d);
        rgba[g] = make_float4(ar * d, ag * d, ab * d, 1.f);
    } else {
        store3(normal + g * 3, br, bgg, bb);
        store3(diffuse + g * 3, br, bgg, bb);
        rgba[g] = make_float4(br, bgg, bb, 0.f);
    }
}

struct MapTable {
    GmrMap m[GMR_MAX_MAPS];
};

// source index pair and weight of output index i: torch's area_pixel_compute_source_index (align_corners = false), whose device build
// contracts scale * (i + 0.5) - 0.5 into one fused multiply-add
__device__ __forceinline__ void src_coord(int i, float scale, int n_in, int* i0, int* i1, float* l1)
{
    const float s = fmaxf(fmaf(scale, (float)i + 0.5f, -0.5f), 0.f);
    const int a = min((int)s, n_in - 1);
    *i0 = a;
    *i1 = a + (a < n_in - 1 ? 1 : 0);
    *l1 = s - (float)a;
}

__global__ __launch_bounds__(NT) void k_resize_flip(int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, MapTable t)
{
    const GmrMap mp = t.m[blockIdx.y];
    const int C = mp.C;
    const int64_t HW = (int64_t)H * W;
    const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= (int64_t)B * HW) return;
    const int b = (int)(g / HW);
    const int Y = (int)((g % HW) / W), X = (int)(g % W);
    float* __restrict__ o = mp.dst + g * C;
    const float* __restrict__ sb = mp.src + (size_t)b * h * w * C;
    if (h == H && w == W) {   // the flip alone: the values are moved, never multiplied (a weight of 0 would turn -0 into +0)
        const float* __restrict__ s = sb + ((size_t)(h - 1 - Y) * w + X) * C;
        if (C == 4) {
            *(float4*)o = *(const float4*)s;
        } else {
            for (int c = 0; c < C; ++c) o[c] = s[c];
        }
        return;
    }
    int y0, y1, x0, x1;
    float ly, lx;
    src_coord(Y, (float)h / (float)H, h, &y0, &y1, &ly);
    src_coord(X, (float)w / (float)W, w, &x0, &x1, &lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* __restrict__ r0 = sb + (size_t)(h - 1 - y0) * w * C;   // row y0 of the flipped source
    const float* __restrict__ r1 = sb + (size_t)(h - 1 - y1) * w * C;
    if (C == 4) {
        const float4 a = *(const float4*)(r0 + (size_t)x0 * 4), bq = *(const float4*)(r0 + (size_t)x1 * 4);
        const float4 c4 = *(const float4*)(r1 + (size_t)x0 * 4), d4 = *(const float4*)(r1 + (size_t)x1 * 4);
        float4 r;
        r.x = hy * (hx * a.x + lx * bq.x) + ly * (hx * c4.x + lx * d4.x);
        r.y = hy * (hx * a.y + lx * bq.y) + ly * (hx * c4.y + lx * d4.y);
        r.z = hy * (hx * a.z + lx * bq.z) + ly * (hx * c4.z + lx * d4.z);
        r.w = hy * (hx * a.w + lx * bq.w) + ly * (hx * c4.w + lx * d4.w);
        *(float4*)o = r;
    } else {
        for (int c = 0; c < C; ++c)
            o[c] = hy * (hx * r0[(size_t)x0 * C + c] + lx * r0[(size_t)x1 * C + c]) + ly * (hx * r1[(size_t)x0 * C + c] + lx * r1[(size_t)x1 * C + c]);
    }
}

__global__ __launch_bounds__(NT) void k_compose_overlay(int32_t HW, const float* __restrict__ splat, const float4* __restrict__ rgba,
                                                        float op, float omo, float* __restrict__ out, uint8_t* __restrict__ out_bytes)
{
    const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= HW) return;
    const float4 m = rgba[g];
    float net[3] = {m.x, m.y, m.z};
    if (splat) {
        const float k = m.w * omo + (1.f - m.w);
#pragma unroll
        for (int c = 0; c < 3; ++c) net[c] = (net[c] * m.w) * op + splat[(size_t)c * HW + g] * k;
    }
    if (out_bytes) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_bytes[(size_t)g * 3 + c] = (uint8_t)(int)(fminf(fmaxf(net[c], 0.f), 1.f) * 255.f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(size_t)c * HW + g] = net[c];
    }
}

}  // namespace gmr

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int gmr_mesh_prepare(int32_t B, int32_t V, int32_t F, const float* verts, const int32_t* tri, const float* rt, int32_t rt_rows,
                     const float* mvp, int32_t mat_mode, float* pos_clip, float* face_normals, void* stream)
{
    if (B < 1 || B > 65535 || V < 0 || F < 0 || F > GMR_MAX_TRIANGLES || (rt_rows != 3 && rt_rows != 4) ||
        (mat_mode != GMR_MAT_ROWS && mat_mode != GMR_MAT_CAMERA) || (mat_mode == GMR_MAT_CAMERA && rt_rows != 4))
        return fail(GMR_E_ARG, "gmr_mesh_prepare: bad arguments (B=%d V=%d F=%d rt_rows=%d mat_mode=%d)", B, V, F, rt_rows, mat_mode);
    if ((V > 0 && (!verts || !mvp || !pos_clip)) || (F > 0 && (!verts || !tri || !rt || !face_normals)))
        return fail(GMR_E_ARG, "gmr_mesh_prepare: NULL device pointer");
    const int n = V > F ? V : F;
    if (n == 0) return GMR_OK;
    hipLaunchKernelGGL(gmr::k_mesh_prepare, dim3((unsigned)((n + gmr::NT - 1) / gmr::NT), B), dim3(gmr::NT), 0, (hipStream_t)stream, V, F,
                       verts, tri, rt, rt_rows, mvp, mat_mode, (float4*)pos_clip, face_normals);
    LAUNCH_CHECK(GMR_E_HIP, "k_mesh_prepare");
    return GMR_OK;
}

int gmr_mesh_shade(int32_t B, int32_t F, int32_t H, int32_t W, const float* rast, const float* face_normals, const float* face_colors,
                   int32_t lighting, float bg_r, float bg_g, float bg_b, const float* bg_image, float* albedo, float* normal,
                   float* diffuse, float* rgba, void* stream)
{
    if (!shape_ok(B, 0, F, H, W) || (lighting != GMR_LIGHT_CONSTANT && lighting != GMR_LIGHT_FRONT))
        return fail(GMR_E_ARG, "gmr_mesh_shade: bad arguments (B=%d F=%d H=%d W=%d lighting=%d)", B, F, H, W, lighting);
    if (!rast || !albedo || !normal || !diffuse || !rgba || (F > 0 && !face_normals))
        return fail(GMR_E_ARG, "gmr_mesh_shade: NULL device pointer");
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(gmr::k_mesh_shade, dim3((unsigned)((n + gmr::NT - 1) / gmr::NT)), dim3(gmr::NT), 0, (hipStream_t)stream, B, F, H, W,
                       (const float4*)rast, face_normals, face_colors, lighting, bg_r, bg_g, bg_b, bg_image, albedo, normal, diffuse,
                       (float4*)rgba);
    LAUNCH_CHECK(GMR_E_HIP, "k_mesh_shade");
    return GMR_OK;
}

int gmr_resize_flip(int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, int32_t n_maps, const GmrMap* maps, void* stream)
{
    if (!shape_ok(B, 0, 0, H, W) || !shape_ok(B, 0, 0, h, w) || n_maps < 1 || n_maps > GMR_MAX_MAPS || !maps)
        return fail(GMR_E_ARG, "gmr_resize_flip: bad arguments (B=%d h=%d w=%d H=%d W=%d n_maps=%d)", B, h, w, H, W, n_maps);
    gmr::MapTable t;
    for (int i = 0; i < GMR_MAX_MAPS; ++i) {
        t.m[i] = maps[i < n_maps ? i : 0];
        if (t.m[i].C < 1 || t.m[i].C > 65536)
            return fail(GMR_E_ARG, "gmr_resize_flip: map %d has C=%d", i, t.m[i].C);
        if (!t.m[i].src || !t.m[i].dst) return fail(GMR_E_ARG, "gmr_resize_flip: NULL device pointer");
        if (t.m[i].src == t.m[i].dst) return fail(GMR_E_ARG, "gmr_resize_flip: dst must not alias src");
    }
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(gmr::k_resize_flip, dim3((unsigned)((n + gmr::NT - 1) / gmr::NT), n_maps), dim3(gmr::NT), 0, (hipStream_t)stream, B, h,
                       w, H, W, t);
    LAUNCH_CHECK(GMR_E_HIP, "k_resize_flip");
    return GMR_OK;
}

int gmr_compose_overlay(int32_t H, int32_t W, const float* splat, const float* rgba, float opacity, float one_minus_opacity, float* out,
                        uint8_t* out_bytes, void* stream)
{
    if (!shape_ok(1, 0, 0, H, W)) return fail(GMR_E_ARG, "gmr_compose_overlay: bad arguments (H=%d W=%d)", H, W);
    if (!rgba || ((out != nullptr) == (out_bytes != nullptr)))
        return fail(GMR_E_ARG, "gmr_compose_overlay: NULL device pointer, or not exactly one of out and out_bytes");
    const int32_t n = H * W;
    hipLaunchKernelGGL(gmr::k_compose_overlay, dim3((unsigned)((n + gmr::NT - 1) / gmr::NT)), dim3(gmr::NT), 0, (hipStream_t)stream, n, splat,
                       (const float4*)rgba, opacity, one_minus_opacity, out, out_bytes);
    LAUNCH_CHECK(GMR_E_HIP, "k_compose_overlay");
    return GMR_OK;
}

}  // extern "C"
