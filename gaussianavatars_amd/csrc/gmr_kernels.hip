// gmr_kernels.hip -- the mesh overlay's triangle rasterizer and analytic antialias (include/gmr.h).
//
// k_mesh_setup      one thread per (batch, triangle): a 24-float record (three edge functions, the z/w plane), the pixel bbox,
//                   and per workgroup of 256 triangles (a "chunk") the union of their bboxes.
// k_mesh_raster     one workgroup per 16x16 screen tile, one pixel per lane: walks the chunks in triangle order, skips a chunk whose
//                   box misses the tile, compacts the triangles whose bbox meets the tile into LDS (ballot + prefix, order kept) and
//                   runs the depth test over them with (z, id) in registers; the winner's (u, v, z/w) are evaluated once more in double
//                   from its vertices.  One float4 store per pixel.
// k_mesh_antialias  one thread per pixel: gathers the blend contributions of its four neighbour pairs (no scatter, no atomics).
//
// Watertightness without fixed point: an edge function belongs to the EDGE, not to the triangle.  It is computed from the edge's
// endpoints in canonical order (lower vertex index first) and the triangle negates it when it walks the edge the other way, so two
// triangles that share an edge evaluate exactly negated values at every pixel (this TU is built with -ffp-contract=off).  The
// function is evaluated relative to the nearer projected endpoint (ties: the lower index), so a pixel centre that is exactly a
// projected vertex evaluates exactly 0 on every edge through that vertex: some triangle of the fan always covers it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "../../include/gmr.h"
#include "lib_common.h"

namespace gmr {

constexpr int NT = 256;       // threads per workgroup; also triangles per chunk
constexpr int TS = 16;        // screen tile edge (TS * TS == NT)
constexpr int REC = 24;       // floats per triangle record: 3 x (qa.x, qa.y, qb.x, qb.y, n.x, n.y, n.z), then z/w = (zA, zB, zC) . (px, py, 1)
constexpr int REC4 = REC / 4;
static_assert(TS * TS == NT, "one pixel per lane");

__device__ __forceinline__ bool in_range(int i, int n) { return i >= 0 && i < n; }

__device__ __forceinline__ void load_vertex(const float* pos, int b, int V, int i, double v[4])
{
    const float* p = pos + ((size_t)b * V + i) * 4;
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
    v[3] = p[3];
}

// (a.x, a.y, a.w) x (b.x, b.y, b.w)
__device__ __forceinline__ void cross_xyw(const double a[4], const double b[4], double r[3])
{
    r[0] = a[1] * b[3] - a[3] * b[1];
    r[1] = a[3] * b[0] - a[0] * b[3];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(NT) void k_mesh_setup(int32_t V, int32_t F, int32_t H, int32_t W, const float* __restrict__ pos,
                                                   const int32_t* __restrict__ tri, float4* __restrict__ rec, int4* __restrict__ bbox,
                                                   int4* __restrict__ cbox)
{
    __shared__ int sb[4];
    const int b = blockIdx.y, t = blockIdx.x * NT + threadIdx.x;
    const size_t BF = (size_t)gridDim.y * F;
    if (threadIdx.x == 0) {
        sb[0] = INT_MAX;
        sb[1] = INT_MAX;
        sb[2] = -1;
        sb[3] = -1;
    }
    __syncthreads();
    if (t < F) {
        int4 bb = make_int4(INT_MAX, INT_MAX, -1, -1);   // culled: meets no tile
        float r[REC];
#pragma unroll
        for (int k = 0; k < REC; ++k) r[k] = 0.f;
        int idx[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
        bool live = in_range(idx[0], V) && in_range(idx[1], V) && in_range(idx[2], V) && idx[0] != idx[1] && idx[1] != idx[2] &&
                    idx[0] != idx[2];
        double v[3][4];
        if (live) {
            for (int i = 0; i < 3; ++i) {
                load_vertex(pos, b, V, idx[i], v[i]);
                for (int c = 0; c < 4; ++c) live = live && isfinite(v[i][c]);
            }
        }
        if (live) {   // trivial rejects: every vertex behind w = 0, beyond the far plane or before the near plane
            bool allw = true, allfar = true, allnear = true;
            for (int i = 0; i < 3; ++i) {
                allw = allw && v[i][3] <= 0.0;
                allfar = allfar && v[i][2] > v[i][3];
                allnear = allnear && v[i][2] < -v[i][3];
            }
            live = !(allw || allfar || allnear);
        }
        double adj[3][3], det = 0.0;
        if (live) {
            for (int i = 0; i < 3; ++i) cross_xyw(v[(i + 1) % 3], v[(i + 2) % 3], adj[i]);   // row i of adj[x y w]: b_i ~ adj[i] . (px, py, 1)
            det = v[0][0] * adj[0][0] + v[0][1] * adj[0][1] + v[0][3] * adj[0][2];
            live = det != 0.0 && isfinite(det);
        }
        if (live) {
            const double s = det > 0.0 ? 1.0 : -1.0;
            for (int i = 0; i < 3; ++i) {   // edge i: opposite vertex i, walked from j = i+1 to k = i+2
                const int j = (i + 1) % 3, k = (i + 2) % 3;
                const bool fwd = idx[j] < idx[k];
                const int a = fwd ? j : k, c = fwd ? k : j;   // canonical: lower vertex index first
                double n[3];
                cross_xyw(v[a], v[c], n);
                const float sg = (fwd ? 1.f : -1.f) * (float)s;
                float* e = r + 7 * i;
                if (v[a][3] > 0.0 && v[c][3] > 0.0) {   // both endpoints project: evaluate relative to an endpoint, n.z drops out
                    e[0] = (float)(v[a][0] / v[a][3]);
                    e[1] = (float)(v[a][1] / v[a][3]);
                    e[2] = (float)(v[c][0] / v[c][3]);
                    e[3] = (float)(v[c][1] / v[c][3]);
                    e[6] = 0.f;
                } else {                                // homogeneous form about the origin
                    e[6] = sg * (float)n[2];
                }
                e[4] = sg * (float)n[0];                // rounded once per edge, then negated: exactly opposite in the two triangles
                e[5] = sg * (float)n[1];
            }
            double za = 0.0, zb = 0.0, zc = 0.0;
            for (int i = 0; i < 3; ++i) {
                za += v[i][2] * adj[i][0];
                zb += v[i][2] * adj[i][1];
                zc += v[i][2] * adj[i][2];
            }
            r[21] = (float)(za / det);
            r[22] = (float)(zb / det);
            r[23] = (float)(zc / det);
            if (v[0][3] > 0.0 && v[1][3] > 0.0 && v[2][3] > 0.0) {
                double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
                for (int i = 0; i < 3; ++i) {
                    const double X = (v[i][0] / v[i][3] + 1.0) * 0.5 * W - 0.5, Y = (v[i][1] / v[i][3] + 1.0) * 0.5 * H - 0.5;
                    x0 = fmin(x0, X);
                    x1 = fmax(x1, X);
                    y0 = fmin(y0, Y);
                    y1 = fmax(y1, Y);
                }
                // one pixel of margin against rounding; clamped in double before the conversion
                x0 = fmax(floor(x0) - 1.0, 0.0);
                y0 = fmax(floor(y0) - 1.0, 0.0);
                x1 = fmin(ceil(x1) + 1.0, (double)(W - 1));
                y1 = fmin(ceil(y1) + 1.0, (double)(H - 1));
                if (x0 <= x1 && y0 <= y1) bb = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
            } else {
                bb = make_int4(0, 0, W - 1, H - 1);   // a vertex at w <= 0: no projected bound, the whole image
            }
        }
        const size_t o = (size_t)b * F + t;
#pragma unroll
        for (int k = 0; k < REC4; ++k) rec[k * BF + o] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        bbox[o] = bb;
        if (bb.x <= bb.z) {   // integer min / max: the result does not depend on the order
            atomicMin(&sb[0], bb.x);
            atomicMin(&sb[1], bb.y);
            atomicMax(&sb[2], bb.z);
            atomicMax(&sb[3], bb.w);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) cbox[(size_t)b * gridDim.x + blockIdx.x] = make_int4(sb[0], sb[1], sb[2], sb[3]);
}

__device__ __forceinline__ float edge_eval(const float* e, float px, float py)
{
    const float dxa = px - e[0], dya = py - e[1], dxb = px - e[2], dyb = py - e[3];
    const bool ub = fabsf(dxb) + fabsf(dyb) < fabsf(dxa) + fabsf(dya);   // the nearer endpoint; the lower index on a tie
    const float dx = ub ? dxb : dxa, dy = ub ? dyb : dya;
    return (e[4] * dx + e[5] * dy) + e[6];
}

__device__ __forceinline__ bool misses(int4 bb, int tx0, int ty0, int tx1, int ty1)
{
    return bb.x > tx1 || bb.z < tx0 || bb.y > ty1 || bb.w < ty0;
}

__global__ __launch_bounds__(NT) void k_mesh_raster(int32_t V, int32_t F, int32_t H, int32_t W, const float* __restrict__ pos,
                                                    const int32_t* __restrict__ tri, const float4* __restrict__ rec,
                                                    const int4* __restrict__ bbox, const int4* __restrict__ cbox, float4* __restrict__ rast)
{
    __shared__ float4 srec[NT * REC4];   // 24 KiB
    __shared__ int sid[NT];
    __shared__ int scount[NT / 64];
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * TS, ty0 = blockIdx.y * TS;
    const int tx1 = min(tx0 + TS - 1, W - 1), ty1 = min(ty0 + TS - 1, H - 1);
    const int x = tx0 + (threadIdx.x & (TS - 1)), y = ty0 + (threadIdx.x / TS);
    const float px = (float)(2 * x + 1) / (float)W - 1.f, py = (float)(2 * y + 1) / (float)H - 1.f;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t BF = (size_t)gridDim.z * F;
    const int nch = (F + NT - 1) / NT;
    float bz = INFINITY;
    int bid = -1;
    for (int c = 0; c < nch; ++c) {
        if (misses(cbox[(size_t)b * nch + c], tx0, ty0, tx1, ty1)) continue;   // uniform over the workgroup
        const int t = c * NT + threadIdx.x;
        const bool hit = t < F && !misses(bbox[(size_t)b * F + t], tx0, ty0, tx1, ty1);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) scount[wv] = __popcll(m);
        __syncthreads();
        int off = 0, n = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            off += w < wv ? scount[w] : 0;
            n += scount[w];
        }
        if (hit) {   // slots in triangle order: the depth test's tie rule (lower index wins) is the loop order
            const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
            sid[slot] = t;
            const size_t o = (size_t)b * F + t;
#pragma unroll
            for (int k = 0; k < REC4; ++k) srec[slot * REC4 + k] = rec[k * BF + o];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            float r[REC];
#pragma unroll
            for (int k = 0; k < REC4; ++k) {
                const float4 q = srec[i * REC4 + k];
                r[4 * k] = q.x;
                r[4 * k + 1] = q.y;
                r[4 * k + 2] = q.z;
                r[4 * k + 3] = q.w;
            }
            const float e0 = edge_eval(r, px, py), e1 = edge_eval(r + 7, px, py), e2 = edge_eval(r + 14, px, py);
            if (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) {
                const float s = (e0 + e1) + e2;   // > 0  <=>  c.w > 0
                const float z = (r[21] * px + r[22] * py) + r[23];
                if (s > 0.f && z >= -1.f && z <= 1.f && z < bz) {
                    bz = z;
                    bid = sid[i];
                }
            }
        }
        __syncthreads();   // srec / scount are rewritten by the next chunk
    }
    if (x >= W || y >= H) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bid >= 0) {
        // The winner's (u, v, z/w) once more in double from its vertices: the float edge functions decide coverage and depth order,
        // but on a sliver (a grazing face a fraction of a pixel wide) their rounding is a visible share of the barycentrics.
        double v[3][4], e[3];
        for (int i = 0; i < 3; ++i) load_vertex(pos, b, V, tri[3 * (size_t)bid + i], v[i]);   // indices checked by k_mesh_setup
        const double dpx = (double)(2 * x + 1) / W - 1.0, dpy = (double)(2 * y + 1) / H - 1.0;
        for (int i = 0; i < 3; ++i) {
            double r[3];
            cross_xyw(v[(i + 1) % 3], v[(i + 2) % 3], r);
            e[i] = r[0] * dpx + r[1] * dpy + r[2];
        }
        const double s = e[0] + e[1] + e[2], cw = e[0] * v[0][3] + e[1] * v[1][3] + e[2] * v[2][3];
        const double cz = e[0] * v[0][2] + e[1] * v[1][2] + e[2] * v[2][2];
        o = make_float4((float)(e[0] / s), (float)(e[1] / s), (float)(cz / cw), (float)(bid + 1));
    }
    rast[((size_t)b * H + y) * W + x] = o;
}

// triangle index of a rast texel, or -1 for an empty pixel (anything that is not a whole number in [1, F] counts as empty)
__device__ __forceinline__ int rast_id(float w, int F)
{
    return (w >= 1.f && w <= (float)F && w == floorf(w)) ? (int)w - 1 : -1;
}

// sign of det[x y w] of triangle f, 0 when it cannot be formed
__device__ int orientation(const float* pos, const int32_t* tri, int b, int V, int f)
{
    double v[3][4];
    for (int i = 0; i < 3; ++i) {
        const int vi = tri[3 * (size_t)f + i];
        if (!in_range(vi, V)) return 0;
        load_vertex(pos, b, V, vi, v[i]);
    }
    double r[3];
    cross_xyw(v[1], v[2], r);
    const double d = v[0][0] * r[0] + v[0][1] * r[1] + v[0][3] * r[2];
    return d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
}

// Where the first silhouette edge of triangle f (order v0v1, v1v2, v2v0) crosses the segment between the pixel centres
// P = (xp, yp) and Q = (xq, yq) (4-neighbours): t in [0, 1] along P -> Q.  False when no silhouette edge crosses it.
__device__ bool silhouette_crossing(const float* pos, const int32_t* tri, const int32_t* nbr, int b, int V, int F, int H, int W, int f,
                                    int xp, int yp, int xq, int yq, double* t_out)
{
    int idx[3];
    double v[3][4];
    for (int i = 0; i < 3; ++i) {
        idx[i] = tri[3 * (size_t)f + i];
        if (!in_range(idx[i], V)) return false;
        load_vertex(pos, b, V, idx[i], v[i]);
    }
    int of = 2;   // F's orientation, computed once it is needed
    const bool horiz = yp == yq;
    for (int k = 0; k < 3; ++k) {
        const double* A = v[k];
        const double* C = v[(k + 1) % 3];
        if (!(A[3] > 0.0) || !(C[3] > 0.0)) continue;
        const int n = nbr[3 * (size_t)f + k];
        bool sil = n < 0 || n >= F;
        if (!sil) {
            if (of == 2) {
                double r[3];
                cross_xyw(v[1], v[2], r);
                const double d = v[0][0] * r[0] + v[0][1] * r[1] + v[0][3] * r[2];
                of = d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
            }
            sil = of * orientation(pos, tri, b, V, n) < 0;
        }
        if (!sil) continue;
        // the edge in pixel-centre coordinates (pixel (i, j) at (i, j))
        const double ax = (A[0] / A[3] + 1.0) * 0.5 * W - 0.5, ay = (A[1] / A[3] + 1.0) * 0.5 * H - 0.5;
        const double cx = (C[0] / C[3] + 1.0) * 0.5 * W - 0.5, cy = (C[1] / C[3] + 1.0) * 0.5 * H - 0.5;
        // along = the axis of the P -> Q segment, across = the other one
        const double a_al = horiz ? ax : ay, a_ac = horiz ? ay : ax, c_al = horiz ? cx : cy, c_ac = horiz ? cy : cx;
        const double p_al = horiz ? xp : yp, q_al = horiz ? xq : yq, line = horiz ? yp : xp;
        const double d_ac = c_ac - a_ac;
        if (!(d_ac != 0.0)) continue;   // parallel to the segment (or not finite)
        const double s = (line - a_ac) / d_ac;
        if (!(s >= 0.0 && s <= 1.0)) continue;   // outside the edge's finite extent
        const double cross_al = a_al + s * (c_al - a_al);
        const double t = (cross_al - p_al) / (q_al - p_al);
        if (!(t >= 0.0 && t <= 1.0)) continue;
        *t_out = t;
        return true;
    }
    return false;
}

__global__ __launch_bounds__(NT) void k_mesh_antialias(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, int32_t C,
                                                       const float* __restrict__ color, const float4* __restrict__ rast,
                                                       const float* __restrict__ pos, const int32_t* __restrict__ tri,
                                                       const int32_t* __restrict__ nbr, float* __restrict__ out)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= (int64_t)B * HW) return;
    const int b = (int)(g / HW);
    const int y = (int)((g % HW) / W), x = (int)(g % W);
    const float4 me = rast[g];
    const int id_me = rast_id(me.w, F);
    float wk[4];
    int64_t gk[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {   // left, right, below (y - 1), above (y + 1)
        wk[d] = 0.f;
        gk[d] = g;
        const int xn = x + (d == 0 ? -1 : (d == 1 ? 1 : 0)), yn = y + (d == 2 ? -1 : (d == 3 ? 1 : 0));
        if (xn < 0 || xn >= W || yn < 0 || yn >= H) continue;
        const int64_t gn = ((int64_t)b * H + yn) * W + xn;
        const float4 ot = rast[gn];
        const int id_ot = rast_id(ot.w, F);
        if (id_me == id_ot) continue;
        bool me_front;   // is this pixel P (its triangle F the front one)?
        if (id_me < 0)
            me_front = false;
        else if (id_ot < 0)
            me_front = true;
        else
            me_front = me.z < ot.z || (me.z == ot.z && id_me < id_ot);
        const int f = me_front ? id_me : id_ot;
        double t;
        const bool hit = me_front ? silhouette_crossing(pos, tri, nbr, b, V, F, H, W, f, x, y, xn, yn, &t)
                                  : silhouette_crossing(pos, tri, nbr, b, V, F, H, W, f, xn, yn, x, y, &t);
        if (!hit) continue;
        if (me_front && t < 0.5) wk[d] = (float)(0.5 - t);          // P += (0.5 - t) (c_Q - c_P)
        else if (!me_front && t > 0.5) wk[d] = (float)(t - 0.5);    // Q += (t - 0.5) (c_P - c_Q)
        gk[d] = gn;
    }
    const float* cs = color + g * C;
    float* co = out + g * C;
    for (int c = 0; c < C; ++c) {
        const float c0 = cs[c];
        float acc = c0;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (wk[d] > 0.f) acc += wk[d] * (color[gk[d] * C + c] - c0);
        co[c] = acc;
    }
}

}  // namespace gmr

// ---------------------------------------------------------------------------------------------------------------
static bool shape_ok(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W)
{
    return B >= 1 && B <= 65535 && V >= 0 && F >= 0 && F <= GMR_MAX_TRIANGLES && H >= 1 && W >= 1 &&
           (int64_t)B * H * W < ((int64_t)1 << 31) && (H + gmr::TS - 1) / gmr::TS <= 65535;
}

static int64_t n_chunks(int32_t F) { return ((int64_t)F + gmr::NT - 1) / gmr::NT; }

extern "C" {

int gmr_abi_version(void) { return GMR_ABI_VERSION; }
const char* gmr_last_error(void) { return g_err; }

int64_t gmr_workspace_bytes(int32_t B, int32_t F)
{
    if (B < 1 || F < 0) return 0;
    return (int64_t)B * F * (gmr::REC4 + 1) * 16 + (int64_t)B * n_chunks(F) * 16;
}

int gmr_rasterize(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float* pos, const int32_t* tri, float* rast,
                  void* workspace, void* stream)
{
    if (!shape_ok(B, V, F, H, W)) return fail(GMR_E_ARG, "gmr_rasterize: bad arguments (B=%d V=%d F=%d H=%d W=%d)", B, V, F, H, W);
    if (!rast || (F > 0 && (!pos || !tri || !workspace)))
        return fail(GMR_E_ARG, "gmr_rasterize: NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t BF = (size_t)B * F;
    float4* rec = (float4*)workspace;
    int4* bbox = (int4*)(rec + gmr::REC4 * BF);
    int4* cbox = bbox + BF;
    if (F > 0) {
        hipLaunchKernelGGL(gmr::k_mesh_setup, dim3((unsigned)n_chunks(F), B), dim3(gmr::NT), 0, s, V, F, H, W, pos, tri, rec, bbox, cbox);
        LAUNCH_CHECK(GMR_E_HIP, "k_mesh_setup");
    }
    dim3 grid((W + gmr::TS - 1) / gmr::TS, (H + gmr::TS - 1) / gmr::TS, B);
    hipLaunchKernelGGL(gmr::k_mesh_raster, grid, dim3(gmr::NT), 0, s, V, F, H, W, pos, tri, rec, bbox, cbox, (float4*)rast);
    LAUNCH_CHECK(GMR_E_HIP, "k_mesh_raster");
    return GMR_OK;
}

int gmr_antialias(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, int32_t C, const float* color, const float* rast,
                  const float* pos, const int32_t* tri, const int32_t* neighbours, float* out, void* stream)
{
    if (!shape_ok(B, V, F, H, W) || C < 1)
        return fail(GMR_E_ARG, "gmr_antialias: bad arguments (B=%d V=%d F=%d H=%d W=%d C=%d)", B, V, F, H, W, C);
    if (!color || !rast || !out || (F > 0 && (!pos || !tri || !neighbours)))
        return fail(GMR_E_ARG, "gmr_antialias: NULL device pointer");
    if (color == out) return fail(GMR_E_ARG, "gmr_antialias: out must not alias color");
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(gmr::k_mesh_antialias, dim3((unsigned)((n + gmr::NT - 1) / gmr::NT)), dim3(gmr::NT), 0, (hipStream_t)stream, B, V,
                       F, H, W, C, color, (const float4*)rast, pos, tri, neighbours, out);
    LAUNCH_CHECK(GMR_E_HIP, "k_mesh_antialias");
    return GMR_OK;
}

}  // extern "C"

#include "gmr_overlay.h"   // ABI 2: prepare, shade, resize / flip, compose (include/gmr_overlay.h)
