// gdc_knn.h -- the 3-nearest-neighbour distances of include/gdc.h (gdc_knn3_dist2): simple-knn's distCUDA2 as an EXACT search on the spatial
// order of gdc_order.h.
//
//   k_knn_gather    one thread per sorted position r: the point perm[r] into pts[r] (x, y, z, 0 -- 16 bytes, so that the search reads a point
//                   with one access), and per run of KNN_CHUNK consecutive sorted points its box: per-axis min / max by shuffles inside the
//                   run (a run never straddles a wave), lo | hi as two 16-byte records
//   k_knn_search    one query per lane, in sorted order, so that the 64 queries of a wave are neighbours in space.  The ±3 neighbours in the
//                   sorted sequence give `reject`, an upper bound of the query's third-smallest distance; then every chunk is visited in
//                   order, its box through an LDS tile of KNN_TILE boxes the workgroup loads together (the footprint does not grow with P),
//                   and the chunk's points are scanned -- at a wave-uniform address, every lane against the same point -- unless NO lane of
//                   the wave wants it (__ballot).  The result goes to dist2_out[perm[r]]: input row order.
//
// Why the pruning is exact, and why this translation unit must stay -ffp-contract=off: a distance is d2 = (dx*dx + dy*dy) + dz*dz with
// dx = x_i - x_j, every operation rounded once in fp32.  The box distance is THE SAME expression on the per-axis gaps g = 0 when the query is
// inside [lo, hi], p - hi or lo - p otherwise.  For a point q of the box |p - q| >= g on every axis in exact arithmetic; an fp32 subtraction,
// multiplication and addition are monotonic in their operands (rounding is monotonic), so fl(d2(p, q)) >= fl(box_d2) for every q in the box.
// `box_d2 > limit` therefore proves that every distance into the box exceeds `limit`, and with limit = min(best[2], reject) >= the true
// third-smallest distance no neighbour that belongs to the answer is ever skipped: the three values are the ones an fp32 brute force over all
// j finds (ties for the third place have the same value).  A fused multiply-add in one of the two expressions and not in the other would
// break the inequality by an ulp.
//
// Loop bounds depend on P only (a NaN fails `box_d2 > limit` and merely scans more), nothing is stored outside [0, P), no atomics, no
// workgroup waits on another.  Included by gdc_kernels.hip only.
#pragma once

namespace gdc {

constexpr int KNN_CHUNK = GDC_KNN_CHUNK;   // sorted points per box
constexpr int KNN_TILE = BLOCK;            // boxes per LDS tile: thread t of the workgroup loads box t
constexpr int KNN_SEED = 3;                // the seed window: r - 3 .. r + 3 (simple-knn's)
static_assert(KNN_CHUNK >= 2 && KNN_CHUNK <= 64 && (KNN_CHUNK & (KNN_CHUNK - 1)) == 0, "a chunk is a power-of-two run of lanes inside one wave");

typedef float f4a __attribute__((ext_vector_type(4)));   // 16-byte aligned: pts and boxes start on 16-byte boundaries of the workspace

// the one distance expression: query first
__device__ __forceinline__ float knn_d2(float px, float py, float pz, float qx, float qy, float qz)
{
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the same expression on the gaps to a box
__device__ __forceinline__ float knn_box_d2(float px, float py, float pz, const f4a lo, const f4a hi)
{
    const float gx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// d into the ascending triple b: a three-stage compare-exchange, no branch
__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2)
{
    float t = fmaxf(b0, d);
    b0 = fminf(b0, d);
    d = fmaxf(b1, t);
    b1 = fminf(b1, t);
    b2 = fminf(b2, d);
}

__global__ __launch_bounds__(BLOCK) void k_knn_gather(int P, const float* __restrict__ xyz, const int* __restrict__ perm, f4a* __restrict__ pts,
                                                      f4a* __restrict__ boxes)
{
    const int tid = (int)threadIdx.x;
    const int r = (int)(blockIdx.x * BLOCK) + tid;
    const bool live = r < P;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (live) {
        const int i = perm[r];
        f4a p = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)i < (unsigned)P) p.x = xyz[3 * (size_t)i], p.y = xyz[3 * (size_t)i + 1], p.z = xyz[3 * (size_t)i + 2];
        pts[r] = p;
        lo[0] = hi[0] = p.x, lo[1] = hi[1] = p.y, lo[2] = hi[2] = p.z;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int d = KNN_CHUNK / 2; d > 0; d >>= 1) {
            lo[j] = fminf(lo[j], __shfl_xor(lo[j], d));
            hi[j] = fmaxf(hi[j], __shfl_xor(hi[j], d));
        }
    if (live && (tid & (KNN_CHUNK - 1)) == 0) {   // (r is a multiple of KNN_CHUNK: BLOCK is one)
        const int c = r / KNN_CHUNK;
        boxes[2 * (size_t)c] = f4a{lo[0], lo[1], lo[2], 0.f};
        boxes[2 * (size_t)c + 1] = f4a{hi[0], hi[1], hi[2], 0.f};
    }
}

__global__ __launch_bounds__(BLOCK) void k_knn_search(int P, int nboxes, const f4a* __restrict__ pts, const f4a* __restrict__ boxes,
                                                      const int* __restrict__ perm, float* __restrict__ out)
{
    __shared__ f4a tile[2 * KNN_TILE];
    const int tid = (int)threadIdx.x;
    const int r = (int)(blockIdx.x * BLOCK) + tid;
    const bool live = r < P;
    const float inf = __builtin_huge_valf();
    f4a p = {0.f, 0.f, 0.f, 0.f};
    if (live) p = pts[r];
    // the seed: an upper bound of the third-smallest distance from the neighbours in the sorted sequence (+inf while fewer than three exist)
    float s0 = inf, s1 = inf, s2 = inf;
#pragma unroll
    for (int k = -KNN_SEED; k <= KNN_SEED; ++k) {
        const int j = r + k;
        if (k != 0 && live && j >= 0 && j < P) {
            const f4a q = pts[j];
            knn_insert(knn_d2(p.x, p.y, p.z, q.x, q.y, q.z), s0, s1, s2);
        }
    }
    const float reject = s2;
    float b0 = inf, b1 = inf, b2 = inf;
    for (int base = 0; base < nboxes; base += KNN_TILE) {   // (bounds from P alone: every wave of the workgroup meets every barrier)
        const int n = nboxes - base < KNN_TILE ? nboxes - base : KNN_TILE;
        __syncthreads();
        if (tid < n) {
            tile[2 * tid] = boxes[2 * (size_t)(base + tid)];
            tile[2 * tid + 1] = boxes[2 * (size_t)(base + tid) + 1];
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const float limit = fminf(b2, reject);
            const float bd = knn_box_d2(p.x, p.y, p.z, tile[2 * t], tile[2 * t + 1]);
            if (__ballot(live && !(bd > limit)) == 0ull) continue;   // no lane wants the chunk
            const int first = (base + t) * KNN_CHUNK;
            const int last = first + KNN_CHUNK < P ? first + KNN_CHUNK : P;
            for (int j = first; j < last; ++j) {   // wave-uniform address: one point against the wave's 64 queries
                const f4a q = pts[j];
                const float d = knn_d2(p.x, p.y, p.z, q.x, q.y, q.z);
                knn_insert(j == r ? inf : d, b0, b1, b2);   // the query itself is left out by INDEX: a duplicate is a neighbour at 0
            }
        }
    }
    if (!live) return;
    const int row = perm[r];
    if ((unsigned)row >= (unsigned)P) return;
    float v = 0.f;   // P == 1: no neighbour
    if (P >= 4) v = ((b0 + b1) + b2) / 3.0f;
    else if (P == 3) v = (b0 + b1) / 2.0f;
    else if (P == 2) v = b0;
    out[row] = v;
}

// the workspace: pts[P] | boxes[2 * nboxes] (16-byte records) | perm[P] | the order workspace of gdc_order.h
struct KnnWorkspace { f4a* pts; f4a* boxes; int* perm; void* order; int nboxes; };

static KnnWorkspace carve_knn(void* base, int P)
{
    KnnWorkspace w;
    w.nboxes = (int)(((int64_t)P + KNN_CHUNK - 1) / KNN_CHUNK);
    w.pts = (f4a*)base;
    w.boxes = w.pts + P;
    w.perm = (int*)(w.boxes + 2 * (size_t)w.nboxes);
    w.order = (void*)(w.perm + P);
    return w;
}

}  // namespace gdc
