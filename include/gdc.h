/*
 * gdc.h -- C ABI of adaptive density control ("Gaussian density control"): the end state of the reference's
 * `densify_and_prune` (scene/gaussian_model.py:501-515: densify_and_clone, densify_and_split, prune_points) in five launches
 * and ONE host read, for the six leaves, their twelve Adam moments, the three statistics, `binding` and `binding_counter`.
 * tests/densify_ref.py states the same contract in float64 numpy.  Since ABI 2 also the spatial re-sort that follows it (last block below).
 *
 * Conventions as gop.h: DEVICE pointers, fp32 / int32, contiguous, 4-byte aligned; 0 / <0 return codes with gdc_last_error();
 * everything is enqueued on `stream`.  gdc_plan() ends with the only host synchronisation of a call: it waits for the 16-byte
 * block of the four segment totals.  No float atomics (the two per-face counters are integer atomics: the result does not depend on
 * the order of the adds), no workgroup waits on another, no device-side persistent state.
 *
 * Inputs: P rows of the leaves, the statistics accum / denom (P), optionally binding (P, int32 or int64), face_scaling (F) and
 * binding_counter (F, int32), noise (2, P, 3) unit normals, and the scalars of GdcParams.
 *
 * Per splat i (all in fp32, the translation unit is compiled with -ffp-contract=off):
 *     g = accum[i] / denom[i], NaN -> 0 (+inf kept)
 *     w_j = exp(scaling[i][j]) * (bound ? face_scaling[binding[i]] : 1),  S = max_j w_j          ("world scale")
 *     o = 1 / (1 + exp(-opacity[i]))
 *     clone  iff |g| >= max_grad and S <= percent_dense * extent     the original stays, one identical copy is appended
 *     split  iff  g  >= max_grad and S >  percent_dense * extent     the original goes, two children c = 0, 1 are appended:
 *         q = rotation[i] / |rotation[i]|, R = R(q) (w, x, y, z)
 *         xyz_c     = R * (noise[c][i] * w) + xyz[i]            (world scale added to the local position, as the reference does)
 *         scaling_c = log((w / face_scaling) / 1.6)             (unbound: log(exp(scaling) / 1.6)); every other leaf is copied
 *     candidate(row) iff o < min_opacity, or -- when max_screen_size != 0 -- S_row > 0.1 * extent, S_row from the ROW's own scaling
 *         (a child's is max_j exp(scaling_c[j]) * face_scaling).  max_radii2D is NOT an input: the reference has zeroed it
 *         (densification_postfix) before its prune reads it, so its `max_radii2D > max_screen_size` term never fires.
 *     face protection (bound): cnt[f] = binding_counter[f] + clones on f + splits on f (two children minus the original);
 *         cand[f] = candidate rows on f; the candidates of f are removed iff cnt[f] - cand[f] > 0, else all of them stay.
 *         Unbound: every candidate is removed.
 *
 * Outputs, N = n_orig + n_clone + n_c0 + n_c1 rows in the reference's order -- surviving originals, clones, c = 0 children,
 * c = 1 children, each segment in source order:
 *     src[r]  the source row of a surviving original, -1 - source of a new row
 *     leaves  gathered / computed as above;  moments: gathered for originals, +0.0 for new rows;  the three statistics: +0.0
 *     binding[r] = binding[source];  binding_counter[f] = cnt[f] - (removed ? cand[f] : 0)  (== bincount(binding) when it was on entry)
 *
 * The spatial order (ABI 2): gdc_morton_order() is io.morton_order's permutation of the splats along the Z-order curve of their bounding
 * box, bit for bit, and gdc_permute() moves every per-splat tensor by it in one launch.  Nothing is read back, nothing synchronises and
 * nothing is allocated: both calls can be recorded into a graph.
 *     position   unbound: p = xyz[i].  Bound: p = centre[binding[i]] + 1e-3f * xyz[i] in fp32 -- one rounded multiply, one rounded add, no
 *                contraction -- with centre the (F, 3) fp32 table of the template's face centres; a binding outside [0, F) reads nothing
 *                and uses the centre (0, 0, 0) (an int64 binding is compared as 64 bits here)
 *     box        lo, hi = per-axis min / max of p over the splats: exact, so the order of the reduction does not matter (integer
 *                atomics on an order-preserving encoding of the floats; no float atomics)
 *     quantise   in fp64, in numpy's order: q = clip(trunc(((double)p - lo) / max((double)hi - lo, 1e-30) * 1023.0), 0, 1023), clamped
 *                before the conversion to an integer
 *     code       bit b (0..9) of axis a (0..2) goes to bit 3 b + a
 *     order      ascending code, ties by row index: perm[r] = the row that comes r-th, a stable LSD radix sort of (code, row) in four
 *                8-bit passes of histogram, scan and scatter (three launches each; no workgroup waits on another); a scatter ranks the
 *                keys of its 256-key chunk by a ballot match per digit bit, lanes and waves in order, so every pass is stable and the
 *                result does not depend on scheduling
 *     non-finite positions are outside the contract (numpy's answer is undefined); perm is still a permutation of 0..P-1, the same on
 *                every call, and nothing is stored out of range
 *
 * The nearest neighbours (additive to ABI 2): gdc_knn3_dist2() is simple-knn's distCUDA2 -- per point the mean squared distance to its 3
 * nearest other points, what the reference initialises the scales of an unbound model from (scene/gaussian_model.py:190-192) -- as an EXACT
 * search on that order.  Kernels only (the order's 15 launches, one gather, one search): no host read, no allocation, it can be recorded.
 *     value      d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j and so on, every operation rounded once in fp32, in that order (no
 *                contraction).  dist2[i] = ((b0 + b1) + b2) / 3.0f over the three smallest d2(i, j), j != i, in ascending order.  j is left
 *                out by INDEX, not by distance: a duplicate of point i is a neighbour at distance 0
 *     few points P - 1 < 3: the mean over the P - 1 neighbours there are ((b0 + b1) / 2.0f, b0); P == 1 gives 0.0f; P == 0 launches nothing
 *     exactness  the value equals what an fp32 brute force over all j with the arithmetic above gives; when two candidates tie for the
 *                third place either is taken, the value being the same
 *     method     the unbound order above; the positions gathered into it in one pass, with the box (per-axis min / max) of every run of
 *                GDC_KNN_CHUNK consecutive sorted points; one query per lane in sorted order, so that a wave's 64 queries are neighbours
 *                in space; the third-smallest distance to the +-3 neighbours in the sorted sequence bounds the answer from above; then the
 *                chunks are walked, and one is scanned unless its box is farther than min(best[2], that bound) for every lane of the wave
 *     pruning    the box distance is the same expression with the same roundings on the per-axis gaps (0 inside the box, p - hi or lo - p
 *                otherwise).  Rounding is monotonic, so it is a lower bound of every fp32 d2 into that box, and `box_d2 > bound` skips
 *                nothing that belongs to the answer.  This is why the library is compiled with -ffp-contract=off
 *     output     scattered back through the permutation: dist2_out is in INPUT row order
 *     no float atomics, no workgroup waits on another, two calls give the same bits
 *     non-finite positions are outside the contract: every loop bound depends on P alone and nothing is stored out of range
 */
#ifndef GDC_H
#define GDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stays 2: gdc_knn_workspace_bytes / gdc_knn3_dist2 are additive and no earlier entry changed.  A library built before them is caught by the
 * loader's per-symbol check (_lib._load), not by this number. */
#define GDC_ABI_VERSION 2
#define GDC_OK 0
#define GDC_E_ARG (-1)
#define GDC_E_HIP (-2)
/* splats per workgroup of the decide / resolve / apply kernels: the unit of the three-step scan */
#define GDC_CHUNK 256
/* tensors one gather launch moves (the table rides in the kernel arguments) */
#define GDC_MAX_TENSORS 24
/* output rows per workgroup of the gather: 16 lanes share a row */
#define GDC_ROWS 16
/* P stays below this: an output row index (< 2 P) is an int32 */
#define GDC_MAX_SPLATS (1 << 30)
/* sorted points per box of gdc_knn3_dist2's search: a power of two, 2 ... 64 (a chunk is a run of lanes of one wave) */
#ifndef GDC_KNN_CHUNK
#define GDC_KNN_CHUNK 32
#endif

/* how the gather treats one tensor */
#define GDC_COPY 0      /* every row: copy of the source row */
#define GDC_MOMENT 1    /* surviving original: copy; new row: +0.0 */
#define GDC_ZERO 2      /* every row: +0.0 (src is not read) */
#define GDC_XYZ 3       /* copy; child: xyz_c */
#define GDC_SCALING 4   /* copy; child: scaling_c */

int gdc_abi_version(void);
const char* gdc_last_error(void);

typedef struct {
    float max_grad;
    float min_opacity;
    float extent;
    float percent_dense;
    float max_screen_size;   /* 0 = None */
} GdcParams;

typedef struct {
    const void* src;     /* P rows (NULL for GDC_ZERO) */
    void* dst;           /* N rows */
    int32_t row_floats;  /* 4-byte elements per row, >= 0; 0: nothing moves (an SH degree 0 model's _features_rest) */
    int32_t kind;        /* GDC_COPY ... GDC_SCALING */
} GdcTensor;

/* bytes of the scratch buffer both calls share (4-byte aligned): the totals block, cnt / cand (F each), the per-chunk sums and a byte per splat */
int64_t gdc_workspace_bytes(int32_t P, int32_t F);

/* decide -> resolve -> scan of the chunk sums.  binding NULL = unbound (F = 0, face_scaling / binding_counter / counter_out ignored).
 * counter_out (F, int32) receives the new binding_counter.  totals (HOST, 4 x int32): n_orig, n_clone, n_c0, n_c1 -- read back once,
 * after which the stream is idle.  P == 0 launches nothing, reports four zeros and, when F > 0 and both counter pointers are given, copies
 * binding_counter to counter_out (an empty binding may be NULL). */
int gdc_plan(int32_t P, int32_t F, const GdcParams* params, const void* scaling, const void* opacity, const void* accum, const void* denom,
             const void* binding, int32_t binding_is_i64, const void* face_scaling, const void* binding_counter, void* counter_out,
             void* workspace, int32_t* totals, void* stream);

/* apply -> gather, on the workspace gdc_plan left (same P, F and binding) and the totals it reported: writes src (N, int32), binding_out
 * (N, dtype of binding; NULL when unbound) and every tensor of the HOST table (ntensors <= GDC_MAX_TENSORS, rows per `kind`).  xyz,
 * scaling, rotation and noise are the inputs of the children.  N == 0 launches nothing. */
int gdc_emit(int32_t P, int32_t F, const int32_t* totals, int32_t ntensors, const GdcTensor* tensors, const void* xyz, const void* scaling,
             const void* rotation, const void* noise, const void* binding, int32_t binding_is_i64, const void* face_scaling,
             void* src_out, void* binding_out, void* workspace, void* stream);

/* bytes of gdc_morton_order's scratch buffer (4-byte aligned; its contents need not survive between calls): the box and the digit totals,
 * two key and two row buffers of P words and the RADIX x chunks table.  Monotonic in P; -1 when P is outside [0, GDC_MAX_SPLATS). */
int64_t gdc_order_workspace_bytes(int32_t P);

/* perm_out (P, int32) = the spatial order of the text above: 3 + 4 x 3 launches (kernels only).  xyz (P, 3) fp32; binding (P, int32 or
 * int64) and face_centers (F, 3) fp32 are given together (bound, F > 0) or both NULL (unbound).  P == 0 launches nothing; P == 1 gives {0}. */
int gdc_morton_order(int32_t P, int32_t F, const void* xyz, const void* binding, int32_t binding_is_i64, const void* face_centers,
                     void* perm_out, void* workspace, void* stream);

/* dst[r] = src[perm[r]], r < P, for every tensor of the HOST table (ntensors <= GDC_MAX_TENSORS, every kind GDC_COPY, dst and src distinct
 * buffers of P rows) in ONE launch of the gather's row mover: 16 lanes per row, 16-byte pieces typed for 4-byte alignment.  An int64 tensor is
 * a row of two 4-byte elements; row_floats == 0 moves nothing; perm[r] outside [0, P) reads nothing and writes +0.0.  P == 0 or
 * ntensors == 0 launches nothing. */
int gdc_permute(int32_t P, const void* perm, int32_t ntensors, const GdcTensor* tensors, void* stream);

/* bytes of gdc_knn3_dist2's scratch buffer (16-byte aligned; its contents need not survive between calls): the sorted positions (16 bytes a
 * point), the chunk boxes (32 bytes each), the permutation and the order's own scratch.  Monotonic in P; -1 when P is outside
 * [0, GDC_MAX_SPLATS). */
int64_t gdc_knn_workspace_bytes(int32_t P);

/* dist2_out (P, fp32, input row order) = the mean squared distance of every row of xyz (P, 3) fp32 to its 3 nearest other rows, per the text
 * above: 15 + 2 launches.  NULL pointers, P < 0 and P >= GDC_MAX_SPLATS return GDC_E_ARG before anything touches a device; P == 0 launches
 * nothing (and needs no pointer). */
int gdc_knn3_dist2(int32_t P, const void* xyz, void* dist2_out, void* workspace, void* stream);

/* Optional per-kernel timing, as gop_profile_* (include/gop.h). */
int gdc_profile_enable(int on);
int gdc_profile_collect(void);
int gdc_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gdc_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GDC_H */
