/*
 * gdc.h -- C ABI of adaptive density control ("Gaussian density control"): the end state of the reference's
 * `densify_and_prune` (scene/gaussian_model.py:501-515: densify_and_clone, densify_and_split, prune_points) in five launches
 * and ONE host read, for the six leaves, their twelve Adam moments, the three statistics, `binding` and `binding_counter`.
 * tests/densify_ref.py states the same contract in float64 numpy.
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
 */
#ifndef GDC_H
#define GDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDC_ABI_VERSION 1
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

/* Optional per-kernel timing, as gop_profile_* (include/gop.h). */
int gdc_profile_enable(int on);
int gdc_profile_collect(void);
int gdc_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gdc_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GDC_H */
