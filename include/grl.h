/*
 * grl.h -- C ABI of the fused splat regularisers ("Gaussian regulariser losses"): the two terms the reference's loop adds for
 * every mesh-bound model (train.py:134-146 with metric_xyz = metric_scale = False, the defaults of arguments/__init__.py:100-105),
 *
 *     xyz   : mean over visible splats of  relu(||_xyz_i|| - threshold_xyz)
 *     scale : mean over visible splats of  || relu(exp(_scaling_i) - threshold_scale) ||
 *
 * in ONE launch forward and ONE launch backward, without the boolean-mask gather (a nonzero and a host wait per term in composed
 * torch) and without a per-splat buffer between the two passes: the backward recomputes from the inputs.
 *
 * Conventions as gls.h: DEVICE pointers, fp32, contiguous; 0 / <0 return codes with grl_last_error(); everything is enqueued on
 * `stream`; nothing synchronises, allocates or copies to the host.  `visible` is P bytes, zero / non-zero (a torch.bool tensor).
 * Rows whose base pointers are 16-byte aligned (`visible`: 4-byte) are read and written 16 bytes per lane; any other alignment (a
 * multiple of 4; `visible`: any) takes the element-wise path of the same kernel.
 *
 * Contract, per splat i, c = number of visible splats (fp32, every operation rounded on its own: the translation unit is compiled
 * with -ffp-contract=off; division and square root correctly rounded; exp is the device library's expf):
 *
 *   relu(d)      = 0 where d <= 0, else d  (a NaN stays a NaN, as in torch)
 *   xyz term     n = sqrt(x*x + y*y + z*z),  a_i = relu(n - t_xyz)
 *                d_xyz[i] = (g_xyz / c) * (xyz_i / n)          where visible[i] and n - t_xyz > 0
 *                         = +0.0                               otherwise (n == 0 and n == t_xyz included)
 *   scale term   e_j = exp(s_j),  v_j = relu(e_j - t_s),  b_i = sqrt(v_0*v_0 + v_1*v_1 + v_2*v_2)
 *                d_log_scaling[i][j] = ((g_scale / c) * (v_j / b_i)) * e_j     where visible[i] and v_j > 0
 *                                    = +0.0                                    otherwise
 *   means        xyz_mean = (sum of a_i over visible i) / c,   scale_mean = (sum of b_i over visible i) / c
 *                c == 0: both means are NaN (mean() of an empty tensor) and both gradients are all +0.0
 *
 * Non-finite inputs are not hidden: a NaN or +-Inf among the visible rows reaches the mean it belongs to (the per-workgroup partials
 * are plain floats, the thresholds are applied with comparisons that let a NaN through); the gradients of non-finite rows are
 * unspecified.  Invisible rows are never read into a sum, whatever they hold.
 *
 * Reductions run in a fixed order: a workgroup reduces its GRL_SLAB splats in a fixed tree and writes one partial per term; the
 * workgroup that arrives last (one integer atomic per workgroup on the arrival word) sums the partials in double in a fixed tree over
 * the workgroup index, writes `out` and resets the arrival word -- whatever the data held.  No float atomics: two calls on the same
 * inputs return identical bits.
 */
#ifndef GRL_H
#define GRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_ABI_VERSION 1
#define GRL_OK 0
#define GRL_E_ARG (-1)
#define GRL_E_HIP (-2)
/* splats one workgroup reads (256 lanes, four consecutive splats each) */
#define GRL_SLAB 1024
/* P must stay below this: the count of visible splats is handed out as an exact float */
#define GRL_MAX_SPLATS (1 << 24)

int grl_abi_version(void);
const char* grl_last_error(void);

/* Bytes of caller-owned scratch for P splats: the arrival word (a 16-byte block at the start) and one 16-byte partial per workgroup.
 * The caller zeroes it ONCE when it allocates it; every call leaves it ready for the next call on the same stream.  Two streams must
 * not share one scratch.  <0 (GRL_E_ARG) for P < 0 or P >= GRL_MAX_SPLATS. */
int64_t grl_scratch_bytes(int32_t P);

/* out[4] = {xyz_mean, scale_mean, count, 0}.  P == 0 launches no kernel and sets out = {NaN, NaN, 0, 0} with two stream-ordered fills
 * (xyz, log_scaling, visible and scratch may then be NULL).  P >= GRL_MAX_SPLATS is GRL_E_ARG. */
int grl_forward(int32_t P, const void* xyz, const void* log_scaling, const void* visible, float threshold_xyz, float threshold_scale,
                void* out, void* scratch, void* stream);

/* `out` is what grl_forward wrote for the same inputs (only the count is read).  g_xyz / g_scale: single DEVICE floats, the upstream
 * gradients of the two means; either may be NULL, meaning zero.  d_xyz / d_log_scaling: (P,3), either may be NULL, meaning not wanted
 * (both NULL: nothing is launched).  Every row of a requested output is written -- the caller passes uninitialised memory; a
 * requested output whose g is NULL is all zeros.  P == 0 launches nothing. */
int grl_backward(int32_t P, const void* xyz, const void* log_scaling, const void* visible, float threshold_xyz, float threshold_scale,
                 const void* out, const void* g_xyz, const void* g_scale, void* d_xyz, void* d_log_scaling, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gop_profile_* (include/gop.h). */
int grl_profile_enable(int on);
int grl_profile_collect(void);
int grl_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int grl_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GRL_H */
