/*
 * gms.h -- C ABI of the fused METRIC-SPACE splat regularisers ("Gaussian metric-space regularisers"): the two terms the reference's loop
 * adds for a mesh-bound model when --metric_xyz / --metric_scale are set (train.py:136 and :143),
 *
 *     xyz   : mean over visible splats of  || relu(_xyz_i * face_scaling[binding_i] - threshold_xyz) ||
 *     scale : mean over visible splats of  || relu(exp(_scaling_i) * face_scaling[binding_i] - threshold_scale) ||
 *
 * in ONE launch forward and ONE launch backward for the per-splat gradients, plus one more backward launch when the gradient into
 * `face_scaling` is wanted: the per-face reduction over the binding's CSR (binding.binding_csr, the rows-then-faces scheme of
 * gab_bind_backward_csr).  No boolean-mask gather, no host wait, no per-splat buffer between forward and backward (the backward
 * recomputes from the inputs), and get_scaling's binding launch is not repeated.  grl.h holds the local forms of the same two terms.
 *
 * Conventions as grl.h: DEVICE pointers, fp32, contiguous; 0 / <0 return codes with gms_last_error(); everything is enqueued on
 * `stream`; nothing synchronises, allocates or copies to the host.  `visible` is P bytes, zero / non-zero (a torch.bool tensor).
 * `binding` is P int32 or, with index_is_i64 != 0, P int64 (as gab.h).  `face_scaling` is F floats.  When every per-splat base pointer
 * of a call is 16-byte aligned (`visible`: 4-byte) a lane reads and writes 16 bytes at a time; any other alignment (a multiple of the
 * element size; `visible`: any) takes the element-wise path of the same kernel.  The gather from `face_scaling` is 4 bytes per splat.
 *
 * Contract, per splat i, f = face_scaling[binding[i]], c = number of visible splats (fp32, every operation rounded on its own: the
 * translation unit is compiled with -ffp-contract=off; division and square root correctly rounded; exp is the device library's expf):
 *
 *   relu(d)      = 0 where d <= 0, else d  (a NaN stays a NaN, as in torch)
 *   xyz term     u_j = relu(x_j * f - t_xyz),  m_i = sqrt((u_0*u_0 + u_1*u_1) + u_2*u_2)          (the relu is per component)
 *                d_xyz[i][j] = (g_xyz / c) * (u_j / m_i) * f                      where visible[i] and u_j > 0,  else +0.0
 *   scale term   e_j = expf(s_j),  v_j = relu(e_j * f - t_s),  b_i = sqrt((v_0*v_0 + v_1*v_1) + v_2*v_2)
 *                d_log_scaling[i][j] = (g_scale / c) * (v_j / b_i) * f * e_j      where visible[i] and v_j > 0,  else +0.0
 *   means        xyz_mean = (sum of m_i over visible i) / c,   scale_mean = (sum of b_i over visible i) / c
 *   faces        d_face_scaling[k] = sum over visible i with binding[i] == k of
 *                                    (g_xyz / c) * sum_j (u_j / m_i) x_j  +  (g_scale / c) * sum_j (v_j / b_i) e_j
 *   The three gradient lines start from the fp32 values above (u_j, v_j, e_j, f, and g / c as one fp32 division) and are formed in
 *   double -- the norm of the same u_j (v_j) in double, the quotients, the products -- then rounded to fp32 once; a face's splats are
 *   added in double in a fixed order before that one rounding.  Faces without splats: +0.0.
 *   m_i == 0 (b_i == 0, the fp32 norms of the forward) contributes zero everywhere: torch's subgradient of norm at 0.
 *   c == 0: both means are NaN (mean() of an empty tensor) and every gradient is +0.0.
 *
 * A term is selected per call: the forward computes the xyz term iff `xyz` is not NULL and the scale term iff `log_scaling` is not NULL;
 * the backward takes a term iff its upstream gradient is not NULL.  A term that is off is neither read nor computed.
 *
 * binding[i] outside [0, F) never reads out of bounds: such a visible splat has f = NaN (which reaches its means) and contributes to no
 * face.  Non-finite inputs are not hidden: a NaN or +-Inf among the visible rows reaches the mean it belongs to; the gradients of
 * non-finite rows are unspecified.  Invisible rows are never read into a sum, whatever they hold.
 *
 * Reductions run in a fixed order.  Forward: a lane adds its visible terms in splat order, a workgroup reduces its GMS_SLAB splats in a
 * fixed tree and writes one partial per term; the workgroup that arrives last (one integer atomic per workgroup on the arrival word)
 * sums the partials in a fixed tree over the workgroup index, writes `out` and resets the arrival word -- whatever the data held.  The
 * sums are carried in double from the first addition on.  Faces: 16 lanes per face, lane l adds entries l, l + 16, ... of the face's
 * contiguous CSR run, then a fixed tree.  No float atomics anywhere: two calls on the same inputs return identical bits.
 */
#ifndef GMS_H
#define GMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMS_ABI_VERSION 1
#define GMS_OK 0
#define GMS_E_ARG (-1)
#define GMS_E_HIP (-2)
/* splats one workgroup reads (256 lanes, four consecutive splats each) */
#define GMS_SLAB 1024
/* P must stay below this: the count of visible splats is handed out as an exact float */
#define GMS_MAX_SPLATS (1 << 24)
/* bytes per splat of the backward's `rows`: the splat's one contribution to its face, parked at its CSR slot */
#define GMS_ROW_BYTES 8

int gms_abi_version(void);
const char* gms_last_error(void);

/* Bytes of caller-owned forward scratch for P splats bound to F faces: the arrival word (a 16-byte block at the start) and one 32-byte
 * partial per workgroup (F does not enter the size; it is checked like everywhere else).  The caller zeroes it ONCE when it allocates
 * it; every call leaves it ready for the next call on the same stream.  Two streams must not share one scratch.
 * <0 (GMS_E_ARG) for P < 0, P >= GMS_MAX_SPLATS or F < 1. */
int64_t gms_scratch_bytes(int32_t P, int32_t F);

/* out[4] = {xyz_mean, scale_mean, count, 0}; the mean of a term that is off (NULL xyz / NULL log_scaling) is written as +0.0.  Both
 * NULL is GMS_E_ARG.  P == 0 launches no kernel and sets out = {NaN, NaN, 0, 0} with two stream-ordered fills (every other pointer
 * may then be NULL).  P >= GMS_MAX_SPLATS is GMS_E_ARG. */
int gms_forward(int32_t P, int32_t F, const void* xyz, const void* log_scaling, const void* face_scaling, const void* binding,
                int32_t index_is_i64, const void* visible, float threshold_xyz, float threshold_scale, void* out, void* scratch,
                void* stream);

/* `out` is what gms_forward wrote for the same inputs (only the count is read).  g_xyz / g_scale: single DEVICE floats, the upstream
 * gradients of the two means; a NULL one switches its term off (`xyz` / `log_scaling` may then be NULL too).  d_xyz / d_log_scaling:
 * (P,3), d_face_scaling: F floats; each may be NULL, meaning not wanted (all NULL: nothing is launched).  Every element of a requested
 * output is written -- the caller passes uninitialised memory; a requested output whose term is off is all zeros.
 * d_face_scaling needs the binding's CSR, face_begin (F + 1 int32) and slot (P int32, the splat's position in face order), and `rows`,
 * P * GMS_ROW_BYTES bytes of uninitialised 8-byte aligned memory: the first launch parks every splat's contribution there, a second
 * launch sums each face's run.  Without d_face_scaling the three may be NULL and the second launch does not happen.
 * P == 0 launches no kernel (a requested d_face_scaling is zero-filled on the stream). */
int gms_backward(int32_t P, int32_t F, const void* xyz, const void* log_scaling, const void* face_scaling, const void* binding,
                 int32_t index_is_i64, const void* visible, float threshold_xyz, float threshold_scale, const void* out,
                 const void* g_xyz, const void* g_scale, void* d_xyz, void* d_log_scaling, void* d_face_scaling,
                 const void* face_begin, const void* slot, void* rows, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gop_profile_* (include/gop.h). */
int gms_profile_enable(int on);
int gms_profile_collect(void);
int gms_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gms_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GMS_H */
