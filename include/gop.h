/*
 * gop.h -- C ABI of the fused optimizer step ("Gaussian optimizer"): the line that follows the backward pass in the
 * reference's loop, `gaussians.optimizer.step()` (train.py:209), for the optimizer the reference constructs
 * (scene/gaussian_model.py:222: torch.optim.Adam(l, lr=0.0, eps=1e-15), nine parameter groups, twelve tensors).
 *
 *   gop_adam_step   torch.optim.Adam's update (amsgrad=False, weight_decay=0, maximize=False) of up to GOP_MAX_TENSORS
 *                   tensors in ONE launch: every tensor has its own learning rate and its own step count, both folded
 *                   into two host-computed floats per tensor.
 *
 * Conventions as gls.h: DEVICE pointers, fp32, contiguous; 0 / <0 return codes with gop_last_error(); everything is
 * enqueued on `stream`, nothing synchronises, no device-side persistent state.  The descriptor table is a HOST array: it
 * travels by value in the kernel arguments (no H2D copy, no staging buffer), so the caller may rebuild it on every step --
 * the pointers change at every densification.
 *
 * Arithmetic, per element, in fp32 (fma = one fused multiply-add, rounded once; every other operation is rounded on its own; the
 * translation unit is compiled with -ffp-contract=off, so the compiler fuses nothing else; division and square root are correctly
 * rounded; denormals are kept):
 *
 *     m  = fma(one_minus_beta1, g - m, m)                  (Tensor.lerp_(grad, 1 - beta1), weight < 0.5:  m + w * (g - m))
 *     v  = v * beta2
 *     v  = fma(one_minus_beta2, g * g, v)                  (addcmul_(grad, grad, value = 1 - beta2):      v + w * (g * g))
 *     q  = sqrt(v) / bias_correction2_sqrt + eps
 *     p  = fma(-step_size, m / q, p)                       (addcdiv_(exp_avg, denom, value = -step_size): p - s * (m / q))
 *
 * which is torch's _multi_tensor_adam (amsgrad=False, weight_decay=0, maximize=False) operation by operation, with the three
 * multiply-adds fused exactly where torch's own GPU foreach kernels fuse them: on the MI355X with torch 2.10 the results are bit for
 * bit those of torch.optim.Adam on the same device (tests/test_optim_gpu.py reports it; what it requires is the bar stated there).
 * Evaluated without fusing -- torch's CPU path -- the same expressions differ from these by a rounding of m and of v per step.
 * g = 0 on m = v = 0 gives q = eps, m / q = 0 and p unchanged (eps > 0: with eps = 0 that element is 0 / 0, as in torch).
 */
#ifndef GOP_H
#define GOP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOP_ABI_VERSION 1
#define GOP_OK 0
#define GOP_E_ARG (-1)
#define GOP_E_HIP (-2)
/* tensors per launch: the table (52 bytes per tensor) has to fit the 4 KiB kernel-argument segment */
#define GOP_MAX_TENSORS 32
/* elements of one tensor that one workgroup updates */
#define GOP_SLAB 2048

int gop_abi_version(void);
const char* gop_last_error(void);

typedef struct {
    void* param;                  /* n floats, updated in place */
    const void* grad;             /* n floats */
    void* exp_avg;                /* n floats, updated in place */
    void* exp_avg_sq;             /* n floats, updated in place */
    int64_t n;                    /* >= 0; an empty tensor is skipped */
    float step_size;              /* lr / (1 - beta1^step), formed in double on the host as torch does */
    float bias_correction2_sqrt;  /* sqrt(1 - beta2^step), likewise */
} GopAdamTensor;

/* One Adam step of `ntensors` tensors (HOST array), ceil(ntensors / GOP_MAX_TENSORS) launches.  The four arrays of a tensor
 * whose pointers are all 16-byte aligned are read and written 16 bytes per lane; any other alignment (a multiple of 4) takes
 * the element-wise path of the same kernel.  The arrays of different tensors must not overlap.
 * one_minus_beta1 / one_minus_beta2 are formed here as (float)(1.0 - (double)beta): for beta2 = 0.999f that is
 * 0.00099998713, 1.3e-5 away from the 0.001f torch multiplies by (torch rounds the double 1 - 0.999 to fp32; a float beta has
 * already lost those digits).  A caller that holds the betas in double -- optim.FusedAdam -- uses gop_adam_step_ex. */
int gop_adam_step(int32_t ntensors, const GopAdamTensor* tensors, float beta1, float beta2, float eps, void* stream);

/* The same with the two complements given by the caller, each formed in double and rounded once, as torch passes them:
 * one_minus_beta1 = (float)(1.0 - beta1), one_minus_beta2 = (float)(1.0 - beta2). */
int gop_adam_step_ex(int32_t ntensors, const GopAdamTensor* tensors, float beta1, float one_minus_beta1, float beta2,
                     float one_minus_beta2, float eps, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gls_profile_* (include/gls.h): off by default; when on, every
 * launch of this library is bracketed by an event pair; gop_profile_collect() synchronises the pending pairs, ADDS their elapsed times
 * to a table keyed by kernel name and returns the number of table entries; gop_profile_entry(i, ...) reads entry i (-1 past the end);
 * gop_profile_reset() empties the table. */
int gop_profile_enable(int on);
int gop_profile_collect(void);
int gop_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gop_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GOP_H */
