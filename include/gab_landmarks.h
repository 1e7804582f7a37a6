/*
 * gab_landmarks.h -- the landmark and root-centring entries of libgab_hip.so: the two switches of FlameHead.forward
 * (flame_model/flame.py:532-553, flame_model/lbs.py:60-98) that include/gab.h's gab_flame_* leave out.
 *
 * A companion of gab.h (which it includes for GabRig, the return codes and the conventions: device pointers, fp32, contiguous
 * tensors, everything enqueued on `stream`, nothing synchronises), in a header of its own because gab.h's list of entries is frozen
 * at ABI 5: these are purely additive exports of the same library, GAB_ABI_VERSION does not move, and a library built before them
 * fails to resolve them when gaussianavatars_amd._lib.gab_landmarks() first asks (never a fallback).  One pose per call, like gab_flame_*.
 */
#ifndef GAB_LANDMARKS_H
#define GAB_LANDMARKS_H

#include "gab.h"

#ifdef __cplusplus
extern "C" {
#endif

/* landmarks[l][c] = sum_k lmk_bary[l][k] * verts[faces[lmk_face[l]][k]][c], k ascending as an fmaf chain, one lane per (landmark,
 * coordinate), one launch; L == 0 returns GAB_OK without one.  lmk_face: int32 (L,), lmk_bary: fp32 (L,3); `faces` as
 * gab_face_frames_forward.  An lmk_face entry outside [0, F) cannot be reported without a read-back: the caller validates the embedding
 * on the host when it is attached; the kernels skip such an entry (its landmark is NaN, it adds nothing to a gradient) and never
 * address through it. */
int gab_landmarks_forward(int32_t V, int32_t F, int32_t L, const float* verts /*(V,3)*/, const void* faces /*(F,3)*/, int32_t index_is_i64,
                          const int32_t* lmk_face, const float* lmk_bary, float* landmarks /*(L,3)*/, void* stream);

/* d_verts[v] (+)= sum over (l,k) with faces[lmk_face[l]][k] == v of lmk_bary[l][k] * d_landmarks[l], without atomics: the caller builds
 * a CSR over the vertices once per (faces, embedding) -- lmk_order (int32, 3L): the corner numbers 3 l + k sorted by (vertex, l, k);
 * vert_begin (int32, V+1): offsets of every vertex's row in it -- and one lane per vertex walks its row in that order, so the result is the
 * same bits run after run.  accumulate != 0: the row sums are ADDED to d_verts (the gradient arriving from another consumer of the
 * vertices); accumulate == 0: every element of d_verts is WRITTEN, zeros for the vertices no landmark touches -- the lanes run over all V
 * vertices, so nobody zero-fills the buffer first (no memset, no gab_zero_buffers call). */
int gab_landmarks_backward(int32_t V, int32_t F, int32_t L, const void* faces, int32_t index_is_i64, const int32_t* lmk_face,
                           const float* lmk_bary, const int32_t* lmk_order, const int32_t* vert_begin, const float* d_landmarks /*(L,3)*/,
                           float* d_verts /*(V,3)*/, int32_t accumulate, void* stream);

/* root[c] = sum_v J_regressor[0][v] * v_shaped[v][c]: the root joint, which lbs leaves where it is (it rotates about itself: the first
 * transform of flame_model/lbs.py:283-296 has the rest joint as its translation column), so this IS J[:, 0] of flame.py:533 before the
 * translation.  One workgroup; each of its 16 waves sums a fixed contiguous span of v, the 16 partial sums are added in wave order. */
int gab_root_joint(const GabRig* rig, const float* v_shaped /*(V,3)*/, float* root /*3*/, void* stream);

/* out[v][c] = (verts[v][c] - root[c]) + translation[c]: flame.py:533 and :536 in the reference's order, for vertices computed with a zero
 * translation.  `out` may alias `verts`. */
int gab_root_center(int32_t V, const float* verts /*(V,3)*/, const float* root /*3*/, const float* translation /*3*/, float* out /*(V,3)*/,
                    void* stream);

/* The backward of gab_root_joint + gab_root_center for dL/d out = d_out (the gradient of `verts` is d_out itself):
 * s[c] = sum_v d_out[v][c] (one workgroup, fixed order, as gab_root_joint), d_translation[c] = s[c] (NULL to skip) and
 * d_v_shaped[v][c] = -J_regressor[0][v] * s[c], fully written -- the buffer gab_flame_backward takes as dL_dv_shaped. */
int gab_root_center_backward(const GabRig* rig, const float* d_out /*(V,3)*/, float* d_v_shaped /*(V,3)*/, float* d_translation /*3 or NULL*/,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAB_LANDMARKS_H */
