// Per-element arithmetic of the RepBlock BatchNorm passes, shared by every kernel that forms it: the elementwise passes of
// rep_bn.hip and the data-gradient kernel that forms the branch gradients in its own prologue (conv_rows.hip, MODE 2).  All of them
// compile these explicit fma chains and no other expression, so the same inputs give the same bits wherever they are computed.
#pragma once
#include "common.h"

__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf16lo(v[i]); f[2 * i + 1] = bf16hi(v[i]); }
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    return v;
}
__device__ __forceinline__ void load8f(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[4 + i] = b[i]; }
}

// pre-activation of the fused block output.  ONE explicit fma chain used by the forward apply and by the backward kernels that
// recompute the ReLU mask from it (hc_rep_bwd_*_z): the same inputs give the same bits, so (z > 0) there IS (out > 0) here
// (out = bf16(relu(z)) > 0 exactly when z > 0: a positive fp32 never rounds to a bf16 zero above 2^-134).
template <bool HAS_ID>
__device__ __forceinline__ float rep_preact(float a3, float f3, float a1, float f1, float a0, float f0, float sh) {
    float z = __builtin_fmaf(a1, f1, sh);
    if (HAS_ID) z = __builtin_fmaf(a0, f0, z);
    return __builtin_fmaf(a3, f3, z);
}

// backward apply: dz = g where the block's output (or its recomputed pre-activation) `fo` is positive, and the gradient of one
// branch's conv output y from the coefficients (A, B, C) of hc_rep_bn_bwd_finalize: dy = A dz + (B y + C)
__device__ __forceinline__ float rep_bwd_dz(float fo, float g) { return fo > 0.f ? g : 0.f; }
__device__ __forceinline__ float rep_bwd_branch(float A, float dz, float B, float y, float Cc) {
    return __builtin_fmaf(A, dz, __builtin_fmaf(B, y, Cc));
}
