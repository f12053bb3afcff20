// bn_embed.hip — the embedding output of unfused plans.
//
// Where the plan runs the head's pooling as its own operator (INT8 MEAN / attention pooling with the fused tail off or absent, float32
// GAP / attention pooling of fuse=False plans), the pooled vector is already in that operator's output slot.  One launch right behind the
// operator copies it into the caller's buffer, or dequantises it as (float)(q - zp) * scale — the arithmetic of the head kernels' logits.
// The fused kernels (i8_tail2_kernel, i8_tail_kernel, f32_gap_dense_kernel) write the vector themselves from where they pool it.
#include <hip/hip_runtime.h>

#include "bn_kernels.h"

namespace bn {

// one thread per four elements: a dword (int8) or a float4 load, a dword or a float4 store
template <bool SRC_I8, bool DST_F32>
__global__ __launch_bounds__(256) void emb_store_kernel(const void* __restrict__ src, void* __restrict__ dst, long n4, float scale, int zp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    if constexpr (SRC_I8) {
        const int q = reinterpret_cast<const int*>(src)[i];
        if constexpr (DST_F32) {
            float4 v;
            v.x = (float)((int)(int8_t)q - zp) * scale;
            v.y = (float)((int)(int8_t)(q >> 8) - zp) * scale;
            v.z = (float)((int)(int8_t)(q >> 16) - zp) * scale;
            v.w = (float)((q >> 24) - zp) * scale;
            reinterpret_cast<float4*>(dst)[i] = v;
        } else {
            reinterpret_cast<int*>(dst)[i] = q;
        }
    } else {
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    }
}

void launch_emb_store(const void* src, bool src_i8, void* dst, bool dst_f32, int B, int D, float scale, int zp, hipStream_t s) {
    const long n4 = (long)B * D / 4;
    if (n4 <= 0) return;
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (!src_i8)
        hipLaunchKernelGGL((emb_store_kernel<false, true>), grid, dim3(256), 0, s, src, dst, n4, scale, zp);
    else if (dst_f32)
        hipLaunchKernelGGL((emb_store_kernel<true, true>), grid, dim3(256), 0, s, src, dst, n4, scale, zp);
    else
        hipLaunchKernelGGL((emb_store_kernel<true, false>), grid, dim3(256), 0, s, src, dst, n4, scale, zp);
}

}  // namespace bn
