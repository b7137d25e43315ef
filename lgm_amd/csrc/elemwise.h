// lgm_amd/csrc/elemwise.h -- device-side helpers shared by the elementwise / layout kernel files (mvattn.hip,
// gnsilu.hip): element conversions, fixed-order workgroup sums, 4- and 8-element vector accesses, and the host-side
// dtype code -> type dispatch. (attention.hip keeps its own: compiler-native types, other build flags.)
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "common.h"
#include "lgm_attn.h"

namespace lgm {

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float to_f(__half v) { return __half2float(v); }
template <class T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ __half from_f<__half>(float v) { return __float2half(v); }

// sums over a workgroup of 256 / 512 threads; red: 4 / 8 floats of LDS
__device__ __forceinline__ float block_sum256(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // red is reused between calls
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);  // fixed order: every thread gets the same value
}
__device__ __forceinline__ float block_sum512(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // red is reused between calls
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));  // fixed order
}

// 4 / 8 consecutive elements as one access (8 fp32: two); p is aligned to the access: 16 B, or 8 B for 4 x 16 bits
template <class T>
__device__ __forceinline__ void load4(const T *p, float *o) {
    if constexpr (sizeof(T) == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        T e[4];
        *reinterpret_cast<uint2 *>(e) = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = to_f(e[j]);
    }
}
template <class T>
__device__ __forceinline__ void store4(T *p, const float *v) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        T e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) e[j] = from_f<T>(v[j]);
        *reinterpret_cast<uint2 *>(p) = *reinterpret_cast<const uint2 *>(e);
    }
}
template <class T>
__device__ __forceinline__ void load8(const T *p, float *o) {
    if constexpr (sizeof(T) == 4) {
        const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    } else {
        T e[8];
        *reinterpret_cast<uint4 *>(e) = *reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = to_f(e[j]);
    }
}
template <class T>
__device__ __forceinline__ void store8(T *p, const float *v) {
    if constexpr (sizeof(T) == 4) {
        reinterpret_cast<float4 *>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4 *>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        T e[8];
#pragma unroll
        for (int j = 0; j < 8; j++) e[j] = from_f<T>(v[j]);
        *reinterpret_cast<uint4 *>(p) = *reinterpret_cast<const uint4 *>(e);
    }
}

// fn(T{}) with the element type of an LGM_ATTN_F32 / BF16 / F16 code; `who` names the caller in the error text
template <class Fn>
int with_type(const char *who, int code, Fn &&fn) {
    switch (code) {
        case LGM_ATTN_F32: return fn(float{});
        case LGM_ATTN_BF16: return fn(__hip_bfloat16{});
        case LGM_ATTN_F16: return fn(__half{});
    }
    set_error("%s: bad dtype %d", who, code);
    return LGM_E_INVALID;
}

}  // namespace lgm
