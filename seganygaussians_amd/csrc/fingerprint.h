// fingerprint.h -- kernels of the geometry cache: content fingerprints of device arrays (mi_rast_fingerprint) and the hand-over of an
// earlier forward's binning results to a fresh image buffer (mi_rast_forward_reuse).  Independent of every other stage.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

// ---- content fingerprints (mi_rast_fingerprint, include/mi_rast.h) ---------------------------------------------------------
constexpr int MI_FP_MAX = 8;      // arrays per call
constexpr int FP_BLOCKS = 128;    // partial sums per array (summed by the host)
struct FingerprintArgs {
    const uint32_t* ptr[MI_FP_MAX];
    unsigned long long words[MI_FP_MAX];
};
// blockIdx.y = array; every word is hashed together with its position (murmur3's finaliser) and the hashes are summed: order of
// summation does not matter, order of the words does.
__global__ void __launch_bounds__(256) fingerprint_kernel(FingerprintArgs a, unsigned long long* __restrict__ out)
{
    const int k = blockIdx.y;
    const uint32_t* p = a.ptr[k];
    const unsigned long long n = a.words[k];
    unsigned long long sum = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)FP_BLOCKS * 256ull) {
        uint32_t x = p[i] ^ ((uint32_t)i * 0x9E3779B1u + (uint32_t)(i >> 32));
        x ^= x >> 16;
        x *= 0x85EBCA6Bu;
        x ^= x >> 13;
        x *= 0xC2B2AE35u;
        x ^= x >> 16;
        sum += (unsigned long long)x * 0x9E3779B97F4A7C15ull + i;
    }
    __shared__ unsigned long long s_part[4];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);   // (not wave.h's wave_sum: the kernel's code would change)
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) out[k * FP_BLOCKS + blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// mi_rast_forward_reuse (include/mi_rast.h): a fresh image buffer takes over what the binning stages of an earlier forward of the same
// geometry and camera left in theirs -- ranges, {R, longest list, key bits}, the XCD run boundaries -- and gets the blend kernels'
// per-tile walk counters zeroed, as tile_ranges_kernel leaves them.
__global__ void __launch_bounds__(256) reuse_image_state_kernel(uint32_t ntiles, const uint2* __restrict__ src_ranges,
                                                                const int* __restrict__ src_words, uint2* __restrict__ ranges,
                                                                int* __restrict__ words, uint32_t* __restrict__ zero_a,
                                                                uint32_t* __restrict__ zero_b)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < ntiles) {
        ranges[t] = src_ranges[t];
        zero_a[t] = 0u;
        zero_b[t] = 0u;
    }
    if (t < 16u) words[t] = src_words[t];   // {R, longest list, -, key bits, run boundaries}: the 16 words behind the R partial sums
}

}  // namespace mirast
