// antialias.h -- the antialiased render mode (MI_RAST_ANTIALIAS, include/mi_rast.h): the opacity of a Gaussian is scaled by
// h = sqrt(det(Sigma) / det(Sigma + 0.3 I)), the energy the 0.3 px screen filter of cov2d_common adds to its footprint.
// ONE definition of rho and of h for the preprocess kernel and for the geometry backward (geometry.h): the backward recovers the raw
// opacity as w / h from the stored w, so both must round h identically.  Every operation rounded on its own (-ffp-contract=off).
#pragma once

namespace mirast {

__device__ constexpr float AA_RHO_FLOOR = 0.000025f;   // h >= 0.005; at or under it h is a constant: no covariance gradient

// rho = det0 / det1: (a0, b, c0) the 2-D covariance BEFORE the dilation, det1 the determinant after it (nonzero: the det == 0 cull)
__device__ __forceinline__ float aa_rho(float a0, float b, float c0, float det1)
{
    const float det0 = a0 * c0 - b * b;
    return det0 / det1;
}

__device__ __forceinline__ float aa_h(float rho) { return sqrtf(fmaxf(AA_RHO_FLOOR, rho)); }

// What the geometry backward hands to its AA = true instantiation in place of the packed gradients alone: the stored w of the forward
struct GeomBwdPackAA {
    const float* gpack;
    const float4* conic_opacity;
};
template <bool AA>
struct GeomBwdPack { using type = const float* __restrict__; };
template <>
struct GeomBwdPack<true> { using type = GeomBwdPackAA; };
__device__ __forceinline__ const float* packed_gradients(const float* p) { return p; }
__device__ __forceinline__ const float* packed_gradients(const GeomBwdPackAA& p) { return p.gpack; }

}  // namespace mirast
