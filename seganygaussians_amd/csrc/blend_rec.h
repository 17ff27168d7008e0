// blend_rec.h -- the 32-byte geometry record of a Gaussian and the four-byte entry of a tile's blend list: what the preprocess pass
// (geometry.h) writes, the count / emit passes read in index order, the per-tile sort packs, and the blend, lift and geometry
// backward kernels gather per list entry.  Nothing else of the binning stages is needed to walk a list.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirast {

constexpr int ID_BITS = 28;            // list entry = Gaussian id | quadrant mask << 28
constexpr uint32_t ID_MASK = (1u << ID_BITS) - 1u;

// Everything needed to evaluate a Gaussian at a pixel in ONE 32-byte record (the reference gathers id -> xy -> conic per batch
// with dependent loads, forward.cu:318-326): written per VISIBLE Gaussian by the preprocess pass (index_rec, `pm` = radius; the
// slots of culled Gaussians are not written -- depth_key says which), read in index order by the count / emit passes, and what the
// blend kernels gather per list entry.
struct __attribute__((aligned(16))) BlendRec {
    float2 xy;       // pixel-space mean
    uint32_t id;     // index_rec: the DEPTH BITS of the Gaussian (its index is where the record lies; the emit pass gets the sort key with the
                     // record instead of a second 4-byte gather); a staged list record (list_record): the Gaussian index (feature row)
    uint32_t pm;     // (position in the tile list) << 4 | quadrant mask
    float4 co;       // conic A,B,C + opacity
};
static_assert(sizeof(BlendRec) == 32, "BlendRec must be 32 bytes");

// Entry i of a tile's blend list (4 bytes: Gaussian id | quadrant mask << 28, tile_sort.h: emit_blend_list) as a full record: the
// geometry record of that Gaussian (index_rec, written by the preprocess pass) with `pm` = position << 4 | quadrant mask.  For the
// kernels that walk a list in whole batches (blend_fwd.h, blend_bwd.h); the wave kernels gather per quadrant.
__device__ __forceinline__ BlendRec list_record(const uint32_t* __restrict__ lst, const BlendRec* __restrict__ index_rec, int i)
{
    const uint32_t e = lst[i];
    BlendRec r = index_rec[e & ID_MASK];
    r.id = e & ID_MASK;   // (the stored word holds the depth bits)
    r.pm = ((uint32_t)i << 4) | (e >> ID_BITS);
    return r;
}

}  // namespace mirast
