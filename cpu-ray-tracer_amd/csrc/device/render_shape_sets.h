// render_shape_sets.h — crt_render_shape_sets: the frames of many cameras over many shapes of a two-level scene in which SEVERAL BLASes deform per shape.
// render_shapes_kernel<1> (render_shapes.h) with one difference: which instances walk the lane's image is not one kernel argument (`bvh`) but a table in device
// memory, instRoot[blasCount] (layout.h ShapeSetMesh): per instance the image-relative reference of its BVH's node 0, or kInstLive.
//
//   ShapeSetWorld   trace:   hit_light_floor, then tlas_walk over the image's TLAS nodes and Instance records (ShapeWorld<1>'s accessors); an instance whose instRoot word
//                            is a reference walks traverse_bvh_seq over the lane's image from that root, any other instance walks Scene::geom from its record's rootRef;
//                   surface, miss: ShapeWorld<1>'s.
//
// Relocation: every sub-image's references are relative to the IMAGE's first byte (shape_build.hip), so ShapeBvh's one per-lane delta serves every mesh of the set.
// Addressing: the lookup is table + (instRootOff + 4 instance): the table's scalar base and a 32-bit per-lane offset, one dword per instance visit.
// LDS, numerics: render_shapes.h's.
#pragma once
#include "render_shapes.h"

namespace crt {

struct ShapeSetWorld : ShapeWorld<1> {
    uint32_t instRoot;                    // instRoot[blasCount]'s offset in the table (wave-uniform)
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
        int traversed = 0, tested = 0;
        const ShapeBvh mine{table, image};
        hit_light_floor(sc, O, D, h);
        tlas_walk(*this, O, D, rD, h, stk + sc.bvhStack * 64, cn, traversed, [&](uint32_t instance, rec4 ids, f3 Oo, f3 Do, f3 rDo) __attribute__((always_inline)) {
            const uint32_t root = *reinterpret_cast<const uint32_t*>(table + (instRoot + instance * 4u));
            if (root != kInstLive) traverse_bvh_seq(mine, root, Oo, Do, rDo, h, stk, cn, traversed, tested);
            else traverse_bvh_seq(sc, asu(ids.z), Oo, Do, rDo, h, stk, cn, traversed, tested);
        });
        return 0u;
    }
};

// the shape of `view`: an index the build launch has found to lie in [0, S) before this kernel is launched
template <class WORLD>
__device__ __forceinline__ WORLD world_of(const ShapeSetTableDev& t, uint32_t view)
{
    const uint32_t s = t.viewShape ? (uint32_t)t.viewShape[view] : view;
    WORLD w;
    w.table = t.table; w.image = t.imagesOff + s * t.imageStride; w.rootRef = 0u; w.bvh = 0u; w.instRoot = t.instRootOff;
    w.tlas = w.image + t.poseRel; w.inst = w.tlas + t.instRel;
    w.tlasRoot = asu(ldg(t.table, w.tlas).w);                                        // TlasNode 0: {lo, ref}
    return w;
}

// render_shapes_kernel<1>'s launch shape, slab, seeds and camera handling: the same body over the lane's ShapeSetWorld
__global__ __launch_bounds__(256, 4) void render_shape_sets_kernel(const Scene sc, const ShapeSetTableDev st, const float* __restrict__ cams, char* __restrict__ slab,
                                                                  Counters* __restrict__ counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                                  uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, uint32_t nEntries)
{
    render_shape_lanes<ShapeSetWorld>(sc, st, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, nEntries);
}

} // namespace crt
