// layout.h — device-side (HBM) scene layout shared by the uploader (host) and the kernels: the records of the geometry buffer, and every struct handed to a kernel by value (Scene,
// AltAccelDev, TlasAltDev, PrimDev), each defined HERE ONLY: the host that fills one and the kernel that reads it cannot disagree.  No device code; the launch wrappers are launch.h's.
//
// ONE geometry buffer holds every record the traversal touches, so a record address is `geom + 32-bit byte offset`
// (scalar base register + per-lane offset: no 64-bit address arithmetic in the hot loop).  Records are sized and
// aligned for 16-byte vector loads (global_load_dwordx4); a traversal step always fetches the 64 bytes at its record.
//   NodePair  64 B  both children of an interior node in one aligned 64-byte line
//   LeafTri   48 B  Möller–Trumbore operands in leaf order (the triangleIndices indirection is resolved at upload)
//   TlasNode  32 B  reference TLASBVHNode layout, leftRight/BLAS replaced by the node's packed reference; the TLAS child pairs section holds, for every
//                   TLAS interior node, its two child TlasNodes side by side (NodePair layout)
//   Instance 128 B  per-BLAS: invT rows + ids in the first 64 B (what entering the BLAS needs), then T rows
//   ShadeTri  64 B  normals + uvs + material of a triangle, addressed by the global shade index carried in LeafTri
#pragma once
#include <stdint.h>

namespace crt {

// packed node reference carried in registers / on the traversal stack (32 bit)
//   bits 31..30 = 10 : BVH / BLAS interior, bits 0..29 = offset of its NodePair in the geometry buffer, in 16-byte units
//   bits 31..30 = 00 : BVH / BLAS leaf,     bits 0..29 = offset of its first LeafTri, in 16-byte units (never 0);  0 = "traversal done"
//   bits 31..30 = 01 : TLAS interior,       bits 0..14 = left child TlasNode index, bits 15..29 = right child
//   bits 31..30 = 11 : TLAS leaf,           bits 0..15 = BLAS (Instance) index;  0xFFFFFFFF = "return to TLAS level" stack marker
constexpr uint32_t kRefInterior = 0x80000000u;
constexpr uint32_t kRefTlasBit = 0x40000000u;
constexpr uint32_t kRefTlasInterior = 0x40000000u;
constexpr uint32_t kRefTlasLeaf = 0xC0000000u;
constexpr uint32_t kRefReturn = 0xFFFFFFFFu;
constexpr uint32_t kRefDone = 0u;
constexpr uint32_t kRefOffsetMask = 0x3fffffffu;
constexpr uint64_t kMaxGeomBytes = 1ull << 32;     // 32-bit byte offsets

// Pool form of the same reference, used by render_pool_kernel for `cur` and for its traversal stack: the same tags and a record INDEX instead of an offset.
// It comes in two widths, and a scene is uploaded in exactly one of them (Scene::poolRefBits); both are stored in the same uint32_t fields (NodeChild::ref16,
// TlasNode::ref16, Instance::rootRef16, Scene::rootRef16 — the names are the narrow form's).
//   16-bit form (2 bytes per stack entry: LDS is what limits the waves per SIMD): tag in bits 15..14, index in bits 13..0, return marker 0xFFFF.
//               Scenes of <= 16382 node pairs and <= 16382 triangles over all BVHs (kRef16MaxIndex each: the highest index a reference carries is the last
//               triangle's, the triangle count itself).
//   32-bit form (4 bytes per stack entry): tag in bits 31..30, index in bits 29..0, return marker 0xFFFFFFFF.  Every other scene: an index is bounded by
//               kMaxGeomBytes (index * 64 and leafOff + index * 48 stay below 2^32), far below 2^30.
// The tags and what the index counts, in either width:
//   10 : BVH / BLAS interior, index of its NodePair                 (record at            index * 64)
//   00 : BVH / BLAS leaf,     index of its first LeafTri + 1; 0 = "traversal done"   (record at leafOff + (index - 1) * 48; the next triangle of the leaf is ref + 1)
//   01 : TLAS interior,       index of its TLAS child pair         (record at tlasPairOff + index * 64)
//   11 : TLAS leaf,           BLAS (Instance) index                (record at instOff + index * 128);  all ones = "return to TLAS level" marker
constexpr uint32_t kRef16Interior = 0x8000u, kRef16TlasBit = 0x4000u, kRef16TlasLeaf = 0xC000u, kRef16TagMask = 0xC000u, kRef16IndexMask = 0x3fffu;
constexpr uint32_t kRef16Return = 0xFFFFu, kRef16MaxIndex = 0x3ffeu;
constexpr uint32_t kRefWideMaxIndex = 0x3ffffffeu;
// the constants of one width, for the writers of those fields (by the scene's poolRefBits) and for the kernel (by its template parameter)
struct PoolRefForm { uint32_t interior, tlasBit, tlasLeaf, tagMask, indexMask, ret; };
constexpr PoolRefForm pool_ref_form(uint32_t bits)
{
    return bits == 32u ? PoolRefForm{kRefInterior, kRefTlasBit, kRefTlasLeaf, 0xC0000000u, kRefOffsetMask, kRefReturn}
                       : PoolRefForm{kRef16Interior, kRef16TlasBit, kRef16TlasLeaf, kRef16TagMask, kRef16IndexMask, kRef16Return};
}

struct alignas(16) NodeChild { float lo[3]; uint32_t ref; float hi[3]; uint32_t ref16; };   // 32 B; ref / ref16 = the child's packed reference: offset form, pool form
struct alignas(64) NodePair { NodeChild c[2]; };                                           // 64 B

struct alignas(16) LeafTri {              // 48 B = 3 offset units
    float v0[3]; uint32_t shadeIdx;       // vertex0; global index of the triangle's ShadeTri (= shadeBase of its BVH + reference triIdx)
    float e1[3]; int32_t objIdx;          // vertex1 - vertex0; hit object id (tri.objIdx or BLASBVH::objIdx)
    float e2[3]; uint32_t remain;         // vertex2 - vertex0; triangles left in this leaf including this one (>= 1)
};

struct alignas(16) ShadeTri {             // 64 B
    float n0[3], n1[3], n2[3];
    float uv0[2], uv1[2], uv2[2];
    int32_t mat;                          // index into Scene::mats ([0] light, [1] floor, 2.. scene materials)
};

struct alignas(16) TlasNode { float lo[3]; uint32_t ref; float hi[3]; uint32_t ref16; };       // 32 B; ref / ref16 = packed reference of THIS node: offset form, pool form

struct alignas(16) Instance {             // 128 B
    float invT[12];                       // rows 0..2 of BLASBVH::invT (ray -> object space)
    uint32_t shadeBase;                   // first ShadeTri of this BLAS (find_nearest reports triIdx = shadeIdx - shadeBase)
    uint32_t rootRef16;                   // pool-form reference of the BLAS's node 0
    uint32_t rootRef;                     // packed reference of the BLAS's node 0
    int32_t objIdx;
    float T[12];                          // rows 0..2 of BLASBVH::T    (normal -> world space)
    uint32_t triCount;                    // triangles of this BLAS: the bound of a BLAS-local triIdx (hit_record_ok)
    uint32_t pad[3];
};

struct alignas(16) Material {             // 32 B: material + its texture descriptor in one record
    float reflectivity, refractivity;
    float absorption[3];
    uint32_t texOffset;                   // first texel in the pooled texel array
    int32_t texW, texH;                   // texW == 0: untextured (albedo 1,1,1)
};

struct Scene {                            // passed to the kernels BY VALUE (kernel argument segment -> scalar loads, global pointers)
    int32_t kind;                         // 0 FileScene, 1 TLASFileScene
    int32_t depthLimit;
    // camera (template/camera.h)
    float camPos[3], topLeft[3], topRight[3], bottomLeft[3];
    float invW, invH;                     // 1.0f / SCRWIDTH, 1.0f / SCRHEIGHT
    int32_t W, H;
    // light quad / floor plane
    float lightInvT[12]; float lightNrm[3]; float lightSize;
    float lightPos[3];                    // GetLightPos() (file_scene.cpp:156-162): the Whitted integrator's point light
    float floorN[3]; float floorD; float floorInvto;
    Material floorMat;                    // primitiveMaterials[1]: diffuse, textured
    uint32_t skyOffset; int32_t skyW, skyH;
    // pools
    const char* geom;                     // pairs | leaf tris | TLAS nodes | instances | shade records
    uint32_t tlasOff, instOff, shadeOff;  // byte offsets of those sections inside geom
    uint32_t leafOff, tlasPairOff;        // ... of the leaf triangles and of the TLAS child pairs (NodePair layout: the two child TlasNodes of every TLAS interior node side by side)
    uint32_t rootRef16, poolRefBits;      // pool form of rootRef; the width the scene's pool references are written in: 16, 32, or 0 = none (render_pool_kernel cannot run)
    const uint32_t* texels;
    const Material* mats;
    uint32_t rootRef;                     // packed reference of the root (BVH node 0 / TLAS node 0)
    uint32_t stackDepth;                  // dwords per lane of the LDS traversal stack (BVH height + TLAS height + 1 marker + slack)
    uint32_t bvhStack;                    // of which the BVH part (find_nearest_kernel keeps the TLAS entries above it)
    uint32_t lightAxis, floorAxisY;       // 1: light invT has an identity rotation block / floor normal is exactly (0,1,0): short quad / plane tests (kernels.hip)
    uint32_t rootIsPair;                  // 1: rootPair holds the root's two children (always, unless the root itself is a leaf)
    float rootPair[16];                   // NodePair of the root (BVH: its child pair; TLAS: its two child TlasNodes, same 2 x {lo, ref, hi, -} layout)
    // Camera-relative operands of PRIMARY rays, directly behind rootPair (one block for the kernel's scalar loads).  Every primary ray starts at camPos, so these
    // differences and sums are the same for all lanes and all pixels; the device has no scalar float unit and would recompute them per lane and per ray.  The host
    // computes them with the same single-rounded float operation (set_primary, below: the ONLY writer), whenever the camera, the light / floor block or rootPair
    // changes; render_pool_kernel's END pass uses them (new_ray's primary form).
    float primRoot[12];                   // child 1: lo - camPos, hi - camPos; child 2: lo - camPos, hi - camPos
    float primLight[3];                   // camPos.y + lightInvT[7], camPos.x + lightInvT[3], camPos.z + lightInvT[11]   (the lightAxis expressions)
    float primFloor;                      // camPos.y + floorD                                                            (the floorAxisY expression)
    float primRight[3], primDown[3];      // topRight - topLeft, bottomLeft - topLeft
};
constexpr uint32_t kPrimFloats = 22u;     // primRoot .. primDown

// Scene's camera-relative block from its camera, light / floor block and rootPair: each value ONE float operation, the one the kernels perform (host code is
// built with -ffp-contract=off as well)
inline void set_primary(Scene& s)
{
    const float* O = s.camPos;
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 3; k++) {
            s.primRoot[6 * c + k] = s.rootPair[8 * c + k] - O[k];
            s.primRoot[6 * c + 3 + k] = s.rootPair[8 * c + 4 + k] - O[k];
        }
    s.primLight[0] = O[1] + s.lightInvT[7]; s.primLight[1] = O[0] + s.lightInvT[3]; s.primLight[2] = O[2] + s.lightInvT[11];
    s.primFloor = O[1] + s.floorD;
    for (int k = 0; k < 3; k++) { s.primRight[k] = s.topRight[k] - s.topLeft[k]; s.primDown[k] = s.bottomLeft[k] - s.topLeft[k]; }
}

// render_pool_kernel's tile class, one byte per local tile (tile_class.h classify_tiles, on the host): tests that NO primary ray of the tile can pass.  A set bit
// is a proof; 0 is always correct.
constexpr uint32_t kTileNoLight = 1u, kTileNoFloor = 2u, kTileNoTree = 4u;    // the light quad's test, the floor plane's, the slab tests of the root's two children
constexpr uint32_t kTileSky = kTileNoLight | kTileNoFloor | kTileNoTree;      // all three: every path of the tile ends at depth 0 in the sky lookup
// ... and one test that EVERY primary ray of the tile passes: the floor half of hit_light_floor<true> (floorAxisY form), i.e. t = -primFloor / D.y satisfies
// 0 < t < 1e34.  It excludes kTileNoFloor, so a sky tile never carries it.  The debug entries that predate it return the three bits above only.
constexpr uint32_t kTileFloorSure = 8u;
constexpr uint32_t kTileFloor = kTileNoLight | kTileNoTree | kTileFloorSure;  // every primary ray of the tile misses the light and the tree and hits the floor
constexpr uint32_t kTileNoMask = 7u;                                          // the kTileNo* bits

struct Counters { unsigned long long v[8]; };   // order = crt_counters

// crt_refit_device's bottom-up plan of one BVH (refit.hip): one record per node pair, sorted by depth, deepest level first.  A child code is kPlanInterior | the
// BVH-local index of the child's own pair, or the BVH-local leaf slot of a leaf child's first triangle (its triangle count is that LeafTri's `remain`).
struct alignas(16) RefitPlanRec { uint32_t pair, child[2], pad; };
constexpr uint32_t kPlanInterior = 0x80000000u;

// crt_update_transforms_device's result block (tlas_build.hip): this header, then an image of the geometry buffer's [tlasOff, shadeOff) — TLAS nodes, TLAS child
// pairs, Instance records, at the same relative offsets — which the host reads back, checks and only then copies into the geometry buffer.
struct alignas(64) TlasBuildHeader {
    uint32_t status;                      // kTlasBuild*
    uint32_t step;                        // the FindBestMatch call (counted from 1) that found no candidate / at which the bound was hit
    uint32_t height;                      // deepest leaf below node 0, in edges: what flatten_tlas reports
    uint32_t searches;                    // FindBestMatch calls made
    uint32_t staleA;                      // merges after which A lay outside the list (tlas_bvh.cpp's list[B] = list[N-1]; --N with A == N-1)
    uint32_t pad[11];
};
constexpr uint32_t kTlasBuildOk = 0u, kTlasBuildNoCandidate = 1u, kTlasBuildNoEnd = 2u;
// crt_render_poses' pose table (tlas_build.hip tlas_build_poses_kernel writes it, render_poses.h reads it): this header, P TlasBuildHeaders side by side (one
// read-back), then — at imagesOff, imageStride apart, both multiples of 128 — the P images of [tlasOff, shadeOff).  The render kernel addresses the table as it
// addresses the geometry buffer, scalar base + 32-bit byte offset, so the whole table stays within kMaxGeomBytes; an image's Instance records are 128 bytes each
// and lie wholly inside it, which keeps ldp<>'s assumption (64 bytes from a record half's offset are inside the buffer) true.
struct alignas(64) PoseJobHeader {
    uint32_t badView;                     // the lowest view whose view_pose entry lies outside [0, P); kPoseNoBadView: none
    uint32_t pad[15];
};
constexpr uint32_t kPoseNoBadView = 0xffffffffu;
// what the render kernel takes by value: where the table is and how a view finds its pose in it
struct PoseTableDev {
    const char* table; const int32_t* viewPose;   // viewPose == nullptr: view k renders pose k
    uint32_t imagesOff, imageStride, instRel;     // instRel: the Instance records' offset inside an image (instOff - tlasOff)
};
// crt_render_shapes' shape table (shape_build.hip writes it, render_shapes.h reads it): this header, S rows of node-0 boxes (rowFloats each: the live root boxes with
// the refitted BVH's entry replaced; a FileScene's row is that one box), for a two-level scene S TlasBuildHeaders, then — at imagesOff, imageStride apart, both
// multiples of 128 — the S images.  An image holds the refitted BVH's NodePairs at 0, its LeafTris at leafRel and, for a two-level scene, a pose image (the build's
// [tlasOff, shadeOff)) at poseRel.  References inside an image's pairs are IMAGE-RELATIVE 16-byte offsets (the box kernel rewrites them as it copies the pairs), so a
// lane finds a record at table + (its image's offset + (ref << 4)): one per-lane delta.  leafRel >= 64, so a leaf's reference is never 0 here either.  The whole
// table stays within kMaxGeomBytes, as the pose table does.
struct alignas(64) ShapeJobHeader {
    uint32_t badView;                     // the lowest view whose view_shape entry lies outside [0, S); kPoseNoBadView: none
    uint32_t pad[15];
};
// what the build kernels take by value
struct ShapeBuildDev {
    const char* geom; uint32_t leafOff, pairBase, pairCount, triBase, triCount;    // the live BVH: its pairs at 64 pairBase, its leaf slots at leafOff + 48 triBase
    const float* pos;                                                             // S * triCount * 9
    const float* liveRootBox; uint32_t rowFloats, bvh;                            // nullptr (FileScene: rowFloats 6, entry 0) or the device's node-0 boxes
    char* table; uint32_t rowsOff, imagesOff, imageStride, leafRel, S;
};
// what the render kernel takes by value: where the table is and how a view finds its shape in it
struct ShapeTableDev {
    const char* table; const int32_t* viewShape;  // viewShape == nullptr: view k renders shape k
    uint32_t imagesOff, imageStride;
    uint32_t rootRef;                             // the refitted BVH's node 0, image-relative
    uint32_t bvh, poseRel, instRel;               // two-level: the instance that walks the image; the pose image inside an image; the Instance records inside that
};
// crt_render_shape_sets' table: the shape table with M BVHs of a two-level scene deforming per shape.  Behind the S rows of node-0 boxes the header region holds two
// tables that the kernels read from device memory (M and blasCount are the job's, so neither fits a kernel argument): M ShapeSetMesh descriptors at meshOff and the
// per-instance words instRoot[blasCount] at instRootOff.  An image holds, for every m, mesh m's NodePairs at pairRel and its LeafTris at leafRel — offsets of its own
// from the image's first byte —, then the pose image at poseRel.  References inside EVERY sub-image are relative to the image's first byte, not the sub-image's, so
// the one per-lane delta of ShapeBvh (render_shapes.h) still serves every fetch.  The first sub-image is laid out as a single shape's image: leafRel >= 64 for every m.
struct alignas(16) ShapeSetMesh {
    const RefitPlanRec* plan; const uint32_t* levelOff;                           // the BVH's refit plan (refit.hip), its level offsets
    uint32_t levels, rootCode;                                                    // ... its level count and node 0's child code
    uint32_t pairBase, pairCount, triBase, triCount;                              // the live BVH, as ShapeBuildDev names it
    uint32_t bvh;                                                                 // the BLAS (= Instance) index: its entry in a row of node-0 boxes
    uint32_t triFirst;                                                            // its first triangle in a shape's positions = its first leaf slot of the set
    uint32_t pairRel, leafRel;                                                    // where its sub-image's pairs and leaves start inside an image
};
// instRoot[i]: the image-relative reference of node 0 of instance i's BVH if it deforms, kInstLive if the instance walks Scene::geom.  No image-relative reference is
// 0: an interior root has kRefInterior set, a leaf root is at least leafRel >> 4 >= 4.
constexpr uint32_t kInstLive = 0u;
// what the set's build kernels take by value
struct ShapeSetBuildDev {
    const char* geom; uint32_t leafOff;                                           // the live geometry buffer, its leaf section
    const float* pos; uint32_t setTris;                                           // S * setTris * 9: per shape mesh 0's triangles, then mesh 1's, ...
    const float* liveRootBox; uint32_t rowFloats;                                 // the device's node-0 boxes, 6 * blasCount floats
    char* table; uint32_t rowsOff, meshOff, instRootOff, imagesOff, imageStride, S, M;
};
// what the set's render kernel takes by value (ShapeTableDev with the instRoot table in place of the one BVH)
struct ShapeSetTableDev {
    const char* table; const int32_t* viewShape;  // viewShape == nullptr: view k renders shape k
    uint32_t imagesOff, imageStride;
    uint32_t instRootOff;                         // instRoot[blasCount] in the table
    uint32_t poseRel, instRel;                    // the pose image inside an image; the Instance records inside that
};
// The uploaded texture table as the device keeps it (one record per crt_texture, written at upload and never after): what a texture index becomes in a Material
// record or in the sky words.  look_build.hip binds a look's indices through it.
struct alignas(16) TexDesc { uint32_t offset; int32_t w, h; uint32_t pad; };
// crt_render_looks' look table (look_build.hip writes it, render_looks.h reads it): this header, then — at looksOff, lookStride apart, both multiples of 128 — one
// block per look: a LookDev (the light quad, the floor material, the sky words), then the look's 2 + materialCount Material records in Scene::mats' order ([0] light,
// [1] floor, 2.. the scene's), so ShadeTri::mat indexes them as it indexes the live table.  The render kernel addresses the table as the pose table is addressed,
// scalar base + 32-bit byte offset, so the whole table stays within kMaxGeomBytes.
struct alignas(64) LookJobHeader {
    uint32_t badView;                     // the lowest view whose view_look entry lies outside [0, L); kPoseNoBadView: none
    uint32_t pad0;
    unsigned long long badField;          // look << 32 | field of the lowest (look, field) whose texture index is out of range; kLookNoBadField: none
    uint32_t pad[12];
};
constexpr unsigned long long kLookNoBadField = ~0ull;
constexpr uint32_t kLookFieldFloor = 0u, kLookFieldSky = 1u, kLookFieldMaterial = 2u;   // field: floorTexture, skyTexture, 2 + i = materials[i].texture
struct alignas(128) LookDev {             // 128 B
    float lightInvT[12]; float lightNrm[3]; float lightSize;      // Scene's light block, rows 0..2 of the look's invT
    Material floorMat;                                            // Scene::floorMat
    uint32_t skyOffset; int32_t skyW, skyH; uint32_t pad[5];      // Scene's sky words
};
constexpr uint32_t kLookHeaderWords = 36u, kLookMaterialWords = 6u;     // crt_abi.h: crt_look_header, crt_material
// what the build kernel takes by value
struct LookBuildDev {
    const uint32_t* looks; uint32_t L, M;                         // L records of kLookHeaderWords + M * kLookMaterialWords words
    const TexDesc* tex; uint32_t texCount;
    char* table; uint32_t looksOff, lookStride;
    const int32_t* viewLook; uint32_t K;                          // viewLook may be nullptr
};
// what the render kernel takes by value: where the table is and how a view finds its look in it
struct LookTableDev {
    const char* table; const int32_t* viewLook;   // viewLook == nullptr: view k renders look k
    uint32_t looksOff, lookStride;
};
constexpr uint32_t kTlasMaxBlas = 256u;   // tlas_bvh.cpp:21 (nodeIdx[256])

// Whether a crt_hit's indices may be used as addresses by the hit-info query (shade_query.hip): ONE predicate for the host entry, which refuses the call, and for
// the kernel, which writes CRT_MATERIAL_INVALID for the lane.  objects = crt_scene_desc.objCount (FileScene) / bvhCount (two-level); triCountOf(k) = triangles of
// the BVH that object 2 + k's triIdx indexes (FileScene: its one BVH; two-level: BLAS k), asked only for an object that exists.
#if defined(__HIPCC__)
#define CRT_HOST_DEVICE __host__ __device__
#else
#define CRT_HOST_DEVICE
#endif
template <class TriCountOf>
CRT_HOST_DEVICE inline bool hit_record_ok(int32_t objIdx, int32_t triIdx, uint32_t objects, TriCountOf&& triCountOf)
{
    if (objIdx < 2) return objIdx >= -1;                                  // miss, light quad, floor plane: triIdx is not looked at
    if ((uint32_t)(objIdx - 2) >= objects) return false;
    return triIdx >= 0 && (uint32_t)triIdx < triCountOf((uint32_t)(objIdx - 2));
}

// FileScene's alternative acceleration structures (crt_upload_alt_accel; traversal in alt_common.h): the flat KD-tree's nodes, the triangle records both structures
// index, and the view of one uploaded KD-tree + uniform grid that the kernels take by value
struct KdNode { float lo[3]; int32_t left; float hi[3]; int32_t right; float splitDistance; int32_t splitAxis; uint32_t firstTri, triCount; };   // = crt_kd_node, 48 B; left < 0: leaf
struct AltTri { float v0[3]; uint32_t triIdx; float e1[3]; int32_t objIdx; float e2[3]; uint32_t pad; };                                          // 48 B: Möller–Trumbore operands, reference triangle order
struct AltAccelDev {
    const KdNode* kdNodes; const uint32_t* kdRefs; uint32_t kdStack;         // kdStack: entries per lane (tree height + 1)
    const AltTri* tris;
    int32_t res[3]; float cell[3]; float lo[3], hi[3]; const uint32_t* cellStart; const int32_t* cellRefs;
};

// A two-level scene's set of BLASKDTree / BLASGrid structures (crt_upload_blas_accel): every BLAS's arrays are concatenated, a descriptor per BLAS
// says where its part starts.  Triangle records are AltTri (triIdx = the GLOBAL shade index, objIdx = the BLAS's), in each BLAS's order.
struct BlasAltDesc {                      // 72 B, indexed by the BLAS (= Instance) index
    uint32_t nodeBase, refBase, triBase;  // KD: first node, first leaf reference; first triangle record (references inside a BLAS are BLAS-local)
    uint32_t cellBase, cellRefBase;       // grid: first cellStart entry, first cell reference
    int32_t objIdx;                       // BLASKDTree::objIdx / BLASGrid::objIdx
    int32_t res[3]; float cell[3]; float lo[3], hi[3];   // grid: resolution, cellSize, localBounds
};
struct TlasAltDev {                       // passed by value, like AltAccelDev
    const BlasAltDesc* desc;
    const void* kdNodes; const uint32_t* kdRefs; const void* tris;
    const uint32_t* cellStart; const int32_t* cellRefs;
    uint32_t kdStack;                     // KD stack entries per lane: the deepest KD-tree's height + 1 (0 for a grid set)
};

// crt_build_grid_device (grid_build.hip): the grid the host derived from the bounds, handed to the count / fill kernels by value, and the block the kernels report
// through: the six bound keys (min x y z, max x y z: ordered value << 32 | position << 1 | sign of a zero), the non-finite flag, the reference count.
struct GridParams { int32_t res[3]; float cell[3]; float lo[3]; };
struct alignas(16) GridBuildState { unsigned long long key[6]; unsigned long long total; uint32_t nonFinite; uint32_t pad; };

// crt_build_kdtree_device (kd_build.hip): one node of one level of the level-synchronous build, and the block the kernels report through.  A level's nodes are in
// level order; its references are one concatenated array segmented by node ([first, first + count)).  The finalise passes fill the last four words.
struct alignas(16) KdBuildNode {
    float lo[3]; uint32_t first;          // box; first reference of the node in the level's array
    float hi[3]; uint32_t count;
    float splitPos, distance; int32_t axis; uint32_t child;    // axis < 0: leaf; child: the left child's index in the next level (the right one follows it)
    uint32_t subNodes, subRefs;           // nodes / leaf references of the subtree (bottom-up)
    uint32_t pre, firstRef;               // pre-order index; leaf references that precede the node in pre-order (top-down)
};
// the bounds pass's block (the grid build's), then the totals of the level's two scans: nodeTotal = split nodes | leaf references << 32, refTotal = references
// that go left | references that go right << 32 (each half below 2^32: a level holds at most 2^31 - 1 references)
struct alignas(16) KdBuildState { GridBuildState bounds; unsigned long long nodeTotal, refTotal; };
constexpr uint32_t kKdMaxDepth = 20u;     // kdtree.h m_maxBuildDepth: levels 0 .. 20

// crt_build_bvh_device (bvh_build.hip): one node of one level of the level-synchronous binned-SAH build, and the block the kernels report through.  A level's
// nodes are in level order over ONE triangleIndices array: node = slots [first, first + count).  Beside the records live 6 box keys per node (the fold of
// Builder::fit: ordered value << 32 | position << 1 | sign of a zero) and, per level, 3 x 8 bins per node of kBvhBinWords words: count, box min xyz, box max xyz
// as ordered 32-bit keys.
struct alignas(16) BvhBuildNode {
    float lo[3]; uint32_t first;          // box (from the keys, bvh_plane_kernel); first slot
    float hi[3]; uint32_t count;
    uint32_t ckey[6];                     // centroid bounds min xyz, max xyz as ordered keys (nodes of more than 2 triangles)
    float pos; int32_t axis;              // the chosen plane; axis < 0: no plane (<= 2 triangles, or the leaf test held): nothing is partitioned
    uint32_t nLeft, child;                // leftCount of the partition; the left child's index in the next level (the right one follows it), kBvhNone: a leaf
    uint32_t subSplits, pair;             // split nodes of the subtree (bottom-up); number of the node's child pair = split nodes before it in pre-order (top-down)
};
constexpr uint32_t kBvhNone = 0xffffffffu;
constexpr uint32_t kBvhBins = 8u, kBvhBinWords = 7u, kBvhNodeBinWords = 3u * kBvhBins * kBvhBinWords;
// splits / lefts: the totals of the level's two scans (nodes that split; slots that go left); rootBox: node 0's box, written by level 0
struct alignas(16) BvhBuildState { unsigned long long splits, lefts; float rootBox[6]; uint32_t nonFinite, pad; };
// where the rebuilt BVH's records go in the new geometry buffer, and how its references are written (the scene's pool reference form)
struct BvhFlatten { uint32_t pairBase, pairs, triBase, leafOff, interior16, mask16; };
// the other BVHs' pairs carried into the new buffer: the old buffer's pairs, the rebuilt BVH's old range among them, how far the pairs behind it move, how far
// (in 16-byte units) every offset-form leaf reference moves
struct BvhRelocate { uint32_t oldPairs, firstPair, pairCount; int32_t pairDelta, leafDelta16; uint32_t interior16, mask16; };

// PrimitiveScene at one animation time (crt_primitive_scene flattened by crt_upload_primitive_scene; kernels in render_prim.hip), passed to the kernels by value
struct PrimDev {
    float quadInvT[12], quadNrm[3], quadSize;
    float spherePos[3], pad0;
    float cubeInvM[12], cubeM[12], cubeMin[3], cubeMax[3];
    float torusInvT[12], torusT[12], rt2, rc2, r2, pad1;
    float refl[11], refr[11], absorb[33];
    float pad2;
    const uint32_t* red; const uint32_t* blue;     // 512 x 512 texels 0x00RRGGBB (the left / right wall's albedo override), may be null (black)
};

} // namespace crt
