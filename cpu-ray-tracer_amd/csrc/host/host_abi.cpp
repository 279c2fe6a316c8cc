// host_abi.cpp — C wrappers (include/crt_host.h) around the C++ host front.  Exceptions stop here.
#include "../../../include/crt_host.h"
#include "scene.h"
#include "accel_alt.h"

#include <cstdlib>
#include <string>
#include <vector>

using namespace crt;

namespace { thread_local std::string g_err; }

struct crt_host_scene { BaseScene* scene = nullptr; FileScene* file = nullptr; TLASFileScene* tlas = nullptr; KDTree* kd = nullptr; Grid* grid = nullptr;
                        std::vector<BLASKDTree> blasKd; std::vector<BLASGrid> blasGrid;               // TLAS scene: one structure per BLAS
                        std::vector<uint8_t> gridPending, kdPending;                                    // BVHs whose grid / KD-tree was rebuilt on the device and is not mirrored yet
                        bool kdDeviceBuilt = false;                                                   // the KD mirror's nodes are the device's, its triangles still the host's old ones
                        bool gridDeviceBuilt = false; };                                               // the grid mirror's cells are the device's, its triangles still the host's old ones
struct crt_host_renderer { Renderer* r = nullptr; };

// a BVH whose host arrays are stale (refitted on the device only): the calls that would send those arrays are refused
static bool refuse_stale(crt_host_scene* s, const char* what)
{
    const int i = s->scene->FirstStaleBvh();
    if (i < 0) return false;
    g_err = std::string(what) + ": BVH " + std::to_string(i) + " was refitted on the device (crt_host_scene_bvh_refit_device), its host triangles and nodes are stale; "
            "crt_host_scene_bvh_move_and_refit brings the positions to the host again";
    return true;
}

#define GUARD_BEGIN try {
#define GUARD_END(code) } catch (const std::exception& e) { g_err = e.what(); return code; } catch (...) { g_err = "unknown exception"; return code; }

// abi.cpp's, for this file only (the host front includes no HIP header): a synchronous copy of device memory to the host behind what `stream` holds
extern "C" int crt_internal_read_device(crt_ctx* ctx, void* dst, const void* d_src, size_t bytes, void* stream);

extern "C" {

const char* crt_host_last_error(void) { return g_err.c_str(); }
void crt_host_set_error(const char* msg) { g_err = msg ? msg : ""; }      // (other translation units of the host front: primitive_scene.cpp)

int crt_host_scene_load(const char* xml, int kind, const char* base, crt_host_scene** out)
{
    if (!xml || !out) { g_err = "null argument"; return CRT_ERR_INVALID; }
    *out = nullptr;
    if (kind != CRT_SCENE_FILE && kind != CRT_SCENE_TLAS) { g_err = "unknown scene kind"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    crt_host_scene* h = new crt_host_scene();
    try {
        const std::string b = base ? base : "";
        if (kind == CRT_SCENE_FILE) { h->file = new FileScene(xml, b); h->scene = h->file; }
        else { h->tlas = new TLASFileScene(xml, b); h->scene = h->tlas; }
    } catch (...) { delete h; throw; }
    *out = h;
    return CRT_OK;
    GUARD_END(CRT_ERR_IO)
}
void crt_host_scene_free(crt_host_scene* s) { if (s) { delete s->scene; delete s->kd; delete s->grid; delete s; } }
int crt_host_scene_upload(crt_host_scene* s, crt_ctx* ctx)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    if (refuse_stale(s, "crt_host_scene_upload")) return CRT_ERR_STATE;
    GUARD_BEGIN
    const int rc = s->scene->Upload(ctx);
    if (rc != CRT_OK) g_err = crt_last_error(ctx);
    return rc;
    GUARD_END(CRT_ERR_INVALID)
}
int crt_host_scene_kind(crt_host_scene* s) { return s ? s->scene->Kind() : CRT_ERR_INVALID; }
int crt_host_scene_triangle_count(crt_host_scene* s) { return s ? s->scene->GetTriangleCount() : CRT_ERR_INVALID; }
int crt_host_scene_bvh_count(crt_host_scene* s) { return !s ? CRT_ERR_INVALID : (s->file ? 1 : (int)s->tlas->tlas.blas.size()); }

static bool pick(crt_host_scene* s, int i, const std::vector<BVHNode>** nodes, const std::vector<Tri>** tris, const std::vector<uint32_t>** idx, uint32_t* used, uint32_t* depth)
{
    if (!s) return false;
    if (s->file) { if (i != 0) return false; *nodes = &s->file->acc.bvhNodes; *tris = &s->file->acc.triangles; *idx = &s->file->acc.triangleIndices; *used = s->file->acc.nodesUsed; *depth = s->file->acc.maxDepth; return true; }
    if (i < 0 || i >= (int)s->tlas->tlas.blas.size()) return false;
    const BLASBVH* b = s->tlas->tlas.blas[(size_t)i];
    *nodes = &b->bvhNodes; *tris = &b->triangles; *idx = &b->triangleIndices; *used = b->nodesUsed; *depth = b->maxDepth; return true;
}
int crt_host_scene_bvh_info(crt_host_scene* s, int i, uint32_t* nodesUsed, uint32_t* triCount, uint32_t* maxDepth)
{
    const std::vector<BVHNode>* n; const std::vector<Tri>* t; const std::vector<uint32_t>* x; uint32_t u, d;
    if (!pick(s, i, &n, &t, &x, &u, &d)) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    if (nodesUsed) *nodesUsed = u; if (triCount) *triCount = (uint32_t)t->size(); if (maxDepth) *maxDepth = d;
    return CRT_OK;
}
int crt_host_scene_bvh_copy(crt_host_scene* s, int i, crt_bvh_node* nodes, uint32_t* idx, crt_tri* tris)
{
    const std::vector<BVHNode>* n; const std::vector<Tri>* t; const std::vector<uint32_t>* x; uint32_t u, d;
    if (!pick(s, i, &n, &t, &x, &u, &d)) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    if (nodes) memcpy(nodes, n->data(), sizeof(BVHNode) * u);
    if (idx) memcpy(idx, x->data(), 4 * x->size());
    if (tris) memcpy(tris, t->data(), sizeof(Tri) * t->size());
    return CRT_OK;
}
int crt_host_scene_bvh_move_and_refit(crt_host_scene* s, int i, const float* positions, uint32_t triCount)
{
    if (!s || !positions) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    std::vector<Tri>* tris = nullptr;
    BLASBVH* blas = nullptr;
    if (s->file) { if (i != 0) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; } tris = &s->file->acc.triangles; }
    else { if (i < 0 || i >= (int)s->tlas->tlas.blas.size()) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; } blas = s->tlas->tlas.blas[(size_t)i]; tris = &blas->triangles; }
    if (triCount != tris->size()) { g_err = "triangle count does not match the built BVH (Refit keeps the topology)"; return CRT_ERR_INVALID; }
    for (uint32_t t = 0; t < triCount; t++) {
        memcpy((*tris)[t].vertex0, positions + 9 * (size_t)t, 12); memcpy((*tris)[t].vertex1, positions + 9 * (size_t)t + 3, 12);
        memcpy((*tris)[t].vertex2, positions + 9 * (size_t)t + 6, 12);
    }
    if (s->file) s->file->acc.Refit();
    else { blas->Refit(); blas->SetTransform(blas->T); s->tlas->tlas.Build(); }      // world bounds + TLAS follow the refitted BLAS, as a per-frame animation loop does
    if ((size_t)i < s->scene->staleBvh.size()) s->scene->staleBvh[(size_t)i] = 0;    // the host arrays are current again
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
int crt_host_scene_bvh_move_and_rebuild(crt_host_scene* s, int i, const float* positions, uint32_t triCount)
{
    if (!s || !positions) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    std::vector<Tri>* tris = nullptr;
    BLASBVH* blas = nullptr;
    if (s->file) { if (i != 0) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; } tris = &s->file->acc.triangles; }
    else { if (i < 0 || i >= (int)s->tlas->tlas.blas.size()) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; } blas = s->tlas->tlas.blas[(size_t)i]; tris = &blas->triangles; }
    if (triCount != tris->size()) { g_err = "triangle count does not match the built BVH (a rebuild keeps the triangles)"; return CRT_ERR_INVALID; }
    for (uint32_t t = 0; t < triCount; t++) {
        Tri& tr = (*tris)[t];
        memcpy(tr.vertex0, positions + 9 * (size_t)t, 12); memcpy(tr.vertex1, positions + 9 * (size_t)t + 3, 12); memcpy(tr.vertex2, positions + 9 * (size_t)t + 6, 12);
        for (int k = 0; k < 3; k++) tr.centroid[k] = (tr.vertex0[k] + tr.vertex1[k] + tr.vertex2[k]) * 0.3333f;       // model.cpp:77 / blas_bvh.cpp:74
    }
    if (s->file) s->file->acc.Build();
    else { blas->Build(); blas->SetTransform(blas->T); s->tlas->tlas.Build(); }
    if ((size_t)i < s->scene->staleBvh.size()) s->scene->staleBvh[(size_t)i] = 0;    // the host arrays are current again
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
int crt_host_scene_build_bvh_device(crt_host_scene* s, crt_ctx* ctx, int i, const float* d_positions, uint32_t triCount, void* stream)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const int count = s->file ? 1 : (int)s->tlas->tlas.blas.size();
    if (i < 0 || i >= count) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    int rc = crt_build_bvh_device(ctx, (uint32_t)i, d_positions, triCount, stream, nullptr);
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    std::vector<float> pos(9 * (size_t)triCount);
    rc = crt_internal_read_device(ctx, pos.data(), d_positions, pos.size() * 4, stream);
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    if ((rc = crt_host_scene_bvh_move_and_rebuild(s, i, pos.data(), triCount)) != CRT_OK) return rc;
    if (s->tlas) {                                                                   // as after BLASBVH::Build: world bounds from the new root box, TLAS rebuilt, both sent
        rc = s->scene->Update(ctx, CRT_UPDATE_TRANSFORMS);
        if (rc != CRT_OK) g_err = crt_last_error(ctx);
    }
    return rc;
    GUARD_END(CRT_ERR_DEVICE)
}
int crt_host_scene_bvh_refit_device(crt_host_scene* s, crt_ctx* ctx, int i, const float* d_positions, uint32_t triCount, void* stream)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const int count = s->file ? 1 : (int)s->tlas->tlas.blas.size();
    if (i < 0 || i >= count) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    float box[6];
    int rc = crt_refit_device(ctx, (uint32_t)i, d_positions, triCount, stream, box);
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    BVHNode& root = s->file ? s->file->acc.bvhNodes[0] : s->tlas->tlas.blas[(size_t)i]->bvhNodes[0];
    memcpy(root.aabbMin, box, 12); memcpy(root.aabbMax, box + 3, 12);
    s->scene->staleBvh.resize((size_t)count, 0); s->scene->staleBvh[(size_t)i] = 1;
    if (s->tlas) {                                                                   // as after BLASBVH::Refit: world bounds from the new root box, TLAS rebuilt, both sent
        BLASBVH* blas = s->tlas->tlas.blas[(size_t)i];
        blas->SetTransform(blas->T); s->tlas->tlas.Build();
        rc = s->scene->Update(ctx, CRT_UPDATE_TRANSFORMS);
        if (rc != CRT_OK) g_err = crt_last_error(ctx);
    }
    return rc;
    GUARD_END(CRT_ERR_DEVICE)
}
int crt_host_scene_update_transforms_device(crt_host_scene* s, crt_ctx* ctx, const float* d_T, void* stream)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    if (!s->tlas) { g_err = "not a TLAS scene (a FileScene bakes its transforms into the triangles)"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    TLASBVH& tl = s->tlas->tlas;
    const size_t n = tl.blas.size();
    std::vector<float> T(16 * n);                                                    // first, so that the copy waits for d_T's producers only, not for the entry's commit
    const int rb = crt_internal_read_device(ctx, T.data(), d_T, T.size() * 4, stream);
    if (rb != CRT_OK) { g_err = crt_last_error(ctx); return rb; }
    std::vector<crt_tlas_node> nodes(2 * n);
    const int rc = crt_update_transforms_device(ctx, d_T, (uint32_t)n, stream, nodes.data());
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    for (size_t i = 0; i < n; i++) {                                                 // BLASBVH::SetTransform's results; the world box is TLAS leaf 1 + i's
        BLASBVH* b = tl.blas[i];
        memcpy(b->T.cell, &T[16 * i], 64);
        b->invT = b->T.FastInvertedTransformNoScale();
        b->worldBounds.bmin3 = float3(nodes[1 + i].aabbMin[0], nodes[1 + i].aabbMin[1], nodes[1 + i].aabbMin[2]);
        b->worldBounds.bmax3 = float3(nodes[1 + i].aabbMax[0], nodes[1 + i].aabbMax[1], nodes[1 + i].aabbMax[2]);
    }
    tl.tlasNode.resize(2 * n);
    memcpy(tl.tlasNode.data(), nodes.data(), sizeof(crt_tlas_node) * 2 * n);
    tl.nodesUsed = (uint32_t)(2 * n);
    return CRT_OK;
    GUARD_END(CRT_ERR_DEVICE)
}
// the mirror of one grid from the device's (crt_get_grid); false: no live grid (a two-level set still dropped)
static bool mirror_grid(crt_ctx* ctx, uint32_t bvh, Grid& g, int* rc)
{
    int32_t res[3]; float cs[3], lo[3], hi[3]; uint32_t cells = 0, refs = 0;
    *rc = crt_get_grid(ctx, bvh, res, cs, lo, hi, &cells, &refs, nullptr, nullptr);
    if (*rc == CRT_ERR_STATE) { *rc = CRT_OK; return false; }
    if (*rc != CRT_OK) return false;
    g.cellStart.assign((size_t)cells + 1, 0u); g.cellTris.assign(refs, 0);
    *rc = crt_get_grid(ctx, bvh, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g.cellStart.data(), refs ? g.cellTris.data() : nullptr);
    if (*rc != CRT_OK) return false;
    for (int k = 0; k < 3; k++) g.resolution[k] = res[k];
    g.cellSize = float3(cs[0], cs[1], cs[2]); g.localBounds.bmin3 = float3(lo[0], lo[1], lo[2]); g.localBounds.bmax3 = float3(hi[0], hi[1], hi[2]);
    return true;
}
int crt_host_scene_build_grid_device(crt_host_scene* s, crt_ctx* ctx, int i, const float* d_positions, uint32_t triCount, void* stream)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const int count = s->file ? 1 : (int)s->tlas->tlas.blas.size();
    if (i < 0 || i >= count) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    int rc = crt_build_grid_device(ctx, (uint32_t)i, d_positions, triCount, stream);
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    s->gridDeviceBuilt = true;
    if (s->file) {
        if (!s->grid) { s->grid = new Grid(); s->grid->triangles = s->file->acc.triangles; }
        mirror_grid(ctx, 0, *s->grid, &rc);
    } else {
        const std::vector<BLASBVH*>& bl = s->tlas->tlas.blas;
        s->gridPending.resize(bl.size(), 0);
        if (s->blasGrid.size() != bl.size()) {                                       // the set came through crt_upload_blas_accel directly: mirror every BLAS
            s->blasGrid.assign(bl.size(), BLASGrid());
            for (size_t k = 0; k < bl.size(); k++) { s->blasGrid[k].objIdx = bl[k]->objIdx; s->blasGrid[k].triangles = bl[k]->triangles; s->gridPending[k] = 1; }
        }
        s->gridPending[(size_t)i] = 1;
        for (size_t k = 0; k < bl.size() && rc == CRT_OK; k++)
            if (s->gridPending[k] && mirror_grid(ctx, (uint32_t)k, s->blasGrid[k], &rc)) s->gridPending[k] = 0;
    }
    if (rc != CRT_OK) g_err = crt_last_error(ctx);
    return rc;
    GUARD_END(CRT_ERR_DEVICE)
}
// the mirror of one KD-tree from the device's (crt_get_kdtree); false: no live tree (a two-level set still dropped)
static bool mirror_kd(crt_ctx* ctx, uint32_t bvh, KDTree& kd, int* rc)
{
    uint32_t nodes = 0, refs = 0, height = 0;
    *rc = crt_get_kdtree(ctx, bvh, &nodes, &refs, &height, nullptr, nullptr);
    if (*rc == CRT_ERR_STATE) { *rc = CRT_OK; return false; }
    if (*rc != CRT_OK) return false;
    kd.nodes.assign(nodes, crt_kd_node{}); kd.leafTriIndices.assign(refs, 0u);
    *rc = crt_get_kdtree(ctx, bvh, nullptr, nullptr, nullptr, kd.nodes.data(), refs ? kd.leafTriIndices.data() : nullptr);
    if (*rc != CRT_OK) return false;
    // KDTree::nodesUsed counts every node; maxDepth is the deepest node Subdivide went on to split (kdtree.cpp:51)
    kd.nodesUsed = nodes; kd.maxDepth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u});
    while (!st.empty() && nodes) {
        const auto [n, d] = st.back(); st.pop_back();
        const crt_kd_node& nd = kd.nodes[n];
        if (nd.left < 0 || (uint32_t)nd.left >= nodes || (uint32_t)nd.right >= nodes) continue;
        if (d > kd.maxDepth) kd.maxDepth = d;
        st.push_back({(uint32_t)nd.right, d + 1}); st.push_back({(uint32_t)nd.left, d + 1});
    }
    kd.localBounds.bmin3 = float3(kd.nodes[0].aabbMin[0], kd.nodes[0].aabbMin[1], kd.nodes[0].aabbMin[2]);
    kd.localBounds.bmax3 = float3(kd.nodes[0].aabbMax[0], kd.nodes[0].aabbMax[1], kd.nodes[0].aabbMax[2]);
    return true;
}
int crt_host_scene_build_kdtree_device(crt_host_scene* s, crt_ctx* ctx, int i, const float* d_positions, uint32_t triCount, void* stream)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const int count = s->file ? 1 : (int)s->tlas->tlas.blas.size();
    if (i < 0 || i >= count) { g_err = "bvh index out of range"; return CRT_ERR_INVALID; }
    int rc = crt_build_kdtree_device(ctx, (uint32_t)i, d_positions, triCount, stream);
    if (rc != CRT_OK) { g_err = crt_last_error(ctx); return rc; }
    s->kdDeviceBuilt = true;
    if (s->file) {
        if (!s->kd) { s->kd = new KDTree(); s->kd->triangles = s->file->acc.triangles; }
        mirror_kd(ctx, 0, *s->kd, &rc);
    } else {
        const std::vector<BLASBVH*>& bl = s->tlas->tlas.blas;
        s->kdPending.resize(bl.size(), 0);
        if (s->blasKd.size() != bl.size()) {                                         // the set came through crt_upload_blas_accel directly: mirror every BLAS
            s->blasKd.assign(bl.size(), BLASKDTree());
            for (size_t k = 0; k < bl.size(); k++) { s->blasKd[k].objIdx = bl[k]->objIdx; s->blasKd[k].triangles = bl[k]->triangles; s->kdPending[k] = 1; }
        }
        s->kdPending[(size_t)i] = 1;
        for (size_t k = 0; k < bl.size() && rc == CRT_OK; k++)
            if (s->kdPending[k] && mirror_kd(ctx, (uint32_t)k, s->blasKd[k], &rc)) s->kdPending[k] = 0;
    }
    if (rc != CRT_OK) g_err = crt_last_error(ctx);
    return rc;
    GUARD_END(CRT_ERR_DEVICE)
}
int crt_host_bvh_build(const float* positions, uint32_t triCount, uint32_t info[3], crt_bvh_node* nodes, uint32_t* triangleIndices)
{
    if (!positions || triCount == 0) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    std::vector<Tri> tris(triCount);
    for (uint32_t t = 0; t < triCount; t++) {
        Tri& tr = tris[t]; memset(&tr, 0, sizeof(Tri));
        memcpy(tr.vertex0, positions + 9 * (size_t)t, 12); memcpy(tr.vertex1, positions + 9 * (size_t)t + 3, 12); memcpy(tr.vertex2, positions + 9 * (size_t)t + 6, 12);
        for (int k = 0; k < 3; k++) tr.centroid[k] = (tr.vertex0[k] + tr.vertex1[k] + tr.vertex2[k]) * 0.3333f;
    }
    std::vector<BVHNode> n; std::vector<uint32_t> idx; uint32_t used = 0, depth = 0;
    BuildSAH(tris, n, idx, used, depth);
    if (info) {
        uint32_t height = 0;
        std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u});
        while (!st.empty()) {
            const auto [k, d] = st.back(); st.pop_back();
            if (n[k].triCount > 0) { if (d > height) height = d; continue; }
            st.push_back({n[k].leftFirst, d + 1}); st.push_back({n[k].leftFirst + 1, d + 1});
        }
        info[0] = used; info[1] = depth; info[2] = height;
    }
    if (nodes) memcpy(nodes, n.data(), n.size() * sizeof(BVHNode));
    if (triangleIndices) memcpy(triangleIndices, idx.data(), idx.size() * 4);
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
int crt_host_kd_build(const float* positions, uint32_t triCount, uint32_t info[4], crt_kd_node* nodes, uint32_t* refs)
{
    if (!positions || !triCount) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    KDTree kd; kd.triangles.resize(triCount);
    for (uint32_t t = 0; t < triCount; t++) {
        Tri& tr = kd.triangles[t]; memset(&tr, 0, sizeof(Tri));
        memcpy(tr.vertex0, positions + 9 * (size_t)t, 12); memcpy(tr.vertex1, positions + 9 * (size_t)t + 3, 12); memcpy(tr.vertex2, positions + 9 * (size_t)t + 6, 12);
    }
    kd.Build();
    if (info) { info[0] = (uint32_t)kd.nodes.size(); info[1] = (uint32_t)kd.leafTriIndices.size(); info[2] = kd.maxDepth; info[3] = kd.nodesUsed; }
    if (nodes) memcpy(nodes, kd.nodes.data(), kd.nodes.size() * sizeof(crt_kd_node));
    if (refs && !kd.leafTriIndices.empty()) memcpy(refs, kd.leafTriIndices.data(), kd.leafTriIndices.size() * 4);
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
int crt_host_grid_build(const float* positions, uint32_t triCount, int32_t res[3], float f9[9], uint32_t* refCount, uint32_t* cellStart, int32_t* cellRefs)
{
    if (!positions || !triCount) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    Grid g; g.triangles.resize(triCount);
    for (uint32_t t = 0; t < triCount; t++) {
        Tri& tr = g.triangles[t]; memset(&tr, 0, sizeof(Tri));
        memcpy(tr.vertex0, positions + 9 * (size_t)t, 12); memcpy(tr.vertex1, positions + 9 * (size_t)t + 3, 12); memcpy(tr.vertex2, positions + 9 * (size_t)t + 6, 12);
    }
    g.Build();
    for (int k = 0; k < 3; k++) { if (res) res[k] = g.resolution[k]; if (f9) { f9[k] = g.cellSize[k]; f9[3 + k] = g.localBounds.bmin3[k]; f9[6 + k] = g.localBounds.bmax3[k]; } }
    if (refCount) *refCount = (uint32_t)g.cellTris.size();
    if (cellStart) memcpy(cellStart, g.cellStart.data(), g.cellStart.size() * 4);
    if (cellRefs && !g.cellTris.empty()) memcpy(cellRefs, g.cellTris.data(), g.cellTris.size() * 4);
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
// BLASBVH::SetTransform(T) of instance i (blas_bvh.cpp:363-374: T, invT = FastInvertedTransformNoScale, world bounds of the 8 root-box corners)
// followed by TLASBVH::Build (tlas_bvh.cpp:17-55), as an animation loop does per frame; crt_host_scene_update then moves it to the device
int crt_host_scene_set_transform(crt_host_scene* s, int i, const float T[16])
{
    if (!s || !T) { g_err = "null argument"; return CRT_ERR_INVALID; }
    if (!s->tlas || i < 0 || i >= (int)s->tlas->tlas.blas.size()) { g_err = "not a TLAS scene / index out of range (a FileScene bakes its transforms into the triangles)"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    mat4 m; memcpy(m.cell, T, 64);
    s->tlas->tlas.blas[(size_t)i]->SetTransform(m);
    s->tlas->tlas.Build();
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
// the scene's look as a crt_update_look record: *words = crt_look_words(materialCount), the record where `look` is non-NULL
int crt_host_scene_look(crt_host_scene* s, void* look, uint32_t* words)
{
    if (!s || !words) { g_err = "null argument"; return CRT_ERR_INVALID; }
    *words = crt_look_words((uint32_t)s->scene->materials.size());
    if (look) s->scene->Look(look);
    return CRT_OK;
}
// ... and a look taken over by the host scene, for the next crt_host_scene_upload; the device is not touched (crt_update_look changes a live scene's look)
int crt_host_scene_set_look(crt_host_scene* s, const void* look)
{
    if (!s || !look) { g_err = "null argument"; return CRT_ERR_INVALID; }
    const int rc = s->scene->SetLook(look);
    if (rc != CRT_OK) g_err = "crt_host_scene_set_look: a texture index of the look lies outside the scene's textures";
    return rc;
}
int crt_host_scene_update(crt_host_scene* s, crt_ctx* ctx, uint32_t what)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    if ((what & CRT_UPDATE_BOUNDS) && refuse_stale(s, "crt_host_scene_update(CRT_UPDATE_BOUNDS)")) return CRT_ERR_STATE;
    GUARD_BEGIN
    const int rc = s->scene->Update(ctx, what);
    if (rc != CRT_OK) g_err = crt_last_error(ctx);
    return rc;
    GUARD_END(CRT_ERR_DEVICE)
}
int crt_host_scene_blas_transform(crt_host_scene* s, int i, float T[16], float invT[16], float lo[3], float hi[3])
{
    if (!s || !s->tlas || i < 0 || i >= (int)s->tlas->tlas.blas.size()) { g_err = "not a TLAS scene / index out of range"; return CRT_ERR_INVALID; }
    const BLASBVH* b = s->tlas->tlas.blas[(size_t)i];
    memcpy(T, b->T.cell, 64); memcpy(invT, b->invT.cell, 64);
    lo[0] = b->worldBounds.bmin3.x; lo[1] = b->worldBounds.bmin3.y; lo[2] = b->worldBounds.bmin3.z;
    hi[0] = b->worldBounds.bmax3.x; hi[1] = b->worldBounds.bmax3.y; hi[2] = b->worldBounds.bmax3.z;
    return CRT_OK;
}
int crt_host_scene_tlas_copy(crt_host_scene* s, crt_tlas_node* nodes, uint32_t* nodesUsed)
{
    if (!s || !s->tlas) { g_err = "not a TLAS scene"; return CRT_ERR_INVALID; }
    if (nodes) memcpy(nodes, s->tlas->tlas.tlasNode.data(), sizeof(TLASBVHNode) * s->tlas->tlas.tlasNode.size());
    if (nodesUsed) *nodesUsed = s->tlas->tlas.nodesUsed;
    return CRT_OK;
}

int crt_host_camera_state(int w, int h, const float p[3], const float t[3], float camPos[3], float tl[3], float tr[3], float bl[3])
{
    if (w <= 0 || h <= 0 || !p || !t) { g_err = "bad argument"; return CRT_ERR_INVALID; }
    Camera c(w, h);
    c.SetCameraState(float3(p[0], p[1], p[2]), float3(t[0], t[1], t[2]));
    camPos[0] = c.camPos.x; camPos[1] = c.camPos.y; camPos[2] = c.camPos.z;
    tl[0] = c.topLeft.x; tl[1] = c.topLeft.y; tl[2] = c.topLeft.z;
    tr[0] = c.topRight.x; tr[1] = c.topRight.y; tr[2] = c.topRight.z;
    bl[0] = c.bottomLeft.x; bl[1] = c.bottomLeft.y; bl[2] = c.bottomLeft.z;
    return CRT_OK;
}

int crt_host_renderer_create(crt_host_scene* s, int w, int h, int device, crt_host_renderer** out)
{
    if (!s || !out || w < 16 || h < 16) { g_err = "bad argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    crt_host_renderer* r = new crt_host_renderer();
    r->r = new Renderer(s->scene, w, h, device);
    *out = r;
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
void crt_host_renderer_destroy(crt_host_renderer* r) { if (r) { delete r->r; delete r; } }
int crt_host_renderer_init(crt_host_renderer* r) { if (!r) return CRT_ERR_INVALID; GUARD_BEGIN r->r->Init(); return CRT_OK; GUARD_END(CRT_ERR_DEVICE) }
int crt_host_renderer_set_camera(crt_host_renderer* r, const float p[3], const float t[3])
{
    if (!r || !p || !t) return CRT_ERR_INVALID;
    r->r->camera.SetCameraState(float3(p[0], p[1], p[2]), float3(t[0], t[1], t[2]));
    r->r->ResetWhittedPeaks();                                                          // "2. WhittedStyle/renderer.cpp":180-186, 206-212
    return CRT_OK;
}
int crt_host_renderer_set_passes(crt_host_renderer* r, int passes) { if (!r || passes < 1 || passes > 4) { g_err = "passes must be 1..4"; return CRT_ERR_INVALID; } r->r->passes = passes; return CRT_OK; }
int crt_host_renderer_clear(crt_host_renderer* r) { if (!r) return CRT_ERR_INVALID; GUARD_BEGIN r->r->ClearAccumulator(); return CRT_OK; GUARD_END(CRT_ERR_DEVICE) }
int crt_host_renderer_tick(crt_host_renderer* r, float dt) { if (!r) return CRT_ERR_INVALID; GUARD_BEGIN r->r->Tick(dt); return CRT_OK; GUARD_END(CRT_ERR_DEVICE) }
int crt_host_renderer_tick_whitted(crt_host_renderer* r) { if (!r) return CRT_ERR_INVALID; GUARD_BEGIN r->r->TickWhitted(); return CRT_OK; GUARD_END(CRT_ERR_DEVICE) }
int crt_host_renderer_set_inspect(crt_host_renderer* r, int traversal, int tests)
{
    if (!r) return CRT_ERR_INVALID;
    r->r->m_inspectTraversal = traversal != 0; r->r->m_inspectIntersectionTest = tests != 0;
    return CRT_OK;
}
int crt_host_renderer_whitted_metrics(crt_host_renderer* r, crt_whitted_metrics* out, float* averageTraversal, float* averageTests)
{
    if (!r) return CRT_ERR_INVALID;
    const Renderer& R = *r->r;
    if (out) { out->rayHitCount = R.m_rayHitCount; out->totalTraversal = R.m_totalTraversal; out->totalTests = R.m_totalTests; out->peakTraversal = R.m_peakTraversal; out->peakTests = R.m_peakTests; }
    if (averageTraversal) *averageTraversal = R.m_averageTraversal;
    if (averageTests) *averageTests = R.m_averageTests;
    return CRT_OK;
}
int crt_host_renderer_render(crt_host_renderer* r, int frames) { if (!r) return CRT_ERR_INVALID; GUARD_BEGIN r->r->Render(frames); return CRT_OK; GUARD_END(CRT_ERR_DEVICE) }
int crt_host_renderer_spp(crt_host_renderer* r) { return r ? r->r->spp : CRT_ERR_INVALID; }
float crt_host_renderer_energy(crt_host_renderer* r) { return r ? r->r->energy : 0.0f; }
const float* crt_host_renderer_accumulator(crt_host_renderer* r) { return r ? r->r->accumulator : nullptr; }
const uint32_t* crt_host_renderer_screen(crt_host_renderer* r) { return (r && r->r->screen) ? r->r->screen->pixels.data() : nullptr; }
crt_ctx* crt_host_renderer_ctx(crt_host_renderer* r) { return r ? r->r->ctx : nullptr; }

int crt_host_obj_load(const char* path, uint32_t* corners, float** pos, float** nrm, float** uv)
{
    if (!path || !corners || !pos || !nrm || !uv) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const MeshCorners m = LoadObj(path);
    const size_t n = m.count();
    *corners = (uint32_t)n;
    *pos = (float*)malloc(n * 12); *nrm = (float*)malloc(n * 12); *uv = (float*)malloc(n * 8);
    memcpy(*pos, m.pos.data(), n * 12); memcpy(*nrm, m.nrm.data(), n * 12); memcpy(*uv, m.uv.data(), n * 8);
    return CRT_OK;
    GUARD_END(CRT_ERR_IO)
}
int crt_host_image_load(const char* path, int* w, int* h, uint32_t** pixels)
{
    if (!path || !w || !h || !pixels) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    const Image img = LoadImage(path);
    *w = img.width; *h = img.height;
    *pixels = (uint32_t*)malloc(img.pixels.size() * 4);
    memcpy(*pixels, img.pixels.data(), img.pixels.size() * 4);
    return CRT_OK;
    GUARD_END(CRT_ERR_IO)
}
void crt_host_free(void* p) { free(p); }

// FileScene's alternative accelerators (file_scene.h:10-12: USE_KDTree is what the reference ships): built over the scene's triangle array on the host.
// TLASFileScene with TLAS_USE_KDTree / TLAS_USE_Grid (tlas_file_scene.cpp:40-90): BLASKDTree / BLASGrid per BLAS over its own triangle array.
int crt_host_scene_build_alt(crt_host_scene* s, int kind)
{
    if (!s) { g_err = "null argument"; return CRT_ERR_INVALID; }
    GUARD_BEGIN
    if (kind == CRT_ACCEL_GRID) s->gridDeviceBuilt = false;                          // cells and triangles are both the host's again
    if (kind == CRT_ACCEL_KDTREE) s->kdDeviceBuilt = false;
    if (s->tlas) {
        const std::vector<BLASBVH*>& bl = s->tlas->tlas.blas;
        if (kind == CRT_ACCEL_KDTREE) {
            s->blasKd.assign(bl.size(), BLASKDTree());
            for (size_t i = 0; i < bl.size(); i++) { s->blasKd[i].objIdx = bl[i]->objIdx; s->blasKd[i].triangles = bl[i]->triangles; s->blasKd[i].Build(); }
        } else if (kind == CRT_ACCEL_GRID) {
            s->blasGrid.assign(bl.size(), BLASGrid());
            for (size_t i = 0; i < bl.size(); i++) { s->blasGrid[i].objIdx = bl[i]->objIdx; s->blasGrid[i].triangles = bl[i]->triangles; s->blasGrid[i].Build(); }
        } else { g_err = "unknown accelerator kind"; return CRT_ERR_INVALID; }
        return CRT_OK;
    }
    if (kind == CRT_ACCEL_KDTREE) { delete s->kd; s->kd = new KDTree(); s->kd->triangles = s->file->acc.triangles; s->kd->Build(); }
    else if (kind == CRT_ACCEL_GRID) { delete s->grid; s->grid = new Grid(); s->grid->triangles = s->file->acc.triangles; s->grid->Build(); }
    else { g_err = "unknown accelerator kind"; return CRT_ERR_INVALID; }
    return CRT_OK;
    GUARD_END(CRT_ERR_INVALID)
}
static int describe_alt(const KDTree* kd, const Grid* grid, int kind, crt_alt_accel& a)
{
    memset(&a, 0, sizeof(a)); a.kind = kind;
    if (kind == CRT_ACCEL_KDTREE && kd) {
        a.triangles = kd->triangles.data(); a.triCount = (uint32_t)kd->triangles.size();
        a.kdNodes = kd->nodes.data(); a.kdNodeCount = (uint32_t)kd->nodes.size(); a.kdTriIndices = kd->leafTriIndices.data(); a.kdTriIndexCount = (uint32_t)kd->leafTriIndices.size();
        return CRT_OK;
    }
    if (kind == CRT_ACCEL_GRID && grid) {
        const Grid& g = *grid;
        a.triangles = g.triangles.data(); a.triCount = (uint32_t)g.triangles.size();
        for (int k = 0; k < 3; k++) { a.gridResolution[k] = g.resolution[k]; a.gridCellSize[k] = g.cellSize[k]; a.gridMin[k] = g.localBounds.bmin3[k]; a.gridMax[k] = g.localBounds.bmax3[k]; }
        a.gridCellStart = g.cellStart.data(); a.gridCellTris = g.cellTris.data(); a.gridCellTriCount = (uint32_t)g.cellTris.size();
        return CRT_OK;
    }
    g_err = "accelerator not built (crt_host_scene_build_alt)"; return CRT_ERR_STATE;
}
static int describe_alt(crt_host_scene* s, int kind, crt_alt_accel& a) { return describe_alt(s->kd, s->grid, kind, a); }
// BLAS `i` of a TLAS scene's set
static int describe_blas_alt(crt_host_scene* s, int kind, int i, crt_alt_accel& a)
{
    if (!s->tlas || i < 0 || i >= (int)s->tlas->tlas.blas.size()) { g_err = "not a TLAS scene / BLAS index out of range"; return CRT_ERR_INVALID; }
    if ((kind == CRT_ACCEL_KDTREE && s->blasKd.empty()) || (kind == CRT_ACCEL_GRID && s->blasGrid.empty())) { g_err = "accelerator not built (crt_host_scene_build_alt)"; return CRT_ERR_STATE; }
    return describe_alt(kind == CRT_ACCEL_KDTREE ? &s->blasKd[(size_t)i] : nullptr, kind == CRT_ACCEL_GRID ? &s->blasGrid[(size_t)i] : nullptr, kind, a);
}
int crt_host_scene_upload_alt(crt_host_scene* s, crt_ctx* ctx, int kind)
{
    if (!s || !ctx) { g_err = "null argument"; return CRT_ERR_INVALID; }
    if (kind == CRT_ACCEL_GRID && s->gridDeviceBuilt) {
        g_err = "crt_host_scene_upload_alt: the grid mirror was refreshed from a device build (crt_host_scene_build_grid_device): its cells are of positions the host triangles never "
                "saw, so the upload would pair new cells with old vertices; crt_host_scene_build_alt(CRT_ACCEL_GRID) builds it from the host's triangles again";
        return CRT_ERR_STATE;
    }
    if (kind == CRT_ACCEL_KDTREE && s->kdDeviceBuilt) {
        g_err = "crt_host_scene_upload_alt: the KD-tree mirror was refreshed from a device build (crt_host_scene_build_kdtree_device): its nodes are of positions the host triangles "
                "never saw, so the upload would pair new nodes with old vertices; crt_host_scene_build_alt(CRT_ACCEL_KDTREE) builds it from the host's triangles again";
        return CRT_ERR_STATE;
    }
    if (s->tlas) {
        std::vector<crt_alt_accel> set(s->tlas->tlas.blas.size());
        for (size_t i = 0; i < set.size(); i++) { const int rc = describe_blas_alt(s, kind, (int)i, set[i]); if (rc) return rc; }
        const int rc = crt_upload_blas_accel(ctx, kind, set.data(), (uint32_t)set.size());
        if (rc != CRT_OK) g_err = crt_last_error(ctx);
        return rc;
    }
    crt_alt_accel a; int rc = describe_alt(s, kind, a); if (rc) return rc;
    rc = crt_upload_alt_accel(ctx, &a);
    if (rc != CRT_OK) g_err = crt_last_error(ctx);
    return rc;
}
// sizes: KD-tree -> {nodes, leaf triangle indices, maxDepth, nodesUsed}; grid -> {rx, ry, rz, cell triangle references}
static void alt_info(const KDTree* kd, int kind, const crt_alt_accel& a, uint32_t out[4])
{
    if (kind == CRT_ACCEL_KDTREE) { out[0] = a.kdNodeCount; out[1] = a.kdTriIndexCount; out[2] = kd->maxDepth; out[3] = kd->nodesUsed; }
    else { out[0] = (uint32_t)a.gridResolution[0]; out[1] = (uint32_t)a.gridResolution[1]; out[2] = (uint32_t)a.gridResolution[2]; out[3] = a.gridCellTriCount; }
}
int crt_host_scene_blas_alt_info(crt_host_scene* s, int kind, int blas, uint32_t out[4])
{
    if (!s || !out) { g_err = "null argument"; return CRT_ERR_INVALID; }
    crt_alt_accel a; int rc = describe_blas_alt(s, kind, blas, a); if (rc) return rc;
    alt_info(kind == CRT_ACCEL_KDTREE ? &s->blasKd[(size_t)blas] : nullptr, kind, a, out);
    return CRT_OK;
}
int crt_host_scene_alt_info(crt_host_scene* s, int kind, uint32_t out[4])
{
    if (!s || !out) { g_err = "null argument"; return CRT_ERR_INVALID; }
    crt_alt_accel a; int rc = describe_alt(s, kind, a); if (rc) return rc;
    if (kind == CRT_ACCEL_KDTREE) { out[0] = a.kdNodeCount; out[1] = a.kdTriIndexCount; out[2] = s->kd->maxDepth; out[3] = s->kd->nodesUsed; }
    else { out[0] = (uint32_t)a.gridResolution[0]; out[1] = (uint32_t)a.gridResolution[1]; out[2] = (uint32_t)a.gridResolution[2]; out[3] = a.gridCellTriCount; }
    return CRT_OK;
}
// copies: KD-tree -> nodes (48 B each) + leaf triangle indices; grid -> f[0..2] cellSize, f[3..5] bounds min, f[6..8] bounds max, cellStart (cells + 1), cell triangle references
static void alt_copy(int kind, const crt_alt_accel& a, void* nodesOrCellStart, void* refs, float* f9);
int crt_host_scene_blas_alt_copy(crt_host_scene* s, int kind, int blas, void* nodesOrCellStart, void* refs, float* f9)
{
    if (!s) { g_err = "null argument"; return CRT_ERR_INVALID; }
    crt_alt_accel a; int rc = describe_blas_alt(s, kind, blas, a); if (rc) return rc;
    alt_copy(kind, a, nodesOrCellStart, refs, f9);
    return CRT_OK;
}
int crt_host_scene_alt_copy(crt_host_scene* s, int kind, void* nodesOrCellStart, void* refs, float* f9)
{
    if (!s) { g_err = "null argument"; return CRT_ERR_INVALID; }
    crt_alt_accel a; int rc = describe_alt(s, kind, a); if (rc) return rc;
    alt_copy(kind, a, nodesOrCellStart, refs, f9);
    return CRT_OK;
}
static void alt_copy(int kind, const crt_alt_accel& a, void* nodesOrCellStart, void* refs, float* f9)
{
    if (kind == CRT_ACCEL_KDTREE) { if (nodesOrCellStart) memcpy(nodesOrCellStart, a.kdNodes, (size_t)a.kdNodeCount * 48); if (refs) memcpy(refs, a.kdTriIndices, (size_t)a.kdTriIndexCount * 4); }
    else {
        const size_t cells = (size_t)a.gridResolution[0] * a.gridResolution[1] * a.gridResolution[2];
        if (nodesOrCellStart) memcpy(nodesOrCellStart, a.gridCellStart, (cells + 1) * 4); if (refs) memcpy(refs, a.gridCellTris, (size_t)a.gridCellTriCount * 4);
        if (f9) for (int k = 0; k < 3; k++) { f9[k] = a.gridCellSize[k]; f9[3 + k] = a.gridMin[k]; f9[6 + k] = a.gridMax[k]; }
    }
}

// test entries: the host front's restatements of the tmplmath.h inlines / the Vertex table, same layout as the real-reference harness's probes (tests/golden/make_golden.py)
void crt_host_math_probe(const float* in, uint32_t n, float* out)
{
    using namespace crt;
    for (uint32_t i = 0; i < n; i++, in += 12, out += 120) {
        const float3 a(in[0], in[1], in[2]), b(in[3], in[4], in[5]), ang(in[6], in[7], in[8]), sc(in[9], in[10], in[11]);
        float* o = out;
        const float3 na = normalize(a), rf = a - 2.0f * b * dot(b, a) /* reflect, tmplmath.h:506 */, cr = cross(a, b);
        o[0] = na.x; o[1] = na.y; o[2] = na.z; o[3] = rf.x; o[4] = rf.y; o[5] = rf.z; o[6] = cr.x; o[7] = cr.y; o[8] = cr.z; o[9] = dot(a, b); o += 10;
        const mat4 mt = mat4::Translate(a), rx = mat4::RotateX(ang.x), ry = mat4::RotateY(ang.y), rz = mat4::RotateZ(ang.z), ms = mat4::Scale(sc);
        memcpy(o, mt.cell, 64); memcpy(o + 16, rx.cell, 64); memcpy(o + 32, ry.cell, 64); memcpy(o + 48, rz.cell, 64); memcpy(o + 64, ms.cell, 64); o += 80;
        mat4 m = ry; m.cell[3] = a.x; m.cell[7] = a.y; m.cell[11] = a.z;
        const mat4 inv = m.FastInvertedTransformNoScale();
        memcpy(o, inv.cell, 64); o += 16;
        aabb bb; bb.Grow(a); bb.Grow(b); bb.Grow(sc);
        o[0] = bb.bmin3.x; o[1] = bb.bmin3.y; o[2] = bb.bmin3.z; o[3] = bb.bmax3.x; o[4] = bb.bmax3.y; o[5] = bb.bmax3.z; o[6] = bb.Area(); o += 7;
        aabb b1, b2; b1.Grow(a); b1.Grow(b); b2.Grow(ang); b2.Grow(sc); b1.Grow(b2);
        o[0] = b1.bmin3.x; o[1] = b1.bmin3.y; o[2] = b1.bmin3.z; o[3] = b1.bmax3.x; o[4] = b1.bmax3.y; o[5] = b1.bmax3.z; o[6] = b1.Area();
    }
}
uint32_t crt_host_vertex_dedup(const float* v8, uint32_t n, uint32_t* idx, float* unique8)
{
    crt::MeshCorners m;
    for (uint32_t i = 0; i < n; i++) { m.pos.insert(m.pos.end(), v8 + 8 * i, v8 + 8 * i + 3); m.nrm.insert(m.nrm.end(), v8 + 8 * i + 3, v8 + 8 * i + 6); m.uv.insert(m.uv.end(), v8 + 8 * i + 6, v8 + 8 * i + 8); }
    std::vector<float> P, N, U; std::vector<uint32_t> ix;
    crt::DedupVertices(m, P, N, U, ix);
    memcpy(idx, ix.data(), ix.size() * 4);
    for (size_t k = 0; k < P.size() / 3; k++) { memcpy(unique8 + 8 * k, &P[3 * k], 12); memcpy(unique8 + 8 * k + 3, &N[3 * k], 12); memcpy(unique8 + 8 * k + 6, &U[2 * k], 8); }
    return (uint32_t)(P.size() / 3);
}

} // extern "C"
