// scene.h — C++ front of the MI355X back end: the reference's scene / camera / renderer surface re-implemented on
// top of the C ABI (include/crt_abi.h).  A host application written against the reference's classes
//   FileScene / TLASFileScene   (infra/scene/file_scene.h, tlas_file_scene.h: ctor(path), FindNearest, members)
//   Camera                      (template/camera.h: GetPrimaryRay inputs, SetCameraState)
//   Renderer                    ("3. PathTracer/renderer.h": Init, Tick, ClearAccumulator, accumulator, spp, passes, energy)
// can switch to these with the same calls; construction (XML + OBJ + textures + SAH-BVH / TLAS build) stays on the CPU,
// FindNearest and the whole tile loop of Tick run on the GPU.
#pragma once
#include "accel.h"
#include "loaders.h"

#include <memory>
#include <string>
#include <vector>

namespace crt {

struct Ray {                       // template/ray.h subset that crosses the FindNearest seam
    Ray() = default;
    Ray(const float3& origin, const float3& direction, float distance = 1e34f, int idx = -1) : O(origin), D(direction), t(distance), objIdx(idx) {}
    float3 O, D;
    float t = 1e34f;
    float2 barycentric;
    int objIdx = -1, triIdx = -1;
    int traversed = 0, tested = 0;
    bool inside = false;
};

struct Material {                  // template/material.h
    bool isLight = false;
    float reflectivity = 0, refractivity = 0;
    float3 absorption;
    int texture = -1;              // index into BaseScene::textures (the reference owns a Texture through unique_ptr)
};

struct HitInfo {                   // infra/hit_info.h, plus the albedo the same query computes
    float3 normal;                 // already flipped to face the ray
    float2 uv;
    Material* material = nullptr;  // &primitiveMaterials[0 / 1] or materials[k]
    float3 albedo;                 // material->GetAlbedo(uv) (template/material.h: the material's texture at uv, or 1)
};

class BaseScene {                  // infra/scene/base_scene.h
public:
    virtual ~BaseScene() = default;
    // flattens and uploads the built scene to the device context (the one call the reference's classes lack)
    int Upload(crt_ctx* ctx);
    // in-place device update after instance motion (BLASBVH::SetTransform + TLASBVH::Build) / Refit: crt_update_scene with this scene's description
    int Update(crt_ctx* ctx, uint32_t what);
    // The scene's look as a crt_update_look record (crt_look_words(materialCount) words): Look writes the current one; SetLook takes one over — the light quad, the
    // floor / skydome texture indices and the materials — so that Upload describes the scene with that look.  Neither touches a device.
    void Look(void* out) const;
    int SetLook(const void* look);
    // scene.FindNearest(ray): one ray through crt_find_nearest (use the batch ABI for many)
    void FindNearest(Ray& ray);
    // scene.IsOccluded(ray): one shadow ray {O, D, t} through crt_is_occluded (light quad bounded by t, then the BVH / TLAS over the whole ray)
    bool IsOccluded(const Ray& ray);
    // scene.GetHitInfo(ray, I) for a ray FindNearest has hit (objIdx >= 0): one record through crt_get_hit_info
    HitInfo GetHitInfo(const Ray& ray, const float3& I);
    // scene.GetSkyColor(ray): one ray through crt_get_sky_color
    float3 GetSkyColor(const Ray& ray);
    float3 GetLightPos() const;
    float3 GetLightColor() const { return float3(24, 24, 22); }
    virtual int GetTriangleCount() const = 0;
    virtual int Kind() const = 0;
    // filled by the subclasses' constructors
    std::string sceneName;
    std::vector<Image> textures;   // [0] floor, [1] skydome, then material textures
    std::vector<Material*> materials;
    Material primitiveMaterials[2];                          // [0] the light (isLight), [1] the floor (texture 0): file_scene.cpp:10-12
    int objCount = 0, materialCount = 0, objIdUsed = 2;
    mat4 lightT, lightInvT; float lightSize = 0.5f;          // Quad light(0, 1)
    int floorTexture = 0, skyTexture = 1;                    // indices into textures (file_scene.cpp:10-19 loads them first)
    float3 floorN{0, 1, 0}; float floorD = 1, floorInvto = 1; // Plane floor(1, (0,1,0), 1, texW/100)
    float animTime = 0;
    void SetTime(float t) { animTime = t; }
    // BVHs refitted on the device only (crt_host_scene_bvh_refit_device): their host triangles / nodes are stale, so Upload and Update(CRT_UPDATE_BOUNDS), which
    // would send them, return CRT_ERR_STATE while one is marked
    std::vector<uint8_t> staleBvh;
    int FirstStaleBvh() const { for (size_t i = 0; i < staleBvh.size(); i++) if (staleBvh[i]) return (int)i; return -1; }
protected:
    void LoadCommon(const SceneData& sd, const std::string& baseDir);
    virtual void Describe(crt_scene_desc& d, std::vector<crt_bvh>& bvhs, std::vector<int32_t>& objMat) = 0;
    struct DescKeep { std::vector<crt_bvh> bvhs; std::vector<int32_t> objMat; std::vector<crt_material> mats; std::vector<crt_texture> tex; };
    void BuildDesc(crt_scene_desc& d, DescKeep& keep);
    crt_ctx* bound = nullptr;
};

class FileScene : public BaseScene {      // infra/scene/file_scene.{h,cpp} with USE_BVH
public:
    explicit FileScene(const std::string& filePath, const std::string& baseDir = "");
    ~FileScene() override;
    int GetTriangleCount() const override { return acc.GetTriangleCount() * objCount; }   // file_scene.cpp:222-230 (UI figure, bug-compatible)
    int Kind() const override { return CRT_SCENE_FILE; }
    uint32_t GetMaxTreeDepth() const { return acc.maxDepth; }
    BVH acc;
    std::vector<Model*> models;
protected:
    void Describe(crt_scene_desc& d, std::vector<crt_bvh>& bvhs, std::vector<int32_t>& objMat) override;
};

class TLASFileScene : public BaseScene {  // infra/scene/tlas_file_scene.{h,cpp} with TLAS_USE_BVH
public:
    explicit TLASFileScene(const std::string& filePath, const std::string& baseDir = "");
    ~TLASFileScene() override;
    int GetTriangleCount() const override { int n = 0; for (auto* b : tlas.blas) n += b->GetTriangleCount(); return n; }
    int Kind() const override { return CRT_SCENE_TLAS; }
    TLASBVH tlas;
protected:
    void Describe(crt_scene_desc& d, std::vector<crt_bvh>& bvhs, std::vector<int32_t>& objMat) override;
};

class Camera {                     // template/camera.h:14-30, 61-73 (keyboard handling is the shell's business)
public:
    Camera(int width, int height) : aspect((float)width / (float)height)
    {
        camPos = float3(0, 0, -2); camTarget = float3(0, 0, -1);
        topLeft = float3(-aspect, 1, 0); topRight = float3(aspect, 1, 0); bottomLeft = float3(-aspect, -1, 0);
    }
    void SetCameraState(const float3& position, const float3& target);
    float aspect;
    float3 camPos, camTarget, topLeft, topRight, bottomLeft;
};

struct Surface { std::vector<uint32_t> pixels; int width = 0, height = 0; };   // template/surface.h: only `pixels` is touched by the path

class Renderer {                   // "3. PathTracer/renderer.{h,cpp}" — TheApp::Init / Tick
public:
    Renderer(BaseScene* scene, int width, int height, int device = 0);
    ~Renderer();
    void Init();
    void ClearAccumulator();
    void Tick(float deltaTime);
    void Render(int frames);       // `frames` Ticks in one submission (no per-frame read-back)
    void TickWhitted();            // one Tick of the Whitted-style renderer ("2. WhittedStyle/renderer.cpp":131-157): accumulator = Trace(primary)
    void ResetWhittedPeaks() { m_averageTraversal = m_averageTests = 0; m_peakTraversal = m_peakTests = 0; }   // what a camera change does ("2. WhittedStyle/renderer.cpp":180-186, 206-212)
    void Shutdown() {}
    // data members the shell / UI reads (renderer.h:46-53)
    std::vector<float> accumulatorStorage; float* accumulator = nullptr;   // float4[W*H], refreshed by Tick
    BaseScene* scene;
    Camera camera;
    int spp = 1, passes = 1;
    bool animating = false;
    float energy = 0, anim_time = 0;
    // performance report of Tick (renderer.cpp:159-161): running average of the frame time in ms, frames per second, primary rays per ms
    float m_avg = 10, m_fps = 0, m_rps = 0, m_alpha = 1;
    // the Whitted renderer's inspection switches and metrics ("2. WhittedStyle/renderer.h":25-33); hit count and totals are the last TickWhitted's, as exact integers
    // (the reference sums them in float), the peaks are carried from Tick to Tick until the camera changes
    bool m_inspectTraversal = false, m_inspectIntersectionTest = false;
    uint64_t m_rayHitCount = 0, m_totalTraversal = 0, m_totalTests = 0;
    float m_averageTraversal = 0, m_averageTests = 0;
    int m_peakTraversal = 0, m_peakTests = 0;
    int depthLimit = 5;
    Surface* screen = nullptr; Surface ownScreen;
    crt_ctx* ctx = nullptr;
    int width, height, device;
private:
    void PushCamera();
};

} // namespace crt
