// b32_pose.hip -- the modeler's bones on the device: a rigged resident mesh is posed ONCE per change of the bone table, into the slot's
// own vertices (b32_scene_set_rig, b32_scene_pose; the host side is in b32_scene.hip).
//
// Reference: the modeler skins per vertex on the host in four places per frame -- the draw (modeler/viewport.rs:1196-1240), the box
// selection (:1677-1694), the selection brackets (:1796-1810) and the hover (:2401-2421) -- all with rotate_by_euler(v.pos, bone_rot) +
// bone_pos (modeler/state.rs:30-54).  The arithmetic is in b32_pose_body.h.
//
// GPU form.  Everything that reads a slot's vertices (k_setup, the wire list it writes, k_pick, k_hover, k_box_select, k_pack_streams,
// k_merge_mesh) reads B32Vertex records; a pose pass writes posed records there and none of those kernels changes.
//   k_pose_rest   one lane per vertex: position and normal of the slot's vertices into the rest stream (24 B per vertex).
//   k_pose        one lane per vertex: rest stream + bone index -> position and normal of the slot's vertex (uv and colour are not
//                 touched).  Always from the rest stream, so poses never accumulate.  The bone table is the kernel argument (64 x 32 B):
//                 two poses in flight never see each other's table and the host keeps no staging buffer alive.  The workgroup copies it
//                 into LDS first -- a lane's bone index is divergent, and a divergent index into the argument block would otherwise become
//                 a private copy of the table (scratch).
#include "b32_pose_body.h"

namespace b32 {

struct PoseTable { B32Bone b[B32_MAX_BONES]; };
struct PoseArgs {
    const float* rest;              // nv x (position, normal)
    const uint16_t* bone_of;        // nv
    B32Vertex* verts;
    uint32_t nv, n_bones;           // n_bones <= B32_MAX_BONES
};
static_assert(sizeof(B32Bone) == 32 && sizeof(PoseTable) == 2048 && sizeof(PoseTable) + sizeof(PoseArgs) <= 3072, "B32Bone layout / kernel argument size");
static_assert(offsetof(B32Vertex, pos) == 0 && offsetof(B32Vertex, normal) == 20 && sizeof(B32Vertex) == 36, "B32Vertex layout");

__global__ __launch_bounds__(256) void k_pose_rest(const B32Vertex* verts, uint32_t nv, float* rest) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nv) return;
    const uint32_t* v = reinterpret_cast<const uint32_t*>(verts + i);
    uint32_t* r = reinterpret_cast<uint32_t*>(rest) + (size_t)i * 6;
    r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[5]; r[4] = v[6]; r[5] = v[7];
}

__global__ __launch_bounds__(256) void k_pose(PoseArgs a, PoseTable table) {
    __shared__ uint32_t bones[sizeof(PoseTable) / 4];
    {   // 8 words per bone, two trips of 256 lanes (the words past n_bones are never read)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&table);
        const uint32_t words = a.n_bones * 8u;
        for (uint32_t k = threadIdx.x; k < words; k += 256u) bones[k] = src[k];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nv) return;
    const uint32_t b = a.bone_of[i];
    const uint32_t* r = reinterpret_cast<const uint32_t*>(a.rest) + (size_t)i * 6;
    uint32_t* v = reinterpret_cast<uint32_t*>(a.verts + i);
    if (b >= a.n_bones) {           // bone_transforms.get(idx) == None (B32_BONE_NONE included): the rest bits
        v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[5] = r[3]; v[6] = r[4]; v[7] = r[5];
        return;
    }
    B32Bone bn;
    {
        const uint32_t* w = bones + b * 8u;
        bn.pos[0] = __uint_as_float(w[0]); bn.pos[1] = __uint_as_float(w[1]); bn.pos[2] = __uint_as_float(w[2]);
        bn.cos_x = __uint_as_float(w[3]); bn.sin_x = __uint_as_float(w[4]); bn.cos_z = __uint_as_float(w[5]); bn.sin_z = __uint_as_float(w[6]);
        bn.rotate = w[7];
    }
    float rest[6], out[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) rest[k] = __uint_as_float(r[k]);
    pose_vertex(&bn, rest, out);
    v[0] = __float_as_uint(out[0]); v[1] = __float_as_uint(out[1]); v[2] = __float_as_uint(out[2]);
    v[5] = __float_as_uint(out[3]); v[6] = __float_as_uint(out[4]); v[7] = __float_as_uint(out[5]);
}

void launch_pose_rest(hipStream_t s, const B32Vertex* verts, uint32_t nv, float* rest) {
    if (!nv) return;
    hipLaunchKernelGGL(k_pose_rest, dim3((uint32_t)(((unsigned long long)nv + 255u) / 256u)), dim3(256), 0, s, verts, nv, rest);
}

void launch_pose(hipStream_t s, const float* rest, const uint16_t* bone_of, B32Vertex* verts, uint32_t nv, const B32Bone* bones, uint32_t n_bones) {
    if (!nv) return;
    PoseArgs a{ rest, bone_of, verts, nv, n_bones };
    PoseTable t{};
    for (uint32_t k = 0; k < n_bones && k < B32_MAX_BONES; ++k) t.b[k] = bones[k];
    hipLaunchKernelGGL(k_pose, dim3((uint32_t)(((unsigned long long)nv + 255u) / 256u)), dim3(256), 0, s, a, t);
}

}  // namespace b32
