// b32_mirror.hip -- the modeler's mirror editing on the device: b32_scene_build_mirror writes into a DERIVED slot the mesh the reference
// assembles from the combined mesh while MirrorSettings is enabled; b32_mirror_counts.
//
// Reference: behind the selected object's vertices the draw appends their twins -- mirrored in local space, then skinned by the source
// vertex's bone, colour dimmed -- and behind each of the object's triangles its twin with reversed winding; later objects' vertices shift
// (modeler/viewport.rs:1209-1311).  A twin stands DIRECTLY behind its source face: equal painter's keys and equal depths are decided by face
// order, so the twins cannot be a tail behind the body.  The arithmetic of one output is b32_mirror_body.h.
//
// GPU form.  The source slot keeps the combined mesh and is what pose, patch, hover, box selection and the overlays address; the derived
// slot is what the frame draws.
//   k_mirror_mesh<RIGGED>  one lane per OUTPUT element, gather form: lane t writes vertex t while t < nv_out and face t while t < nf_out
//                          (the grid is sized by the larger count), whole dwords, 9 per vertex and 5 per face, as k_pose moves them.  A
//                          copied or shifted vertex is its source's dwords; a twin reads the LOCAL position and normal (the rest stream of
//                          a rigged source, else the vertex itself), flips one sign bit in each and, on a rigged source, runs pose_vertex
//                          with the source vertex's bone.  The bone table travels by value in the launch like k_pose's -- two builds in
//                          flight never see each other's table -- and is staged in LDS only in the rigged instantiation: a lane's bone
//                          index is divergent, and a divergent index into the argument block would become a private copy of the table
//                          (scratch; b32_pose.hip).  Lane 0 writes the slot's device-side face count.  No atomics, no scratch.
#include "b32_host.h"
#include "b32_mirror_body.h"

namespace b32 {

struct MirrorTable { B32Bone b[B32_MAX_BONES]; };
struct MirrorArgs {
    B32Mirror m;
    const uint32_t* verts;          // the source's body: bv x 9 dwords
    const uint32_t* faces;          // bf x 5 dwords
    const uint32_t* rest;           // rigged: bv x 6 dwords
    const uint16_t* bone_of;        // rigged: bv
    uint32_t* out_verts; uint32_t* out_faces; uint32_t* consts;
    uint32_t nv_out, nf_out, n_bones;   // n_bones <= B32_MAX_BONES
};
static_assert(sizeof(B32Mirror) == 32 && sizeof(MirrorTable) == 2048 && sizeof(MirrorTable) + sizeof(MirrorArgs) <= 3072, "B32Mirror layout / kernel argument size");
static_assert(sizeof(B32Vertex) == 36 && sizeof(B32Face) == 20 && offsetof(B32Vertex, uv) == 12 && offsetof(B32Vertex, normal) == 20 && offsetof(B32Vertex, r) == 32 &&
              offsetof(B32Vertex, blend) == 35, "B32Vertex / B32Face layout");

template <bool RIGGED>
__global__ __launch_bounds__(256) void k_mirror_mesh(MirrorArgs a, MirrorTable table) {
    __shared__ uint32_t bones[RIGGED ? sizeof(MirrorTable) / 4 : 1];
    if (RIGGED) {                   // 8 words per bone, two trips of 256 lanes (the words past n_bones are never read)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&table);
        const uint32_t words = a.n_bones * 8u;
        for (uint32_t k = threadIdx.x; k < words; k += 256u) bones[k] = src[k];
        __syncthreads();
    }
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t == 0u) { a.consts[0] = a.nf_out; a.consts[1] = 0u; a.consts[2] = 0u; a.consts[3] = 0u; }     // (h_consts of an upload)
    if (t < a.nv_out) {
        bool twin;
        const uint32_t s = mirror_vertex_source(a.m, t, twin);
        const uint32_t* v = a.verts + (size_t)s * 9;
        uint32_t w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = v[k];
        if (twin) {
            uint32_t local[6] = { w[0], w[1], w[2], w[5], w[6], w[7] };
            uint32_t b = B32_BONE_NONE;
            if (RIGGED) {
                const uint32_t* r = a.rest + (size_t)s * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) local[k] = r[k];
                b = a.bone_of[s];
            }
            uint32_t o[9];
            if (RIGGED && b < a.n_bones) {      // (each call names its bone statically: the record stays in registers)
                const uint32_t* q = bones + b * 8u;
                B32Bone bn;
                bn.pos[0] = __uint_as_float(q[0]); bn.pos[1] = __uint_as_float(q[1]); bn.pos[2] = __uint_as_float(q[2]);
                bn.cos_x = __uint_as_float(q[3]); bn.sin_x = __uint_as_float(q[4]); bn.cos_z = __uint_as_float(q[5]); bn.sin_z = __uint_as_float(q[6]);
                bn.rotate = q[7];
                mirror_twin_vertex(w, local, a.m.axis, a.m.dim, &bn, o);
            } else {                            // bone_transforms.get(idx) == None (B32_BONE_NONE included), or no rig: the mirrored bits
                mirror_twin_vertex(w, local, a.m.axis, a.m.dim, nullptr, o);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = o[k];
        }
        uint32_t* d = a.out_verts + (size_t)t * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = w[k];
    }
    if (t < a.nf_out) {
        uint32_t kind;
        const uint32_t s = mirror_face_source(a.m, t, kind);
        const uint32_t* f = a.faces + (size_t)s * 5;
        uint32_t in[5], o[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) in[k] = f[k];
        mirror_face(in, kind, a.m.v_count, o);
        uint32_t* d = a.out_faces + (size_t)t * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) d[k] = o[k];
    }
}

}  // namespace b32

extern "C" {

int b32_mirror_counts(uint32_t nv, uint32_t nf, const B32Mirror* mirror, uint32_t* nv_out, uint32_t* nf_out) {
    return mirror_counts(nv, nf, mirror, nv_out, nf_out);
}

// Another mesh in `dst`, like an upload's (geometry_replaced); `src` is read and nothing of it changes.  The ordering argument is the
// pose's: the kernel is main-stream work behind whatever wrote src's vertices and in front of dst's next frame.
int b32_scene_build_mirror(b32_ctx* c, b32_scene* src_slot, b32_scene* dst_slot, const B32Mirror* mirror) {
    if (!c || !mirror) return B32_E_ARG;
    b32_scene* src = scene_of(c, src_slot);
    b32_scene* dst = scene_of(c, dst_slot);
    if (!src || !dst || src == dst) return B32_E_ARG;
    const uint32_t bv = src->body_nv(), bf = src->body_nf();
    uint32_t nv = 0, nf = 0;
    { const int rcm = mirror_counts(bv, bf, mirror, &nv, &nf); if (rcm) return rcm; }
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    int rc;
    // the face tally of the built mesh from src's host copy of its faces (the first build after src's upload synchronises once; face patches
    // of src keep the copy current): the range's faces count twice, a texture's blend mode is dst's.  own and alpha do not depend on the
    // textures, so a src none of whose faces blends needs the walk only for a dst with a blending texture
    if ((rc = patch_fetch_faces(c, src))) return rc;
    FaceTally tally;
    if (src->tally.own != 0 || src->tally.alpha != 0 || dst->tex_blend_any) {
        const auto blends = [dst](uint32_t t) { return tex_blends(dst, t); };
        tally = tally_faces(src->h_faces.data(), bf, blends);
        for (uint32_t k = 0; k < mirror->f_count; ++k) tally_face(tally, src->h_faces[mirror->f_first + k], true, blends);
    }
    if ((rc = ensure(c, dst->d_verts, dst->cap_verts, (size_t)nv + 1))) return rc;
    if ((rc = ensure(c, dst->d_faces, dst->cap_faces, (size_t)nf + 1))) return rc;
    if (!dst->d_consts) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&dst->d_consts), 16 * sizeof(uint32_t)));
    if ((rc = ensure_work(c, nf))) return rc;
    const bool same_nf = dst->nf == nf;
    dst->nv = nv; dst->nf = nf;
    geometry_replaced(*dst, edit_words(c), same_nf, blend_fresh(tally, *dst, dst->fmt8, dst->tex_blend_any, dst->blend_texels8));
    const bool rigged = src->have_rig;
    MirrorArgs a{};
    a.m = *mirror;
    a.verts = reinterpret_cast<const uint32_t*>(src->d_verts); a.faces = reinterpret_cast<const uint32_t*>(src->d_faces);
    a.rest = rigged ? reinterpret_cast<const uint32_t*>(src->d_rest) : nullptr; a.bone_of = rigged ? src->d_bone_of : nullptr;
    a.out_verts = reinterpret_cast<uint32_t*>(dst->d_verts); a.out_faces = reinterpret_cast<uint32_t*>(dst->d_faces); a.consts = dst->d_consts;
    a.nv_out = nv; a.nf_out = nf;
    a.n_bones = rigged ? (uint32_t)std::min<size_t>(src->h_bones.size(), B32_MAX_BONES) : 0u;
    MirrorTable t{};
    for (uint32_t k = 0; k < a.n_bones; ++k) t.b[k] = src->h_bones[k];
    const uint32_t lanes = std::max(nv, nf);
    const uint32_t groups = (uint32_t)(((unsigned long long)lanes + 255u) / 256u);
    if (rigged) hipLaunchKernelGGL(k_mirror_mesh<true>, dim3(groups ? groups : 1u), dim3(256), 0, c->stream, a, t);
    else hipLaunchKernelGGL(k_mirror_mesh<false>, dim3(groups ? groups : 1u), dim3(256), 0, c->stream, a, t);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}

}  // extern "C"
