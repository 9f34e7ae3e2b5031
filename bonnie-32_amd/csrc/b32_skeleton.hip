// b32_skeleton.hip -- the modeler's bone octahedra on the device: the tail of a resident mesh (b32_scene_build_skeleton; the host side
// is in b32_scene.hip).
//
// Reference: while bones are shown the modeler appends skeleton_to_triangles' six vertices and eight faces per bone
// (modeler/skeleton.rs:412-477, :565-660) to the frame's combined mesh before its one render call (modeler/viewport.rs:1196-1395).  The
// arithmetic is in b32_skeleton_body.h.
//
// GPU form.  The host has already computed every tip, dropped the degenerate bones and resolved colour and alpha (64 bones: the table it
// copies anyway), so what arrives is the list of DRAWN octahedra, by value in the kernel argument (65 x 32 B): two builds in flight never
// see each other's table and nothing is uploaded.
//   k_skeleton_mesh   one workgroup of 64 lanes per octahedron, of which 14 work: lanes 0..5 write its vertices, lanes 6..13 its faces.
//                     The octahedron's index is the workgroup's, so its record is read from the argument block with scalar loads -- a
//                     per-lane index into the block would become a private copy of the table (scratch).  No LDS.  Workgroup 0 also
//                     writes the scene's face count where the first radix pass reads it (what an upload copies there).
#include "b32_skeleton_body.h"

namespace b32 {

struct SkelTable { SkelOct o[SKEL_MAX_OCTS]; };
struct SkelArgs {
    B32Vertex* verts;               // the slot's vertices: the tail starts at first_vertex
    B32Face* faces;                 // ... and at first_face
    uint32_t* consts;               // b32_scene::d_consts
    uint32_t first_vertex, first_face, n_octs;      // n_octs <= SKEL_MAX_OCTS
};
static_assert(sizeof(SkelTable) == 2080 && sizeof(SkelTable) + sizeof(SkelArgs) <= 3072, "SkelOct layout / kernel argument size");
static_assert(sizeof(B32Vertex) == 36 && sizeof(B32Face) == 20, "B32Vertex / B32Face layout");

__global__ __launch_bounds__(64) void k_skeleton_mesh(SkelArgs a, SkelTable table) {
    const uint32_t oct = blockIdx.x, k = threadIdx.x;
    if (oct == 0u && k == 63u) { a.consts[0] = a.first_face + a.n_octs * SKEL_OCT_FACES; a.consts[1] = 0u; a.consts[2] = 0u; a.consts[3] = 0u; }
    if (oct >= a.n_octs || k >= SKEL_OCT_ELEMS) return;
    const SkelOct& o = table.o[oct];
    const uint32_t v0 = a.first_vertex + oct * SKEL_OCT_VERTS;
    if (k < SKEL_OCT_VERTS) {
        B32Vertex v;
        skel_vertex(o, k, v);
        a.verts[(size_t)v0 + k] = v;
    } else {
        B32Face f;
        skel_face(o, k - SKEL_OCT_VERTS, v0, f);
        a.faces[(size_t)a.first_face + (size_t)oct * SKEL_OCT_FACES + (k - SKEL_OCT_VERTS)] = f;
    }
}

void launch_skeleton_mesh(hipStream_t s, const SkelOct* octs, uint32_t n_octs, B32Vertex* verts, uint32_t first_vertex, B32Face* faces, uint32_t first_face,
                          uint32_t* consts) {
    if (n_octs > SKEL_MAX_OCTS) n_octs = SKEL_MAX_OCTS;
    SkelArgs a{ verts, faces, consts, first_vertex, first_face, n_octs };
    SkelTable t{};
    for (uint32_t k = 0; k < n_octs; ++k) t.o[k] = octs[k];
    hipLaunchKernelGGL(k_skeleton_mesh, dim3(n_octs ? n_octs : 1u), dim3(64), 0, s, a, t);
}

}  // namespace b32
