// patch_tally_host.cpp -- the host-only part of the in-place edits (csrc/b32_patch_tally.h) in a program of its own, for a build with
// the address and undefined-behaviour sanitizers: random sequences of face patches are validated by the record rules and applied to a
// host copy with the incremental tally, which must equal the tally counted from scratch after every patch; then the slot's bookkeeping
// through the transitions to and from "no face blends", with and without a tail.  Prints "ok" and returns 0, or says what differed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "b32_patch_tally.h"

using namespace b32;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {       // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return n ? (uint32_t)(z % n) : 0u;
}
static B32Face random_face(uint32_t nt) {
    static const uint8_t alphas[] = { 0, 100, 254, 255, 255, 255 };
    B32Face f{};
    f.v[0] = rnd(1000); f.v[1] = rnd(1000); f.v[2] = rnd(1000);
    const uint32_t pick = rnd(nt + 2);
    f.texture_id = pick < nt ? pick : (pick == nt ? nt + 5 : B32_NO_TEXTURE);
    f.black_transparent = (uint8_t)rnd(2);
    f.blend_mode = rnd(2) ? (uint8_t)B32_BLEND_OPAQUE : (uint8_t)rnd(6);
    f.editor_alpha = alphas[rnd(6)];
    return f;
}
static bool same(const FaceTally& a, const FaceTally& b) { return a.own == b.own && a.any == b.any && a.alpha == b.alpha; }

int main() {
    const std::vector<uint32_t> tex_blend{ B32_BLEND_OPAQUE, B32_BLEND_ADD, B32_BLEND_OPAQUE };
    const auto blends = [&](uint32_t t) { return t < tex_blend.size() && tex_blend[t] != B32_BLEND_OPAQUE; };
    for (int round = 0; round < 50; ++round) {
        const uint32_t nf = 1 + rnd(300);
        std::vector<B32Face> faces(nf);
        for (B32Face& f : faces) f = random_face((uint32_t)tex_blend.size());
        FaceTally tally = tally_faces(faces.data(), nf, blends);
        for (int step = 0; step < 20; ++step) {
            std::vector<B32FacePatch> recs;
            for (uint32_t i = 0; i < nf; ++i) if (rnd(4) == 0) recs.push_back({ i, random_face((uint32_t)tex_blend.size()) });
            if (!patch_records_ok(recs.data(), sizeof(B32FacePatch), (uint32_t)recs.size(), nf)) { std::printf("ascending records refused\n"); return 1; }
            for (const B32FacePatch& r : recs) { B32Face& f = faces[r.index]; tally_face(tally, f, false, blends); f = r.f; tally_face(tally, f, true, blends); }
            if (!same(tally, tally_faces(faces.data(), nf, blends))) { std::printf("round %d step %d: the incremental tally differs\n", round, step); return 1; }
            // what the rules refuse: a repeated index, a descending pair, an index at the limit
            if (recs.size() >= 2) {
                std::vector<B32FacePatch> bad = recs;
                bad[1].index = bad[0].index;
                if (patch_records_ok(bad.data(), sizeof(B32FacePatch), (uint32_t)bad.size(), nf)) { std::printf("a repeated index accepted\n"); return 1; }
                bad = recs; std::swap(bad[0].index, bad[1].index);
                if (patch_records_ok(bad.data(), sizeof(B32FacePatch), (uint32_t)bad.size(), nf)) { std::printf("descending indices accepted\n"); return 1; }
                bad = recs; bad.back().index = nf;
                if (patch_records_ok(bad.data(), sizeof(B32FacePatch), (uint32_t)bad.size(), nf)) { std::printf("an index at the limit accepted\n"); return 1; }
            }
        }
    }
    if (!patch_records_ok(nullptr, sizeof(B32FacePatch), 0, 0)) { std::printf("no records refused\n"); return 1; }
    if (!patch_rect_ok(3, 4, 1, 1, 4, 5) || patch_rect_ok(0, 0, 5, 1, 4, 4) || patch_rect_ok(0xFFFFFFFFu, 0, 2, 1, 4, 4) || patch_rect_ok(0, 0, 0, 1, 4, 4)) {
        std::printf("rectangle rule\n"); return 1;
    }
    // all opaque -> one blending face -> all opaque; RGB555 and 8-bit colour; no tail, a tail of 16 opaque faces, a tail with 8 blending faces
    for (int fmt8 = 0; fmt8 < 2; ++fmt8)
        for (uint32_t tail_blend = 0; tail_blend <= 16; tail_blend += 8) {
            const bool has_tail = true;
            std::vector<B32Face> faces(40);
            for (B32Face& f : faces) { f = B32Face{}; f.texture_id = 0; f.blend_mode = B32_BLEND_OPAQUE; f.editor_alpha = 255; }
            FaceTally tally = tally_faces(faces.data(), 40, blends);
            SlotBlend s{ !fmt8 && tail_blend != 0, fmt8 && tail_blend != 0, tail_blend, false, false, 0 };
            B32Face dim = faces[5]; dim.editor_alpha = 100;
            const B32Face steps[2] = { dim, faces[5] };
            for (int k = 0; k < 2; ++k) {
                tally_face(tally, faces[5], false, blends); faces[5] = steps[k]; tally_face(tally, faces[5], true, blends);
                s = tally_slot(tally, s, fmt8 != 0, false, false, has_tail);
                const uint32_t body = k == 0 ? 1u : 0u;
                const bool blend = body + tail_blend != 0;
                if (s.body_blend_faces != body || s.blend_faces != body + tail_blend || (fmt8 ? s.blend8 != blend || s.may_blend : s.may_blend != blend)) {
                    std::printf("fmt8 %d tail %u step %d: bookkeeping differs\n", fmt8, tail_blend, k); return 1;
                }
            }
        }
    std::printf("ok\n");
    return 0;
}
