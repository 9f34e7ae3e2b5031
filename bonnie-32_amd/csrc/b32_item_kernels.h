// b32_item_kernels.h -- what the kernels that turn caller input into B32Prim records share (b32_world.hip, b32_gizmo.hip,
// b32_room_overlay.hip, b32_overlay.hip, b32_object_overlay.hip): the drawn / dropped / rejected counting tail, a wave's minimum and
// maximum of a key, and the pair of kernels of a one-lane-per-item producer whose small batches travel in the kernel argument.
#pragma once
#include "b32_device.h"

namespace b32 {

// ---- the counting tail: one add per wave into LDS, one per workgroup and counter into memory (100 000 single adds to one address take a
// millisecond; integer sums, so the totals do not depend on the order of the adds).  outcome_tally() at the kernel's start, ONE of the two
// outcome_count forms at its end.  Both hold a barrier and the tail works wave-wide, so EVERY lane of the workgroup must reach them: a
// lane without an item takes part with an outcome that counts nothing (`live` in the item kernels below).
__device__ __forceinline__ uint32_t* outcome_tally() {
    __shared__ uint32_t tally[3];                               // the workgroup's drawn / dropped / rejected
    if (threadIdx.x < 3u) tally[threadIdx.x] = 0u;
    __syncthreads();
    return tally;
}
__device__ __forceinline__ void outcome_flush(const uint32_t* tally, unsigned long long* counts) {
    __syncthreads();
    if (threadIdx.x < 3u && tally[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}
// which: the counter this lane's item adds one to (0 drawn, 1 dropped, 2 rejected); anything else: none
__device__ __forceinline__ void outcome_count(uint32_t* tally, unsigned long long* counts, uint32_t which) {
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const unsigned long long m = __ballot(which == k);      // (wave64: one bit per lane)
        if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&tally[k], (uint32_t)__popcll(m));
    }
    outcome_flush(tally, counts);
}
// packed: this lane's calls per counter in three 10-bit fields (counter k at bit 10 * k).  A wave's sum of a field must stay under 1024:
// at most 15 calls per lane and counter.
__device__ __forceinline__ void outcome_count_packed(uint32_t* tally, unsigned long long* counts, uint32_t packed) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) packed += (uint32_t)__shfl_xor((int)packed, o, 64);
    if ((threadIdx.x & 63u) == 0u && packed) {
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) { const uint32_t c = (packed >> (10u * k)) & 1023u; if (c) atomicAdd(&tally[k], c); }
    }
    outcome_flush(tally, counts);
}

// ---- a wave's minimum / maximum of an orderable key (overlay_key, b32_overlay_body.h) in every lane: k_overlay_points' and
// k_scene_bounds' bounds.  Cross-lane only, no LDS round trip.
__device__ __forceinline__ uint32_t overlay_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t overlay_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// ---- one lane per item.  A producer P states  Args, Row, SMALL,  n(a) (the batch's rows),  rows(a) (where they lie on the device)  and
// item(a, row, i, live)  (row i; `live`: i < n, the other lanes only take part in the counting).  Its two __global__ kernels call
// item_small (at most SMALL rows out of the kernel argument: one workgroup) and item_large; launch_items picks between them.
template <class P> struct ItemBatch { typename P::Row r[P::SMALL]; };
template <class P>
__device__ __forceinline__ void item_small(const typename P::Args& a, const ItemBatch<P>& batch) {
    const uint32_t i = threadIdx.x;
    const bool live = i < P::n(a);
    P::item(a, live ? batch.r[i] : typename P::Row{}, i, live);
}
template <class P>
__device__ __forceinline__ void item_large(const typename P::Args& a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P::n(a);
    P::item(a, live ? P::rows(a)[i] : typename P::Row{}, i, live);
}
// small != nullptr: n <= SMALL rows passed by value
template <class P>
void launch_items(hipStream_t s, void (*k_small)(typename P::Args, ItemBatch<P>), void (*k_large)(typename P::Args), const typename P::Args& a,
                  const typename P::Row* small) {
    const uint32_t n = P::n(a);
    if (!n) return;
    if (small) {
        ItemBatch<P> batch{};
        for (uint32_t i = 0; i < n && i < P::SMALL; ++i) batch.r[i] = small[i];
        hipLaunchKernelGGL(k_small, dim3(1), dim3(256), 0, s, a, batch);
        return;
    }
    hipLaunchKernelGGL(k_large, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace b32
