// gsr_features.h -- internal interface between csrc/grid.hip (the point grid and the hybrid search over it),
// csrc/features.hip (FPFH, feature matching, RANSAC) and csrc/fgr.hip (Fast Global Registration).  Not part of include/gsr_hip.h.
#pragma once
#include "gsr_common.h"

namespace gsr {

// Largest max_nn the hybrid search takes: a wave keeps its candidates in an LDS list of GSR_HYBRID_CAP entries and prunes it
// to the max_nn best whenever it would overflow, so max_nn must leave room for a wave's worth of new candidates.
#define GSR_HYBRID_CAP 1024
#define GSR_HYBRID_MAX_NN 512

// Open3D KDTreeSearchParamHybrid(radius, max_nn) for every point of the cloud against the cloud itself, on a point grid of its own
// (GridIndex, gsr_grid.h): nbr[i * max_nn + k] = input index of the k-th neighbour of point i in (d^2, index) order, cnt[i] = how many,
// where d^2 = (p_i - p_j)^2 summed x, y, z in float64 from the float32 coordinates and a neighbour satisfies d^2 <= radius^2.
// xyz_dev, nbr_dev, cnt_dev: device memory.  Enqueued on `stream`, synchronises it before returning.
int32_t hybrid_search_dev(const float* xyz_dev, int64_t n, double radius, int max_nn, int device, hipStream_t stream, int* nbr_dev,
                          int* cnt_dev);

// The counter-based sampler of include/gsr_hip.h, shared by the RANSAC hypotheses (features.hip) and the FGR triples (fgr.hip).
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// row j of hypothesis / trial k among m correspondences
__host__ __device__ __forceinline__ uint32_t ransac_draw(uint64_t seed, uint64_t k, uint32_t j, uint32_t m) {
    const uint64_t z = splitmix64(seed ^ splitmix64(k * 64ull + (uint64_t)j));
    return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}

}  // namespace gsr
